"""The summary itself, rendered on the device: the launch wrappers of libavsum_render.so (include/avsum_render.h, whose
comment is the definition) and the numpy restatements of what it computes.

The chain used to stop at a list of (start, end) tuples on the host (KeyshotResult.host()) or a uint8 mask
(select_mask_device).  From a mask, ``summary_index`` makes the list of picked frames and the runs of picked frames per
video on the device (RenderTables holds the capacities, host numbers, so no launch waits for a count); ``summary_frames``
gathers the picked frames in a form an encoder takes - BGR, the source's own YUV layout, another layout of the same depth
(``repack``), or YUV 4:2:0 made from BGR frames (``bgr_to_yuv``, the forward of yuv.yuv_to_bgr) -; ``summary_audio`` cuts
the matching samples out of the concatenated tracks, with an optional linear fade per run.  Nothing is read back until
a result's host(), which downloads the small tables and never pixels or samples.  Host tensors are refused: there is no
CPU fallback.  ``summary_index_host``, ``bgr_to_yuv_host``, ``bgr_to_frames_host``, ``repack_host`` and
``summary_audio_host`` are the definitions in numpy, for tests and studies: the kernels are held to them bit for bit.
"""
import ctypes

import numpy as np
import torch

from . import yuv as _yuv
from ._render_abi import (AUDIO_COLS, FORWARD_INTS, MAX_ROW_SUM, SHIFT, SURFACE_FIELDS, SURFACE_INTS, TOTAL_COLS, check, lib)
from ._yuv_abi import SURFACE_FIELDS as _YUV_SURFACE_FIELDS
from .ingest import Nv12Frames
from .ops import RenderTables, _device_arg, _p, _stream, _tables_arg, gather_rows
from .yuv import YuvFrames

__all__ = ["FORWARD_MATRICES", "FORWARD_MATRICES_F64", "RenderTables", "SummaryIndex", "SummaryRender", "summary_index",
           "summary_frames", "summary_audio", "bgr_to_yuv", "repack", "summary_index_host", "bgr_to_yuv_host",
           "bgr_to_frames_host", "repack_host", "store_samples_host", "summary_audio_host", "audio_bounds_host"]

assert SURFACE_FIELDS == _YUV_SURFACE_FIELDS and SURFACE_INTS == len(SURFACE_FIELDS)   # YuvFrames.surface() serves both
assert (SHIFT, MAX_ROW_SUM, FORWARD_INTS, TOTAL_COLS, AUDIO_COLS) == (20, 1 << 20, 10, 3, 3)

# (y_off, yb, yg, yr, ub, ug, ur, vb, vg, vr): the three-decimal formulas whose inverses ingest.MATRICES_F64 holds ...
FORWARD_MATRICES_F64 = {
    "bt601": (16, 0.098, 0.504, 0.257, 0.439, -0.291, -0.148, -0.071, -0.368, 0.439),
    "bt709": (16, 0.062, 0.614, 0.183, 0.439, -0.339, -0.101, -0.040, -0.399, 0.439),
}
# ... and rint(c * 2^20) of them: the integers of the header's definition
FORWARD_MATRICES = {name: (m[0],) + tuple(int(np.rint(c * (1 << SHIFT))) for c in m[1:])
                    for name, m in FORWARD_MATRICES_F64.items()}


def _forward(matrix, what):
    """The ten integers of ``matrix``: a name of FORWARD_MATRICES or a sequence (y_off, yb, yg, yr, ub, ug, ur, vb, vg,
    vr)."""
    if isinstance(matrix, str):
        if matrix not in FORWARD_MATRICES:
            raise ValueError(f"{what}: matrix must be one of {sorted(FORWARD_MATRICES)} or ten integers, got '{matrix}'")
        matrix = FORWARD_MATRICES[matrix]
    m = tuple(int(c) for c in matrix)
    if len(m) != FORWARD_INTS or not 0 <= m[0] <= 255 or any(sum(abs(c) for c in m[1 + 3 * r:4 + 3 * r]) > MAX_ROW_SUM
                                                              for r in range(3)):
        raise ValueError(f"{what}: a forward matrix is (y_off in 0..255, three rows of three coefficients, each row's "
                         f"sum of magnitudes <= 2^20), got {m}")
    return m


def _as_yuv(frames, what):
    if isinstance(frames, Nv12Frames):
        return YuvFrames.from_nv12(frames)
    if not isinstance(frames, YuvFrames):
        raise ValueError(f"{what}: frames must be a uint8 BGR tensor [N, h, w, 3], an ingest.Nv12Frames or a yuv.YuvFrames")
    return frames


def _layout(f):
    """What two descriptions share when frames can be copied whole between them."""
    return (f.height, f.width, f.sample_bytes, f.shift, f.pitch_y, f.pitch_c, f.chroma_step, f.u_offset, f.v_offset,
            f.frame_stride)


def _surface_arg(f):
    return (ctypes.c_int64 * SURFACE_INTS)(*f.surface())


# --------------------------------------------------------------------------- results
class SummaryIndex:
    """What summary_index leaves on the device for V videos: ``frame_index`` int64 [frame_cap] (the global source frame
    of summary frame j, videos in order; -1 from the true count on), ``frame_offsets`` int64 [V + 1], ``runs`` int64
    [run_cap, 2] (video-relative (start, end) of every maximal stretch of picked frames inside one video; (-1, -1) from
    the true count on), ``run_offsets`` int64 [V + 1], ``totals`` int64 [V, 3] = (runs, frames, samples - 0 until
    summary_audio fills it), TRUE counts even past a capacity, ``count`` (a one-element view of frame_offsets: the
    summary's frames, on the device), with ``plan`` (the RenderTables).  Nothing has been read back; host() is the one
    download."""

    def __init__(self, plan, frame_index, frame_offsets, runs, run_offsets, totals):
        self.plan, self.frame_index, self.frame_offsets = plan, frame_index, frame_offsets
        self.runs, self.run_offsets, self.totals = runs, run_offsets, totals
        self.count = frame_offsets[plan.nvideos:]
        self._host = None

    def _download(self, extra=()):
        nv, cap = self.plan.nvideos, self.plan.run_cap
        flat = torch.cat([self.frame_offsets, self.run_offsets, self.totals.reshape(-1), self.runs.reshape(-1)]
                         + [e.reshape(-1) for e in extra]).cpu().numpy()
        parts = np.split(flat, np.cumsum([nv + 1, nv + 1, TOTAL_COLS * nv, 2 * cap]))
        frame_offsets, run_offsets, totals, runs = parts[0], parts[1], parts[2].reshape(nv, TOTAL_COLS), parts[3].reshape(cap, 2)
        if frame_offsets[nv] > self.plan.frame_cap or run_offsets[nv] > cap:
            raise RuntimeError(f"summary_index: {int(frame_offsets[nv])} frames in {int(run_offsets[nv])} runs exceed the "
                               f"capacities {self.plan.frame_cap} and {cap}")
        host = {"runs": [[(int(s), int(e)) for s, e in runs[run_offsets[v]:run_offsets[v + 1]]] for v in range(nv)],
                "frames": totals[:, 1].copy(), "run_counts": totals[:, 0].copy(), "frame_offsets": frame_offsets,
                "run_offsets": run_offsets}
        return host, parts[4]

    def host(self):
        """{"runs": per video the list of (start, end) tuples, video-relative; "frames", "run_counts": int64 [V];
        "frame_offsets", "run_offsets": int64 [V + 1]}: ONE download, kept.  Raises where a total exceeds its capacity
        (the device tables are then cut short, never overrun)."""
        if self._host is None:
            self._host = self._download()[0]
        return self._host


class SummaryRender:
    """What FrameScoringPipeline.render_device returns: ``index`` (the SummaryIndex), ``frames`` (a uint8 BGR tensor
    [frame_cap, h, w, 3] or a YuvFrames of frame_cap frames; only the first index.count are the summary), ``audio`` fp32
    [sample_cap] and ``audio_offsets`` int64 [V + 1] on the device (None without a waveform).  host() is the one download
    of the small tables - never of pixels or samples."""

    def __init__(self, index, frames, audio=None, audio_offsets=None):
        self.index, self.frames, self.audio, self.audio_offsets = index, frames, audio, audio_offsets
        self._host = None

    def host(self):
        """SummaryIndex.host()'s dictionary and, with audio, "audio_offsets" int64 [V + 1] and "samples" int64 [V]: ONE
        download, kept.  Raises where a total exceeds its capacity."""
        if self._host is None:
            if self.audio is None:
                self._host = dict(self.index.host())
            else:
                # (the totals are read again: their third column is the audio cut's)
                self.index._host = None
                host, offsets = self.index._download([self.audio_offsets])
                if offsets[-1] > self.audio.numel():
                    raise RuntimeError(f"summary_audio: {int(offsets[-1])} samples exceed the capacity {self.audio.numel()}")
                self.index._host = host
                self._host = dict(host, audio_offsets=offsets, samples=np.diff(offsets))
        return self._host


# --------------------------------------------------------------------------- launch wrappers
def summary_index(mask, tables, row=0):
    """The frame list and the runs of a selection, on the device, in three launches with no atomics.  ``mask``: a uint8
    device tensor [N] (1 = the frame is in the summary: select_mask_device's, or any), or [K, N] / an
    evaluation.keyshots.KeyshotResult, of which row ``row`` is rendered.  ``tables``: the ops.RenderTables of the
    videos (RenderTables.from_keyshots(result) sizes it by a result's plan).  Returns a SummaryIndex."""
    if not isinstance(mask, torch.Tensor):
        mask = getattr(mask, "mask", mask)
    _tables_arg(tables, RenderTables, "summary_index")
    dev = tables.device
    _device_arg(mask, "mask", "summary_index", (torch.uint8,), device=dev, contiguous=False)
    if mask.dim() == 2:
        if not 0 <= int(row) < mask.shape[0]:
            raise ValueError(f"summary_index: row {row} outside the {mask.shape[0]} rows of the mask")
        mask = mask[int(row)]
    if mask.dim() != 1 or mask.numel() != tables.frames or not mask.is_contiguous():
        raise ValueError(f"summary_index: the mask must be a contiguous row of {tables.frames} frames, got {list(mask.shape)}")
    nv = tables.nvideos
    small = torch.empty(2 * (nv + 1) + TOTAL_COLS * nv + 2 * tables.ntiles, dtype=torch.int64, device=dev)
    frame_offsets, run_offsets = small[:nv + 1], small[nv + 1:2 * nv + 2]
    totals = small[2 * nv + 2:2 * nv + 2 + TOTAL_COLS * nv].view(nv, TOTAL_COLS)
    work = small[2 * nv + 2 + TOTAL_COLS * nv:]
    frame_index = torch.empty(tables.frame_cap, dtype=torch.int64, device=dev)
    runs = torch.empty((tables.run_cap, 2), dtype=torch.int64, device=dev)
    check(lib().avsr_summary_index(_p(mask), tables.frames, tables.offsets.ctypes.data_as(ctypes.c_void_p), _p(tables.offsets_t),
                                   nv, _p(tables.tiles_t), tables.ntiles, _p(work), _p(frame_index), tables.frame_cap,
                                   _p(frame_offsets), _p(runs), tables.run_cap, _p(run_offsets), _p(totals), _stream()),
          "avsr_summary_index")
    return SummaryIndex(tables, frame_index, frame_offsets, runs, run_offsets, totals)


def _index_arg(index, count, what, dev):
    """(device index or None, count) of a gathered pixel call: ``index`` a SummaryIndex (its list, its capacity), an
    int64 device vector, or None."""
    if isinstance(index, SummaryIndex):
        index = index.frame_index
    if index is not None:
        _device_arg(index, "index", what, (torch.int64,), ndim=1, device=dev)
    return index, (None if count is None else int(count))


def bgr_to_yuv(frames, out, index=None, count=None, matrix="bt601"):
    """YUV 4:2:0 of (gathered) BGR frames, written where an encoder reads it: frame i < count of ``out`` (a YuvFrames over
    the caller's tensor, of any layout it describes, 8-bit or 10-bit) is frames[index[i]] converted by the forward
    definition of include/avsum_render.h (frame i without an index; count defaults to every entry of the index, or every
    frame).  An index outside the frames is skipped, and bytes of ``out`` that belong to no sample are left as they
    were.  ``matrix``: a name of FORWARD_MATRICES or ten integers.  Returns ``out``.  = bgr_to_frames_host."""
    _device_arg(frames, "frames", "bgr_to_yuv", (torch.uint8,), shape=(None, None, None, 3))
    dev = frames.device
    if not isinstance(out, YuvFrames):
        raise ValueError("bgr_to_yuv: out must be a yuv.YuvFrames describing the destination")
    _device_arg(out.data, "out.data", "bgr_to_yuv", (torch.uint8,), device=dev)
    if (out.height, out.width) != tuple(frames.shape[1:3]):
        raise ValueError(f"bgr_to_yuv: frames of {frames.shape[1]}x{frames.shape[2]}, out of {out.height}x{out.width}")
    index, count = _index_arg(index, count, "bgr_to_yuv", dev)
    limit = frames.shape[0] if index is None else index.numel()
    count = limit if count is None else count
    if not 0 <= count <= min(limit, out.frames):
        raise ValueError(f"bgr_to_yuv: count {count} outside 0 .. {min(limit, out.frames)} (the index, the frames of out)")
    forward = (ctypes.c_int * FORWARD_INTS)(*_forward(matrix, "bgr_to_yuv"))
    check(lib().avsr_bgr_to_yuv_u8(_p(frames), frames.shape[0], _p(out.data), _surface_arg(out), forward, _p(index), count,
                                   _stream()), "avsr_bgr_to_yuv_u8")
    return out


def repack(frames, out, index=None, count=None):
    """The samples of (gathered) YUV 4:2:0 frames in another layout of the SAME depth - a software decoder's I420 to the
    NV12 a hardware encoder takes: frame i < count of ``out`` (a YuvFrames over the caller's tensor) holds the samples of
    frames[index[i]].  A differing depth is refused with a ValueError: it would need tone mapping to mean anything.
    Returns ``out``.  = repack_host."""
    frames = _as_yuv(frames, "repack")
    _device_arg(frames.data, "frames.data", "repack", (torch.uint8,))
    dev = frames.device
    if not isinstance(out, YuvFrames):
        raise ValueError("repack: out must be a yuv.YuvFrames describing the destination")
    _device_arg(out.data, "out.data", "repack", (torch.uint8,), device=dev)
    if out.depth != frames.depth:
        raise ValueError(f"repack: the source is {frames.depth}-bit, the destination {out.depth}-bit: a repack copies "
                         "samples (changing the depth needs tone mapping)")
    if (out.height, out.width) != (frames.height, frames.width):
        raise ValueError(f"repack: frames of {frames.height}x{frames.width}, out of {out.height}x{out.width}")
    index, count = _index_arg(index, count, "repack", dev)
    limit = frames.frames if index is None else index.numel()
    count = limit if count is None else count
    if not 0 <= count <= min(limit, out.frames):
        raise ValueError(f"repack: count {count} outside 0 .. {min(limit, out.frames)} (the index, the frames of out)")
    check(lib().avsr_repack_u8(_p(frames.data), _surface_arg(frames), _p(out.data), _surface_arg(out), _p(index), count,
                               _stream()), "avsr_repack_u8")
    return out


def summary_frames(frames, index, out=None, matrix="bt601"):
    """The frames of a summary, gathered by ``index`` (a SummaryIndex) at its capacity - no host count sizes a launch; the
    -1 entries past the true count are skipped by every route.  ``frames``: a uint8 BGR device tensor [N, h, w, 3], an
    ingest.Nv12Frames or a yuv.YuvFrames of the N frames of the index's plan.  ``out``: None (the source's own format,
    frame_cap frames, zeros past the count), "bgr", or a YuvFrames over a caller's tensor of at least frame_cap frames
    describing the destination layout.  Routes: BGR -> BGR and YUV -> the same description are ops.gather_rows on the
    rows; YUV -> BGR is yuv.yuv_to_bgr gathered (``matrix`` then names one of ingest.MATRICES); BGR -> YUV is bgr_to_yuv
    (``matrix`` one of FORWARD_MATRICES); YUV -> another layout of the same depth is repack.  Returns the BGR tensor or
    the destination YuvFrames."""
    if not isinstance(index, SummaryIndex):
        raise ValueError("summary_frames: index must be a render.SummaryIndex")
    plan, cap = index.plan, index.plan.frame_cap
    if isinstance(out, str) and out != "bgr":
        raise ValueError(f"summary_frames: out is None, 'bgr' or a YuvFrames, got '{out}'")
    if isinstance(out, YuvFrames) and out.frames < cap:
        raise ValueError(f"summary_frames: out holds {out.frames} frames, the capacity is {cap}")
    if isinstance(frames, torch.Tensor):
        _device_arg(frames, "frames", "summary_frames", (torch.uint8,), shape=(plan.frames, None, None, 3), device=plan.device)
        if out is None or isinstance(out, str):
            return gather_rows(frames, index.frame_index, index.count,
                               torch.zeros((cap,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=frames.device))
        return bgr_to_yuv(frames, out, index, cap, matrix)
    src = _as_yuv(frames, "summary_frames")
    _device_arg(src.data, "frames.data", "summary_frames", (torch.uint8,), device=plan.device)
    if src.frames != plan.frames:
        raise ValueError(f"summary_frames: {src.frames} frames, the index was made for {plan.frames}")
    if isinstance(out, str):
        bgr = torch.zeros((cap, src.height, src.width, 3), dtype=torch.uint8, device=src.device)
        return _yuv.yuv_to_bgr(src, index.frame_index, cap, matrix, out=bgr)
    if out is None:
        out = src.like(torch.zeros((cap,) + tuple(src.data.shape[1:]), dtype=torch.uint8, device=src.device))
    if _layout(out) == _layout(src):
        rows = out.data.view(out.frames, out.frame_stride)[:cap]
        gather_rows(src.data.view(src.frames, src.frame_stride), index.frame_index, index.count, rows)
        return out
    return repack(src, out, index, cap)


def _audio_cut(wave, index, plan, fade, out):
    _device_arg(wave, "wave", "summary_audio", (torch.float32,), ndim=1, numel=plan.samples, device=plan.device)
    if int(fade) < 0:
        raise ValueError(f"summary_audio: fade must be >= 0, got {fade}")
    if out is None:
        out = torch.zeros(plan.sample_cap, dtype=torch.float32, device=plan.device)
    else:
        _device_arg(out, "out", "summary_audio", (torch.float32,), ndim=1, device=plan.device)
        if out.numel() < 1:
            raise ValueError("summary_audio: out is empty")
    nv = plan.nvideos
    small = torch.empty(nv + 1 + AUDIO_COLS * plan.run_cap, dtype=torch.int64, device=plan.device)
    check(lib().avsr_audio_cut(_p(wave), plan.wave_offsets.ctypes.data_as(ctypes.c_void_p), _p(plan.wave_offsets_t), nv,
                               _p(plan.fps_t), plan.sr, int(fade), _p(index.runs), plan.run_cap, _p(index.run_offsets),
                               _p(small[nv + 1:]), _p(out), out.numel(), _p(small[:nv + 1]), _p(index.totals), _stream()),
          "avsr_audio_cut")
    return out, small[:nv + 1]


def summary_audio(wave, wave_offsets, index, fps, sr=16000, fade=0, out=None):
    """The audio of a summary: for every run (s, e) of ``index`` (a SummaryIndex) the samples a .. b of its video's track,
    a = min(int64(floor(float64(s) / fps_v * float64(sr))), len_v) and b likewise from e - process_decoded's arithmetic,
    in fp64 on the device -, run after run.  ``wave``: fp32 device [S], the tracks concatenated; ``wave_offsets``: host
    [V + 1]; ``fps``: one number or one per video (float64 on the host, uploaded with the plan).  ``fade`` > 0 ramps the
    first and last min(fade, L // 2) samples of every run linearly (one fp32 division and one fp32 multiplication per
    sample; 0: a pure copy).  Returns (audio fp32 [sample_cap] - ``out`` where given, zeros past the count otherwise -,
    audio_offsets int64 [V + 1] on the device) and fills the third column of index.totals.  = summary_audio_host."""
    if not isinstance(index, SummaryIndex):
        raise ValueError("summary_audio: index must be a render.SummaryIndex")
    base = index.plan
    plan = RenderTables(base.offsets, base.frame_cap, base.run_cap, None if base.bare else base.capacity, wave_offsets, fps,
                        sr, device=base.device)
    return _audio_cut(wave, index, plan, fade, out)


# --------------------------------------------------------------------------- the definitions, in numpy
def summary_index_host(mask, offsets, frame_cap=None, run_cap=None):
    """The tables of summary_index for a numpy mask [N] and host offsets [V + 1], each at its capacity (None: as large as
    needed): {"frame_index" (-1 past the count), "frame_offsets", "runs" ((-1, -1) past the count), "run_offsets",
    "totals" int64 [V, 3], "per_video": the runs of every video as a list of tuples}."""
    mask, offsets = np.asarray(mask) != 0, np.asarray(offsets, dtype=np.int64)
    nv = offsets.size - 1
    picked, runs, per_video = np.flatnonzero(mask), [], []
    for v in range(nv):
        m = np.concatenate([[False], mask[offsets[v]:offsets[v + 1]], [False]]).astype(np.int8)
        edge = np.diff(m)                                   # +1 where a run starts, -1 one past where it ends
        mine = list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))
        per_video.append(mine)
        runs += mine
    frame_cap = max(picked.size, 1) if frame_cap is None else int(frame_cap)
    run_cap = max(len(runs), 1) if run_cap is None else int(run_cap)
    frame_index = np.full(frame_cap, -1, dtype=np.int64)
    frame_index[:min(picked.size, frame_cap)] = picked[:frame_cap]
    run_table = np.full((run_cap, 2), -1, dtype=np.int64)
    run_table[:min(len(runs), run_cap)] = np.array(runs, dtype=np.int64).reshape(-1, 2)[:run_cap]
    totals = np.zeros((nv, TOTAL_COLS), dtype=np.int64)
    totals[:, 0] = [len(r) for r in per_video]
    totals[:, 1] = [int(mask[offsets[v]:offsets[v + 1]].sum()) for v in range(nv)]
    return {"frame_index": frame_index, "frame_offsets": np.concatenate([[0], np.cumsum(totals[:, 1])]), "runs": run_table,
            "run_offsets": np.concatenate([[0], np.cumsum(totals[:, 0])]), "totals": totals, "per_video": per_video}


def bgr_to_yuv_host(bgr, matrix="bt601", depth=8):
    """(Y int64 [..., h, w], U, V int64 [..., h / 2, w / 2]) of a uint8 BGR array [..., h, w, 3] (h, w even): the forward
    definition of include/avsum_render.h in 64-bit integers (numpy's >> on int64 is the arithmetic shift)."""
    if depth not in (8, 10):
        raise ValueError(f"bgr_to_yuv_host: depth is 8 or 10, got {depth}")
    k, top = depth - 8, (1 << depth) - 1
    y_off, yb, yg, yr, ub, ug, ur, vb, vg, vr = (np.int64(c) for c in _forward(matrix, "bgr_to_yuv_host"))
    bgr = np.asarray(bgr).astype(np.int64)
    h, w = bgr.shape[-3:-1]
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    y = np.clip(((yb * b + yg * g + yr * r + (1 << (SHIFT - 1 - k))) >> (SHIFT - k)) + (y_off << k), 0, top)
    sb, sg, sr = (c.reshape(c.shape[:-2] + (h // 2, 2, w // 2, 2)).sum(axis=(-3, -1)) for c in (b, g, r))
    u = np.clip(((ub * sb + ug * sg + ur * sr + (1 << (SHIFT + 1 - k))) >> (SHIFT + 2 - k)) + (128 << k), 0, top)
    v = np.clip(((vb * sb + vg * sg + vr * sr + (1 << (SHIFT + 1 - k))) >> (SHIFT + 2 - k)) + (128 << k), 0, top)
    return y, u, v


def store_samples_host(into, dst, rows, y, u, v):
    """Writes the sample planes y [R, h, w], u, v [R, h / 2, w / 2] into frames ``rows`` of the numpy byte buffer ``into``
    [frames, frame_stride] as ``dst`` (a YuvFrames, of any tensor) lays them out: a one-byte sample as the byte, a two-byte
    sample as the little-endian word sample << shift.  No other byte is touched."""
    yy, xx = np.arange(dst.height)[:, None], np.arange(dst.width)[None, :]
    cy, cx = np.arange(dst.height // 2)[:, None], np.arange(dst.width // 2)[None, :]
    chroma = cy * dst.pitch_c + cx * dst.chroma_step
    rows = np.asarray(rows, dtype=np.int64)
    for at, plane in ((yy * dst.pitch_y + xx * dst.sample_bytes, y), (dst.u_offset + chroma, u), (dst.v_offset + chroma, v)):
        plane = np.asarray(plane).astype(np.int64)
        if dst.sample_bytes == 1:
            into[rows[:, None, None], at[None]] = plane
        else:
            word = plane << dst.shift
            into[rows[:, None, None], at[None]] = word & 255
            into[rows[:, None, None], at[None] + 1] = word >> 8
    return into


def _rows_of(index, count, source_frames):
    """(destination rows, source frames) of a gathered call: the entries of the index inside the source."""
    index = np.arange(count) if index is None else np.asarray(index, dtype=np.int64)[:count]
    keep = (index >= 0) & (index < source_frames)
    return np.flatnonzero(keep), index[keep]


def bgr_to_frames_host(bgr, dst, matrix="bt601", index=None, count=None, into=None):
    """uint8 [dst.frames, frame_stride]: what bgr_to_yuv leaves in a destination that held ``into`` (zeros when None)."""
    bgr = np.asarray(bgr)
    into = np.zeros((dst.frames, dst.frame_stride), dtype=np.uint8) if into is None else np.array(into, dtype=np.uint8)
    count = (bgr.shape[0] if index is None else len(index)) if count is None else int(count)
    rows, source = _rows_of(index, count, bgr.shape[0])
    if rows.size:
        store_samples_host(into.reshape(dst.frames, dst.frame_stride), dst, rows, *bgr_to_yuv_host(bgr[source], matrix, dst.depth))
    return into


def repack_host(data, src, dst, index=None, count=None, into=None):
    """uint8 [dst.frames, frame_stride]: what repack leaves in a destination that held ``into`` (zeros when None), from
    the numpy bytes ``data`` that ``src`` describes."""
    if src.depth != dst.depth:
        raise ValueError("repack_host: a repack copies samples: the depths must agree")
    into = np.zeros((dst.frames, dst.frame_stride), dtype=np.uint8) if into is None else np.array(into, dtype=np.uint8)
    count = (src.frames if index is None else len(index)) if count is None else int(count)
    rows, source = _rows_of(index, count, src.frames)
    if rows.size:
        y, u, v = _yuv.yuv_samples_host(data, src)
        store_samples_host(into.reshape(dst.frames, dst.frame_stride), dst, rows, y[source], u[source, ::2, ::2], v[source, ::2, ::2])
    return into


def audio_bounds_host(frame, fps, sr, length):
    """min(int64(floor(float64(frame) / fps * float64(sr))), length): the sample a frame boundary falls on."""
    return min(int(np.floor(np.float64(frame) / np.float64(fps) * np.float64(sr))), int(length))


def summary_audio_host(wave, wave_offsets, runs_per_video, fps, sr=16000, fade=0):
    """(audio float32 [samples], audio_offsets int64 [V + 1]) of a numpy waveform: the definition of summary_audio, the
    fade in float32 (one division, one multiplication)."""
    wave, wave_offsets = np.asarray(wave, dtype=np.float32), np.asarray(wave_offsets, dtype=np.int64)
    nv = wave_offsets.size - 1
    fps = np.asarray(fps, dtype=np.float64).reshape(-1)
    fps = np.repeat(fps, nv) if fps.size == 1 else fps
    pieces, counts = [], []
    for v in range(nv):
        track, n = wave[wave_offsets[v]:wave_offsets[v + 1]], 0
        for s, e in runs_per_video[v]:
            a, b = audio_bounds_host(s, fps[v], sr, track.size), audio_bounds_host(e, fps[v], sr, track.size)
            piece, length = track[a:b].copy(), b - a
            f = min(int(fade), length // 2)
            if f:
                i = np.arange(length)
                up = (i + 1).astype(np.float32) / np.float32(f + 1)
                down = (length - i).astype(np.float32) / np.float32(f + 1)
                piece[:f] = piece[:f] * up[:f]
                piece[length - f:] = piece[length - f:] * down[length - f:]
            pieces.append(piece)
            n += length
        counts.append(n)
    audio = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.float32)
    return audio.astype(np.float32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
