"""Planar, semi-planar and 10-bit YUV 4:2:0 frames read where they lie: the launch wrappers of libavsum_yuv.so
(include/avsum_yuv.h) and the numpy restatements of its pixel definition.

ingest.Nv12Frames covers what a hardware decoder writes for 8-bit video.  A software decode (ffmpeg, PyAV, decord)
hands over I420 / YV12 - three planes -, a hardware decoder writes P010 for 10-bit HEVC / AV1 - 16-bit words, the sample
in the top ten bits - and a software decoder yuv420p10le - the sample in the low ten bits.  ``YuvFrames`` describes a batch
of any of them in ONE device tensor by the eleven integers of the header; ``yuv_to_bgr`` (the definition),
``yuv_resize_gather`` (the bytes of ops.resize_gather on the converted frames) and ``yuv_hsv_frame_diff_batch`` (the
integers of ops.hsv_frame_diff_batch on the converted frames) take the arguments of their ingest.nv12_* counterparts and
read the surfaces without a dense BGR copy.  The output is uint8 BGR: a 10-bit sample's two extra bits enter the matrix
and the one rounding to a grey level instead of being dropped first.  Host tensors are refused: there is no CPU
fallback.  ``yuv_samples_host`` / ``yuv_to_bgr_host`` / ``yuv_to_bgr_f64`` are the sample addressing, the integer
definition (in int64) and the float formula it approximates, in numpy, for tests and studies.
"""
import ctypes

import numpy as np
import torch

from ._yuv_abi import MATRIX_INTS, MAX_COEF, SHIFT, SURFACE_FIELDS, SURFACE_INTS, check, lib
from .ingest import MATRICES, MATRICES_F64, Nv12Frames, _matrix, _matrix_arg
from .ops import ShotTables, _device_arg, _p, _stream, _tables_arg

__all__ = ["YuvFrames", "MATRICES", "MATRICES_F64", "yuv_to_bgr", "yuv_resize_gather", "yuv_hsv_frame_diff_batch",
           "yuv_resize_band", "yuv_samples_host", "yuv_to_bgr_host", "yuv_to_bgr_f64", "frames_to_bgr_host",
           "frames_to_bgr_f64"]

assert (SHIFT, MAX_COEF, MATRIX_INTS) == (20, 1 << 22, 6)      # the limits ingest._matrix enforces are this header's too


def _planes_meet(delta, pitch, step, sb, ch, cw):
    """avsy_chroma_planes_meet (yuv.hip): do two chroma planes of one pitch and step, ``delta`` bytes apart, share a byte?"""
    delta = abs(delta)
    for dr in (delta // pitch, delta // pitch + 1):
        if dr > ch - 1:
            continue
        rest = delta - dr * pitch
        for dc in (rest // step, rest // step + 1):
            if -(cw - 1) <= dc <= cw - 1 and -sb < rest - dc * step < sb:
                return True
    return False


def _meets_luma(off, pitch_y, pitch_c, step, sb, h, w):
    """avsy_chroma_meets_luma (yuv.hip): does a sample of the chroma plane at ``off`` share a byte with a luma sample?"""
    ch, cw, luma_end = h // 2, w // 2, (h - 1) * pitch_y + w * sb
    if off >= luma_end:
        return False
    for r in range(ch):
        a = off + r * pitch_c
        b = a + (cw - 1) * step + sb
        if a >= luma_end:
            break
        y = a // pitch_y
        while y < h and y * pitch_y < b:
            ya = y * pitch_y
            c = 0 if ya - sb - a < 0 else (ya - sb - a) // step + 1
            if c < cw and a + c * step < ya + w * sb:
                return True
            y += 1
    return False


class YuvFrames:
    """N YUV 4:2:0 surfaces of ``height`` x ``width`` pixels in one uint8 tensor ``data`` [N, frame_bytes] or
    [N, rows, pitch] (only its first extent and the bytes per frame matter), described by the fields of
    include/avsum_yuv.h: ``sample_bytes`` (1, or 2 for ten bits in a little-endian 16-bit word), ``shift`` (0, or 6 where
    the sample is in the word's top bits), ``pitch_y``, ``pitch_c``, ``chroma_step`` (bytes from one U sample to the next),
    ``u_offset`` and ``v_offset`` (bytes from the frame's first byte).  The constructors ``i420``, ``yv12``, ``i010``,
    ``nv12``, ``nv21``, ``p010`` and ``from_nv12`` fill them for the layouts decoders deliver.  What belongs to no sample
    (pitch padding, gaps between planes, spare rows; the other six bits of a 16-bit word) is never looked at.  Only the
    tensor's metadata is looked at here, so a description can be validated for a host or meta tensor; the launch wrappers
    insist on a device tensor."""

    def __init__(self, data, height, width, sample_bytes=1, shift=0, pitch_y=None, pitch_c=None, chroma_step=None,
                 u_offset=None, v_offset=None):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() not in (2, 3):
            raise ValueError("YuvFrames: data must be a uint8 tensor [N, frame_bytes] or [N, rows, pitch]")
        if not data.is_contiguous():
            raise ValueError(f"YuvFrames: data must be contiguous, got strides {list(data.stride())}")
        h, w, sb, shift = int(height), int(width), int(sample_bytes), int(shift)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"YuvFrames: height and width must be even and at least 2, got {h}x{w}")
        if sb not in (1, 2) or shift not in (0, 6) or (sb == 1 and shift):
            raise ValueError(f"YuvFrames: sample_bytes is 1 or 2 and shift 0 or 6 (0 for one-byte samples), got "
                             f"{sb} and {shift}")
        if pitch_y is None:
            pitch_y = data.shape[2] if data.dim() == 3 else w * sb
        missing = [k for k, v in (("pitch_c", pitch_c), ("chroma_step", chroma_step), ("u_offset", u_offset),
                                  ("v_offset", v_offset)) if v is None]
        if missing:
            raise ValueError(f"YuvFrames: {', '.join(missing)} must be given (or use one of the layout constructors)")
        pitch_y, pitch_c, step, u_off, v_off = int(pitch_y), int(pitch_c), int(chroma_step), int(u_offset), int(v_offset)
        stride = int(np.prod(data.shape[1:], dtype=np.int64))
        ch, cw = h // 2, w // 2
        if pitch_y < w * sb:
            raise ValueError(f"YuvFrames: pitch_y {pitch_y} below the {w * sb} bytes of a luma row")
        if step < sb:
            raise ValueError(f"YuvFrames: chroma_step {step} below the {sb} bytes of a sample")
        crow = (cw - 1) * step + sb
        if pitch_c < crow:
            raise ValueError(f"YuvFrames: pitch_c {pitch_c} below the {crow} bytes of a chroma row")
        if u_off < 0 or v_off < 0:
            raise ValueError(f"YuvFrames: negative plane offset (u_offset {u_off}, v_offset {v_off})")
        ends = {"luma": (h - 1) * pitch_y + w * sb, "U": u_off + (ch - 1) * pitch_c + crow,
                "V": v_off + (ch - 1) * pitch_c + crow}
        for plane, end in ends.items():
            if end > stride:
                raise ValueError(f"YuvFrames: the {plane} plane ends at byte {end}, a frame has {stride} bytes")
        if sb == 2 and (pitch_y | pitch_c | step | u_off | v_off | stride | data.storage_offset()) % 2:
            raise ValueError("YuvFrames: two-byte samples need an even base, pitch_y, pitch_c, chroma_step, u_offset, "
                             "v_offset and frame stride")
        if _planes_meet(v_off - u_off, pitch_c, step, sb, ch, cw):
            raise ValueError(f"YuvFrames: the U and V planes overlap (u_offset {u_off}, v_offset {v_off})")
        if _meets_luma(u_off, pitch_y, pitch_c, step, sb, h, w) or _meets_luma(v_off, pitch_y, pitch_c, step, sb, h, w):
            raise ValueError(f"YuvFrames: a chroma plane overlaps the luma plane (u_offset {u_off}, v_offset {v_off}, "
                             f"luma ends at {ends['luma']})")
        self.data, self.frames, self.height, self.width = data, int(data.shape[0]), h, w
        self.sample_bytes, self.shift, self.depth = sb, shift, 8 if sb == 1 else 10
        self.pitch_y, self.pitch_c, self.chroma_step = pitch_y, pitch_c, step
        self.u_offset, self.v_offset, self.frame_stride = u_off, v_off, stride

    # ------------------------------------------------------------------ the layouts decoders deliver
    @staticmethod
    def _pitch(data, default):
        return int(data.shape[2]) if isinstance(data, torch.Tensor) and data.dim() == 3 else default

    @classmethod
    def _planar(cls, data, h, w, sb, pitch_y, pitch_c, u_offset, v_offset, u_first):
        h, w = int(h), int(w)
        pitch_y = cls._pitch(data, w * sb) if pitch_y is None else int(pitch_y)
        if pitch_c is None:
            if pitch_y % (2 * sb):
                raise ValueError(f"YuvFrames: pitch_c must be given where pitch_y ({pitch_y}) has no half")
            pitch_c = pitch_y // 2
        first, second = h * pitch_y, h * pitch_y + (h // 2) * int(pitch_c)
        if u_offset is None:
            u_offset = first if u_first else second
        if v_offset is None:
            v_offset = second if u_first else first
        return cls(data, h, w, sb, 0, pitch_y, pitch_c, sb, u_offset, v_offset)

    @classmethod
    def i420(cls, data, h, w, pitch_y=None, pitch_c=None, u_offset=None, v_offset=None):
        """yuv420p: the luma plane, then a U plane and a V plane of h / 2 rows of w / 2 bytes.  pitch_c defaults to half of
        pitch_y, the planes to lying back to back."""
        return cls._planar(data, h, w, 1, pitch_y, pitch_c, u_offset, v_offset, True)

    @classmethod
    def yv12(cls, data, h, w, pitch_y=None, pitch_c=None, u_offset=None, v_offset=None):
        """I420 with the V plane before the U plane."""
        return cls._planar(data, h, w, 1, pitch_y, pitch_c, u_offset, v_offset, False)

    @classmethod
    def i010(cls, data, h, w, pitch_y=None, pitch_c=None, u_offset=None, v_offset=None):
        """yuv420p10le: I420 of little-endian 16-bit words, the sample in the low ten bits.  Pitches and offsets in bytes."""
        return cls._planar(data, h, w, 2, pitch_y, pitch_c, u_offset, v_offset, True)

    @classmethod
    def _semi(cls, data, h, w, sb, shift, pitch, uv_offset, u_first):
        h, w = int(h), int(w)
        pitch = cls._pitch(data, w * sb) if pitch is None else int(pitch)
        uv_offset = h * pitch if uv_offset is None else int(uv_offset)
        u, v = (uv_offset, uv_offset + sb) if u_first else (uv_offset + sb, uv_offset)
        return cls(data, h, w, sb, shift, pitch, pitch, 2 * sb, u, v)

    @classmethod
    def nv12(cls, data, h, w, pitch=None, uv_offset=None):
        """The luma plane, then one plane of (U, V) byte pairs of the same pitch, at ``uv_offset`` (default h * pitch)."""
        return cls._semi(data, h, w, 1, 0, pitch, uv_offset, True)

    @classmethod
    def nv21(cls, data, h, w, pitch=None, uv_offset=None):
        """NV12 with (V, U) pairs."""
        return cls._semi(data, h, w, 1, 0, pitch, uv_offset, False)

    @classmethod
    def p010(cls, data, h, w, pitch=None, uv_offset=None):
        """NV12 of little-endian 16-bit words with the sample in the top ten bits.  pitch and uv_offset in bytes."""
        return cls._semi(data, h, w, 2, 6, pitch, uv_offset, True)

    @classmethod
    def from_nv12(cls, frames):
        """The same surfaces as an ingest.Nv12Frames (no copy): converts to the bytes of ingest.nv12_to_bgr."""
        if not isinstance(frames, Nv12Frames):
            raise ValueError("YuvFrames.from_nv12: frames must be an ingest.Nv12Frames")
        return cls.nv12(frames.data, frames.height, frames.width, frames.pitch, frames.uv_offset)

    # ------------------------------------------------------------------
    @property
    def device(self):
        return self.data.device

    @property
    def nbytes(self):
        return self.frames * self.frame_stride

    @property
    def shape(self):
        """The shape of the BGR tensor these frames stand for."""
        return (self.frames, self.height, self.width, 3)

    @property
    def planar(self):
        """U and V in planes of their own (False: V one sample beside U) - the form the kernels are compiled for."""
        return not (self.chroma_step == 2 * self.sample_bytes and abs(self.v_offset - self.u_offset) == self.sample_bytes)

    def like(self, data):
        """The same description over another tensor of data's shape (a host copy, a device upload)."""
        return YuvFrames(data, self.height, self.width, self.sample_bytes, self.shift, self.pitch_y, self.pitch_c,
                         self.chroma_step, self.u_offset, self.v_offset)

    def pinned_like(self):
        """An uninitialised pinned host tensor of data's shape: fill it with decoded surfaces, then
        ``ops.pull_copy(pinned, frames.data)`` uploads them - 1.5 (8-bit) or 3 (10-bit) bytes per pixel, no conversion on
        the host."""
        return torch.empty(self.data.shape, dtype=torch.uint8, pin_memory=True)

    def surface(self):
        """The eleven integers of h_surface, in the header's order."""
        return tuple({"n": self.frames, "h": self.height, "w": self.width}.get(f, getattr(self, f, None))
                     for f in SURFACE_FIELDS)

    def _args(self):
        return (_p(self.data), (ctypes.c_int64 * SURFACE_INTS)(*self.surface()))


def _frames_arg(frames, what, device=None):
    if not isinstance(frames, YuvFrames):
        raise ValueError(f"{what}: frames must be a YuvFrames")
    _device_arg(frames.data, "frames.data", what, (torch.uint8,), device=device)
    return frames


# --------------------------------------------------------------------------- launch wrappers
def yuv_to_bgr(frames, index=None, count=None, matrix="bt601", out=None):
    """uint8 [count, h, w, 3] BGR: row i is frame index[i] of ``frames`` converted (frame i without an index; count
    defaults to every entry of the index, or every frame).  ``index`` int64 device vector of at least ``count`` entries;
    ``count`` a host integer; ``out`` [at least count, h, w, 3] (allocated when None): its rows from ``count`` on and the
    row of an index outside the frames are left as they were.  The integer definition of include/avsum_yuv.h =
    frames_to_bgr_host."""
    _frames_arg(frames, "yuv_to_bgr")
    dev = frames.device
    if index is not None:
        _device_arg(index, "index", "yuv_to_bgr", (torch.int64,), ndim=1, device=dev)
    limit = frames.frames if index is None else index.numel()
    count = limit if count is None else int(count)
    if not 0 <= count <= limit:
        raise ValueError(f"yuv_to_bgr: count {count} outside 0 .. {limit}")
    if out is None:
        out = torch.empty((count, frames.height, frames.width, 3), dtype=torch.uint8, device=dev)
    else:
        _device_arg(out, "out", "yuv_to_bgr", (torch.uint8,), shape=(None, frames.height, frames.width, 3), device=dev)
        if out.shape[0] < count:
            raise ValueError(f"yuv_to_bgr: out holds {out.shape[0]} frames, count is {count}")
    check(lib().avsy_to_bgr_u8(*frames._args(), _matrix_arg(matrix, "yuv_to_bgr"), _p(index), count, _p(out), _stream()),
          "avsy_to_bgr_u8")
    return out


def yuv_resize_gather(frames, index, count, sizes, matrix="bt601", outs=None):
    """ops.resize_gather(yuv_to_bgr(frames), index, count, sizes) byte for byte, in ONE launch and without the BGR
    frames: a workgroup stages the luma and chroma rows its output rows read and converts per tap.  ``sizes``: one or
    two (dh, dw).  Returns a list of uint8 [count, dh, dw, 3] tensors, ``outs`` where given.  Raises (status
    AVSY_E_UNSUPPORTED) where the rows of one output row do not fit the kernel's LDS: see yuv_resize_band."""
    _frames_arg(frames, "yuv_resize_gather")
    dev = frames.device
    _device_arg(index, "index", "yuv_resize_gather", (torch.int64,), ndim=1, device=dev)
    count = int(count)
    if not 0 <= count <= index.numel():
        raise ValueError(f"yuv_resize_gather: count {count} outside 0 .. {index.numel()}, the entries of index")
    sizes = [(int(dh), int(dw)) for dh, dw in sizes]
    if len(sizes) not in (1, 2) or any(dh < 1 or dw < 1 for dh, dw in sizes):
        raise ValueError(f"yuv_resize_gather: sizes must be one or two (dh, dw) of positive extents, got {sizes}")
    if outs is None:
        outs = [torch.empty((count, dh, dw, 3), dtype=torch.uint8, device=dev) for dh, dw in sizes]
    elif len(outs) != len(sizes):
        raise ValueError(f"yuv_resize_gather: {len(outs)} outs for {len(sizes)} sizes")
    for k, ((dh, dw), out) in enumerate(zip(sizes, outs)):
        _device_arg(out, f"outs[{k}]", "yuv_resize_gather", (torch.uint8,), shape=(count, dh, dw, 3), device=dev)
    (dh0, dw0), (dh1, dw1) = sizes[0], sizes[1] if len(sizes) == 2 else (0, 0)
    check(lib().avsy_resize_gather2_u8(*frames._args(), _matrix_arg(matrix, "yuv_resize_gather"), _p(index), count,
                                       _p(outs[0]), dh0, dw0, _p(outs[1]) if len(sizes) == 2 else None, dh1, dw1,
                                       _stream()), "avsy_resize_gather2_u8")
    return list(outs)


def yuv_resize_band(frames, dh, dw):
    """The output rows per workgroup (8, 4, 2 or 1) yuv_resize_gather takes for a destination of dh x dw, 0 where it
    refuses the shape.  Host only: ``frames`` may describe a host or meta tensor."""
    if not isinstance(frames, YuvFrames):
        raise ValueError("yuv_resize_band: frames must be a YuvFrames")
    band = lib().avsy_resize_band((ctypes.c_int64 * SURFACE_INTS)(*frames.surface()), int(dh), int(dw))
    check(min(band, 0), "avsy_resize_band")
    return band


def yuv_hsv_frame_diff_batch(frames, tables, step=1, raw=False, matrix="bt601"):
    """ops.hsv_frame_diff_batch(yuv_to_bgr(frames), tables, step, raw) integer for integer, without the BGR frames:
    ``frames`` the videos of ``tables`` (an ops.ShotTables) concatenated."""
    _tables_arg(tables, ShotTables, "yuv_hsv_frame_diff_batch")
    _frames_arg(frames, "yuv_hsv_frame_diff_batch", tables.device)
    if frames.frames != tables.frames:
        raise ValueError(f"yuv_hsv_frame_diff_batch: {frames.frames} frames, the tables hold {tables.frames}")
    if int(step) < 1:
        raise ValueError(f"yuv_hsv_frame_diff_batch: step must be >= 1, got {step}")
    sums = torch.empty((frames.frames, 3), dtype=torch.int32, device=frames.device)
    check(lib().avsy_hsv_diff_batch_u8(*frames._args(), _matrix_arg(matrix, "yuv_hsv_frame_diff_batch"), int(step),
                                       _p(tables.offsets_t), tables.nvideos, _p(sums), _stream()),
          "avsy_hsv_diff_batch_u8")
    return sums if raw else sums.to(torch.int64) & 0xFFFFFFFF


# --------------------------------------------------------------------------- the definition, in numpy
def yuv_samples_host(data, frames):
    """(Y, U, V), each int32 [N, h, w]: the samples of every pixel (the nearest chroma sample, no interpolation) of a numpy
    uint8 array holding the bytes ``frames`` (a YuvFrames, of any tensor) describes."""
    flat = np.asarray(data).reshape(frames.frames, frames.frame_stride)
    sb = frames.sample_bytes

    def sample(at):
        if sb == 1:
            return flat[:, at].astype(np.int32)
        word = flat[:, at].astype(np.int32) | (flat[:, at + 1].astype(np.int32) << 8)
        return (word >> frames.shift) & 1023

    y, x = np.arange(frames.height)[:, None], np.arange(frames.width)[None, :]
    chroma = (y >> 1) * frames.pitch_c + (x >> 1) * frames.chroma_step
    return sample(y * frames.pitch_y + x * sb), sample(frames.u_offset + chroma), sample(frames.v_offset + chroma)


def yuv_to_bgr_host(y, u, v, matrix="bt601", depth=8):
    """uint8 [..., 3] BGR of integer arrays Y, U, V (0 .. 2^depth - 1, one shape), depth 8 or 10: the definition of
    include/avsum_yuv.h in 64-bit integers (numpy's >> on int64 is the arithmetic shift)."""
    if depth not in (8, 10):
        raise ValueError(f"yuv_to_bgr_host: depth is 8 or 10, got {depth}")
    k = depth - 8
    y_off, cy, cub, cug, cvg, cvr = (np.int64(c) for c in _matrix(matrix, "yuv_to_bgr_host"))
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    yy = np.maximum(y - (y_off << k), 0) * cy + np.int64(1 << (SHIFT - 1 + k))
    uu, vv = u - np.int64(128 << k), v - np.int64(128 << k)
    out = np.empty(yy.shape + (3,), dtype=np.uint8)
    for c, total in enumerate((yy + cub * uu, yy + cvg * vv + cug * uu, yy + cvr * vv)):
        assert total.dtype == np.int64
        out[..., c] = np.clip(total >> (SHIFT + k), 0, 255)
    return out


def yuv_to_bgr_f64(y, u, v, matrix="bt601", depth=8):
    """float64 [..., 3] BGR by the three-decimal formula of MATRICES_F64[matrix] (or six numbers) on sample / 2^(depth - 8),
    clipped to 0 .. 255, not rounded: what the integers approximate."""
    y_off, cy, cub, cug, cvg, cvr = MATRICES_F64[matrix] if isinstance(matrix, str) else matrix
    scale = float(1 << (depth - 8))
    y, u, v = (np.asarray(a, dtype=np.float64) / scale for a in (y, u, v))
    yy, uu, vv = np.maximum(y - y_off, 0.0) * cy, u - 128.0, v - 128.0
    return np.clip(np.stack([yy + cub * uu, yy + cvg * vv + cug * uu, yy + cvr * vv], axis=-1), 0.0, 255.0)


def frames_to_bgr_host(data, frames, matrix="bt601"):
    """uint8 [N, h, w, 3]: yuv_to_bgr of the numpy bytes ``data`` that ``frames`` describes, by the integer definition."""
    return yuv_to_bgr_host(*yuv_samples_host(data, frames), matrix, frames.depth)


def frames_to_bgr_f64(data, frames, matrix="bt601"):
    """float64 [N, h, w, 3]: the float formula on the same pixels."""
    return yuv_to_bgr_f64(*yuv_samples_host(data, frames), matrix, frames.depth)
