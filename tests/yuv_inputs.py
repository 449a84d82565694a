"""Seeded YUV 4:2:0 cases, oracles and planted mistakes of the YUV ingest tests (libavsum_yuv.so, avsum_amd/yuv.py):
test_yuv_host.py on the host, test_gpu_yuv.py on the device.  numpy only; both build the same cases from here.

A case is a flat uint8 buffer [frames, frame_stride] and a ``Layout``: the eleven integers of include/avsum_yuv.h by name,
plus the format's name.  ``layout`` computes them for a format, extents, pitches (in SAMPLES, so one table serves one- and
two-byte formats), a gap between the planes and spare bytes after them; ``pack`` writes sample planes into a buffer
that holds SENTINEL_U8 in every byte no sample owns - the pitch padding, the gaps, the spare bytes - and seeded garbage in
the six bits of a 16-bit word that are not the sample (P010: the low six; planar 10-bit: the high six).

Oracles:
  * ``avsum_amd.yuv.frames_to_bgr_host`` - the int64 definition of include/avsum_yuv.h by fancy indexing;
  * ``restatement`` below - the same definition by BYTE ADDRESSES of the flat buffer, written separately so that a planted
    ``mistake`` can misaddress or misround the way a kernel would; without a mistake the host test holds the two equal;
  * ``avsum_amd.yuv.yuv_to_bgr_f64`` - the float formula, within BOUND_10 of the depth-10 integers (nv12_inputs.BOUND of
    the depth-8 ones, which are ingest's).
Everything past the conversion is equality with the BGR kernels on the converted frames: no bound of its own.

MISTAKES are the planted errors; NOTICED_BY names the committed conversion case (format, layout) at which each is noticed.
"""
import collections
import functools

import numpy as np

from nv12_inputs import (CUT_LENGTHS, EMBED_LENGTHS, EMBED_SHOTS, GATHER_INDEX, GATHER_SKIPPED,  # noqa: F401
                         band_rows, offsets_of, scene_cuts)
from pixel_f64_inputs import SENTINEL_U8, source_rows  # noqa: F401  (one restatement of cv_src_pos, shared)

BOUND_10 = 0.5 + 1983 * 2.0 ** -23  # |depth-10 integer definition - float formula|: the sums are in units of 2^-22 of a
#                                     grey level; three coefficients each within 1/2 of c * 2^20, times at most 959, 512 and
#                                     512 (|Y - 64|, |U - 512|, |V - 512| of ten-bit samples) = (959 + 512 + 512) / 2 units
#                                     = 1983 * 2^-23; + 1/2 of the one rounding to a grey level

Layout = collections.namedtuple(
    "Layout", "fmt n h w sample_bytes shift pitch_y pitch_c chroma_step u_offset v_offset frame_stride")

# format -> (sample_bytes, shift, interleaved chroma, U before V)
FORMAT_TABLE = {"i420": (1, 0, False, True), "yv12": (1, 0, False, False), "i010": (2, 0, False, True),
                "nv12": (1, 0, True, True), "nv21": (1, 0, True, False), "p010": (2, 6, True, True)}
FORMATS = ("i420", "yv12", "p010", "i010", "nv21")       # what the conversion layouts run for
ONE_BYTE = tuple(f for f in FORMATS if FORMAT_TABLE[f][0] == 1)


def depth_of(fmt):
    return 8 if FORMAT_TABLE[fmt][0] == 1 else 10


def layout(fmt, n, h, w, pitch_y=None, pitch_c=None, gap=0, spare=0):
    """The Layout of ``n`` frames of h x w in ``fmt``.  pitch_y, pitch_c, gap, spare are in SAMPLES (times sample_bytes =
    bytes); pitch_c counts the samples of one chroma row of the plane as stored: w / 2 for a planar format, w (the U, V
    pairs) for an interleaved one.  ``gap`` samples lie between consecutive planes, ``spare`` after the last."""
    sb, shift, interleaved, u_first = FORMAT_TABLE[fmt]
    pitch_y = (w if pitch_y is None else pitch_y) * sb
    first = h * pitch_y + gap * sb
    if interleaved:
        pitch_c = (w if pitch_c is None else pitch_c) * sb
        u, v = (first, first + sb) if u_first else (first + sb, first)
        step, end = 2 * sb, first + (h // 2) * pitch_c
    else:
        pitch_c = (w // 2 if pitch_c is None else pitch_c) * sb
        second = first + (h // 2) * pitch_c + gap * sb
        u, v = (first, second) if u_first else (second, first)
        step, end = sb, second + (h // 2) * pitch_c
    return Layout(fmt, n, h, w, sb, shift, pitch_y, pitch_c, step, u, v, end + spare * sb)


def fields(L):
    """The keyword arguments of avsum_amd.yuv.YuvFrames(data, L.h, L.w, **fields(L))."""
    return dict(sample_bytes=L.sample_bytes, shift=L.shift, pitch_y=L.pitch_y, pitch_c=L.pitch_c,
                chroma_step=L.chroma_step, u_offset=L.u_offset, v_offset=L.v_offset)


def surface_ints(L):
    """h_surface of L, in the header's order."""
    return [L.n, L.h, L.w, L.sample_bytes, L.shift, L.pitch_y, L.pitch_c, L.chroma_step, L.u_offset, L.v_offset,
            L.frame_stride]


def _addresses(L):
    """(luma [h, w], U [h/2, w/2], V [h/2, w/2]): the byte address of every sample within a frame."""
    y, x = np.arange(L.h)[:, None], np.arange(L.w)[None, :]
    cy, cx = np.arange(L.h // 2)[:, None], np.arange(L.w // 2)[None, :]
    chroma = cy * L.pitch_c + cx * L.chroma_step
    return y * L.pitch_y + x * L.sample_bytes, L.u_offset + chroma, L.v_offset + chroma


def sample_mask(L):
    """bool [frame_stride]: the bytes of a frame that belong to a sample."""
    mask = np.zeros(L.frame_stride, dtype=bool)
    for at in _addresses(L):
        for b in range(L.sample_bytes):
            assert not mask[at + b].any()             # (no two samples share a byte)
            mask[at + b] = True
    return mask


def pack(L, y, u, v, garbage_seed=0):
    """uint8 [n, frame_stride]: the sample planes y [n, h, w], u, v [n, h/2, w/2] (integers of the format's depth) laid
    out as L says; SENTINEL_U8 everywhere else; for two-byte formats the six other bits of every word hold seeded
    garbage (``garbage_seed`` None: zeros)."""
    data = np.full((L.n, L.frame_stride), SENTINEL_U8, dtype=np.uint8)
    rng = None if garbage_seed is None else np.random.default_rng(9000 + garbage_seed)
    for at, plane in zip(_addresses(L), (y, u, v)):
        plane = np.asarray(plane).astype(np.int64)
        assert plane.shape == (L.n,) + at.shape and plane.min() >= 0 and plane.max() < (1 << (8 if L.sample_bytes == 1 else 10))
        if L.sample_bytes == 1:
            data[:, at] = plane
            continue
        other = np.zeros(plane.shape, dtype=np.int64) if rng is None else rng.integers(0, 64, plane.shape)
        word = (plane << L.shift) | (other if L.shift else other << 10)
        data[:, at], data[:, at + 1] = word & 255, word >> 8
    return data


def surface(fmt, h, w, pitch_y=None, pitch_c=None, gap=0, spare=0, frames=3, seed=0, garbage_seed=0):
    """(data, Layout): seeded samples over the format's whole range."""
    L = layout(fmt, frames, h, w, pitch_y, pitch_c, gap, spare)
    rng = np.random.default_rng(8200 + 1000 * h + 10 * w + seed)
    top = 1 << depth_of(fmt)
    y = rng.integers(0, top, (frames, h, w))
    u, v = rng.integers(0, top, (2, frames, h // 2, w // 2))
    data = pack(L, y, u, v, garbage_seed)
    data.setflags(write=False)
    return data, L


# --------------------------------------------------------------------------- conversion cases
# name -> (h, w, pitch_y, planar pitch_c, interleaved pitch_c, gap, spare), pitches and gaps in samples (None: tight).
# "2x2": the smallest frame.  "6x10": pitch_y 16 and a pitch_c of 12 that is NOT half of it, gaps between the planes.
# "36x70": chroma rows of 35 samples - odd, so no vector load may assume a 2-, 4- or 16-byte row length - and several
# workgroups' worth of rows.  "8x16": a width of a multiple of 4 with every pitch and offset a multiple of four samples'
# bytes - where yuv_to_bgr_kernel loads a thread's samples of a plane at once (and, off its base alignment, must not)
LAYOUTS = {"2x2": (2, 2, None, None, None, 0, 0), "6x10": (6, 10, 16, 12, 12, 6, 4), "36x70": (36, 70, 80, 44, 76, 10, 8),
           "8x16": (8, 16, 24, 16, 24, 8, 8)}
LAYOUT_FRAMES = 3
GATHER_COUNT = len(GATHER_INDEX) - 1


def layout_args(fmt, name):
    h, w, pitch_y, pc_planar, pc_inter, gap, spare = LAYOUTS[name]
    return h, w, pitch_y, pc_inter if FORMAT_TABLE[fmt][2] else pc_planar, gap, spare


@functools.lru_cache(maxsize=None)
def layout_case(fmt, name, garbage_seed=0):
    return surface(fmt, *layout_args(fmt, name), frames=LAYOUT_FRAMES, garbage_seed=garbage_seed)


EXHAUSTIVE_LUMAS = (0, 1, 63, 64, 65, 255, 256, 511, 512, 513, 767, 939, 940, 941, 1022, 1023)


@functools.lru_cache(maxsize=None)
def exhaustive_case():
    """(data, Layout): 4 P010 frames of 2048 x 2048.  Chroma row r holds the pairs (U, V) = (r, c), c = 0 .. 1023 - all
    2^20 of them -, and the four lumas of every 2 x 2 block over the four frames are the 16 EXHAUSTIVE_LUMAS: 16.7 M pixels,
    the triples at which int32 sums wrap (Y >= 939 with U near 1023) among them."""
    L = layout("p010", 4, 2048, 2048)
    lumas = np.array(EXHAUSTIVE_LUMAS).reshape(4, 2, 2)
    y = np.tile(lumas[:, None, :, None, :], (1, 1024, 1, 1024, 1)).reshape(4, 2048, 2048)
    u = np.broadcast_to(np.arange(1024)[None, :, None], (4, 1024, 1024))
    v = np.broadcast_to(np.arange(1024)[None, None, :], (4, 1024, 1024))
    data = pack(L, y, u, v, garbage_seed=1)
    data.setflags(write=False)
    return data, L


MISTAKES = ("uv_swapped", "chroma_row_y", "chroma_col_x", "pitch_y_for_pitch_c", "step_dropped", "shift_dropped",
            "mask_dropped", "y_off_unscaled", "round_8bit", "int32_wrap", "no_clamp")
NOTICED_BY = {
    "uv_swapped": ("i420", "2x2"), "chroma_row_y": ("i420", "6x10"), "chroma_col_x": ("yv12", "6x10"),
    "pitch_y_for_pitch_c": ("i420", "6x10"),
    "step_dropped": ("p010", "6x10"),       # chroma_step taken as sample_bytes: every second "U" is a V
    "shift_dropped": ("p010", "2x2"),       # the sample read from the low ten bits of a word that keeps it in the top ten
    "mask_dropped": ("i010", "2x2"),        # the garbage in the high six bits enters the sample
    "y_off_unscaled": ("i010", "6x10"),     # 16 subtracted from a ten-bit luma instead of 64
    "round_8bit": ("i010", "36x70"),        # 2^19 added where half a grey level is 2^21
    "int32_wrap": ("p010", "36x70"),        # a sum past 2^31 wraps negative and is clamped to 0 instead of 255
    "no_clamp": ("i420", "36x70"),
}


def restatement(data, L, matrix="bt601", mistake=None):
    """uint8 [n, h, w, 3] of the flat buffer ``data``: the definition by byte addresses.  A misaddressed byte reads what
    lies there in memory - the padding, another plane, the next frame, zeros after the last."""
    from avsum_amd import ingest
    assert mistake is None or mistake in MISTAKES, mistake
    flat = np.concatenate([np.asarray(data).reshape(-1), np.zeros(L.frame_stride + 2, dtype=np.uint8)]).astype(np.int64)
    sb, k = L.sample_bytes, (0 if L.sample_bytes == 1 else 2)

    def sample(at):
        if sb == 1:
            return flat[at]
        word = flat[at] | (flat[at + 1] << 8)
        word = word >> (0 if mistake == "shift_dropped" else L.shift)
        return word if mistake == "mask_dropped" else word & 1023

    frame = (np.arange(L.n) * L.frame_stride)[:, None, None]
    y, x = np.arange(L.h)[None, :, None], np.arange(L.w)[None, None, :]
    pitch_c = L.pitch_y if mistake == "pitch_y_for_pitch_c" else L.pitch_c
    step = sb if mistake == "step_dropped" else L.chroma_step
    c_row = y if mistake == "chroma_row_y" else y >> 1
    c_col = x if mistake == "chroma_col_x" else x >> 1
    luma = sample(frame + y * L.pitch_y + x * sb)
    u = sample(frame + L.u_offset + c_row * pitch_c + c_col * step)
    v = sample(frame + L.v_offset + c_row * pitch_c + c_col * step)
    if mistake == "uv_swapped":
        u, v = v, u
    y_off, cy, cub, cug, cvg, cvr = (np.int64(c) for c in ingest._matrix(matrix, "restatement"))
    yy = np.maximum(luma - (y_off if mistake == "y_off_unscaled" else y_off << k), 0) * cy
    yy = yy + np.int64(1 << (19 if mistake == "round_8bit" else 19 + k))
    uu, vv = u - np.int64(128 << k), v - np.int64(128 << k)
    sums = np.stack([yy + cub * uu, yy + cvg * vv + cug * uu, yy + cvr * vv], axis=-1)
    assert sums.dtype == np.int64
    if mistake == "int32_wrap":
        sums = ((sums + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)     # what 32-bit arithmetic leaves of every sum
    out = sums >> (20 + k)
    return out.astype(np.uint8) if mistake == "no_clamp" else np.clip(out, 0, 255).astype(np.uint8)


def seeded_triples(count, seed=5):
    """(Y, U, V): ``count`` seeded ten-bit triples."""
    return np.random.default_rng(seed).integers(0, 1024, (3, count))


def repack(fmt, nv12, h, w, uv_row, **kw):
    """(data, Layout): the picture of an NV12 array [n, rows, pitch] (nv12_inputs.surface) in ``fmt``, its samples << 2
    for a ten-bit format - what converts to the bytes of ingest.nv12_to_bgr."""
    nv12 = np.asarray(nv12)
    up = depth_of(fmt) - 8
    y = nv12[:, :h, :w].astype(np.int64) << up
    u = nv12[:, uv_row:uv_row + h // 2, 0:w:2].astype(np.int64) << up
    v = nv12[:, uv_row:uv_row + h // 2, 1:w:2].astype(np.int64) << up
    L = layout(fmt, nv12.shape[0], h, w, **kw)
    return pack(L, y, u, v), L


# --------------------------------------------------------------------------- resize cases
# name -> (format, (h, w, pitch_y, pitch_c, gap, spare), frames, index, sizes)
RESIZE_CASES = {
    "up_both_i420": ("i420", (36, 70, 80, 44, 10, 8), 2, (1, 0), ((224, 224), (299, 299))),
    "up_both_p010": ("p010", (36, 70, 80, 76, 10, 8), 2, (1, 0), ((224, 224), (299, 299))),
    "down_both_i010": ("i010", (360, 640, 640, 320, 0, 0), 2, (1, 0), ((224, 224), (299, 299))),
    "down_both_yv12": ("yv12", (360, 640, 648, 328, 0, 0), 2, (1, 0), ((224, 224), (299, 299))),
    "one_size_nv21": ("nv21", (36, 70, 80, 76, 10, 8), 2, (0, 1, 0), ((299, 299),)),
    # 16 luma + 8 chroma rows of 1280 two-byte samples, 2576 LDS bytes each: band 8 -> 4 (one-byte I420 of the same frame
    # keeps 8)
    "halved_p010": ("p010", (448, 1280, 1280, 1280, 0, 0), 1, (0,), ((224, 224),)),
    "index_i420": ("i420", (36, 70, None, None, 0, 0), 3, GATHER_INDEX, ((224, 224), (7, 65))),
    "index_p010": ("p010", (36, 70, None, None, 0, 0), 3, GATHER_INDEX, ((224, 224), (7, 65))),
}
HALVED = ("halved_p010",)
REFUSED_CASE = ("p010", (2, 30000, None, None, 0, 0), (8, 8))     # one luma row is 60 000 bytes: no band fits
RESIZE_BAND, RESIZE_LDS_BYTES = 8, 64 * 1024


@functools.lru_cache(maxsize=None)
def resize_case(name):
    fmt, args, frames = RESIZE_CASES[name][:3]
    return surface(fmt, *args, frames=frames, seed=5)


def staged_rows(L):
    """(bytes of a staged luma row, bytes of a staged chroma row, staged rows per chroma line): the kernel stages the pairs
    of an interleaved line as one row, a planar line as a U row and a V row."""
    interleaved = L.chroma_step == 2 * L.sample_bytes and abs(L.v_offset - L.u_offset) == L.sample_bytes
    return (L.w * L.sample_bytes, (L.w // 2 - 1) * L.chroma_step + (2 if interleaved else 1) * L.sample_bytes,
            1 if interleaved else 2)


def resize_plan(L, dh, dw):
    """ny_plan (yuv.hip; a band's source rows by cv_band_rows of pixel_bodies.h) from the real row bytes: (band, LDS
    bytes, most luma rows, most chroma lines) of one destination; band 0 when even one output row does not fit."""
    if L.w > 65535 or dh > 65535:
        return 0, 0, 0, 0
    rows = source_rows(dh, L.h)
    luma_bytes, chroma_bytes, per_line = staged_rows(L)
    lrow, crow = ((luma_bytes + 15) & ~15) + 16, ((chroma_bytes + 15) & ~15) + 16
    band = RESIZE_BAND
    while band >= 1:
        nl = nc = 1
        for y_lo, y_hi in band_rows(L.h, dh, band, rows):
            nl, nc = max(nl, y_hi - y_lo + 1), max(nc, (y_hi >> 1) - (y_lo >> 1) + 1)
        total = ((dw * 8 + 15) & ~15) + nl * lrow + nc * per_line * crow + ((band * dw * 3 + 16 + 15) & ~15)
        if total <= RESIZE_LDS_BYTES:
            return band, total, nl, nc
        band >>= 1
    return 0, 0, 0, 0


# --------------------------------------------------------------------------- shot-scan cases
HSV_FORMATS = ("i420", "p010", "i010", "nv21")
HSV_LAYOUT = (18, 34, 48, 20, 6, 4)          # (h, w, pitch_y, pitch_c, gap, spare); pitch_c serves both chroma forms
HSV_LAYOUT_INTERLEAVED_PITCH = 40
HSV_OFFSETS = (0, 1, 3, 8)                   # videos of 1, 2 and 5 frames
HSV_STEPS = (1, 2, 3)
HSV_BIG = ((360, 640, None, None, 0, 0), (0, 1, 4))  # 230 400 pixels: 64 workgroups per frame at step 1
HSV_BIG_FORMATS = ("i420", "p010")


@functools.lru_cache(maxsize=None)
def hsv_case(fmt, big=False):
    args, frames = (HSV_BIG[0], HSV_BIG[1][-1]) if big else (HSV_LAYOUT, HSV_OFFSETS[-1])
    h, w, pitch_y, pitch_c, gap, spare = args
    if not big and FORMAT_TABLE[fmt][2]:
        pitch_c = HSV_LAYOUT_INTERLEAVED_PITCH
    return surface(fmt, h, w, pitch_y, pitch_c, gap, spare, frames=frames, seed=11)


# --------------------------------------------------------------------------- end to end
E2E_FORMATS = ("i420", "p010")
E2E_LAYOUT = (36, 70, 80, None, 10, 8)       # (h, w, pitch_y, pitch_c, gap, spare): pitch_c 44 planar, 76 interleaved


def _e2e_args(fmt):
    h, w, pitch_y, _, gap, spare = E2E_LAYOUT
    return h, w, pitch_y, 76 if FORMAT_TABLE[fmt][2] else 44, gap, spare


@functools.lru_cache(maxsize=None)
def scene_batch(fmt):
    """(data, Layout, offsets): nv12_inputs.scene_batch's picture in ``fmt`` - two videos whose scenes are flat (Y, U, V)
    fields far apart, every frame with its own +-3 grey levels of luma noise; ten-bit samples are the 8-bit ones << 2, the
    luma with seeded low bits (the chroma without: one scene is grey, where a quarter level of chroma turns the hue) - cuts
    exactly where the scenes change."""
    h, w = E2E_LAYOUT[:2]
    rng = np.random.default_rng(77)
    up = depth_of(fmt) - 8
    scenes = [((40, 90, 200), (200, 180, 60), (110, 30, 120)), ((220, 128, 128), (60, 200, 40))]
    ys, us, vs = [], [], []
    for video, lengths in zip(scenes, CUT_LENGTHS):
        for (yv, uv, vv), length in zip(video, lengths):
            low = rng.integers(0, 1 << up, (length, h, w)) if up else 0
            ys.append(((yv + rng.integers(-3, 4, (length, h, w))) << up) + low)
            us.append(np.full((length, h // 2, w // 2), uv << up))
            vs.append(np.full((length, h // 2, w // 2), vv << up))
    y, u, v = (np.concatenate(p) for p in (ys, us, vs))
    L = layout(fmt, y.shape[0], *_e2e_args(fmt))
    data = pack(L, y, u, v)
    data.setflags(write=False)
    return data, L, offsets_of([sum(lengths) for lengths in CUT_LENGTHS])


@functools.lru_cache(maxsize=None)
def embed_batch(fmt):
    """(data, Layout, offsets): sum(EMBED_LENGTHS) seeded frames of the end-to-end layout."""
    data, L = surface(fmt, *_e2e_args(fmt), frames=sum(EMBED_LENGTHS), seed=3)
    return data, L, offsets_of(EMBED_LENGTHS)
