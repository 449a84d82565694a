"""Seeded NV12 cases, oracles and planted mistakes of the NV12 ingest tests (libavsum_ingest.so, avsum_amd/ingest.py):
test_nv12_host.py on the host, test_gpu_nv12.py on the device.  numpy only; both build the same cases from here.

Oracles:
  * ``avsum_amd.ingest.nv12_to_bgr_host`` - the integer definition of include/avsum_ingest.h by fancy indexing;
  * ``restatement`` below - the same definition by BYTE ADDRESSES of the flat buffer (frame * frame_stride +
    y * pitch + x ...), written separately so that a planted ``mistake`` can misaddress the way a kernel would; without
    a mistake the host test holds the two equal;
  * ``avsum_amd.ingest.nv12_to_bgr_f64`` - the float formula, within 0.5 + 493 * 2^-21 of the integers.
Everything past the conversion is equality with the BGR kernels on the converted frames: no bound of its own.

MISTAKES are the planted errors; NOTICED_BY names the committed conversion case at which each is noticed.  INERT lists
the one "mistake" that cannot change a byte, and why; the host test shows both that it changes none and that it is
noticed one step earlier, in the integers before the clamp.
"""
import functools

import numpy as np

from avsum_amd import ingest
from pixel_f64_inputs import SENTINEL_U8, source_rows  # noqa: F401  (one restatement of cv_src_pos, shared)

BOUND = 0.5 + 493 * 2.0 ** -21     # |integer definition - float formula|: three coefficients each within 1/2 of c * 2^20,
#                                    times at most 239, 127 and 127 (|Y - 16|, |U - 128|, |V - 128|), over 2^20; + 1/2 of
#                                    the rounding to a grey level

# --------------------------------------------------------------------------- conversion cases
# (h, w, pitch, uv_row): the smallest frame; pitch > w with rows between the planes; several rows of blocks
LAYOUTS = ((2, 2, 2, 2), (6, 10, 16, 8), (36, 70, 80, 40))
LAYOUT_FRAMES = 3
GATHER_INDEX = (2, 2, 1, 0, 3, 1)            # a repeat, a descending run, and (entry 4) one row outside the 3 frames
GATHER_SKIPPED = 4

MISTAKES = ("uv_swapped", "y_off_dropped", "chroma_row_y", "chroma_col_x", "w_for_pitch", "trunc_negative", "no_clamp")
NOTICED_BY = {"uv_swapped": (2, 2, 2, 2), "y_off_dropped": (2, 2, 2, 2), "chroma_row_y": (6, 10, 16, 8),
              "chroma_col_x": (2, 2, 2, 2), "w_for_pitch": (6, 10, 16, 8), "no_clamp": (36, 70, 80, 40)}
INERT = {
    # a negative sum is floor-shifted to <= -1 and truncated to <= 0: either way the clamp makes it 0, and for sums
    # >= 0 the two shifts agree - so no uint8 output can tell them apart; the integers before the clamp can
    "trunc_negative": "every negative sum is clamped to 0 whichever way it was rounded",
}


def surface(h, w, pitch, uv_row, frames=LAYOUT_FRAMES, seed=0, spare_rows=1):
    """uint8 [frames, uv_row + h / 2 + spare_rows, pitch]: seeded bytes in the two planes, SENTINEL_U8 in every byte a
    kernel must not read (the pitch padding, the rows between and after the planes)."""
    rng = np.random.default_rng(7100 + 1000 * h + 10 * w + seed)
    data = np.full((frames, uv_row + h // 2 + spare_rows, pitch), SENTINEL_U8, dtype=np.uint8)
    data[:, :h, :w] = rng.integers(0, 256, (frames, h, w), dtype=np.uint8)
    data[:, uv_row:uv_row + h // 2, :w] = rng.integers(0, 256, (frames, h // 2, w), dtype=np.uint8)
    return data


def planes_mask(h, w, pitch, uv_row, rows):
    """bool [rows, pitch]: the bytes of a frame that belong to a plane."""
    mask = np.zeros((rows, pitch), dtype=bool)
    mask[:h, :w] = True
    mask[uv_row:uv_row + h // 2, :w] = True
    return mask


@functools.lru_cache(maxsize=None)
def layout_case(layout):
    data = surface(*layout)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def exhaustive_case():
    """uint8 [64, 768, 512], frames of 512 x 512: chroma row r holds the pairs (U, V) = (r, c), c = 0 .. 255 - all
    65 536 of them - and the four lumas of every 2 x 2 block of frame k are 4k .. 4k + 3: every (Y, U, V) once."""
    data = np.empty((64, 768, 512), dtype=np.uint8)
    k = np.arange(64)[:, None, None]
    y, x = np.arange(512)[None, :, None], np.arange(512)[None, None, :]
    data[:, :512] = 4 * k + 2 * (y & 1) + (x & 1)
    data[:, 512:, 0::2] = np.arange(256, dtype=np.uint8)[None, :, None]
    data[:, 512:, 1::2] = np.arange(256, dtype=np.uint8)[None, None, :]
    data.setflags(write=False)
    return data


def restatement(data, h, w, uv_row, matrix="bt601", mistake=None, clamp=True):
    """[N, h, w, 3] of a uint8 [N, rows, pitch]: the definition by byte addresses.  A misaddressed byte reads what lies
    there in memory - the padding, the other plane, the next frame, zeros after the last.  clamp=False: the int32 sums
    after the shift, before the clamp."""
    assert mistake is None or mistake in MISTAKES, mistake
    n, rows, pitch = data.shape
    flat = np.concatenate([np.asarray(data).reshape(-1), np.zeros(rows * pitch + 2, dtype=np.uint8)]).astype(np.int32)
    frame = (np.arange(n) * rows * pitch)[:, None, None]
    y, x = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    step = w if mistake == "w_for_pitch" else pitch
    luma = flat[frame + y * step + x]
    c_row = y if mistake == "chroma_row_y" else y >> 1
    c_col = x if mistake == "chroma_col_x" else x & ~1
    c_at = frame + uv_row * pitch + c_row * step + c_col
    u, v = flat[c_at], flat[c_at + 1]
    if mistake == "uv_swapped":
        u, v = v, u
    y_off, cy, cub, cug, cvg, cvr = (np.int32(c) for c in ingest._matrix(matrix, "restatement"))
    if mistake == "y_off_dropped":
        y_off = np.int32(0)
    yy = np.maximum(luma - y_off, 0) * cy + np.int32(1 << 19)
    uu, vv = u - np.int32(128), v - np.int32(128)
    sums = np.stack([yy + cub * uu, yy + cvg * vv + cug * uu, yy + cvr * vv], axis=-1)
    assert sums.dtype == np.int32
    if mistake == "trunc_negative":
        out = np.where(sums < 0, -((-sums) >> 20), sums >> 20)      # C's division: towards zero
    else:
        out = sums >> 20
    if not clamp:
        return out
    return out.astype(np.uint8) if mistake == "no_clamp" else np.clip(out, 0, 255).astype(np.uint8)


def all_triples(y_lo, y_hi):
    """(Y, U, V) int32 grids of the lumas y_lo .. y_hi - 1 with every chroma pair."""
    g = np.arange(256, dtype=np.int32)
    return np.meshgrid(np.arange(y_lo, y_hi, dtype=np.int32), g, g, indexing="ij")


# --------------------------------------------------------------------------- resize cases
# name -> (h, w, pitch, uv_row, frames, index, sizes)
RESIZE_CASES = {
    "up_both": (36, 70, 80, 40, 2, (1, 0), ((224, 224), (299, 299))),
    "down_both": (360, 640, 640, 360, 2, (1, 0), ((224, 224), (299, 299))),
    "one_size": (36, 70, 80, 40, 2, (0, 1, 0), ((299, 299),)),
    "halved": (448, 2560, 2560, 448, 1, (0,), ((224, 224),)),     # 16 luma + 8 chroma rows of 2576 LDS bytes: band 8 -> 4
    "index": (36, 70, 70, 36, 3, GATHER_INDEX, ((224, 224), (7, 65))),
}
RESIZE_BAND, RESIZE_LDS_BYTES = 8, 64 * 1024


@functools.lru_cache(maxsize=None)
def resize_case(name):
    h, w, pitch, uv_row, frames = RESIZE_CASES[name][:5]
    data = surface(h, w, pitch, uv_row, frames, seed=5)
    data.setflags(write=False)
    return data


def resize_plan(sh, sw, dh, dw):
    """ni_plan (ingest.hip; a band's source rows by cv_band_rows of pixel_bodies.h): (band, LDS bytes, most luma rows,
    most chroma rows) of one destination; band 0 when even one output row does not fit."""
    rows = source_rows(dh, sh)
    lrow = ((sw + 15) & ~15) + 16
    band = RESIZE_BAND
    while band >= 1:
        nl = nc = 1
        for y_lo, y_hi in band_rows(sh, dh, band, rows):
            nl, nc = max(nl, y_hi - y_lo + 1), max(nc, (y_hi >> 1) - (y_lo >> 1) + 1)
        total = ((dw * 8 + 15) & ~15) + (nl + nc) * lrow + ((band * dw * 3 + 16 + 15) & ~15)
        if total <= RESIZE_LDS_BYTES:
            return band, total, nl, nc
        band >>= 1
    return 0, 0, 0, 0


def band_rows(sh, dh, band, rows=None):
    """[(y_lo, y_hi)]: the first and last luma row every band of ``band`` output rows reads."""
    rows = source_rows(dh, sh) if rows is None else rows
    return [(int(rows[lo]), min(int(rows[min(lo + band, dh) - 1]) + 1, sh - 1)) for lo in range(0, dh, band)]


# --------------------------------------------------------------------------- shot-scan cases
HSV_LAYOUT = (18, 34, 48, 20)                # (h, w, pitch, uv_row)
HSV_OFFSETS = (0, 1, 3, 8)                   # videos of 1, 2 and 5 frames
HSV_STEPS = (1, 2, 3)
HSV_BIG = ((360, 640, 640, 360), (0, 1, 4))  # 230 400 pixels: 64 workgroups per frame at step 1


@functools.lru_cache(maxsize=None)
def hsv_case(layout, frames):
    data = surface(*layout, frames=frames, seed=11)
    data.setflags(write=False)
    return data


# --------------------------------------------------------------------------- end to end
E2E_LAYOUT = (36, 70, 80, 40)
CUT_LENGTHS = ((16, 17, 15), (18, 16))       # scene lengths of the two videos: cuts at 16, 33 and at 18
EMBED_LENGTHS = (12, 9)
EMBED_SHOTS = ([(0, 6), (6, 12)], [(0, 9)])  # frames 0, 3 | 6, 9 | 0, 3, 6: seven sampled frames in three shots


def offsets_of(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


@functools.lru_cache(maxsize=None)
def scene_batch():
    """(uint8 [81, rows, pitch], offsets): two videos whose scenes are flat (Y, U, V) fields far apart, every frame with
    its own +-3 of luma noise - cuts exactly where the scenes change."""
    h, w, pitch, uv_row = E2E_LAYOUT
    rng = np.random.default_rng(77)
    scenes = [((40, 90, 200), (200, 180, 60), (110, 30, 120)), ((220, 128, 128), (60, 200, 40))]
    frames = []
    for video, lengths in zip(scenes, CUT_LENGTHS):
        for (yv, uv, vv), length in zip(video, lengths):
            f = np.full((length, uv_row + h // 2 + 1, pitch), SENTINEL_U8, dtype=np.uint8)
            f[:, :h, :w] = yv + rng.integers(-3, 4, (length, h, w))
            f[:, uv_row:uv_row + h // 2, 0:w:2] = uv
            f[:, uv_row:uv_row + h // 2, 1:w:2] = vv
            frames.append(f)
    data = np.concatenate(frames)
    data.setflags(write=False)
    return data, offsets_of([sum(lengths) for lengths in CUT_LENGTHS])


def scene_cuts():
    """[[(start, end)]] per video: what detect_shots returns for scene_batch."""
    out = []
    for lengths in CUT_LENGTHS:
        edges = offsets_of(lengths)
        out.append(list(zip(edges[:-1], edges[1:])))
    return out
