"""Inputs, float64 references, restatements, planted mistakes and the bounds of the per-kernel tests of the kernels that
touch raw uint8 pixels: avs_resize_bilinear_u8, avs_frames_normalize_u8, avs_hsv_frame_diff_u8, avs_pull_copy_u8
(csrc/visual.hip), avs_resize_bilinear_gather2_u8 (csrc/stage1_batch.hip) and avs_hsv_frame_diff_batch_u8
(csrc/shots_batch.hip): test_pixel_f64_host.py on the host, test_gpu_pixel_f64.py on the device.  numpy / torch on the CPU
only: both build the same seeded cases from here.

References - the definitions in float64, none of them written from memory of OpenCV:
  * resize: half-pixel centres, src = (d + 0.5) s / dsize - 0.5 clamped to [0, s - 1], a linear blend of the two
    neighbours per axis, no rounding (``resize_reference``);
  * HSV: V = max, S = 255 diff / V (0 at V = 0), H = 30 (g - b) / diff, 30 (b - r) / diff + 60 or 30 (r - g) / diff + 120
    by the channel that is the maximum, modulo 180, 0 at diff = 0 (``hsv_reference``);
  * normalise: ((v / denom - mean) / std) a + b (``normalize_eval`` in float64).

Restatements - CPU copies of the kernels' own arithmetic: ``resize_restatement`` (11-bit coefficients, 32-bit integers;
equal to oracle.cnn.cv_resize_linear_u8), ``hsv_restatement`` / ``hsv_sums`` (12-bit division tables; equal to
oracle.shots.bgr2hsv_u8), ``normalize_eval`` in fp32 with every operation rounded, ``pull_copy_restatement`` (the unit
walk of pull_copy_kernel).  ``mistake`` plants one deliberate error (MISTAKES); NOTICED_BY names the case at which the
host test shows it to be noticed; INERT lists the "mistakes" the host test shows to change no byte, and why.

Bounds - derived here, none measured on the code under test: ``resize_bound`` (grey levels), HSV_S_BOUND and
HSV_H_BOUND; everything else is equality with a restatement, and the fp32 normalise restatement is held to float64 by
scorer_f64_inputs.compare unchanged."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from scorer_f64_inputs import EPS32, compare as _compare  # noqa: F401  (one definition of the bound, shared)
from test_gpu_f16x2 import emu_pack  # noqa: F401  (the AVS_F16X2 format restated on the CPU, shared)

F32 = np.float32
SENTINEL_U8 = 0xA5          # fill of every byte a kernel must not write

# --------------------------------------------------------------------------- launch constants the cases rely on
# (test_pixel_f64_host.py checks each against the source text of its launcher)
THREADS = 256
GRID_CAP = 16384            # resize_bilinear_kernel, frames_normalize_kernel<float / bf16>: most workgroups
GRID_CAP_H2 = 4096          # frames_normalize_h2_kernel
HSV_WG_PIXELS = 256 * 8     # avs_hsv_frame_diff(_batch)_u8: one workgroup per 2048 strided pixels ...
HSV_WG_CAP = 64             # ... 64 at the most
HSV_MAX_FRAMES = 65536      # per call of the per-video form (grid y)
RG_BAND, RG_THREADS, RG_LDS_BYTES = 8, 256, 64 * 1024
PULL_MAX_WORKGROUPS = 1024

RESIZE_MISTAKES = ("no_half_pixel", "s1_unclamped", "clamp_at_smax", "clamp_at_smax_s1_unclamped", "coef_truncated",
                   "plus2_dropped", "shift4_skipped", "scale_swapped")
REFERENCE_CATCHES = ("no_half_pixel", "clamp_at_smax_s1_unclamped", "plus2_dropped", "scale_swapped")      # the ‡ mistakes
HSV_MISTAKES = ("h_not_wrapped", "g_before_r", "round_dropped", "sdiv_from_diff", "step_rows_only", "prev_across_videos",
                "last_workgroup_dropped")
NORM_MISTAKES = ("zero_channel_not_zero", "pad_normalised", "affine_before_std", "h2_pair_swapped", "h2_lo_from_pixel0")
PULL_MISTAKES = ("remainder_one_stride_late", "tail_from_offset_0", "last_unit_skipped")
MISTAKES = RESIZE_MISTAKES + HSV_MISTAKES + NORM_MISTAKES + PULL_MISTAKES

# "mistakes" that change nothing, shown on the host (test_inert_mistakes_change_nothing) and therefore not planted:
INERT = {
    # where s1 = s0 + 1 would leave the row, the upper clamp has already set f = 0: the neighbour's weight is 0, its
    # value never reaches the result (a kernel with this mistake reads one byte run past the row, and multiplies by 0)
    "s1_unclamped": "the weight of the unclamped neighbour is 0",
    # v == r == g: g - b = diff and b - r + 2 diff = diff; v == g == b and v == r == b alike: where two channels tie for
    # the maximum the branches agree, so their order does not matter
    "g_before_r": "the branches agree wherever two channels tie for the maximum",
}


def compare(got, ref, cpu32, scale=None):
    """scorer_f64_inputs.compare on numpy arrays / torch tensors."""
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return _compare(as_t(got), as_t(ref), as_t(cpu32), scale)


def cdiv(a, b):
    return -(-a // b)


# =========================================================================== resize
# (source h, w) -> (destination h, w)
RESIZE_PAIRS = (((1, 1), (3, 5)), ((1, 9), (4, 20)), ((9, 1), (20, 4)), ((2, 2), (7, 7)), ((5, 7), (1, 1)),
                ((8, 12), (4, 6)), ((12, 9), (4, 3)), ((37, 53), (36, 300)), ((64, 64), (64, 64)),
                ((240, 320), (224, 224)),
                ((150, 11), (16, 9)),        # ratio 9.4: a band of 8 output rows spans 75 source rows
                ((20, 2200), (16, 40)))      # 10 source rows of 6600 bytes: more than 64 KiB at 8 output rows, the band is halved
CONTENTS = ("noise", "hramp", "vramp", "checker")
RESIZE_FRAMES = 3
RESIZE_BIG = SimpleNamespace(frames=65537, src=(3, 5), dst=(8, 8), base=7)     # frame k is base frame k % 7
GATHER_INDEX = (2, 2, 1, 0, 3, 1)            # a repeat, a descending run, and (entry 4) one row outside the 3 frames
GATHER_SKIPPED = 4
GATHER_SECOND = (7, 65)                      # the second destination: dh < 8, one lane trip and one pixel
GATHER_OFFSETS = (0, 1, 15)


@functools.lru_cache(maxsize=None)
def resize_case(src, content, frames=RESIZE_FRAMES):
    """uint8 [frames, h, w, 3] (read-only).  noise: seeded; hramp / vramp: 0 .. 255 along x / y, channel c shifted by 40 c
    and frame k reversed for odd k; checker: 0 and 255 by the parity of x + y + frame, inverted in channel 1 - the largest
    neighbour difference at every pixel."""
    h, w = src
    if content == "noise":
        out = np.random.default_rng(9100 + 1000 * h + w).integers(0, 256, (frames, h, w, 3), dtype=np.uint8)
    else:
        y, x, k, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(frames), np.arange(3), indexing="ij")
        if content == "hramp":
            v = np.rint(255.0 * np.where(k % 2 == 1, w - 1 - x, x) / max(w - 1, 1)) + 40 * c
        elif content == "vramp":
            v = np.rint(255.0 * np.where(k % 2 == 1, h - 1 - y, y) / max(h - 1, 1)) + 40 * c
        else:
            assert content == "checker", content
            v = 255 * ((x + y + k + (c == 1)) % 2)
        out = np.ascontiguousarray((v.astype(np.int64) % 256).astype(np.uint8).transpose(2, 0, 1, 3))
    out.setflags(write=False)
    return out


def _positions64(dn, sn):
    """float64 source positions of dn destination centres in a source of sn, clamped: (i0, i1, fraction)."""
    pos = np.clip((np.arange(dn) + 0.5) * (sn / dn) - 0.5, 0.0, sn - 1.0)
    i0 = np.minimum(np.floor(pos).astype(np.int64), sn - 1)
    return i0, np.minimum(i0 + 1, sn - 1), pos - i0


def resize_reference(frames, dh, dw):
    """float64 [n, dh, dw, 3]: the bilinear resize by its definition, not rounded."""
    src = np.asarray(frames, dtype=np.float64)
    y0, y1, fy = _positions64(dh, src.shape[1])
    x0, x1, fx = _positions64(dw, src.shape[2])
    fx, fy = fx[None, None, :, None], fy[None, :, None, None]
    hor = src[:, :, x0] * (1.0 - fx) + src[:, :, x1] * fx
    return hor[:, y0] * (1.0 - fy) + hor[:, y1] * fy


def resize_coefs(dn, sn, scale=None, mistake=None):
    """cv_linear_coef (pixel_bodies.h, the one text of all three resize kernels) for every destination index:
    (s0, s1, c0, c1) int64 [dn].  The position in fp32, the fraction by an exact fp32 subtraction, both coefficients rounded to 11 bits."""
    scale = 1.0 / (dn / sn) if scale is None else scale
    d = np.arange(dn)
    f = (d * scale if mistake == "no_half_pixel" else (d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    low = s < 0
    f[low], s[low] = 0, 0
    high = s >= (sn if mistake in ("clamp_at_smax", "clamp_at_smax_s1_unclamped") else sn - 1)
    f[high], s[high] = 0, sn - 1
    s1 = s + 1 if mistake in ("s1_unclamped", "clamp_at_smax_s1_unclamped") else np.minimum(s + 1, sn - 1)
    to_int = np.trunc if mistake == "coef_truncated" else np.rint
    c0 = to_int((F32(1.0) - f) * F32(2048.0)).astype(np.int64)
    c1 = to_int(f * F32(2048.0)).astype(np.int64)
    return s, s1, c0, c1


def source_rows(dn, sn):
    """cv_src_pos (pixel_bodies.h) for every destination index: the first source row of each."""
    return resize_coefs(dn, sn)[0]


def resize_restatement(frames, dh, dw, mistake=None):
    """uint8 [n, dh, dw, 3]: resize_bilinear_kernel's arithmetic in 32-bit integers (numpy int32 wraps as the device's
    int does).  A neighbour index past the end of a row reads what lies there in memory: the next row, the next frame,
    and zeros after the last frame."""
    assert mistake is None or mistake in RESIZE_MISTAKES
    n, sh, sw, _ = frames.shape
    sy, sx = (1.0 / (dh / sh), 1.0 / (dw / sw))
    if mistake == "scale_swapped":
        sy, sx = sx, sy
    x0, x1, a0, a1 = resize_coefs(dw, sw, sx, mistake)
    y0, y1, b0, b1 = resize_coefs(dh, sh, sy, mistake)
    flat = np.concatenate([np.asarray(frames, dtype=np.int32).reshape(-1), np.zeros((sw + 1) * 3 * 2, dtype=np.int32)])
    img = (np.arange(n) * sh)[:, None, None, None]
    c = np.arange(3)[None, None, None, :]

    def px(yy, xx):     # the byte at ((img * sh + y) * sw + x) * 3 + c, rows and columns of any index
        return flat[((img + yy[None, :, None, None]) * sw + xx[None, None, :, None]) * 3 + c]

    a0, a1 = a0.astype(np.int32)[None, None, :, None], a1.astype(np.int32)[None, None, :, None]
    b0, b1 = b0.astype(np.int32)[None, :, None, None], b1.astype(np.int32)[None, :, None, None]
    with np.errstate(over="ignore"):
        s0 = px(y0, x0) * a0 + px(y0, x1) * a1
        s1 = px(y1, x0) * a0 + px(y1, x1) * a1
        if mistake != "shift4_skipped":
            s0, s1 = s0 >> 4, s1 >> 4
        v = ((b0 * s0) >> 16) + ((b1 * s1) >> 16) + np.int32(0 if mistake == "plus2_dropped" else 2) >> 2
    assert v.dtype == np.int32
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_bound(sh, sw):
    """The largest distance, in grey levels, of a correct 11-bit fixed-point evaluation (resize_bilinear_kernel's
    scheme) from ``resize_reference``, for a source of sh x sw.  With p the neighbours (0 .. 255), f the exact fraction:

      1. position: (d + 0.5) scale - 0.5 is rounded to fp32 once; a value below s has a half-ulp of at most 2^-24 s.  The
         blend is continuous and piecewise linear in the position (across a change of the integer part and across the
         clamps too) with slope at most 255 (the neighbour difference), so each axis costs at most 255 * 2^-24 * s, and
         the fp32 rounding of 1 - f (positions in (0, 1) only) another 255 * 2^-25: together below
         255 * 2^-24 * (sh + sw + 1).  f - floor(f) is exact.
      2. coefficients: c1 = rint(2048 f), c0 = rint(2048 (1 - f)), each within 1/2 of its value, and c0 + c1 = 2048 (the
         host test asserts it for every table of the cases), so the blend (p0 c0 + p1 c1) / 2048 is off by
         |p1 - p0| / 2 / 2048 <= 255 * 2^-12 per axis: 255 * 2^-11 for both.
      3. S >> 4 drops at most 15/16 of a unit of S / 16; the result is b (S >> 4) / 2^18 with b0 + b1 = 2048, so the two
         truncations together lower it by at most 2048 * (15 / 16) / 2^18 = 15 / 2048.
      4. each >> 16 lowers its term by less than one unit of a quarter level: below 1/2 level together.
      5. (x + 2) >> 2 rounds the INTEGER x / 4 to the nearest level, halves up: it raises by at most 1/2 (x = 2 mod 4) and
         lowers by at most 1/4 (x = 1 mod 4).
    Steps 3 and 4 only lower, so the result lies at most (2) + (3) + (4) + 1/4 below and at most (2) + 1/2 above the exact
    value, plus (1) either way; the clamp to 0 .. 255 moves it towards the reference, which lies in that range:

      bound = 255 * 2^-11 + 15 / 2048 + 1/2 + 1/4 + 255 * 2^-24 * (sh + sw + 1)  =  0.8818 + 1.5e-5 (sh + sw + 1)."""
    return 255.0 / 2048 + 15.0 / 2048 + 0.5 + 0.25 + 255.0 * 2.0 ** -24 * (sh + sw + 1)


def gather_plan(sh, sw, dh, dw):
    """rg_plan (stage1_batch.hip; a band's source rows by cv_band_rows of pixel_bodies.h): (band, LDS bytes, most source
    rows a band reads) of one destination; band 0 when even one output row does not fit."""
    rows = source_rows(dh, sh)
    band = RG_BAND
    while band >= 1:
        span = 1
        for lo in range(0, dh, band):
            hi = min(lo + band, dh)
            span = max(span, min(int(rows[hi - 1]) + 1, sh - 1) - int(rows[lo]) + 1)
        in_bytes = (span * sw * 3 + 16 + 15) & ~15
        out_bytes = (band * dw * 3 + 16 + 15) & ~15
        total = ((dw * 8 + 15) & ~15) + in_bytes + out_bytes
        if total <= RG_LDS_BYTES:
            return band, total, span
        band >>= 1
    return 0, 0, 0


def grid_trips(items, cap, threads=THREADS):
    """(workgroups, trips of the grid-stride loop) of a launch of min(cdiv(items, threads), cap) workgroups."""
    grid = min(cdiv(items, threads), cap)
    return grid, cdiv(items, grid * threads)


# =========================================================================== HSV
HSV_S_BOUND = 0.5 + 255 * 0.5 / 4096          # see hsv_reference
HSV_H_BOUND = 0.5 + 5 * 255 * 0.5 / 4096
HSV_SIZES = ((1, 1), (1, 300), (130, 127), (47, 45), (363, 364))
HSV_STEPS = (1, 2, 3)
HSV_FRAMES = 8
HSV_VIDEOS = (0, 1, 3, 6, 8)                  # the 8 frames cut into videos of 1, 2, 3 and the remaining 2 frames


def hsv_reference(bgr):
    """float64 (H in [0, 180), S, V) of uint8 [..., 3] BGR pixels, by the definition.

    Bounds of the 12-bit tables (HSV_S_BOUND, HSV_H_BOUND): the kernel holds sdiv = rint(255 * 4096 / V) and
    hdiv = rint(180 * 4096 / (6 diff)), each within 1/2 of its value, and computes (diff * sdiv + 2048) >> 12 and
    (hh * hdiv + 2048) >> 12, hh = g - b, b - r + 2 diff or r - g + 4 diff.  The product is off by at most
    diff * 0.5 / 4096 <= 255 * 0.5 / 4096 for S and by |hh| * 0.5 / 4096 <= 5 * 255 * 0.5 / 4096 for H (|hh| <= 5 diff);
    adding 2048 and shifting rounds to the nearest integer, halves up: another 1/2.  V is a maximum: exact.  H is compared
    on the circle (a hue just below 0 is stored as 0, just below 180 of the definition)."""
    b, g, r = [np.asarray(bgr[..., i], dtype=np.float64) for i in range(3)]
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    safe_v, safe_d = np.where(v > 0, v, 1.0), np.where(diff > 0, diff, 1.0)
    s = np.where(v > 0, 255.0 * diff / safe_v, 0.0)
    h = np.where(v == r, 30.0 * (g - b) / safe_d, np.where(v == g, 30.0 * (b - r) / safe_d + 60.0, 30.0 * (r - g) / safe_d + 120.0))
    return np.where(diff > 0, np.mod(h, 180.0), 0.0), s, v


def circular(a, b, period=180.0):
    d = np.abs(np.asarray(a, dtype=np.float64) - b) % period
    return np.minimum(d, period - d)


@functools.lru_cache(maxsize=None)
def _div_tables():
    idx = np.arange(1, 256)
    sdiv, hdiv = np.zeros(256, dtype=np.int32), np.zeros(256, dtype=np.int32)
    sdiv[1:] = np.rint((255 << 12) / (1.0 * idx))
    hdiv[1:] = np.rint((180 << 12) / (6.0 * idx))
    return sdiv, hdiv


def hsv_restatement(bgr, mistake=None):
    """int32 (h, s, v) of uint8 [..., 3]: bgr2hsv_u8 (avs_internal.h) in the device's 32-bit integers."""
    sdiv, hdiv = _div_tables()
    b, g, r = [bgr[..., i].astype(np.int32) for i in range(3)]
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    half = 0 if mistake == "round_dropped" else 1 << 11
    s = (diff * sdiv[diff if mistake == "sdiv_from_diff" else v] + half) >> 12
    if mistake == "g_before_r":
        hh = np.where(v == g, b - r + 2 * diff, np.where(v == r, g - b, r - g + 4 * diff))
    else:
        hh = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    hh = (hh * hdiv[diff] + half) >> 12
    if mistake != "h_not_wrapped":
        hh = np.where(hh < 0, hh + 180, hh)
    return hh, s, v


def hsv_grid(h, w, step):
    """(strided pixels, workgroups per frame, trips of the pixel loop) of avs_hsv_frame_diff_u8 and its batch form."""
    npx = cdiv(h, step) * cdiv(w, step)
    wgs = max(1, min(cdiv(npx, HSV_WG_PIXELS), HSV_WG_CAP))
    return npx, wgs, cdiv(npx, wgs * THREADS)


def hsv_sums(frames, step=1, offsets=None, mistake=None):
    """int64 [n, 3]: hsv_frame_diff_kernel's sums of |dH|, |dS|, |dV| of every frame against the previous one over the
    pixels [::step, ::step]; zeros in row 0 and, with ``offsets`` (the batch form), in every video's first row."""
    assert mistake is None or mistake in HSV_MISTAKES
    n, h, w, _ = frames.shape
    sub = frames[:, ::step] if mistake == "step_rows_only" else frames[:, ::step, ::step]
    hsv = np.stack(hsv_restatement(sub, mistake), -1).astype(np.int64).reshape(n, -1, 3)
    d = np.abs(hsv[1:] - hsv[:-1])
    if mistake == "last_workgroup_dropped":
        _, wgs, _ = hsv_grid(h, w, step)
        d = d[:, (np.arange(d.shape[1]) // THREADS) % wgs != wgs - 1]       # pixel i belongs to workgroup (i / 256) % wgs
    sums = np.zeros((n, 3), dtype=np.int64)
    sums[1:] = d.sum(1)
    if offsets is not None and mistake != "prev_across_videos":
        sums[[o for o in offsets[:-1]]] = 0
    return sums


@functools.lru_cache(maxsize=None)
def hsv_case(size):
    """uint8 [8, h, w, 3] seeded noise, a tenth of the pixels grey and a few black (diff = 0, V = 0); read-only."""
    h, w = size
    rng = np.random.default_rng(9200 + 1000 * h + w)
    f = rng.integers(0, 256, (HSV_FRAMES, h, w, 3), dtype=np.uint8)
    grey = rng.random((HSV_FRAMES, h, w)) < 0.1
    f[grey] = f[grey][:, :1]
    f[rng.random((HSV_FRAMES, h, w)) < 0.02] = 0
    f.setflags(write=False)
    return f


def hsv_cube():
    """uint8 [257, 256, 256, 3]: frame 0 black, frame 1 + b holds the colour (b, g = y, r = x) - all 2^24 colours."""
    f = np.zeros((257, 256, 256, 3), dtype=np.uint8)
    f[1:, :, :, 0] = np.arange(256, dtype=np.uint8)[:, None, None]
    f[1:, :, :, 1] = np.arange(256, dtype=np.uint8)[None, :, None]
    f[1:, :, :, 2] = np.arange(256, dtype=np.uint8)[None, None, :]
    return f


# =========================================================================== normalise
NORM_STATS = {255.0: ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
              1.0: ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375))}
NORM_AFFINE = (0.458, 0.448, 0.45, -0.03, -0.088, -0.188)        # a0 a1 a2 b0 b1 b2
NORM_SRC = (12, 23)                                              # w odd; 276 pixels: every byte value in every channel
NORM_PADS = tuple((pt, pl) for pt in (0, 2) for pl in (0, 1, 3))
NORM_FORMATS = ("f32", "bf16", "f16x2")
NORM_BIG = {"f32": 262145, "bf16": 262145, "f16x2": 131073}      # frames of 2 x 2 into 4 x 4, pad 1 / 1
NORM_BIG_BASE = 5


def norm_geometry(pad_t, pad_l, src=NORM_SRC):
    """(out_h, out_w): two rows below the image, and one or two columns to its right (out_w even, as AVS_F16X2 asks)."""
    h, w = src
    ow = w + pad_l + 1
    return h + pad_t + 2, ow + ow % 2


@functools.lru_cache(maxsize=None)
def norm_case(src=NORM_SRC, frames=2):
    """uint8 [frames, h, w, 3]: pixel i of frame k holds (37 k + i + 85 c) mod 256 in channel c, frame 1 reversed."""
    h, w = src
    i = np.arange(h * w).reshape(h, w)
    f = np.stack([((37 * k + (i if k % 2 == 0 else i[::-1, ::-1]))[..., None] + 85 * np.arange(3)) % 256 for k in range(frames)])
    f = f.astype(np.uint8)
    f.setflags(write=False)
    return f


def normalize_eval(frames, denom, affine, out_h, out_w, pad_t, pad_l, dtype=F32, mistake=None):
    """[n, out_h, out_w, 4] in ``dtype``: frames_normalize_kernel's expression, every operation rounded to ``dtype`` (the
    build does not contract): f = v / denom; f = (f - mean) / std; f = f * a; f = f + b; zero padding and a zero fourth
    channel.  The constants are the fp32 values the kernel is handed, in either dtype."""
    assert mistake is None or mistake in NORM_MISTAKES
    mean, std = (np.array(v, dtype=F32).astype(dtype) for v in NORM_STATS[float(denom)])
    n, h, w, _ = frames.shape
    f = frames.astype(dtype) / dtype(denom)
    if affine is not None and mistake == "affine_before_std":
        a, b = (np.array(v, dtype=F32).astype(dtype) for v in (affine[:3], affine[3:]))
        f = ((f - mean) * a + b) / std
    else:
        f = (f - mean) / std
        if affine is not None:
            a, b = (np.array(v, dtype=F32).astype(dtype) for v in (affine[:3], affine[3:]))
            f = f * a
            f = f + b
    assert f.dtype == dtype
    out = np.zeros((n, out_h, out_w, 4), dtype=dtype)
    if mistake == "pad_normalised":
        out[..., :3] = (dtype(0) - mean) / std
    out[:, pad_t:pad_t + h, pad_l:pad_l + w, :3] = f
    if mistake == "zero_channel_not_zero":
        out[..., 3] = out[..., 2]
    return out


def h2_words(image32, mistake=None):
    """int16 [pairs, 2, 8]: the AVS_F16X2 image of the fp32 image [n, oh, ow, 4] (ow even), packed by emu_pack - per
    pixel pair the 8 hi halves (pixel 0: c0 c1 c2 0, pixel 1: c0 c1 c2 0), then the 8 lo halves."""
    packed = emu_pack(torch.from_numpy(np.ascontiguousarray(image32)).reshape(-1, 8))
    runs = packed.contiguous().view(torch.int16).reshape(-1, 2, 8).clone()
    if mistake == "h2_pair_swapped":
        runs = torch.cat([runs[:, :, 4:], runs[:, :, :4]], 2)
    elif mistake == "h2_lo_from_pixel0":
        runs[:, 1, 4:] = runs[:, 1, :4]
    return runs


# =========================================================================== pull copy
PULL_WORKGROUPS = (1, 3, 16)
PULL_TAILS = (0, 1, 15)
PULL_BIG_WORKGROUPS = 1024


def pull_units(workgroups):
    s = THREADS * workgroups
    return (0, 1, s - 1, 3 * s, 4 * s - 1, 4 * s, 4 * s + 1, 7 * s + 5)


def pull_source(nbytes):
    return np.random.default_rng(9300 + nbytes % 9973).integers(0, 256, nbytes, dtype=np.uint8)


def pull_copy_restatement(src, workgroups, mistake=None):
    """(dst uint8 [bytes] over a SENTINEL_U8 fill, copies int64 [n16]): pull_copy_kernel's walk over the 16-byte units -
    four units a stride apart per trip while i + 3 stride < n16, the remainder a stride apart, the byte tail by the first
    threads of workgroup 0 - and how often each unit was written."""
    assert mistake is None or mistake in PULL_MISTAKES
    nbytes = len(src)
    n16, stride = nbytes // 16, THREADS * workgroups
    copies = np.zeros(n16, dtype=np.int64)
    i = np.arange(stride, dtype=np.int64)
    live = np.ones(stride, dtype=bool)
    while True:
        live &= i + 3 * stride < n16
        if not live.any():
            break
        for q in range(4):
            np.add.at(copies, i[live] + q * stride, 1)
        i = np.where(live, i + 4 * stride, i)
    if mistake == "remainder_one_stride_late":
        i = i + stride
    while (i < n16).any():
        np.add.at(copies, i[i < n16], 1)
        i = i + stride
    if mistake == "last_unit_skipped" and n16 > 0 and n16 % (4 * stride) == 0:
        copies[n16 - 1] = 0
    dst = np.full(nbytes, SENTINEL_U8, dtype=np.uint8)
    done = np.repeat(copies > 0, 16)
    dst[:n16 * 16][done] = src[:n16 * 16][done]
    tail = nbytes - n16 * 16
    dst[n16 * 16:] = src[:tail] if mistake == "tail_from_offset_0" else src[n16 * 16:]
    return dst, copies


# =========================================================================== where each mistake is noticed
NOTICED_BY = {
    # resize: (pair, content); the ‡ ones (REFERENCE_CATCHES) also lie outside resize_bound of the float64 reference there
    "no_half_pixel": (((240, 320), (224, 224)), "checker"),
    # (clamp_at_smax alone keeps the fraction of a position past the last centre, but s1 is clamped to s0: both neighbours
    # are the last pixel and the coefficients sum to 2048, so only the split of the two >> 16 truncations differs - seen by
    # the bit comparison, inside the bound; with s1 unclamped as well the neighbour is read past the row)
    "clamp_at_smax": (((2, 2), (7, 7)), "checker"),
    "clamp_at_smax_s1_unclamped": (((2, 2), (7, 7)), "checker"),
    "coef_truncated": (((37, 53), (36, 300)), "noise"),
    "plus2_dropped": (((240, 320), (224, 224)), "noise"),
    "shift4_skipped": (((8, 12), (4, 6)), "checker"),
    "scale_swapped": (((37, 53), (36, 300)), "hramp"),
    # HSV: (size, step); the batch mistake at the cut of HSV_VIDEOS
    "h_not_wrapped": ((47, 45), 1),
    "round_dropped": ((47, 45), 2),
    "sdiv_from_diff": ((1, 300), 1),
    "step_rows_only": ((130, 127), 3),
    "prev_across_videos": ((47, 45), 1),
    "last_workgroup_dropped": ((47, 45), 1),
    # normalise: (affine, denom, (pad_t, pad_l))
    "zero_channel_not_zero": (False, 255.0, (0, 0)),
    "pad_normalised": (False, 255.0, (0, 0)),
    "affine_before_std": (True, 255.0, (2, 3)),
    "h2_pair_swapped": (False, 1.0, (0, 1)),
    "h2_lo_from_pixel0": (False, 255.0, (0, 1)),
    # pull copy: (workgroups, index into pull_units(workgroups), tail)
    "remainder_one_stride_late": (3, 2, 0),
    "tail_from_offset_0": (1, 1, 15),
    "last_unit_skipped": (16, 5, 1),
}
