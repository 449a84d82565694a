"""Cases, float64 references, restatements and the error bound of the per-instance tests of the two plain convolution
entry points, avs_conv2d_nhwc and avs_conv2d_nhwc_split (test_conv_f64_host.py on the host, test_gpu_conv_f64.py on
the device).  torch-CPU only: both build the same seeded cases from here.  EPS32, the rules, the fp32 bound's form, the
bf16 step and fmaf come from gemm_f64_inputs, which does the same for avs_gemm_nt.

``plan`` restates igemm_plan (csrc/igemm.hip) for stats = in_affine = tile_rows = affine = 0: (es, split, bn, spatial,
linear, rowb, pipe, wr, fastk, epi, tap), with few_f32, narrow, wide96, fast64_only and the tall rule, its thresholds
READ from the AVS_RULE lines.  ``tile_choice`` is the part of it that chooses the tile; with stats=True it is pinned by
the host test on the library's recorded answers (tests/golden/igemm_plan_host.json).

REACHABLE is the set of instance tuples (dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap) that igemm_lift
to igemm_lift_staging can launch for EPI_PLAIN, EPI_BRELU and EPI_ANY from these entry points: every tuple of the
product of the fields' values that ``unreachable`` gives no reason against (the reasons are the `if constexpr` gates
and the rules that feed them).  LEFT_OUT holds the reachable tuples no case is built for, each with its reason.  The
host test asserts that the plans of CASES are exactly REACHABLE minus LEFT_OUT.

AVS_F32_ACC64: ops.conv2d_raw passes the dtype code through and conv_geometry takes it (not with AVS_W_KSTEP32), so it
has cases - the grid below (every walk x both step lengths x the three planned epilogues; the kernel is the one
general-epilogue instance per walk and step) and the geometry family.

Two operand sets per case: "a" - N(0, 1), filters scaled by K^-0.5, the frames scaled in turn by FRAME_SCALES (1, 2^-10,
2^10; AVS_F16X2: 1, 2^-5, 2^7, which keeps |x|, |w| and the outputs far below 65504 / 4 and the typical value inside
fp16's normal range), so an output row carries its own frame's magnitude and a read across a frame boundary stands
out by orders of magnitude; "b" - small integers, exact in any summation order (``exact_headroom``), so the result has
to EQUAL the float64 convolution (rounded once for bf16).  The input is always generated as the WIDER tensor (all
channels of a channel-sliced input, the whole map of a cropped one), so that an ignored stride reads other numbers.

The 256-row tiles by rule need g_tall_min_tiles tall tiles (the shifted-row form exists only there: AVS_TILE_256 keeps
the classic walk).  No cheaper shape reaches these instances: the rule counts tiles, cout <= 64 already has the fewest
columns per tile, and cin is the smallest that the form's other conditions allow.  Their frames repeat a base of
TALL_PERIOD = 7 frames (a prime), built on the device by index: frames are independent, so the reference is 7 frames of
float64 and every output row is still compared.

The bound is per element, with S = |alpha| * (|x| conv |w|) + |bias| in float64 and e32 the largest error over the
output row (a pixel's cout values) of the same expression in fp32 on the CPU:
    AVS_F32        |got - ref| <= 4 * e32 + 8 * eps32 * S                   (gemm_f64_inputs.fp32_term)
    AVS_F32_ACC64  |got - ref| <= 8 * eps32 * S
    AVS_BF16       |got - ref| <= half a bf16 step of ref + the fp32 term
    AVS_F32_SPLIT  |got - restatement| <= the fp32 term, |restatement - ref| <= SPLIT_C * 2^-15 * S
    AVS_F16X2      |got - restatement| <= the fp32 term + 2^-21 |restatement| + 2^-25 (the output's own packing step),
                   |restatement - ref| <= F16X2_C * 2^-22 * S
(restatement: hi = bf16 / fp16 (x), lo = bf16 / fp16 (x - hi), ah*bh + ah*bl + al*bh in float64).  SPLIT_C and F16X2_C
are twice the largest ratio of the restatement over all cases and both operand sets, measured on the CPU against the
float64 reference (never against the kernel): *_MEASURED, recomputed by the host test."""
import collections
import functools
import itertools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gemm_f64_inputs import ACC64, BF16, EPS32, F32, RULES, SPLIT, _fma, bf16_half_step, fp32_term, read_rules  # noqa: F401
from f16x2_format import emu_pack, emu_unpack  # the AVS_F16X2 format restated in plain torch

F16X2 = 4                                             # AVS_F16X2 (avsum_hip.h)
DTYPES = (F32, BF16, ACC64, SPLIT, F16X2)
DTYPE_NAMES = {F32: "f32", BF16: "bf16", ACC64: "acc64", SPLIT: "split", F16X2: "f16x2"}
RELU = 1                                              # AVS_ACT_RELU
TILE_AUTO, TILE_128, TILE_256, GENERIC = 0, 1, 2, 4   # avs_conv_desc.variant: AVS_TILE_*, AVS_STAGING_GENERIC
W_ROWS, W_KSTEP32 = 0, 1
E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -6
TALL_PERIOD = 7
FRAME_SCALES = {False: (1.0, 2.0 ** -10, 2.0 ** 10), True: (1.0, 2.0 ** -5, 2.0 ** 7)}       # keyed by dtype == F16X2
SPLIT_C_MEASURED = 0.4969        # largest |restatement - ref| / (2^-15 * S) over every split case and both operand sets
F16X2_C_MEASURED = 0.5927        # largest |restatement - ref| / (2^-22 * S) over every f16x2 case and both operand sets
SPLIT_C = 2 * SPLIT_C_MEASURED
F16X2_C = 2 * F16X2_C_MEASURED
MISTAKES = ("pad_lr_reads_row", "pad_tb_reads_frame", "sh_sw_exchanged", "ph_pw_exchanged", "kw_major_taps",
            "last_step_dropped", "px_stride_ignored", "row_stride_ignored", "tile_seam", "second_dest_offset",
            "relu_cols_ignored", "alpha_after_bias", "relu_before_bias")
EPILOGUES = {                      # name: (bias given, activation, alpha)
    "plain": (False, 0, 1.0), "brelu": (True, RELU, 1.0), "bias": (True, 0, 1.0), "relu": (False, RELU, 1.0),
    "scaled": (True, 0, 0.125)}
ANY = ("bias", "relu", "scaled")   # the three that take EPI_ANY


def es_of(dtype):
    return 2 if dtype == BF16 else 4


# --------------------------------------------------------------------------- the plan, restated
def tile_choice(dtype, m, n, k, plain, brelu, tile_mode, stats=False, rules=None):
    """(bn, tiles_n, tall) as igemm_plan chooses them for batch = 1 and no BatchNorm form; ``stats``: the statistics
    epilogue (no few_f32, no bias + ReLU), which only the host test's pin on the recorded answers uses."""
    r = rules or RULES
    assert r["pipe3"] == 1
    es = es_of(dtype)
    brelu = brelu and not stats
    few_f32 = dtype == F32 and not stats and -(-m // 128) * -(-n // 128) < 256
    narrow = n <= 64 or dtype == ACC64 or few_f32
    bn = 64 if narrow else 128
    tiles_n = -(-n // bn)
    wide96 = False
    if dtype == F16X2 and not narrow and brelu and k * 4 >= r["tall_min_k_bytes"] and tile_mode in (TILE_AUTO, TILE_256):
        t96 = -(-n // 96)
        if t96 * 96 * 100 <= tiles_n * 128 * 85 and (tile_mode == TILE_256 or -(-m // 256) * t96 >= r["tall_min_tiles"]):
            wide96, bn, tiles_n = True, 96, t96
    can = dtype in (BF16, SPLIT, F16X2) and (plain or brelu) and k * es > 128
    tall = wide96 or (can and (tile_mode == TILE_256 or (tile_mode == TILE_AUTO and -(-m // 256) * tiles_n >= r["tall_min_tiles"]
                                                           and (narrow or k * es >= r["tall_min_k_bytes"]))))
    return bn, tiles_n, tall


def out_extent(h, w, kh, kw, sh, sw, ph, pw):
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def taps_ok(geometry, variant, strides):
    """igemm_taps_ok: the shapes the shifted-row form takes under bias + ReLU."""
    n, h, w, cin, kh, kw, sh, sw, ph, pw, cout = geometry
    x_img, x_row, x_px = strides
    ho, wo = out_extent(h, w, kh, kw, sh, sw, ph, pw)
    return ((variant & 3) != TILE_256 and 1 < kh * kw <= 32 and sh == 1 and sw == 1 and 2 * ph + 1 == kh and 2 * pw + 1 == kw and
            ho == h and wo == w and ph * w + pw <= 64 and x_px >= cin and x_row == w * x_px and x_img == h * w * x_px and
            cin % 16 == 0)


def plan(dtype, geometry, epilogue, variant=0, strides=None, rules=None):
    """(es, split, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap) of a plain convolution, as igemm_plan chooses
    them.  geometry = (n, h, w, cin, kh, kw, sh, sw, ph, pw, cout), epilogue = (bias given, act, alpha), strides =
    (x_img_stride, x_row_stride, x_px_stride) in elements (None: dense).  The buffer window is taken to hold (every
    case here is far below 2 GiB: asserted)."""
    r = rules or RULES
    n, h, w, cin, kh, kw, sh, sw, ph, pw, cout = geometry
    has_bias, act, alpha = epilogue
    x_img, x_row, x_px = strides or (h * w * cin, w * cin, cin)
    ho, wo = out_extent(h, w, kh, kw, sh, sw, ph, pw)
    es, m, k = es_of(dtype), n * ho * wo, kh * kw * cin
    split = {SPLIT: 1, F16X2: 2}.get(dtype, 0)
    plain = not has_bias and act == 0 and alpha == 1.0
    brelu = has_bias and act == RELU and alpha == 1.0
    bn, tiles_n, tall = tile_choice(dtype, m, cout, k, plain, brelu, variant & 3, False, r)
    spatial = not (ph == 0 and pw == 0 and (ho - 1) * sh + kh - 1 < h and (wo - 1) * sw + kw - 1 < w)
    linear = (not spatial and kw == 1 and k == cin and sh == 1 and sw == 1 and
              (ho * wo == 1 or (x_row == wo * x_px and x_img == ho * wo * x_px)))
    fast64_only = not (variant & GENERIC) and cin % (64 // es) == 0 and cin % (128 // es) != 0 and k // cin <= 32
    rowb = 64 if tall or fast64_only or k * es <= r["rowb_threshold_bytes"] else 128
    pipe = rowb == 64 and dtype != ACC64 and k * es > 2 * rowb
    wr = 4 if pipe and tall else 2
    assert ((256 // (ho * wo) + 2) * x_img + (kh + ph) * x_row + (kw + pw) * x_px + cin) * es < 2 ** 31
    bke = rowb // es
    fastk = dtype != ACC64 and not (variant & GENERIC) and cin % bke == 0 and k % bke == 0 and k // cin <= 32
    epi = "plain" if plain else "brelu" if brelu else "any"
    tap = (spatial and pipe and wr == 4 and fastk and split == 2 and epi == "brelu" and
           taps_ok(geometry, variant, (x_img, x_row, x_px)))
    return es, split, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap


def unreachable(dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap):
    """Why no call of the two entry points launches this instance, or None.  From igemm_plan's rules and the `if constexpr`
    gates of igemm_lift .. igemm_lift_staging."""
    if spatial and linear:
        return "the linear walk is the dense 1x1 / stride-1 input without padding"
    if bn == 96 and not (dtype == F16X2 and epi == "brelu" and wr == 4):
        return "96-wide tiles: the AVS_F16X2 bias + ReLU form on the 256-row tiles only (igemm_lift_form)"
    if dtype == ACC64 and (bn != 64 or pipe or wr != 2 or fastk):
        return "AVS_F32_ACC64 is narrow by rule, on the classic 128-row walk with the generic staging (igemm_lift_tile)"
    if dtype == F16X2 and epi == "any":
        return "AVS_F16X2 takes the compile-time epilogues only (igemm_plan refuses the others)"
    if pipe and rowb != 64:
        return "the 3-buffer pipeline exists on 64-byte steps only"
    if wr == 4 and not pipe:
        return "the 256-row tiles are built on the pipeline"
    if wr == 4 and dtype not in (BF16, SPLIT, F16X2):
        return "256-row tiles: bf16, fp32-split and f16x2 only"
    if wr == 4 and epi == "any":
        return "256-row tiles: the compile-time epilogues only"
    if tap and not (dtype == F16X2 and epi == "brelu" and spatial and pipe and wr == 4 and fastk and rowb == 64):
        return "the shifted-row form: AVS_F16X2 bias + ReLU on the pipelined 256-row tiles with the scalar tap walk"
    return None


FIELDS = (DTYPES, (64, 96, 128), (False, True), (False, True), (64, 128), (False, True), (2, 4), (False, True),
          ("plain", "brelu", "any"), (False, True))
REACHABLE = frozenset(t for t in itertools.product(*FIELDS) if unreachable(*t) is None)


def left_out(dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap):
    """Why CASES has no case for this reachable tuple, or None."""
    if dtype == F32 and bn == 128 and (spatial, linear, rowb, pipe, fastk, epi) != (False, True, 64, False, True, "brelu"):
        return ("AVS_F32 leaves few_f32 from 256 tiles of 128 x 128 on (a 2048 x 2048 output per case): the one case "
                "f32-wide-m2048-n2048-brelu holds the 128-wide tile; its staging forms are the 64-wide tile's code")
    return None


LEFT_OUT = {t: left_out(*t) for t in REACHABLE if left_out(*t)}


# --------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "name dtype n h w cin cout kh kw sh sw ph pw epi variant w_layout xwide xc0 crop "
                                      "ypad yc0 period split")


def _case(name, dtype, hw, cin, cout, k=(1, 1), s=(1, 1), p=(0, 0), epi="plain", n=3, variant=0, w_layout=0, xwide=None, xc0=0,
          crop=None, ypad=0, yc0=0, period=None, split=None):
    """crop = (H, W, y0, x0): the [h, w] window at (y0, x0) of an H x W map; xwide / xc0: channels [xc0, xc0 + cin) of an
    xwide-channel tensor; ypad / yc0: columns [yc0, yc0 + cout) of pixels cout + ypad wide; split = (n_split,
    relu_cols, pad and column offset of the second destination)."""
    h, w = hw
    assert h != w and epi in EPILOGUES
    return Case(f"{DTYPE_NAMES[dtype]}-{name}-{epi}", dtype, n, h, w, cin, cout, k[0], k[1], s[0], s[1], p[0], p[1], epi, variant,
                w_layout, xwide or cin, xc0, crop, ypad, yc0, period, split)


def geometry(case):
    return (case.n, case.h, case.w, case.cin, case.kh, case.kw, case.sh, case.sw, case.ph, case.pw, case.cout)


def strides(case):
    """(x_img_stride, x_row_stride, x_px_stride, offset of the first element) of the input view, in elements."""
    hf, wf, y0, x0 = case.crop or (case.h, case.w, 0, 0)
    return hf * wf * case.xwide, wf * case.xwide, case.xwide, (y0 * wf + x0) * case.xwide + case.xc0


def extent(case):
    return out_extent(case.h, case.w, case.kh, case.kw, case.sh, case.sw, case.ph, case.pw)


def case_plan(case, rules=None):
    return (case.dtype,) + plan(case.dtype, geometry(case), EPILOGUES[case.epi], case.variant, strides(case)[:3], rules)


def instance(case, rules=None):
    """The case's tuple in REACHABLE's fields."""
    dtype, es, split, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap = case_plan(case, rules)
    return dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap


def frames(case):
    """Frames of the input (and of the reference) that are distinct: the base of a periodic case, else n."""
    return min(case.n, case.period) if case.period else case.n


MAPS = ((9, 7), (11, 9), (13, 11))


def _grid_case(t, i):
    """A smallest case that the rules put on the instance ``t`` (None: tap, which only the tall family reaches)."""
    dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap = t
    if tap:
        return None
    e = 4 // es_of(dtype)                       # elements per 4 bytes: cin below is in fp32 elements
    wide96 = bn == 96
    generic = False
    if rowb == 64 and not pipe:                 # at most 128 bytes: one or two taps
        cin, k = (16 if fastk else 8), ((1, 2) if spatial else (1, 1))
    elif rowb == 64:                            # pipelined: more than 128 bytes, at most the threshold (or fast64_only)
        if fastk:
            cin = 32 if wide96 else 16
        else:
            generic = i % 2 == 0
            cin = (32 if wide96 else 16) if generic else 40
        k = (1, 1) if linear else (3, 3)
        if linear:
            cin = {16: 48, 32: 256, 40: 264 if wide96 else 40}[cin]
    else:                                       # 128-byte steps: above the threshold, not fast64_only
        if fastk:
            cin = 544 if linear else 64
        else:
            generic = i % 2 == 0
            cin = (544 if linear else 64) if generic else (520 if linear else 72)
        k = (1, 1) if linear else (3, 3)
    if linear:
        s, p = (1, 1), (0, 0)
    elif spatial:
        s, p = (1, 1), ((0, 1) if k == (1, 2) else (1, 1))
    else:
        s, p = ((2, 1) if k == (1, 1) else (1, 1)), (0, 0)
    cout = {64: 40, 96: 72, 128: 104 if dtype == F16X2 else 72}[bn]
    if dtype == F32 and bn == 128:
        return _case("wide-m2048-n2048", F32, (32, 16), 16, 2048, epi="brelu", n=4)
    name = (f"grid-{'sp' if spatial else 'lin' if linear else 'ns'}-{k[0]}x{k[1]}-c{cin * e}-n{cout}-r{rowb}"
            f"{'-fk' if fastk else '-gen' if generic else '-odd'}{'-t256' if wr == 4 else ''}")
    return _case(name, dtype, MAPS[i % 3], cin * e, cout, k, s, p, ANY[i % 3] if epi == "any" else epi,
                 variant=(GENERIC if generic else 0) | (TILE_256 if wr == 4 else 0), w_layout=W_KSTEP32 if i % 4 == 1 and
                 dtype != ACC64 and (k[0] * k[1] * cin) % 16 == 0 else W_ROWS)


GEOMETRIES = (       # name, map, kernel, stride, pad, extra
    ("1x1", (9, 7), (1, 1), (1, 1), (0, 0), {}),
    ("1x1-s21", (11, 9), (1, 1), (2, 1), (0, 0), {}),
    ("1x1-chslice", (9, 7), (1, 1), (1, 1), (0, 0), dict(xpad=24, xc0=8)),
    ("1x1-crop", (9, 7), (1, 1), (1, 1), (0, 0), dict(crop=(12, 11, 2, 3))),
    ("3x3-p1", (9, 7), (3, 3), (1, 1), (1, 1), {}),
    ("3x3-s2-p1", (13, 11), (3, 3), (2, 2), (1, 1), {}),
    ("3x3-s12-p10", (11, 9), (3, 3), (1, 2), (1, 0), {}),
    ("3x3-p0", (9, 7), (3, 3), (1, 1), (0, 0), {}),
    ("3x3-p2", (9, 7), (3, 3), (1, 1), (2, 2), {}),
    ("1x1-crop-s12", (9, 7), (1, 1), (1, 2), (0, 0), dict(crop=(10, 9, 1, 1))),
    ("3x3-p3", (9, 7), (3, 3), (1, 1), (3, 3), dict(epi="brelu")),        # windows that lie wholly in the padding: output = epilogue of 0
    ("3x3-p1-chslice-crop", (9, 7), (3, 3), (1, 1), (1, 1), dict(xpad=16, xc0=8, crop=(11, 10, 1, 2))),
    ("1x7-p03", (9, 7), (1, 7), (1, 1), (0, 3), {}),
    ("7x1-p30", (9, 7), (7, 1), (1, 1), (3, 0), {}),
    ("5x5-s2-p2", (13, 11), (5, 5), (2, 2), (2, 2), {}),
    ("2x2-s2", (12, 10), (2, 2), (2, 2), (0, 0), {}),
)


def _build_cases():
    cases = []
    # 1. one smallest case per reachable instance (but the shifted-row form: family 6)
    seen = set()
    for i, t in enumerate(sorted(REACHABLE)):
        if t in LEFT_OUT:
            continue
        c = _grid_case(t, i)
        if c is not None and c.name not in seen:
            seen.add(c.name)
            cases.append(c)
    for dtype in DTYPES:
        e = 4 // es_of(dtype)
        epis = ("plain", "brelu") if dtype == F16X2 else tuple(EPILOGUES)
        # 2. the geometries, the epilogues in turn, on a destination that is a channel slice (y_px_stride = cout + 8)
        for i, (name, hw, k, s, p, extra) in enumerate(GEOMETRIES):
            cin = 24 * e if dtype != F16X2 else 24
            cases.append(_case(name, dtype, hw, cin, 40, k, s, p, extra.get("epi", epis[i % len(epis)]), xwide=cin + extra.get("xpad", 0) * e,
                               xc0=extra.get("xc0", 0) * e, crop=extra.get("crop"), ypad=8 if i % 2 else 0, yc0=8 if i % 4 == 1 else 0))
        cases.append(_case("7x7-s2-p3-c16", dtype, (13, 11), 16 * e if dtype != F16X2 else 16, 40, (7, 7), (2, 2), (3, 3),
                           epis[1]))                                            # 49 taps: the general gather
        # 3. cin either side of one reduction step and of fast64_only, with the tap walk and with STAGING_GENERIC
        for j, cf in enumerate((8, 16, 24, 32, 48, 96)):
            for generic in (0, GENERIC):
                cases.append(_case(f"3x3-p1-c{cf * e}{'-gen' if generic else ''}", dtype, MAPS[j % 3], cf * e, 40, (3, 3), (1, 1), (1, 1),
                                   epis[(j + (generic > 0)) % len(epis)], variant=generic))
        #    ... and STAGING_GENERIC on the two shortest classes (the instance is the one the misaligned cin reaches: the
        #    flag alone differs): K below one step, and K of 128 bytes (no pipeline)
        cases.append(_case(f"1x1-c{8 * e}-gen", dtype, (9, 7), 8 * e, 40, epi=epis[0], variant=GENERIC))
        cases.append(_case(f"1x2-p01-c{16 * e}-gen", dtype, (11, 9), 16 * e, 40, (1, 2), (1, 1), (0, 1), epis[1], variant=GENERIC))
        # 4. tiles: cout of 8 .. 136 (bf16: the 16-byte store with ypad = 8 / 0 and its scalar fallback with ypad = 3 or an
        #    odd column offset), the row counts either side of a tile (n * Ho * Wo with one frame), the tile variants and
        #    both weight layouts
        odd = 0 if dtype == F16X2 else 3
        for j, cout in enumerate((8, 64, 72, 128, 136)):
            cases.append(_case(f"3x3-p1-n{cout}", dtype, (9, 7), 16 * e, cout, (3, 3), (1, 1), (1, 1), epis[j % len(epis)],
                               ypad=(0, 8, odd)[j % 3], yc0=(0, 8, 1 if odd else 0)[j % 3]))
        for cout in () if dtype == F16X2 else (40, 136):   # a 16-byte row stride at a column offset that is not 16 bytes; an odd row stride
            cases.append(_case(f"3x3-p1-n{cout}-yc3", dtype, (9, 7), 16 * e, cout, (3, 3), (1, 1), (1, 1), epis[cout % 5], ypad=8, yc0=3))
            cases.append(_case(f"3x3-p1-n{cout}-odd-ldc", dtype, (9, 7), 16 * e, cout, (3, 3), (1, 1), (1, 1), epis[cout % 3], ypad=3, yc0=2))
        for j, (rows, hw) in enumerate(((127, (127, 1)), (128, (16, 8)), (129, (43, 3)), (255, (17, 15)), (256, (32, 8)),
                                        (257, (257, 1)))):
            cases.append(_case(f"1x1-rows{rows}", dtype, hw, 16 * e, 72, epi=epis[j % len(epis)], n=1))
            cases.append(_case(f"3x3-p1-rows{rows}", dtype, hw, 16 * e, 40, (3, 3), (1, 1), (1, 1), epis[(j + 1) % len(epis)], n=1,
                               variant=(TILE_AUTO, TILE_128, TILE_256)[j % 3]))
        for variant, tag in ((TILE_AUTO, "auto"), (TILE_128, "t128"), (TILE_256, "t256")):
            for layout in (W_ROWS,) if dtype == ACC64 else (W_ROWS, W_KSTEP32):
                cases.append(_case(f"3x3-s2-p1-c32-{tag}-{'kstep' if layout else 'rows'}", dtype, (13, 11), 32 * e, 72, (3, 3), (2, 2),
                                   (1, 1), epis[(variant + layout) % 2], variant=variant, w_layout=layout))
        # 5. every epilogue on one asymmetric shape with a row and a column tail, into a channel slice
        for epi in epis:
            cases.append(_case("epilogue-3x3-s12", dtype, (11, 9), 16 * e, 72, (3, 3), (1, 2), (1, 0), epi, ypad=16, yc0=8))
    # 6. tall by rule (AVS_TILE_AUTO): g_tall_min_tiles tall tiles on 9 x 7 maps, one frame past them, so that the tiles
    #    straddle the frames at changing offsets (256 = 4 * 63 + 4).  The shifted-row form: "same" filters on 64-, 96- and
    #    128-wide tiles at the smallest cin that is a multiple of 16 with K * 4 >= g_tall_min_k_bytes.  No cheaper shape
    #    reaches these instances: the rule counts tiles
    min_tiles, min_k = RULES["tall_min_tiles"], RULES["tall_min_k_bytes"]
    nframes = lambda tiles_n: -(-(-(-min_tiles // tiles_n) * 256) // 63) + 1
    for k, p in (((3, 3), (1, 1)), ((1, 7), (0, 3)), ((7, 1), (3, 0))):
        cin = -(-min_k // (4 * k[0] * k[1] * 16)) * 16
        for cout, tiles_n in ((8, 1), (96, 1), (136, 2), (104, 1)):
            cases.append(_case(f"tall-{k[0]}x{k[1]}-c{cin}-n{cout}", F16X2, (9, 7), cin, cout, k, (1, 1), p, "brelu", n=nframes(tiles_n),
                               w_layout=W_KSTEP32 if cout == 96 else W_ROWS, period=TALL_PERIOD))
    cases.append(_case("tall-3x3-c32-n8-chslice", F16X2, (9, 7), 32, 8, (3, 3), (1, 1), (1, 1), "brelu", n=nframes(1), xwide=56, xc0=16,
                       ypad=8, period=TALL_PERIOD))
    for dtype, cin in ((BF16, 32), (SPLIT, 16), (F16X2, 16)):       # the classic walk on 256-row tiles by rule
        cases.append(_case("tall-3x3-s1-p1-n8", dtype, (9, 7), cin, 8, (3, 3), (1, 1), (1, 1), "plain", n=nframes(1), ypad=8,
                           period=TALL_PERIOD))
    # 7. avs_conv2d_nhwc_split: n_split inside the first column tile, on a tile seam and in the last tile; relu_cols of 0,
    #    of n_split and between the two; both destinations slices of wider buffers
    for j, (cout, n_split, between) in enumerate(((200, 40, 16), (200, 128, 64), (200, 168, 80), (72, 8, 40))):
        for relu_cols in (0, n_split, between):
            cases.append(_case(f"split{n_split}of{cout}-relu{relu_cols}", F16X2, (9, 7), 40, cout, epi="brelu", ypad=16, yc0=8,
                               split=(n_split, relu_cols, 8 + 8 * (j % 2), 8)))
        cases.append(_case(f"split{n_split}of{cout}", F16X2, (9, 7), 40, cout, epi="plain", ypad=16, yc0=8, split=(n_split, 0, 8, 0)))
    # 8. n = 0: AVS_OK and nothing written
    for dtype in DTYPES:
        cases.append(_case("n0", dtype, (9, 7), 16 * (4 // es_of(dtype)), 40, (3, 3), (1, 1), (1, 1), "brelu", n=0, ypad=8))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(cases)


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# --------------------------------------------------------------------------- operands
def _tdt(case):
    return torch.bfloat16 if case.dtype == BF16 else torch.float32


def top_of(case):
    return 4 if case.dtype == BF16 else 8


@functools.lru_cache(maxsize=16)
def operands(case, which):
    """The operand set ``which`` ("a" random, "b" small integers) of a case.  x_buf [frames, H, W, xwide] is the WHOLE
    tensor the input is a view of and w_buf [cout, K] the filters in (kh, kw, cin) order, both as the entry point is
    given them (fp32 values, bf16-representable for bf16; AVS_F16X2: the packed images); xv / wv hold the VALUES (for
    AVS_F16X2 what the packed images unpack to); x = the view [frames, h, w, cin] of xv.  Nothing here is modified by a
    test."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{which}".encode()))
    nf = max(1, frames(case))
    hf, wf, y0, x0 = case.crop or (case.h, case.w, 0, 0)
    k = case.kh * case.kw * case.cin
    has_bias, act, alpha = EPILOGUES[case.epi]
    top = top_of(case)
    if which == "a":
        scale = torch.tensor(FRAME_SCALES[case.dtype == F16X2])[torch.arange(nf) % 3].view(nf, 1, 1, 1)
        xv = torch.randn(nf, hf, wf, case.xwide, generator=g) * scale
        wv = torch.randn(case.cout, k, generator=g) * k ** -0.5
        # of the size of the middle frames' products and of either sign: the ReLU clips about half of their outputs, and
        # the orders of alpha, bias and ReLU all give different results
        bias = torch.randn(case.cout, generator=g) * abs(alpha) if has_bias else None
    else:
        xv = torch.randint(-top, top + 1, (nf, hf, wf, case.xwide), generator=g).float()
        wv = torch.randint(-top, top + 1, (case.cout, k), generator=g).float()
        bias = torch.randint(-2 * top, 2 * top + 1, (case.cout,), generator=g).float() if has_bias else None
    if case.dtype == F16X2:
        x_buf, w_buf = emu_pack(xv), emu_pack(wv)
        xv, wv = emu_unpack(x_buf), emu_unpack(w_buf)
    else:
        xv, wv = xv.to(_tdt(case)).float(), wv.to(_tdt(case)).float()
        x_buf, w_buf = xv, wv
    x = xv[:, y0:y0 + case.h, x0:x0 + case.w, case.xc0:case.xc0 + case.cin]
    return SimpleNamespace(x_buf=x_buf, w_buf=w_buf, xv=xv, wv=wv, x=x, bias=bias)


def exact_headroom(case):
    """(largest possible |partial sum| of operand set "b" in units of its step, largest |operand|): the first below 2^24
    (AVS_F16X2: also the sum itself below 65504, where its hi | lo image is exact) makes every fp32 partial sum exact
    in any order; the second below 2^8 makes the operands exact in bf16 and fp16, so there are no lo halves."""
    has_bias, act, alpha = EPILOGUES[case.epi]
    top = top_of(case)
    step = min(1.0, abs(alpha))
    return (abs(alpha) * case.kh * case.kw * case.cin * top * top + (2 * top if has_bias else 0)) / step, top


# --------------------------------------------------------------------------- reference, restatement, bound
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _conv(case, x, w):
    """F.conv2d of the NHWC x [f, h, w, cin] with the filters w [cout, K]: [f * Ho * Wo, cout]."""
    w4 = w.reshape(case.cout, case.kh, case.kw, case.cin).permute(0, 3, 1, 2)
    y = F.conv2d(_nchw(x), w4, None, (case.sh, case.sw), (case.ph, case.pw))
    return y.permute(0, 2, 3, 1).reshape(-1, case.cout)


def _epilogue(case, acc, bias, dtype):
    has_bias, act, alpha = EPILOGUES[case.epi]
    b = bias.to(dtype) if has_bias else torch.zeros((), dtype=dtype)
    return acc * alpha + b


def _relu_mask(case, mistake=None):
    """Columns that the ReLU applies to: all, or those below relu_cols (> 0) of avs_conv2d_nhwc_split."""
    cols = torch.ones(case.cout, dtype=torch.bool)
    if case.split and case.split[1] > 0 and mistake != "relu_cols_ignored":
        cols = torch.arange(case.cout) < case.split[1]
    return cols


def _relu(case, v, mistake=None):
    if EPILOGUES[case.epi][1] != RELU:
        return v
    return torch.where(_relu_mask(case, mistake) & (v < 0), torch.zeros_like(v), v)


def reference(case, which):
    """float64 act(alpha * conv(x, w) + bias) on the operand values the kernel is given: [frames * Ho * Wo, cout]."""
    o = operands(case, which)
    return _relu(case, _epilogue(case, _conv(case, o.x.double(), o.wv.double()), o.bias, torch.float64))


def magnitude(case, which):
    """S = |alpha| * (|x| conv |w|) + |bias| in float64."""
    o = operands(case, which)
    has_bias, act, alpha = EPILOGUES[case.epi]
    s = abs(alpha) * _conv(case, o.x.double().abs(), o.wv.double().abs())
    return s + o.bias.double().abs() if has_bias else s


def explicit_reference(case, which):
    """The same as ``reference`` by an explicit loop over output pixels and taps (the host test compares the two)."""
    o = operands(case, which)
    ho, wo = extent(case)
    x, w4 = o.x.double(), o.wv.double().reshape(case.cout, case.kh, case.kw, case.cin)
    acc = torch.zeros(x.shape[0], ho, wo, case.cout, dtype=torch.float64)
    for oy in range(ho):
        for ox in range(wo):
            for i in range(case.kh):
                for j in range(case.kw):
                    iy, ix = oy * case.sh - case.ph + i, ox * case.sw - case.pw + j
                    if 0 <= iy < case.h and 0 <= ix < case.w:
                        acc[:, oy, ox] += x[:, iy, ix] @ w4[:, i, j].t()
    return _relu(case, _epilogue(case, acc.reshape(-1, case.cout), o.bias, torch.float64))


def leaves(case):
    """(a tap leaves the image to the left or right, to the top or bottom)."""
    ho, wo = extent(case)
    return (case.pw > 0 or (wo - 1) * case.sw - case.pw + case.kw - 1 >= case.w,
            case.ph > 0 or (ho - 1) * case.sh - case.ph + case.kh - 1 >= case.h)


def applies(case, mistake):
    """Does the planted mistake change what this case computes (by more than a rounding)?"""
    if case.n == 0:
        return False
    dtype, es, split, bn, spatial, linear, rowb = case_plan(case)[:7]
    has_bias, act, alpha = EPILOGUES[case.epi]
    x_img, x_row, x_px, _ = strides(case)
    k = case.kh * case.kw * case.cin
    lr, tb = leaves(case)
    # (above the first frame and below the last lies no other row unless the input is a window of a larger map)
    return {"pad_lr_reads_row": lr, "pad_tb_reads_frame": tb and (frames(case) > 1 or case.crop is not None),
            "sh_sw_exchanged": case.sh != case.sw, "ph_pw_exchanged": case.ph != case.pw,
            "kw_major_taps": case.kh > 1 and case.kw > 1,
            "last_step_dropped": k % (rowb // es) != 0,
            "px_stride_ignored": x_px != case.cin and case.h * case.w > 1,
            "row_stride_ignored": x_row != case.w * x_px and case.h > 1,
            "tile_seam": case.cout > bn,
            "second_dest_offset": case.split is not None,
            "relu_cols_ignored": case.split is not None and act == RELU and 0 < case.split[1] < case.cout,
            "alpha_after_bias": alpha != 1.0 and has_bias,
            "relu_before_bias": act == RELU and has_bias}[mistake]


def im2col(case, o, mistake=None):
    """A [frames * Ho * Wo, K] fp32 in (kh, kw, cin) order, gathered from the flat input by the kernel's own address
    arithmetic: frame * x_img_stride + iy * x_row_stride + ix * x_px_stride + channel for the taps inside the image, zero
    for the others.  ``mistake`` changes the bounds tests, the tap coordinates or the strides; an address outside the
    tensor reads zero."""
    x_img, x_row, x_px, off = strides(case)
    ho, wo = extent(case)
    sh, sw, ph, pw = case.sh, case.sw, case.ph, case.pw
    if mistake == "sh_sw_exchanged":
        sh, sw = sw, sh
    if mistake == "ph_pw_exchanged":
        ph, pw = pw, ph
    if mistake == "px_stride_ignored":
        x_px = case.cin
    if mistake == "row_stride_ignored":
        x_row = case.w * x_px
    flat = o.xv.reshape(-1)
    nf = o.xv.shape[0]
    f = torch.arange(nf).view(nf, 1, 1, 1, 1, 1)
    oy, ox = torch.arange(ho).view(1, ho, 1, 1, 1, 1), torch.arange(wo).view(1, 1, wo, 1, 1, 1)
    i, j = torch.arange(case.kh).view(1, 1, 1, case.kh, 1, 1), torch.arange(case.kw).view(1, 1, 1, 1, case.kw, 1)
    c = torch.arange(case.cin).view(1, 1, 1, 1, 1, case.cin)
    iy, ix = oy * sh - ph + i, ox * sw - pw + j
    ok_y = (iy >= 0) & (iy < case.h) if mistake != "pad_tb_reads_frame" else torch.ones_like(iy, dtype=torch.bool)
    ok_x = (ix >= 0) & (ix < case.w) if mistake != "pad_lr_reads_row" else torch.ones_like(ix, dtype=torch.bool)
    addr = off + f * x_img + iy * x_row + ix * x_px + c
    ok = ok_y & ok_x & (addr >= 0) & (addr < flat.numel())
    a = torch.where(ok, flat[addr.clamp(0, flat.numel() - 1)], torch.zeros(()))
    if mistake == "kw_major_taps":               # the t-th tap of the walk is (t % kh, t / kh), the filters stay (kh, kw)
        a = a.transpose(3, 4)
    return a.reshape(nf * ho * wo, -1)


def restatement(case, which, mistake=None):
    """The case in the kernel's order of operations, as float64 [frames * Ho * Wo, cout] holding what the kernel should
    store (AVS_F16X2: before the output's own packing): the im2col rows times the filters - fp32 products summed in fp32
    (AVS_F32, AVS_BF16), the fp32 sums of the reduction steps summed in float64 (AVS_F32_ACC64), ah*bh + ah*bl + al*bh in
    float64 with bf16 / fp16 halves (AVS_F32_SPLIT / AVS_F16X2); then fmaf(acc, alpha, bias), [one bf16 rounding,] the ReLU.
    ``mistake``: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    o = operands(case, which)
    dtype, es, split, bn, spatial, linear, rowb = case_plan(case)[:7]
    has_bias, act, alpha = EPILOGUES[case.epi]
    a, bt = im2col(case, o, mistake), o.wv.t()
    k = a.shape[1]
    if mistake == "last_step_dropped":
        a = a.clone()
        a[:, k // (rowb // es) * (rowb // es):] = 0
    if split:
        half = (lambda t: t.bfloat16().double()) if split == 1 else (lambda t: t.half().double())
        ah, bh = half(a), half(bt)
        al, bl = half(a.double() - ah), half(bt.double() - bh)
        acc = ah @ bh + ah @ bl + al @ bh
    elif dtype == ACC64:
        acc = torch.zeros(a.shape[0], case.cout, dtype=torch.float64)
        step = rowb // es
        for k0 in range(0, k, step):
            acc += (a[:, k0:k0 + step] @ bt[k0:k0 + step]).double()
    else:
        acc = a @ bt
    wide = torch.float64 if split else torch.float32
    bias = o.bias.to(wide) if has_bias else torch.zeros((), dtype=wide)
    relu = lambda x: _relu(case, x, mistake)
    if mistake == "alpha_after_bias":
        v = (acc + bias) * alpha
    elif mistake == "relu_before_bias":
        v, relu = _relu(case, acc * alpha, mistake) + bias, (lambda x: x)
    elif case.epi == "plain":
        v = acc
    elif split:
        v = acc * alpha + bias
    elif dtype == ACC64:
        v = (acc * alpha).float() + bias
    else:
        v = _fma(acc, alpha, bias)
    if not split:
        v = v.float()
    if dtype == BF16:
        v = v.bfloat16()
    v = relu(v).double()
    if mistake == "tile_seam":
        v[:, bn] = v[:, 0]
    if mistake == "second_dest_offset":          # the second destination's columns taken from the first's
        n_split = case.split[0]
        width = min(case.cout - n_split, n_split)
        v[:, n_split:n_split + width] = v[:, :width]
    return v


def fp32_yardstick(case, which):
    """The same expression in fp32 on the CPU (for every dtype: plain fp32 sums, no bf16 rounding, no split)."""
    o = operands(case, which)
    has_bias, act, alpha = EPILOGUES[case.epi]
    acc = _conv(case, o.x.contiguous(), o.wv)
    v = acc if case.epi == "plain" else _fma(acc, alpha, o.bias if has_bias else torch.zeros(()))
    return _relu(case, v).double()


def pack_step(target):
    """The output's own AVS_F16X2 packing step: 2^-21 relative, 2^-25 absolute (test_pack_unpack_bit_exact)."""
    return target.abs() * 2.0 ** -21 + 2.0 ** -25


@functools.lru_cache(maxsize=8)
def bundle(case, which):
    """(ref, target, bound, e32 per row, S) of a case and operand set, float64 [frames * Ho * Wo, cout], computed once and
    shared; a result must lie within ``bound`` of ``target``: the reference, for AVS_F32_SPLIT and AVS_F16X2 their
    restatement."""
    ref, s = reference(case, which), magnitude(case, which)
    e32 = (fp32_yardstick(case, which) - ref).abs().amax(-1, keepdim=True) if ref.numel() else ref.new_zeros(ref.shape[0], 1)
    term = fp32_term(e32, s)
    if case.dtype == ACC64:
        return ref, ref, 8.0 * EPS32 * s, e32, s
    if case.dtype == BF16:
        return ref, ref, bf16_half_step(ref) + term, e32, s
    if case.dtype == SPLIT:
        return ref, restatement(case, which), term, e32, s
    if case.dtype == F16X2:
        target = restatement(case, which)
        return ref, target, term + pack_step(target), e32, s
    return ref, ref, term, e32, s


def restatement_unit(case):
    """The unit of |restatement - ref| / S: the dropped lo*lo product of bf16 (2^-15) or fp16 (2^-22) halves."""
    return {SPLIT: 2.0 ** -15, F16X2: 2.0 ** -22}[case.dtype]


def restatement_ratio(case, which):
    """max |restatement - ref| / (unit * S) of a split or f16x2 case (0 / 0 = 0)."""
    ref, s = reference(case, which), magnitude(case, which)
    if not ref.numel():
        return 0.0
    d = (restatement(case, which) - ref).abs()
    return torch.where(d == 0, d, d / (restatement_unit(case) * s)).max().item()


def exact_result(case, which="b"):
    """What operand set "b" has to give, bit for bit: the float64 convolution, rounded once to bf16 for AVS_BF16."""
    ref = reference(case, which)
    if case.dtype == BF16:
        return ref.float().bfloat16().double()        # the ReLU commutes with the rounding (monotone, keeps the sign)
    assert torch.equal(ref.float().double(), ref)
    return ref


# --------------------------------------------------------------------------- refusals
def desc_fields(dtype=F32, n=3, h=9, w=7, cin=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, ho=None, wo=None, cout=40,
                w_row_stride=None, y_px_stride=None, act=0, alpha=1.0, w_layout=0, variant=0):
    """The 24 fields of avs_conv_desc for a dense NHWC input, in _abi.ConvDesc's order."""
    eh, ew = out_extent(h, w, kh, kw, sh, sw, ph, pw)
    return [dtype, n, h, w, cin, kh, kw, sh, sw, ph, pw, eh if ho is None else ho, ew if wo is None else wo, cout, h * w * cin,
            w * cin, cin, kh * kw * cin if w_row_stride is None else w_row_stride, cout if y_px_stride is None else y_px_stride,
            act, alpha, w_layout, variant, 0]


def refusals():
    """[(label, status, has bias, changes to a valid 3 x 9 x 7 x 16 -> 40 fp32 3x3 call)]: conv_geometry's refusals and
    AVS_F16X2's epilogues.  conv_geometry comes before every check of the operands, so the status is the same with null
    operands."""
    out = [("ho-beyond-padded-input", E_SHAPE, False, dict(ho=10)), ("wo-beyond-padded-input", E_SHAPE, False, dict(wo=8)),
           ("w-row-stride<k", E_SHAPE, False, dict(w_row_stride=9 * 16 - 4)), ("variant-16", E_ARG, False, dict(variant=16)),
           ("w-layout-2", E_ARG, False, dict(w_layout=2)),
           ("kstep32-k-not-64-bytes", E_UNSUPPORTED, False, dict(cin=8, w_layout=W_KSTEP32)),
           ("kstep32-k-not-64-bytes-bf16", E_UNSUPPORTED, False, dict(dtype=BF16, cin=24, w_layout=W_KSTEP32)),
           ("kstep32-acc64", E_UNSUPPORTED, False, dict(dtype=ACC64, w_layout=W_KSTEP32))]
    for label, bias, act, alpha in (("bias-only", True, 0, 1.0), ("relu-only", False, RELU, 1.0), ("scaled", True, 0, 0.125)):
        out.append((f"f16x2-{label}", E_UNSUPPORTED, bias, dict(dtype=F16X2, act=act, alpha=alpha)))
    return out
