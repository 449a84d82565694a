"""Cases, float64 references, fp32 restatements, bounds and planted mistakes of the per-instance tests of the four
BatchNorm convolution entry points - avs_conv2d_nhwc_bnstats, avs_conv2d_nhwc_bnstats_xin, avs_conv2d_nhwc_bnlocal and
avs_conv2d_nhwc_affine (test_bnconv_f64_host.py on the host, test_gpu_bnconv_f64.py on the device).  torch-CPU only: both
build the same seeded cases from here.  The plain-convolution machinery (the case tuple, im2col by the kernel's address
arithmetic, the per-element bounds of the raw output, the rules' thresholds) is conv_f64_inputs', the BatchNorm
parameters, the regimes and the per-(group, channel) bound are convbn_f64_inputs', the AVS_F16P8 format is
test_gpu_f16p8's restatement.

``plan`` restates igemm_plan (csrc/igemm.hip) for stats, in_affine, tile_rows (bnlocal_plan), affine and an AVS_F16P8
input; the thresholds are READ from the source (``read_rules``: the AVS_RULE lines, AVS_RULE_AFFINE_128_MAX_K and the
constants of igemm_params.h).  The instance tuple is FIELD_NAMES; REACHABLE is every tuple of the fields' product that
``unreachable`` gives no reason against: AVS_F16X2 under the three epilogues, AVS_F32 and AVS_F32_SPLIT under EPI_STATS
(exact mode), the two instances of igemm_h2_local224_kernel.  LEFT_OUT holds the reachable tuples no case is built for,
each with its reason.  The host test asserts that the plans of CASES are exactly REACHABLE minus LEFT_OUT and pins the
restatement on the library's two host queries.

Operands: what the format keeps (emu_unpack(emu_pack(.)), AVS_F16P8: emu_p8_unpack(emu_p8_pack(.))), the frames scaled
in turn by FRAME_SCALES[True] (1, 2^-5, 2^7), so that a row read from the neighbouring group stands out.  Regimes as
in convbn_f64_inputs: "normal"; "mean40" (|mean| / std about 40 in channels MEAN40_CH_2D of every group, through a
constant input column; its frames all have magnitude 1, the three magnitudes would be a group's spread); "const" (channel CONST_CH reads the centre tap of a column
that is constant in the frames of one group: variance exactly 0, the output is beta).

Reference: the float64 convolution by an explicit loop over taps (``tap_conv``) on the input VIEW; per-group mean and
centred variance, scale = gamma / sqrt(var + eps), shift = beta - mean * scale; relu(acc * scale + shift + residual')
without intermediate rounding.  With an input affine the input is relu(x * in_scale + in_shift) BEFORE the padding.

Restatement: fp32 on the CPU in the kernels' order - the im2col rows (gathered from the FLAT buffer by the strides) times
the filters in fp32 (AVS_F32_SPLIT, AVS_F16X2: the three products of the bf16 / fp16 halves, hi hi + hi lo + lo hi, each
summed in fp32 - the accumulators the statistics and the epilogues see); AVS_F16X2 statistics as column sums -> the mean of the rows a tile holds of the group -> squares
about that mean, the tiles merged by Chan's update in tile order with each tile's true row count (bn_fold_kernel, chan =
1); AVS_F32 / AVS_F32_SPLIT as E[y^2] - mean^2 clamped at 0 on sums added in tile order (chan = 0); tile-local: one
group's sums, mean = s1 / R, squares about it; fmaf(acc, scale, shift), the residual (its own affine by fmaf) added,
ReLU, one split into the output's format.  The input affine: join, multiply, add, ReLU, split (avs_xin_affine8).

Bounds (no constant chosen here):
  * the raw output of the statistics forms: conv_f64_inputs' per-element bounds unchanged (fp32_term, pack_step, the
    split / f16x2 restatement as target and its F16X2_C / SPLIT_C distance from the float64 reference);
  * the returned (scale, shift): 4 * e32 + 8 * EPS32 * max(1, |ref|) per (group, channel), e32 the restatement's own error
    - relative to max(1, |ref|) and pooled: over the ordinary channels of the same group, over the mean40 channels of the
    whole table (one channel's fp32 rounding passes close to 0 by chance, as convbn_f64_inputs explains for its tables);
    scale is exactly 0 where gamma is 0;
  * the finished outputs (bnlocal, affine): convbn_f64_inputs.compare_groups' form per (group, channel) - ``group_bound``,
    which takes ragged groups - plus the output's own storing step per element: pack_step (2^-21 |v| + 2^-25) for
    AVS_F16X2, 2^-18 |v| + 2^-24 for AVS_F16P8 (test_gpu_f16p8.py);
  * compare_moments for the tile-local cases without residual and ReLU.

Tall family (the nine-tap form under EPI_STATS exists only on 256-row tiles chosen by rule, g_tall_min_tiles): frames
repeat a base of TALL_PERIOD frames, groups are whole frames, the frames per group coprime to the period, so only
TALL_PERIOD distinct groups exist plus the short last one; the input-affine rows repeat with AFF_PERIOD = 3, which gives
TALL_PERIOD * AFF_PERIOD = 21 distinct (frame phase, affine row) pairs.  ``layout`` lists the distinct groups as a small
HOST problem (the references and restatements are computed on it) and maps every device row and group to its host
row and group; the tiles cut the host problem's groups elsewhere than the device's, which moves the restatement's
roundings, not the reference."""
import collections
import functools
import itertools
import math
import os
import re
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import conv_f64_inputs as cfi
import gemm_f64_inputs as gfi
from conv_f64_inputs import (F32, BF16, SPLIT, F16X2, TILE_AUTO, TILE_128, TILE_256, GENERIC, RELU, E_ARG, E_SHAPE,  # noqa: F401
                             E_UNSUPPORTED, TALL_PERIOD, FRAME_SCALES, DTYPE_NAMES, emu_pack, emu_unpack, es_of, fp32_term,
                             out_extent, pack_step)
from convbn_f64_inputs import (BN_EPS, CONST_CH, CONST_COL, GAMMA_SMALL, MEAN40_CH_2D, ONE_COL, REGIMES, _fma,  # noqa: F401
                               compare_groups, compare_moments, randomize_bn)
from scorer_f64_inputs import EPS32
from test_gpu_f16p8 import emu_p8_pack, emu_p8_unpack

E_ALIGN, E_WORKSPACE = -3, -5
TILE_224 = 3
AFF_PERIOD = 3
DTYPES = (F32, SPLIT, F16X2)
FORMS = ("stats", "bnlocal", "affine")
MISTAKES = ("unbiased", "drop_last_row", "first_row_of_next_group", "no_eps", "wave_takes_first_rows_group",
            "third_group_takes_second", "chan_equal_counts", "short_last_group_divides_by_rpg", "in_affine_on_padding",
            "in_relu_ignored", "in_affine_of_group0", "res_affine_of_group0", "relu_before_residual", "p8_remainder_dropped",
            "residual_stride_ignored", "beta_without_mean")
# largest |split / f16x2 restatement - ref| / (unit * S) over the statistics cases (the host test recomputes them): below
# conv_f64_inputs' SPLIT_C / F16X2_C, which therefore hold unchanged
SPLIT_RATIO_MEASURED = 0.4748
F16X2_RATIO_MEASURED = 0.5547


# --------------------------------------------------------------------------- the rules, read from the source
def _params_source():
    return os.path.join(os.path.dirname(gfi._source()), "igemm_params.h")


def read_rules(path=None, params_path=None):
    """conv_f64_inputs' rules + affine_128_max_k (igemm.hip) + stats_min_group_rows, bnlocal_max_groups,
    xin_table_min_group_rows, xin_table_max_cin (igemm_params.h)."""
    r = dict(cfi.read_rules(path))
    with open(path or gfi._source()) as f:
        r["affine_128_max_k"] = int(re.search(r"AVS_RULE_AFFINE_128_MAX_K\s*=\s*(\d+)\s*;", f.read()).group(1))
    with open(params_path or _params_source()) as f:
        hdr = f.read()
    for name in ("STATS_MIN_GROUP_ROWS", "BNLOCAL_MAX_GROUPS", "XIN_TABLE_MIN_GROUP_ROWS", "XIN_TABLE_MAX_CIN"):
        r[name.lower()] = int(re.search(rf"constexpr int {name}\s*=\s*(\d+)\s*;", hdr).group(1))
    return r


RULES = read_rules()


# --------------------------------------------------------------------------- the plan, restated
Plan = collections.namedtuple("Plan", "refusal es split bn tiles_n tile_rows tiles_m spatial linear rowb pipe wr fastk epi tap9 xin "
                                      "xin_table ap8 groupw local224 stat_slots ws_bytes")


def bnlocal_tile_rows(dtype, m, cout, k, rpg, ldc, rules=None):
    """bnlocal_plan: the tile pitch 256 // rpg * rpg, or None where the library refuses."""
    r = rules or RULES
    if rpg <= 0 or rpg > 256:
        return None
    bn = 64 if cout <= 64 else 128
    per_tile = 256 // rpg
    h2 = dtype == F16X2
    es = 4 if h2 else 2
    ok = (dtype in (BF16, F16X2) and cout % bn == 0 and m % rpg == 0 and per_tile * rpg * 4 >= 256 * 3 and
          per_tile <= r["bnlocal_max_groups"] and k * es > 128 and (ldc * es) % (32 if h2 else 16) == 0)
    return per_tile * rpg if ok else None


def tap9_ok(geometry, variant, strides, es):
    """igemm_tap9_ok: 3x3 / stride 1 / pad 1 on a dense input at most 63 pixels wide, the caller not forcing the classic walk."""
    n, h, w, cin, kh, kw, sh, sw, ph, pw, cout = geometry
    x_img, x_row, x_px = strides
    ho, wo = out_extent(h, w, kh, kw, sh, sw, ph, pw)
    return ((variant & 3) != TILE_256 and kh == 3 and kw == 3 and sh == 1 and sw == 1 and ph == 1 and pw == 1 and w <= 63 and
            ho * wo == h * w and wo == w and x_px == cin and x_row == w * cin and x_img == ho * wo * cin and cin % (64 // es) == 0)


def local224_ok(dtype, m, cout, cin, k, tile_rows, rpg, variant):
    """igemm_h2_local224_ok without the clustered forms."""
    return (dtype == F16X2 and (variant & 3) in (TILE_AUTO, TILE_224) and not (variant & GENERIC) and tile_rows == rpg and
            192 < tile_rows <= 224 and cout % 128 == 0 and m % rpg == 0 and cin % 16 == 0 and k % 16 == 0 and k // cin <= 32)


def plan(dtype, geometry, form, rpg, variant=0, strides=None, ldc=None, in_affine=False, x_p8=False, rules=None):
    """igemm_plan for stats (form "stats"), tile_rows ("bnlocal") and affine ("affine"): a Plan; ``refusal`` names the
    first requirement of the plan (or of bnstats_plan / bnlocal_plan / avs_conv2d_nhwc_affine) that the shape misses."""
    r = rules or RULES
    assert form in FORMS and r["pipe3"] == 1
    n, h, w, cin, kh, kw, sh, sw, ph, pw, cout = geometry
    x_img, x_row, x_px = strides or (h * w * cin, w * cin, cin)
    ldc = cout if ldc is None else ldc
    ho, wo = out_extent(h, w, kh, kw, sh, sw, ph, pw)
    es, m, k = es_of(dtype), n * ho * wo, kh * kw * cin
    split = {SPLIT: 1, F16X2: 2}.get(dtype, 0)
    tile_mode = variant & 3
    refuse = lambda why: Plan(why, es, split, *([None] * 19))
    local_rows = 0
    if form == "stats":
        if dtype not in (BF16, F32, SPLIT, F16X2):
            return refuse("bf16 / fp32 / f16x2 only")
        if rpg < r["stats_min_group_rows"]:
            return refuse("groups below STATS_MIN_GROUP_ROWS")
    elif form == "bnlocal":
        local_rows = bnlocal_tile_rows(dtype, m, cout, k, rpg, ldc, r)
        if local_rows is None:
            return refuse("bnlocal_plan")
    else:
        if dtype != F16X2:
            return refuse("built for AVS_F16X2")
        if not (kh == 1 and kw == 1 and ph == 0 and pw == 0 and k * 4 > 128):
            return refuse("1x1 without padding, more than 32 input channels")
        if rpg < 32:
            return refuse("groups of at least 32 rows")
    if dtype == F16X2 and (cout % 8 or ldc % 8):
        return refuse("AVS_F16X2 needs cout and the output strides in multiples of 8 slots")
    ce = 8 if dtype == F16X2 else 16 // es
    if cin % ce or k % ce:
        return refuse("cin / K in multiples of 16 bytes")
    narrow = cout <= 64                                   # (no few_f32: the BatchNorm forms keep the 128-wide tile)
    bn = 64 if narrow else 128
    tiles_n = -(-cout // bn)
    can = dtype in (BF16, SPLIT, F16X2) and k * es > 128
    if tile_mode == TILE_224 and not local_rows:
        return refuse("AVS_TILE_224 is a tile of the tile-local form")
    tall = can and (tile_mode == TILE_256 or (tile_mode == TILE_AUTO and -(-m // 256) * tiles_n >= r["tall_min_tiles"] and
                                              (narrow or k * es >= r["tall_min_k_bytes"])))
    if local_rows:
        tall = True
    dense_rows = x_row == wo * x_px and x_img == ho * wo * x_px
    if x_p8:
        ok = (form == "stats" and not (variant & GENERIC) and (tall or k * 4 <= r["rowb_threshold_bytes"]) and kw == 1 and k == cin and
              k % 32 == 0 and k >= 64 and sh == 1 and sw == 1 and ph == 0 and pw == 0 and dense_rows and x_px % 16 == 0)
        if not ok:
            return refuse("an AVS_F16P8 input: 1x1 / stride 1 on dense rows, cin a multiple of 32 (>= 64)")
    groupw = False
    if form == "affine":
        tall = not (not narrow and (tile_mode == TILE_128 or (tile_mode == TILE_AUTO and k <= r["affine_128_max_k"])))
        if not tall and k * 4 > r["rowb_threshold_bytes"]:
            tall = True
        groupw = rpg % 64 == 0
    tile_rows = local_rows or (256 if tall else 128)
    tiles_m = -(-m // tile_rows)
    spatial = not (ph == 0 and pw == 0 and (ho - 1) * sh + kh - 1 < h and (wo - 1) * sw + kw - 1 < w)
    linear = not spatial and kw == 1 and k == cin and sh == 1 and sw == 1 and (ho * wo == 1 or dense_rows)
    stat_slots = ws = None
    if form == "stats":
        stat_slots = (tile_rows + rpg - 2) // rpg + 1
        ws = (tiles_m * stat_slots * 2 * cout * 4 + 255) // 256 * 256
    if local_rows and local224_ok(dtype, m, cout, cin, k, local_rows, rpg, variant):
        return Plan(None, es, split, bn, tiles_n, tile_rows, tiles_m, spatial, False, 64, True, 4, True, "bnlocal", False, False, False,
                    False, False, "spatial" if spatial else "point", None, None)
    if local_rows and tile_mode == TILE_224:
        return refuse("AVS_TILE_224 takes groups of 193..224 rows, cout in multiples of 128, cin in multiples of 16")
    fast64_only = not (variant & GENERIC) and cin % (64 // es) == 0 and cin % (128 // es) != 0 and k // cin <= 32
    rowb = 64 if tall or fast64_only or k * es <= r["rowb_threshold_bytes"] else 128
    pipe = rowb == 64 and k * es > 2 * rowb
    wr = 4 if pipe and tall else 2
    bke = rowb // es
    fastk = not (variant & GENERIC) and cin % bke == 0 and k % bke == 0 and k // cin <= 32
    tap9 = (spatial and pipe and wr == 4 and fastk and (es == 2 or split == 2) and form in ("stats", "bnlocal") and
            tap9_ok(geometry, variant, (x_img, x_row, x_px), es))
    xin = in_affine and tap9 and split == 2 and form == "stats"
    if in_affine and not xin:
        return refuse("the input affine rides in the AVS_F16X2 nine-tap form only")
    xin_table = xin and rpg >= r["xin_table_min_group_rows"] and cin <= r["xin_table_max_cin"]
    ap8 = x_p8 and split == 2 and form == "stats" and not spatial and pipe and fastk
    if x_p8 and not ap8:
        return refuse("no kernel reads an AVS_F16P8 input for this plan")
    return Plan(None, es, split, bn, tiles_n, tile_rows, tiles_m, spatial, linear, rowb, pipe, wr, fastk, form, tap9, xin, xin_table,
                ap8, groupw, None, stat_slots, ws)


FIELD_NAMES = ("dtype", "bn", "spatial", "linear", "rowb", "pipe", "wr", "fastk", "epi", "tap9", "xin", "ap8", "groupw", "local224")
FIELDS = (DTYPES, (64, 128), (False, True), (False, True), (64, 128), (False, True), (2, 4), (False, True), FORMS, (False, True),
          (False, True), (False, True), (False, True), (None, "spatial", "point"))


def unreachable(dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap9, xin, ap8, groupw, local224):
    """Why no call of the four entry points launches this instance, or None: the `if constexpr` gates of igemm_lift_form /
    igemm_lift_staging and the rules of igemm_plan that feed them."""
    if spatial and linear:
        return "the linear walk is the dense 1x1 / stride-1 input without padding"
    if dtype != F16X2 and epi != "stats":
        return "the tile-local and given-affine forms: AVS_F16X2 (bf16's tile-local instances belong to test_gpu_convbn_f64.py)"
    if local224:
        if (dtype, bn, linear, rowb, pipe, wr, fastk, epi, tap9, xin, ap8, groupw) != (F16X2, 128, False, 64, True, 4, True, "bnlocal",
                                                                                      False, False, False, False):
            return "the 224-row tile: AVS_F16X2 tile-local BatchNorm, 128 columns, its own two instances (the other fields fixed)"
        if (local224 == "spatial") != spatial:
            return "the 224-row tile's two instances are the spatial and the point walk"
        return None
    if pipe and rowb != 64:
        return "the 3-buffer pipeline exists on 64-byte steps only"
    if wr == 4 and not pipe:
        return "the 256-row tiles are built on the pipeline"
    if wr == 4 and dtype == F32:
        return "256-row tiles: fp32-split and f16x2 only"
    if epi == "bnlocal" and wr != 4:
        return "EPI_BNLOCAL runs on the 256-row tiles (igemm_lift_form)"
    if epi == "affine" and (spatial or rowb != 64 or not pipe or not (wr == 4 or bn == 128)):
        return "EPI_AFFINE: 1x1 without padding on the pipelined tiles, 256 rows or (wide outputs) 128 (igemm_lift_form)"
    if groupw and epi != "affine":
        return "GROUPW is an instantiation of the given-affine form"
    if tap9 and not (dtype == F16X2 and spatial and rowb == 64 and pipe and wr == 4 and fastk and epi in ("stats", "bnlocal")):
        return "the nine-tap form: the pipelined 256-row tiles with the scalar tap walk, EPI_STATS and EPI_BNLOCAL"
    if xin and not (tap9 and epi == "stats"):
        return "the input affine rides in the AVS_F16X2 nine-tap statistics form only"
    if ap8 and not (dtype == F16X2 and epi == "stats" and linear and rowb == 64 and pipe and fastk):
        return "an AVS_F16P8 input: the AVS_F16X2 1x1 statistics form on dense rows, pipelined, with the scalar tap walk"
    return None


REACHABLE = frozenset(t for t in itertools.product(*FIELDS) if unreachable(*t) is None)


def left_out(dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap9, xin, ap8, groupw, local224):
    """Why CASES has no case for this reachable tuple, or None."""
    return None


LEFT_OUT = {t: left_out(*t) for t in REACHABLE if left_out(*t)}


# --------------------------------------------------------------------------- the case table
BCase = collections.namedtuple("BCase", "name conv form rpg regime relu res res_pad res_affine xin x_p8 y_p8")


def _c(name, dtype, form, hw, cin, cout, rpg, k=(1, 1), s=(1, 1), p=(0, 0), n=3, regime="normal", relu=False, res=None, res_pad=0,
       res_affine=False, xin=None, x_p8=False, y_p8=False, variant=0, w_layout=0, xwide=None, xc0=0, crop=None, ypad=0, yc0=0,
       period=None):
    """res: None, "h2" (an AVS_F16X2 residual, rows cout + res_pad wide) or "p8"; xin: None or in_relu (0 / 1); the rest as
    conv_f64_inputs._case."""
    assert form in FORMS and regime in REGIMES and res in (None, "h2", "p8") and (res_pad == 0 or res == "h2")
    full = f"{DTYPE_NAMES[dtype]}-{form}-{name}-rpg{rpg}-{regime}"
    conv = cfi.Case(full, dtype, n, hw[0], hw[1], cin, cout, k[0], k[1], s[0], s[1], p[0], p[1], "plain", variant, w_layout,
                    xwide or cin, xc0, crop, ypad, yc0, period, None)
    return BCase(full, conv, form, rpg, regime, relu, res, res_pad, res_affine, xin, x_p8, y_p8)


def rows_of(case):
    ho, wo = cfi.extent(case.conv)
    return case.conv.n * ho * wo


def groups_of(case):
    return -(-rows_of(case) // case.rpg)


def case_plan(case, rules=None):
    c = case.conv
    return plan(c.dtype, cfi.geometry(c), case.form, case.rpg, c.variant, cfi.strides(c)[:3], c.cout + c.ypad, case.xin is not None,
                case.x_p8, rules)


def instance(case, rules=None):
    """The case's tuple in REACHABLE's fields."""
    p = case_plan(case, rules)
    assert p.refusal is None, (case.name, p.refusal)
    return (case.conv.dtype, p.bn, p.spatial, p.linear, p.rowb, p.pipe, p.wr, p.fastk, p.epi, p.tap9, p.xin, p.ap8, p.groupw, p.local224)


def _grid_case(t, i):
    """A smallest case that the rules put on the instance ``t`` (None: the nine-tap form under EPI_STATS, which only the tall
    family reaches, and the 224-row tile, which the tile-local family holds)."""
    dtype, bn, spatial, linear, rowb, pipe, wr, fastk, epi, tap9, xin, ap8, groupw, local224 = t
    if local224 or (tap9 and epi == "stats"):
        return None
    hw = cfi.MAPS[i % 3]
    cout = 64 if bn == 64 else 128
    generic = 0
    if epi == "stats":
        if rowb == 64 and not pipe:                 # at most 128 bytes: one or two taps
            cin, k = (16 if fastk else 8), ((1, 2) if spatial else (1, 1))
        elif rowb == 64:
            cin = 64 if ap8 else 16 if fastk else 40
            k = (1, 1) if linear else (3, 3)
            if linear and not ap8:
                cin = 48 if fastk else 40
        else:
            generic = 0 if fastk or i % 2 else GENERIC
            cin = (544 if linear else 64) if fastk or generic else (520 if linear else 72)
            k = (1, 1) if linear else (3, 3)
        if linear:
            s, p = (1, 1), (0, 0)
        elif spatial:
            s, p = (1, 1), ((0, 1) if k == (1, 2) else (1, 1))
        else:
            s, p = ((2, 1) if k == (1, 1) else (1, 1)), (0, 0)
        cout = 40 if bn == 64 else 72
        # (the 1x2 window has no tap that stays inside the frame for every output pixel: the regimes' constant column needs one)
        name = (f"grid-{'sp' if spatial else 'lin' if linear else 'ns'}-{k[0]}x{k[1]}-c{cin}-n{cout}-r{rowb}"
                f"{'-fk' if fastk else '-gen' if generic else '-odd'}{'-t256' if wr == 4 else ''}{'-p8' if ap8 else ''}")
        return _c(name, dtype, "stats", hw, cin, cout, (64, 65, 100)[i % 3], k, s, p, regime="normal" if k == (1, 2) else REGIMES[i % 3], x_p8=ap8,
                  variant=generic | (TILE_256 if wr == 4 else 0), ypad=8 * (i % 2), yc0=8 * (i % 2))
    if epi == "affine":
        # wr == 2: wide outputs with K <= 128 (or AVS_TILE_128); linear: stride 1; fastk: cin a multiple of 16
        cin = 48 if fastk else 40
        s = (1, 1) if linear else (2, 1)
        rpg = 64 if groupw else (33, 100)[i % 2]
        name = f"grid-{'lin' if linear else 'ns'}-c{cin}-n{cout}{'-fk' if fastk else '-odd'}{'-t256' if wr == 4 else ''}"
        return _c(name, dtype, "affine", hw, cin, cout, rpg, s=s, relu=bool(i % 2), res=(None, "h2")[i % 2], res_pad=8 * (i % 2),
                  variant=TILE_256 if wr == 4 and bn == 128 else 0)
    # bnlocal (always 256-row tiles); the walk: nine-tap (3x3 / 1 / pad 1), classic spatial (3x3 / 2 / pad 1), 1x1 / 2, linear
    cin = 16 if fastk else 40
    if tap9:
        hw, k, s, p = (16, 4), (3, 3), (1, 1), (1, 1)
    elif spatial:
        hw, k, s, p = (32, 8), (3, 3), (2, 2), (1, 1)
    elif linear:
        hw, k, s, p, cin = (16, 4), (1, 1), (1, 1), (0, 0), 48 if fastk else 40
    else:
        hw, k, s, p, cin = (32, 8), (1, 1), (2, 2), (0, 0), 48 if fastk else 40
    name = f"grid-{'tap9' if tap9 else 'sp' if spatial else 'lin' if linear else 'ns'}-c{cin}-n{cout}{'-fk' if fastk else '-odd'}"
    return _c(name, dtype, "bnlocal", hw, cin, cout, 64, k, s, p, n=6, regime=REGIMES[i % 3], relu=bool(i % 2), res=(None, "h2")[i % 2],
              res_pad=8 * (i % 2))


def tall_frames(tiles_n=1):
    """Frames of a 9 x 7 map that give g_tall_min_tiles tall tiles, one frame past them (as conv_f64_inputs)."""
    return -(-(-(-RULES["tall_min_tiles"] // tiles_n) * 256) // 63) + 1


def _build_cases():
    cases = []
    # 1. one smallest case per reachable instance
    seen = set()
    for i, t in enumerate(sorted(REACHABLE, key=repr)):
        if t in LEFT_OUT:
            continue
        c = _grid_case(t, i)
        if c is not None and c.name not in seen:
            seen.add(c.name)
            cases.append(c)
    # 2. tall by rule: the nine-tap form under EPI_STATS, without and with the input affine.  Groups of 2, 3 and 5 frames
    #    (126, 189, 315 rows: the per-row group lookup) and of 8 frames (504 rows >= XIN_TABLE_MIN_GROUP_ROWS: the LDS table),
    #    cin = 144 > XIN_TABLE_MAX_CIN (the lookup again); cout = 72 at cin = 32 (K * 4 >= g_tall_min_k_bytes): the 128-wide
    #    tile; the frame count is no multiple of the group's, so the last group
    #    is short.  (No "mean40" here: a group of several frames mixes the three frame magnitudes, which are its spread.)
    nt = tall_frames()
    for j, (fpg, cin, cout, xin, regime) in enumerate(((3, 16, 8, None, "normal"), (5, 16, 64, None, "normal"), (8, 16, 40, 1, "normal"),
                                                       (2, 16, 8, 0, "const"), (8, 16, 8, 0, "const"), (8, 144, 8, 1, "normal"),
                                                       (3, 32, 72, None, "const"), (8, 32, 72, 1, "normal"))):
        n = nt + (1 if nt % fpg == 0 else 0)
        cases.append(_c(f"tall-3x3-c{cin}-n{cout}-f{fpg}{'' if xin is None else '-xin-relu' if xin else '-xin'}", F16X2, "stats", (9, 7),
                        cin, cout, fpg * 63, (3, 3), (1, 1), (1, 1), n=n, regime=regime, xin=xin, period=TALL_PERIOD,
                        ypad=8 * (j % 2), yc0=8 * (j % 2), w_layout=cfi.W_KSTEP32 if j == 2 else cfi.W_ROWS))
    # 3. groups, EPI_STATS: group sizes that align to waves and that do not, tiles that hold the tail of one group and the head
    #    of the next, groups over three tiles (600 rows: Chan's merge runs twice), a short last group, row counts either side
    #    of a tile; cout of 8 .. 136 into channel slices
    for dtype in DTYPES:
        for j, (rpg, hw, n) in enumerate(((64, (9, 7), 3), (65, (9, 7), 5), (100, (11, 9), 4), (196, (13, 11), 5), (200, (11, 9), 7),
                                          (300, (13, 11), 6), (600, (13, 11), 10))):
            cout = (8, 64, 72, 128, 136)[j % 5]
            cases.append(_c(f"groups-3x3-n{cout}", dtype, "stats", hw, 16, cout, rpg, (3, 3), (1, 1), (1, 1), n=n, regime=REGIMES[j % 3],
                            variant=(TILE_AUTO, TILE_128, TILE_256)[j % 3], ypad=(0, 8, 16)[j % 3], yc0=(0, 8, 8)[j % 3]))
            cases.append(_c(f"groups-1x1-n{cout}", dtype, "stats", hw, 48, cout, rpg, n=n, regime=REGIMES[(j + 1) % 3],
                            variant=(TILE_256, TILE_AUTO, TILE_128)[j % 3], ypad=8, yc0=(0, 8)[j % 2],
                            w_layout=cfi.W_KSTEP32 if j % 4 == 1 else cfi.W_ROWS))
        for j, (rows, hw) in enumerate(((127, (127, 1)), (128, (16, 8)), (129, (43, 3)), (255, (17, 15)), (256, (32, 8)), (257, (257, 1)))):
            cases.append(_c(f"rows{rows}-3x3", dtype, "stats", hw, 16, 40, (64, 100, 65)[j % 3], (3, 3), (1, 1), (1, 1), n=1,
                            regime=REGIMES[j % 3], variant=(TILE_256, TILE_128)[j % 2]))
    for j, rpg in enumerate((64, 100, 200)):          # an AVS_F16P8 input on both tiles
        cases.append(_c("groups-1x1-p8", F16X2, "stats", (11, 9), 64, (72, 64, 136)[j], rpg, n=5, regime=REGIMES[j], x_p8=True,
                        variant=(TILE_128, TILE_256, TILE_AUTO)[j], ypad=8, yc0=8))
    # 4. groups, EPI_BNLOCAL: from the smallest group the host query takes (BNLOCAL_MIN_RPG: six groups per tile, a wave in
    #    three groups) to one group per tile; always a last tile with fewer groups than the first; the nine-tap walk (3x3 /
    #    1 / pad 1), the classic walk (3x3 / 2, 1x1 / 2) and the linear one; residual with a row stride wider than cout
    local = ((BNLOCAL_MIN_RPG, (BNLOCAL_MIN_RPG, 1), 8), (42, (7, 6), 8), (43, (43, 1), 7), (49, (7, 7), 7), (64, (16, 4), 6), (85, (17, 5), 4),
             (100, (20, 5), 3), (128, (16, 8), 3), (192, (16, 12), 2), (225, (25, 9), 2), (256, (32, 8), 2))
    for j, (rpg, hw, n) in enumerate(local):
        walk = j % 4
        k, s, p, cin, ihw = (((3, 3), (1, 1), (1, 1), 16, hw), ((1, 1), (1, 1), (0, 0), 48, hw),
                             ((3, 3), (2, 2), (1, 1), 16, (2 * hw[0], 2 * hw[1])), ((1, 1), (2, 2), (0, 0), 40, (2 * hw[0], 2 * hw[1])))[walk]
        cases.append(_c(f"local-{k[0]}x{k[1]}-s{s[0]}", F16X2, "bnlocal", ihw, cin, (64, 128)[j % 2], rpg, k, s, p, n=n,
                        regime=REGIMES[j % 3], relu=j % 2 == 0, res="h2" if j % 3 == 0 else None, res_pad=8 if j % 3 == 0 else 0,
                        ypad=8 * (j % 2), yc0=8 * (j % 2)))
        cases.append(_c(f"local-bare-{k[0]}x{k[1]}-s{s[0]}", F16X2, "bnlocal", ihw, cin, (128, 64)[j % 2], rpg, k, s, p, n=n,
                        regime=REGIMES[(j + 1) % 3]))                                 # no residual, no ReLU: the moments check
    for rpg, hw in ((196, (28, 7)), (224, (16, 14))):    # the 224-row tile's two instances, and the same shapes on the 256-row tile
        for variant in (TILE_AUTO, TILE_256):
            tag = "t256" if variant else "local224"
            cases.append(_c(f"{tag}-3x3", F16X2, "bnlocal", hw, 16, 128, rpg, (3, 3), (1, 1), (1, 1), n=3, variant=variant,
                            regime=REGIMES[rpg % 3], relu=True, res="h2", res_pad=8))
            cases.append(_c(f"{tag}-1x1", F16X2, "bnlocal", hw, 48, 256, rpg, n=3, variant=variant, regime=REGIMES[(rpg + 1) % 3], ypad=8,
                            yc0=8))
    # 5. groups, EPI_AFFINE: 33 and 100 the general instance (33: three groups in a wave), 64 and 192 GROUPW - also with M
    #    ending inside a wave and with the last group short; cin = 40 has no scalar tap walk; K either side of
    #    AVS_RULE_AFFINE_128_MAX_K against the three tile modes; residual none / f16x2 / AVS_F16P8, its affine, an AVS_F16P8 output
    aff = ((32, (16, 4), 5, 48), (33, (11, 9), 3, 40), (64, (16, 4), 5, 136), (100, (20, 5), 4, 48), (192, (16, 12), 3, 136),
           (600, (13, 11), 9, 40), (64, (9, 7), 5, 48), (192, (11, 9), 5, 136))         # the last two: M = 315 and 495, a short last group
    for j, (rpg, hw, n, cin) in enumerate(aff):
        for v, variant in enumerate((TILE_AUTO, TILE_128, TILE_256)):
            q = j + v
            res = (None, "h2", "p8")[q % 3]
            cases.append(_c(f"1x1-c{cin}-m{n * hw[0] * hw[1]}-{('auto', 't128', 't256')[v]}", F16X2, "affine", hw, cin, (128, 64, 144)[q % 3], rpg, n=n,
                            relu=q % 2 == 0, res=res, res_pad=16 if res == "h2" else 0, res_affine=res is not None and q % 4 < 2,
                            y_p8=q % 3 == 1, variant=variant, ypad=0 if q % 3 == 1 else 16 * (q % 2), yc0=0 if q % 3 == 1 else 8 * (q % 2)))
        cases.append(_c(f"1x1-s2-c{cin}-m{n * hw[0] * hw[1]}", F16X2, "affine", (2 * hw[0], 2 * hw[1]), cin, 72, rpg, s=(2, 2), n=n, relu=j % 2 == 1,
                        res="h2", res_pad=16, res_affine=True))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(cases)


def _min_local_rpg():
    """The smallest group the tile-local form takes by the restated bnlocal_plan (the host test takes the same value from
    the library's query)."""
    return min(r for r in range(1, 257) if bnlocal_tile_rows(F16X2, r * 12, 64, 48, r, 64) is not None)


BNLOCAL_MIN_RPG = _min_local_rpg()
CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# --------------------------------------------------------------------------- the host problem of a (periodic) case
@functools.lru_cache(maxsize=None)
def layout(case):
    """The distinct groups of a case as a small host problem: ``frames`` (base frame of every host frame), ``aff`` (row of
    the input-affine base table of every host group), ``rows`` / ``groups`` of the host problem, ``keys`` (periodic cases:
    {(frame phase, affine row): host group}; the short last device group is host group len(keys))."""
    c = case.conv
    ho, wo = cfi.extent(c)
    fr = ho * wo
    groups = groups_of(case)
    if not c.period:
        return SimpleNamespace(frames=tuple(range(c.n)), aff=tuple(range(groups)), rows=c.n * fr, groups=groups, keys=None, fpg=None)
    fpg = case.rpg // fr
    assert case.rpg == fpg * fr and math.gcd(fpg, c.period) == 1 and c.n % fpg != 0 and case.form == "stats"
    keys = sorted({((g * fpg) % c.period, g % AFF_PERIOD) for g in range(groups - 1)})
    frames, aff = [], []
    for phase, a in keys:
        frames += [(phase + j) % c.period for j in range(fpg)]
        aff.append(a)
    last = groups - 1
    frames += [(last * fpg + j) % c.period for j in range(c.n - last * fpg)]
    aff.append(last % AFF_PERIOD)
    return SimpleNamespace(frames=tuple(frames), aff=tuple(aff), rows=len(frames) * fr, groups=len(keys) + 1,
                           keys={key: i for i, key in enumerate(keys)}, fpg=fpg)


def host_conv(case):
    """The conv_f64_inputs case of the host problem."""
    return case.conv._replace(n=len(layout(case).frames), period=None)


def offsets_of(case):
    """Row offsets of the host problem's groups (the last one may be short)."""
    lay = layout(case)
    return list(range(0, lay.rows, case.rpg)) + [lay.rows]


def device_maps(case, device):
    """(host row of every device row, host group of every device group) as index tensors on ``device``."""
    lay, c = layout(case), case.conv
    m, groups = rows_of(case), groups_of(case)
    r = torch.arange(m, device=device)
    g = torch.arange(groups, device=device)
    if lay.keys is None:
        return r, g
    table = torch.full((c.period, AFF_PERIOD), -1, dtype=torch.long)
    for (phase, a), i in lay.keys.items():
        table[phase, a] = i
    hg = table.to(device)[(g * lay.fpg) % c.period, g % AFF_PERIOD]
    hg[-1] = len(lay.keys)
    assert int(hg.min()) >= 0
    return hg[r // case.rpg] * case.rpg + r % case.rpg, hg


# --------------------------------------------------------------------------- operands
def _seeded(case, tag=""):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{tag}".encode()))


def _signed(shape, g):
    return (torch.rand(shape, generator=g) + 0.5) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def _keep(case, t):
    """What the input's format keeps of t."""
    if case.x_p8:
        return emu_p8_unpack(emu_p8_pack(t), t.shape)
    return emu_unpack(emu_pack(t)) if case.conv.dtype == F16X2 else t.float()


def tap_conv(c, x, w):
    """The convolution of the NHWC view x [f, h, w, cin] with the filters w [cout, K] by an explicit loop over taps, in x's
    dtype: [f * Ho * Wo, cout]."""
    ho, wo = cfi.extent(c)
    w4 = w.reshape(c.cout, c.kh, c.kw, c.cin)
    xp = F.pad(x, (0, 0, c.pw, c.pw, c.ph, c.ph))
    acc = torch.zeros(x.shape[0], ho, wo, c.cout, dtype=x.dtype)
    for i in range(c.kh):
        for j in range(c.kw):
            acc += xp[:, i:i + (ho - 1) * c.sh + 1:c.sh, j:j + (wo - 1) * c.sw + 1:c.sw] @ w4[:, i, j].t()
    return acc.reshape(-1, c.cout)


@functools.lru_cache(maxsize=32)
def operands(case):
    """Everything a call is given, as the BASE tensors the device builds its operands from and as the host problem's:
    x_base [period or n frames, H, W, xwide] / x_buf (its stored image), w_buf, wv, xv (host frames), gamma, beta, isc / ish
    (base table [AFF_PERIOD or groups, cin]), res_buf (stored, rows cout + res_pad wide) / res (values [rows, cout]),
    rsc / rsh.  Nothing here is modified by a test."""
    c, lay = case.conv, layout(case)
    g = _seeded(case)
    nb = c.period or c.n
    hf, wf, y0, x0 = c.crop or (c.h, c.w, 0, 0)
    k = c.kh * c.kw * c.cin
    fscale = torch.tensor(FRAME_SCALES[True])[torch.arange(nb) % 3]
    if case.regime == "mean40":     # (a group of several frames would have the three magnitudes as its spread: all frames alike)
        fscale = torch.ones(nb)
    xb = torch.randn(nb, hf, wf, c.xwide, generator=g) * fscale.view(nb, 1, 1, 1)
    w4 = (torch.randn(c.cout, k, generator=g) * k ** -0.5).reshape(c.cout, c.kh, c.kw, c.cin)
    ci, cj = c.kh // 2, c.kw // 2
    hframes = torch.tensor(lay.frames)
    ho, wo = cfi.extent(c)
    const_group = min(1, lay.groups - 1)
    if case.regime == "const":      # channel CONST_CH reads the centre tap of column CONST_COL alone, constant in one group's frames
        r0, r1 = const_group * case.rpg, min((const_group + 1) * case.rpg, lay.rows)
        touched = hframes[r0 // (ho * wo):(r1 - 1) // (ho * wo) + 1]
        xb[touched, :, :, c.xc0 + CONST_COL] = 1.5
        w4[CONST_CH] = 0.0
        w4[CONST_CH, ci, cj, CONST_COL] = 0.75
    if case.regime == "mean40":     # a constant column of the frame's magnitude; |mean| / std about 40 in MEAN40_CH_2D
        assert case.xin is None
        xb[:, :, :, c.xc0 + ONE_COL] = fscale.view(nb, 1, 1)
        w4[:, :, :, ONE_COL] = 0.0
    xb = _keep(case, xb)
    w4 = _keep(case._replace(x_p8=False), w4.reshape(c.cout, k)).reshape(w4.shape)
    if case.regime == "mean40":
        view0 = xb[:1, y0:y0 + c.h, x0:x0 + c.w, c.xc0:c.xc0 + c.cin]      # frame 0: magnitude 1
        sd = tap_conv(c, view0.double(), w4.reshape(c.cout, k).double()).std(0)
        for ch in (ch for ch in MEAN40_CH_2D if ch < c.cout):
            w4[ch, ci, cj, ONE_COL] = 40.0 * sd[ch].float() * (1.0 if ch % 2 else -1.0)
        w4 = _keep(case._replace(x_p8=False), w4.reshape(c.cout, k)).reshape(w4.shape)
    wv = w4.reshape(c.cout, k).contiguous()
    x_buf = emu_p8_pack(xb) if case.x_p8 else emu_pack(xb) if c.dtype == F16X2 else xb
    w_buf = emu_pack(wv) if c.dtype == F16X2 else wv
    gamma, beta = randomize_bn(c.cout, g)
    o = SimpleNamespace(x_base=xb, x_buf=x_buf, w_buf=w_buf, wv=wv, xv=xb[hframes], gamma=gamma, beta=beta, const_group=const_group,
                        isc=None, ish=None, res=None, res_buf=None, rsc=None, rsh=None)
    o.x = o.xv[:, y0:y0 + c.h, x0:x0 + c.w, c.xc0:c.xc0 + c.cin]
    if case.xin is not None:        # scales of both signs, an exact 0 in column 2
        na = AFF_PERIOD if c.period else lay.groups
        o.isc, o.ish = _signed((na, c.cin), g), torch.randn(na, c.cin, generator=g) * 0.5
        o.isc[:, 2] = 0.0
    if case.res is not None:        # of the rows' own magnitude, the WHOLE wide buffer random: an ignored stride reads other numbers
        rscale = fscale[hframes].repeat_interleave(ho * wo).view(-1, 1)
        wide = torch.randn(lay.rows, c.cout + case.res_pad, generator=g) * rscale
        if case.res == "p8":
            o.res_buf = emu_p8_pack(wide)
            o.res = emu_p8_unpack(o.res_buf, wide.shape)
        else:
            o.res_buf = emu_pack(wide)
            o.res = emu_unpack(o.res_buf)[:, :c.cout]
    if case.res_affine:
        o.rsc, o.rsh = _signed((lay.groups, c.cout), g), torch.randn(lay.groups, c.cout, generator=g)
    return o


def group_of_rows(case):
    """Host group of every host row."""
    return torch.arange(layout(case).rows) // case.rpg


def _in_affine(case, o, x, dtype, mistake=None, padded=False):
    """relu(x * in_scale[g] + in_shift[g]) of the dense input x [f, h, w, cin] (the nine-tap form: output row = input row)
    in ``dtype``; fp32: a multiply, an add, ReLU, one split (avs_xin_affine8).  padded: x carries the padding ring, whose
    pixels take their frame's first / last group."""
    c, lay = case.conv, layout(case)
    gi = torch.tensor(lay.aff)[group_of_rows(case)].view(x.shape[0], c.h, c.w)
    if mistake == "in_affine_of_group0":
        gi = torch.full_like(gi, lay.aff[0])
    if padded:
        gi = F.pad(gi.unsqueeze(1).float(), (c.pw, c.pw, c.ph, c.ph), mode="replicate").squeeze(1).long()
    sc, sf = o.isc.to(dtype)[gi], o.ish.to(dtype)[gi]
    v = x.to(dtype) * sc + sf
    if case.xin and mistake != "in_relu_ignored":
        v = v.clamp_min(0.0)
    return emu_unpack(emu_pack(v)) if dtype == torch.float32 else v


# --------------------------------------------------------------------------- reference
def bn_stats64(acc, offsets, gamma, beta):
    """float64 (scale, shift) [G, n]: per-group mean and centred (biased) variance."""
    sc, sh = [], []
    for r0, r1 in zip(offsets[:-1], offsets[1:]):
        blk = acc[r0:r1]
        mu = blk.mean(0)
        var = ((blk - mu) ** 2).mean(0)
        s = gamma.double() / torch.sqrt(var + torch.tensor(BN_EPS, dtype=torch.float32).double())
        sc.append(s)
        sh.append(beta.double() - mu * s)
    return torch.stack(sc), torch.stack(sh)


def _rows_to_groups(offsets):
    return torch.repeat_interleave(torch.arange(len(offsets) - 1), torch.tensor(offsets[1:]) - torch.tensor(offsets[:-1]))


@functools.lru_cache(maxsize=32)
def reference(case):
    """float64: acc [rows, cout] (the raw convolution), (scale, shift) [G, cout], y (the finished output of the tile-local
    and given-affine forms; the given affine is the float64 BatchNorm's, as the fp32 numbers a caller would hand over)."""
    o, hc = operands(case), host_conv(case)
    x = o.x.double() if case.xin is None else _in_affine(case, o, o.x, torch.float64)
    acc = tap_conv(hc, x, o.wv.double())
    offsets = offsets_of(case)
    sc, sh = bn_stats64(acc, offsets, o.gamma, o.beta)
    given = None
    if case.form == "affine":
        given = (sc.float(), sh.float())
        sc, sh = given[0].double(), given[1].double()
    y = None
    if case.form != "stats":
        gi = _rows_to_groups(offsets)
        y = acc * sc[gi] + sh[gi]
        if o.res is not None:
            r = o.res.double()
            y = y + (r * o.rsc.double()[gi] + o.rsh.double()[gi] if o.rsc is not None else r)
        y = y.clamp_min(0.0) if case.relu else y
    return SimpleNamespace(acc=acc, scale=sc, shift=sh, y=y, given=given)


# --------------------------------------------------------------------------- restatement
def _im2col(case, o, mistake=None):
    """The im2col rows [rows, K] fp32 of the host problem, gathered from the flat input by the strides; with an input affine
    the transformed input (dense: the nine-tap form)."""
    hc = host_conv(case)
    if case.xin is None:
        return cfi.im2col(hc, SimpleNamespace(xv=o.xv))
    if mistake == "in_affine_on_padding":       # the affine applied to the zero padding: a border tap contributes relu(shift)
        xp = F.pad(o.xv, (0, 0, hc.pw, hc.pw, hc.ph, hc.ph))
        a = _in_affine(case, o, xp, torch.float32, padded=True)
        big = hc._replace(h=hc.h + 2 * hc.ph, w=hc.w + 2 * hc.pw, ph=0, pw=0, xwide=hc.cin)
        return cfi.im2col(big, SimpleNamespace(xv=a.contiguous()))
    return cfi.im2col(hc, SimpleNamespace(xv=_in_affine(case, o, o.xv, torch.float32, mistake).contiguous()))


def _tiles_of_group(r0, r1, tile_rows):
    """[(lo, hi)] of the rows [r0, r1) per row tile, in tile order."""
    return [(max(r0, t * tile_rows), min(r1, (t + 1) * tile_rows)) for t in range(r0 // tile_rows, (r1 - 1) // tile_rows + 1)]


def stats_restatement(case, acc, mistake=None):
    """(scale, shift) fp32 [G, cout] of avs_conv2d_nhwc_bnstats from the fp32 accumulators: per row tile the column sums of
    the rows it holds of a group, then (AVS_F16X2, chan = 1) the squares about that tile mean and Chan's merge in tile order
    with each tile's true row count, or (chan = 0) the sums of squares, E[y^2] - mean^2 clamped at 0 (bn_fold_kernel)."""
    o, p = operands(case), case_plan(case)
    offsets = offsets_of(case)
    chan = case.conv.dtype == F16X2
    eps = torch.tensor(0.0 if mistake == "no_eps" else BN_EPS, dtype=torch.float32)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    scale, shift = torch.zeros(len(offsets) - 1, acc.shape[1]), torch.zeros(len(offsets) - 1, acc.shape[1])
    for g, (r0, r1) in enumerate(zip(offsets[:-1], offsets[1:])):
        if mistake == "drop_last_row":
            r1 -= 1
        if mistake == "first_row_of_next_group":
            r1 = r1 + 1 if r1 < acc.shape[0] else r1
        cnt = r1 - r0
        if mistake == "short_last_group_divides_by_rpg":
            cnt = case.rpg
        tiles = _tiles_of_group(r0, r1, p.tile_rows)
        if chan:
            n, mean, m2 = f32(0), torch.zeros(acc.shape[1]), torch.zeros(acc.shape[1])
            left = cnt
            for i, (lo, hi) in enumerate(tiles):
                blk = acc[lo:hi]
                nt = f32(p.tile_rows if mistake == "chan_equal_counts" else (left if i == len(tiles) - 1 else hi - lo))
                left -= hi - lo
                s1 = blk.sum(0)
                tmean = s1 / f32(hi - lo)
                s2 = ((blk - tmean) ** 2).sum(0)
                mt = s1 / nt
                d, nn = mt - mean, n + nt
                mean = mean + d * (nt / nn)
                m2 = m2 + s2 + d * d * (n * nt / nn)
                n = nn
            var = m2 / n
        else:
            s1, s2 = torch.zeros(acc.shape[1]), torch.zeros(acc.shape[1])
            for lo, hi in tiles:
                s1, s2 = s1 + acc[lo:hi].sum(0), s2 + (acc[lo:hi] * acc[lo:hi]).sum(0)
            inv_n = f32(1) / f32(cnt)
            mean = s1 * inv_n
            var = (s2 * inv_n - mean * mean).clamp_min(0.0)
        if mistake == "unbiased":
            var = var * (f32(cnt) / f32(max(cnt - 1, 1)))
        scale[g] = o.gamma / torch.sqrt(var + eps)
        shift[g] = o.beta if mistake == "beta_without_mean" else o.beta - mean * scale[g]
    return scale, shift


def local_stats_restatement(case, acc, mistake=None):
    """(scale, shift) fp32 [G, cout] of the tile-local form: a group's column sums, mean = s1 * (1 / R), the squares about it,
    var = s2 * (1 / R) (EPI_BNLOCAL's two rounds; igemm_h2_local224_kernel's the same)."""
    o = operands(case)
    rpg = case.rpg
    groups = acc.shape[0] // rpg
    eps = torch.tensor(0.0 if mistake == "no_eps" else BN_EPS, dtype=torch.float32)
    inv_n = torch.ones((), dtype=torch.float32) / float(rpg)
    scale, shift = torch.zeros(groups, acc.shape[1]), torch.zeros(groups, acc.shape[1])
    for g in range(groups):
        r0, r1 = g * rpg, (g + 1) * rpg
        if mistake == "drop_last_row":
            r1 -= 1
        if mistake == "first_row_of_next_group":
            r1 = r1 + 1 if r1 < acc.shape[0] else r1
        blk = acc[r0:r1]
        mean = blk.sum(0) * inv_n
        var = ((blk - mean) ** 2).sum(0) * inv_n
        if mistake == "unbiased":
            var = var * (float(rpg) / float(rpg - 1))
        scale[g] = o.gamma / torch.sqrt(var + eps)
        shift[g] = o.beta if mistake == "beta_without_mean" else o.beta - mean * scale[g]
    return scale, shift


def _group_per_row(case, mistake=None):
    """The group whose affine the epilogue applies to every host row: the row's own, or a planted mistake's - a wave (64 rows
    from the tile's first) taking its first row's group for all of them, or taking its second group for the rows of its
    third."""
    p, rpg = case_plan(case), case.rpg
    rows = layout(case).rows
    r = torch.arange(rows)
    last = (rows - 1) // rpg
    if mistake not in ("wave_takes_first_rows_group", "third_group_takes_second"):
        return r // rpg
    if case.form == "bnlocal":       # groups and waves count from the tile's first row; tiles lie tile_rows apart
        t, rt = r // p.tile_rows, r % p.tile_rows
        first = (rt // 64 * 64) // rpg
        k = first if mistake == "wave_takes_first_rows_group" else torch.minimum(rt // rpg, first + 1)
        return torch.minimum(t * (p.tile_rows // rpg) + k, torch.tensor(last))
    first = (r // 64 * 64) // rpg
    return first if mistake == "wave_takes_first_rows_group" else torch.minimum(r // rpg, first + 1)


def store(case, v):
    """What the output's format keeps of the fp32 values v [rows, cout]: one split."""
    return emu_p8_unpack(emu_p8_pack(v), v.shape) if case.y_p8 else emu_unpack(emu_pack(v))


def store_step(case, target):
    """The storing step of the output's format per element: pack_step for AVS_F16X2, 2^-18 |v| + 2^-24 for AVS_F16P8."""
    return target.abs() * 2.0 ** -18 + 2.0 ** -24 if case.y_p8 else pack_step(target)


def finish(case, acc, scale, shift, mistake=None):
    """The epilogue of the tile-local and given-affine forms in fp32: fmaf(acc, scale[g], shift[g]), the residual added (its
    own affine by fmaf), ReLU, one split into the output's format."""
    o = operands(case)
    gi = _group_per_row(case, mistake)
    v = _fma(acc, scale[gi], shift[gi])
    relu = case.relu
    if mistake == "relu_before_residual" and relu:
        v, relu = v.clamp_min(0.0), False
    if o.res is not None:
        r = o.res
        if mistake == "p8_remainder_dropped" and case.res == "p8":
            r = r.half().float()
        if mistake == "residual_stride_ignored":
            flat = (emu_unpack(o.res_buf) if case.res == "h2" else o.res).reshape(-1)
            r = flat[:r.numel()].reshape(r.shape)
        if o.rsc is not None:
            gr = torch.zeros_like(gi) if mistake == "res_affine_of_group0" else torch.arange(acc.shape[0]) // case.rpg
            r = _fma(r, o.rsc[gr], o.rsh[gr])
        v = v + r
    v = v.clamp_min(0.0) if relu else v
    return store(case, v)


def split_target(case, a, wv):
    """conv_f64_inputs' float64 restatement of the AVS_F32_SPLIT / AVS_F16X2 product: ah bh + ah bl + al bh with bf16 / fp16
    halves."""
    half = (lambda t: t.bfloat16().double()) if case.conv.dtype == SPLIT else (lambda t: t.half().double())
    bt = wv.t()
    ah, bh = half(a), half(bt)
    al, bl = half(a.double() - ah), half(bt.double() - bh)
    return ah @ bh + ah @ bl + al @ bh


def split_acc32(case, a, wv):
    """The fp32 accumulators of the AVS_F32_SPLIT / AVS_F16X2 product: the three products of the bf16 / fp16 halves, each summed
    in fp32, added in fp32 (the order inside the matrix cores is not restated)."""
    half = (lambda t: t.bfloat16().float()) if case.conv.dtype == SPLIT else (lambda t: t.half().float())
    bt = wv.t()
    ah, bh = half(a), half(bt)
    al, bl = half(a - ah), half(bt - bh)
    return ah @ bh + ah @ bl + al @ bh


def restatement(case, mistake=None):
    """The case in the kernels' order of operations: acc (fp32 accumulators; AVS_F32_SPLIT and AVS_F16X2: of the three products
    of the halves), yard (the plain fp32 product: conv_f64_inputs' yardstick of the raw output's bound), raw (what the statistics forms store, before
    the output's own packing, float64), scale / shift (fp32 [G, cout], the forms that compute them), y (the finished
    output, what the format keeps)."""
    assert mistake is None or mistake in MISTAKES
    o = operands(case)
    a = _im2col(case, o, mistake)
    if mistake == "p8_remainder_dropped" and case.x_p8:
        a = a.half().float()
    yard = a @ o.wv.t()
    acc = split_acc32(case, a, o.wv) if case.conv.dtype in (SPLIT, F16X2) else yard
    out = SimpleNamespace(acc=acc, yard=yard, raw=None, scale=None, shift=None, y=None)
    if case.form == "stats":
        out.raw = split_target(case, a, o.wv) if case.conv.dtype in (SPLIT, F16X2) else acc.double()
        out.scale, out.shift = stats_restatement(case, acc, mistake)
    elif case.form == "bnlocal":
        out.scale, out.shift = local_stats_restatement(case, acc, mistake)
        out.y = finish(case, acc, out.scale, out.shift, mistake)
    else:
        sc, sh = reference(case).given
        if mistake == "beta_without_mean":
            sh = o.beta.expand_as(sh)
        out.y = finish(case, acc, sc, sh, mistake)
    return out


def applies(case, mistake):
    """Does the planted mistake change what this case computes (by more than a rounding)?"""
    p, lay, c = case_plan(case), layout(case), case.conv
    form, rpg = case.form, case.rpg
    stats_like = form in ("stats", "bnlocal")
    short = lay.rows % rpg != 0
    tiles = [_tiles_of_group(r0, r1, p.tile_rows) for r0, r1 in zip(offsets_of(case)[:-1], offsets_of(case)[1:])]
    gi, gw, g3 = (_group_per_row(case, m) for m in (None, "wave_takes_first_rows_group", "third_group_takes_second"))
    return {"unbiased": stats_like, "drop_last_row": stats_like, "first_row_of_next_group": stats_like and lay.groups > 1,
            "no_eps": stats_like and case.regime == "const",
            "wave_takes_first_rows_group": form != "stats" and not torch.equal(gi, gw),
            "third_group_takes_second": form != "stats" and not torch.equal(gi, g3),
            "chan_equal_counts": form == "stats" and c.dtype == F16X2 and any(len(t) > 1 and len({hi - lo for lo, hi in t}) > 1 for t in tiles),
            "short_last_group_divides_by_rpg": form == "stats" and short,
            "in_affine_on_padding": case.xin is not None, "in_relu_ignored": bool(case.xin),
            "in_affine_of_group0": case.xin is not None and len(set(lay.aff)) > 1,
            "res_affine_of_group0": case.res_affine and lay.groups > 1,
            "relu_before_residual": form != "stats" and case.relu and case.res is not None,
            "p8_remainder_dropped": case.res == "p8" or case.x_p8,
            "residual_stride_ignored": case.res_pad > 0,
            "beta_without_mean": True}[mistake]


# --------------------------------------------------------------------------- bounds
def group_bound(ref, cpu32, offsets):
    """convbn_f64_inputs.compare_groups' bound for ragged groups, spread over the rows: 4 * e32 + 8 * EPS32 * max(1, max |ref|),
    e32 and the maximum taken over a group's rows of one channel.  [rows, n] float64."""
    out = torch.empty_like(ref)
    for r0, r1 in zip(offsets[:-1], offsets[1:]):
        e32 = (cpu32[r0:r1].double() - ref[r0:r1]).abs().amax(0)
        out[r0:r1] = 4.0 * e32 + 8.0 * EPS32 * ref[r0:r1].abs().amax(0).clamp_min(1.0)
    return out


def table_bound(case, ref, cpu32):
    """The bound of a returned (scale | shift) table [G, n]: (4 * e32 + 8 * EPS32) * max(1, |ref|), e32 the restatement's error
    relative to max(1, |ref|), the largest over the ordinary channels of the group; over the mean40 channels of all groups."""
    mag = ref.abs().clamp_min(1.0)
    rel = (cpu32.double() - ref).abs() / mag
    kind = torch.zeros(ref.shape[1], dtype=torch.bool)
    if case.regime == "mean40":
        kind[[ch for ch in MEAN40_CH_2D if ch < ref.shape[1]]] = True
    e32 = torch.zeros_like(ref)
    if bool(kind.any()):            # E[y^2] - mean^2 at mean^2 / var = 1600: one rounding of a number 1600 times the variance, so
        e32[:, kind] = rel[:, kind].max()       # the yardstick is the largest of ALL such samples of the table (convbn_f64_inputs)
    if bool((~kind).any()):
        e32[:, ~kind] = rel[:, ~kind].amax(1, keepdim=True)
    return (4.0 * e32 + 8.0 * EPS32) * mag


def ratio_unit(case):
    return {SPLIT: 2.0 ** -15, F16X2: 2.0 ** -22}[case.conv.dtype]


@functools.lru_cache(maxsize=16)
def bundle(case):
    """Everything a result is held to, on the host problem (float64; no test modifies it): ref (``reference``), rs
    (``restatement``), and per check (target, bound) - raw: the statistics forms' stored output per element (+ raw_ref,
    raw_slack: the target's own allowed distance from the float64 convolution), scale / shift: the returned tables, y: the
    finished output per element."""
    ref, rs, o = reference(case), restatement(case), operands(case)
    b = SimpleNamespace(ref=ref, rs=rs, raw=None, raw_slack=None, scale=None, shift=None, y=None, offsets=offsets_of(case))
    if case.form == "stats":
        a = _im2col(case, o)
        s = a.double().abs() @ o.wv.double().abs().t()
        e32 = (rs.yard.double() - ref.acc).abs().amax(-1, keepdim=True)
        term = fp32_term(e32, s)
        dtype = case.conv.dtype
        if dtype == F32:
            b.raw = (ref.acc, term)
        else:
            b.raw = (rs.raw, term + (pack_step(rs.raw) if dtype == F16X2 else 0.0))
            # (with an input affine the float64 reference transforms the input without rounding: its distance from the target
            #  is the transform's, which e32 holds, not the dropped lo * lo product's)
            b.raw_slack = None if case.xin is not None else (cfi.SPLIT_C if dtype == SPLIT else cfi.F16X2_C) * ratio_unit(case) * s
        b.scale = (ref.scale, table_bound(case, ref.scale, rs.scale))
        b.shift = (ref.shift, table_bound(case, ref.shift, rs.shift))
    else:
        b.y = (ref.y, group_bound(ref.y, rs.y, b.offsets) + store_step(case, ref.y))
    return b


def has_moments(case):
    return case.form == "bnlocal" and case.res is None and not case.relu


def outside(case, result):
    """{check: elements of ``result`` (a restatement-shaped namespace on the host problem) outside its bound}."""
    b = bundle(case)
    out = {}
    for name, got in (("raw", result.raw), ("scale", result.scale), ("shift", result.shift), ("y", result.y)):
        held = getattr(b, name)
        if held is not None:
            target, bound = held
            out[name] = int((~((got.double() - target).abs() <= bound)).sum())
    if has_moments(case):
        lay = layout(case)
        ok = compare_moments(result.y, b.ref.y, b.rs.y, lay.groups, case.rpg)[0]
        out["moments"] = 0 if ok else 1
    return out


def restatement_ratio(case):
    """max |split / f16x2 restatement - ref| / (unit * S) of a statistics case (0 / 0 = 0)."""
    b, o = bundle(case), operands(case)
    s = _im2col(case, o).double().abs() @ o.wv.double().abs().t()
    d = (b.rs.raw - b.ref.acc).abs()
    return torch.where(d == 0, d, d / (ratio_unit(case) * s)).max().item()


# --------------------------------------------------------------------------- the entry points' argument lists
ENTRY_POINTS = {"bnstats": "avs_conv2d_nhwc_bnstats", "bnstats_xin": "avs_conv2d_nhwc_bnstats_xin", "bnlocal": "avs_conv2d_nhwc_bnlocal",
                "affine": "avs_conv2d_nhwc_affine"}
POINTERS = {"bnstats": ("x", "w", "y", "gamma", "beta", "scale", "shift", "ws"),
            "bnstats_xin": ("x", "w", "y", "gamma", "beta", "scale", "shift", "ws", "in_scale", "in_shift"),
            "bnlocal": ("x", "w", "y", "gamma", "beta", "residual"),
            "affine": ("x", "w", "y", "scale", "shift", "residual", "res_scale", "res_shift")}


def desc_fields(formats=0, **changes):
    """conv_f64_inputs.desc_fields + the formats field."""
    fields = cfi.desc_fields(**changes)
    fields[23] = formats
    return fields


def entry_args(entry, a, rpg, ldr=0, ws_bytes=0, in_relu=0, eps=BN_EPS, stream=None):
    """The arguments of an entry point after the descriptor; a = {name: address or None}."""
    if entry in ("bnstats", "bnstats_xin"):
        args = (a["x"], a["w"], a["y"], rpg, a["gamma"], a["beta"], eps, a["scale"], a["shift"], a["ws"], ws_bytes)
        return args + ((a["in_scale"], a["in_shift"], in_relu, stream) if entry == "bnstats_xin" else (stream,))
    if entry == "bnlocal":
        return (a["x"], a["w"], a["y"], rpg, a["gamma"], a["beta"], eps, a.get("residual"), ldr, stream)
    return (a["x"], a["w"], a["y"], rpg, a["scale"], a["shift"], a.get("residual"), ldr, a.get("res_scale"), a.get("res_shift"), stream)


# --------------------------------------------------------------------------- refusals
def refusals():
    """[(label, entry point, status, descriptor changes to a valid 6 x 16 x 4 x 48 -> 64 AVS_F16X2 1x1 call, keyword changes)]:
    one per AVS_REQUIRE of the four entry points (and of bnstats_plan, bnlocal_plan, igemm_plan's AVS_F16P8 and AVS_TILE_224
    requirements) that a shape or an argument can trip before anything is launched.  Keywords: rpg, and null / misalign =
    names of the arguments given as null or 8 bytes off, ws_short = the workspace one byte short."""
    base = dict(dtype=F16X2, n=6, h=16, w=4, cin=48, kh=1, kw=1, ph=0, pw=0, cout=64)
    nine = dict(base, cin=16, kh=3, kw=3, ph=1, pw=1)
    out = [
        ("stats-bf16-only", "bnstats", E_ARG, dict(base, dtype=cfi.ACC64), {}),
        ("stats-activation", "bnstats", E_ARG, dict(base, act=RELU), {}),
        ("stats-rpg-0", "bnstats", E_ARG, base, dict(rpg=0)),
        ("stats-rpg-63", "bnstats", E_UNSUPPORTED, base, dict(rpg=63)),
        ("stats-cout-not-8", "bnstats", E_SHAPE, dict(base, dtype=F16X2, cout=60, y_px_stride=64), {}),
        ("stats-tile-224", "bnstats", E_UNSUPPORTED, dict(base, variant=TILE_224), {}),
        ("stats-p8-cin-48", "bnstats", E_UNSUPPORTED, dict(base, formats=1), {}),
        ("stats-p8-f32", "bnstats", E_UNSUPPORTED, dict(base, dtype=F32, cin=64, formats=1), {}),
        ("stats-null-gamma", "bnstats", E_ARG, base, dict(null=("gamma",))),
        ("stats-null-ws", "bnstats", E_ARG, base, dict(null=("ws",))),
        ("stats-ws-short", "bnstats", E_WORKSPACE, base, dict(ws_short=True)),
        ("stats-ws-misaligned", "bnstats", E_ALIGN, base, dict(misalign=("ws",))),
        ("xin-null-in-scale", "bnstats_xin", E_ARG, nine, dict(null=("in_scale",))),
        ("xin-1x1", "bnstats_xin", E_UNSUPPORTED, base, {}),
        ("xin-128-row-tiles", "bnstats_xin", E_UNSUPPORTED, dict(nine, variant=TILE_128), {}),
        ("xin-misaligned-in-shift", "bnstats_xin", E_ARG, dict(nine, h=9, w=7, n=tall_frames()), dict(rpg=126, misalign=("in_shift",))),
        ("local-rpg-0", "bnlocal", E_ARG, base, dict(rpg=0)),
        ("local-rpg-below-min", "bnlocal", E_UNSUPPORTED, base, dict(rpg=32)),
        ("local-rpg-300", "bnlocal", E_UNSUPPORTED, dict(base, n=75), dict(rpg=300)),
        ("local-ragged-groups", "bnlocal", E_UNSUPPORTED, dict(base, n=7), dict(rpg=128)),
        ("local-cout-72", "bnlocal", E_UNSUPPORTED, dict(base, cout=72), {}),
        ("local-f32", "bnlocal", E_UNSUPPORTED, dict(base, dtype=F32), {}),
        ("local-k-32", "bnlocal", E_UNSUPPORTED, dict(base, cin=32), {}),
        ("local-null-beta", "bnlocal", E_ARG, base, dict(null=("beta",))),
        ("local-y-misaligned", "bnlocal", E_ALIGN, base, dict(misalign=("y",))),
        ("local-residual-stride-short", "bnlocal", E_ALIGN, base, dict(ldr=56)),
        ("local-residual-misaligned", "bnlocal", E_ALIGN, base, dict(misalign=("residual",))),
        ("local-tile-224-at-64-rows", "bnlocal", E_UNSUPPORTED, dict(base, variant=TILE_224), {}),
        ("affine-f32", "affine", E_UNSUPPORTED, dict(base, dtype=F32), {}),
        ("affine-3x3", "affine", E_UNSUPPORTED, nine, {}),
        ("affine-k-32", "affine", E_UNSUPPORTED, dict(base, cin=32), {}),
        ("affine-rpg-31", "affine", E_UNSUPPORTED, base, dict(rpg=31)),
        ("affine-null-scale", "affine", E_ARG, base, dict(null=("scale",))),
        ("affine-res-scale-without-shift", "affine", E_ARG, base, dict(null=("res_shift",))),
        ("affine-res-affine-without-residual", "affine", E_ARG, base, dict(null=("residual",))),
        ("affine-res-scale-misaligned", "affine", E_ALIGN, base, dict(misalign=("res_scale",))),
        ("affine-residual-stride-not-8", "affine", E_ALIGN, base, dict(ldr=68)),
        ("affine-p8-output-cout-72", "affine", E_UNSUPPORTED, dict(base, cout=72, formats=2), {}),
    ]
    return out
