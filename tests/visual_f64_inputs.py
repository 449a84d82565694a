"""Inputs, float64 references, fp32 restatements, planted mistakes and the bound of the per-kernel tests of the visual
front end's BatchNorm and pooling kernels (csrc/visual.hip: avs_bn_batch_stats, avs_bn_apply, avs_pool2d_nhwc,
avs_bn_maxpool_nhwc, avs_global_avgpool_nhwc, avs_segment_mean_f32): test_visual_f64_host.py on the host,
test_gpu_visual_f64.py on the device.  torch-CPU only: both build the same seeded cases from here.

Formats.  An INSTANCE is (fmt, narrow): "f32"; "bf16" wide (narrow None: the 8-channel instances); "bf16" narrow, forced
three ways - "c" (c % 8 != 0), "stride" (a stride % 8 != 0) and "view" (an operand only 8-byte aligned) - and "f16x2",
whose operands are built with emu_pack / emu_unpack of test_gpu_f16x2.py, never with the device's conversion kernels.
Inputs are the values the format STORES (``store``); the float64 references work on those, so operand rounding is not
charged to a kernel.

The bound is scorer_f64_inputs.compare unchanged: 4 * e32 + 8 * eps32 * scale, e32 the error of the same operation
restated in fp32 on the CPU.  A restatement ends with the format's own rounding (``store`` again), so e32 carries the
format's resolution.  scale = max(1, max|ref|); for bn_apply and bn_maxpool max(1, max(|x||scale| + |shift| +
|residual|)), the magnitude of the TERMS, because the affine cancels where mean >> spread.  Where a result is a stored
value or has one rounding in a fixed order the tests ask for equality instead: max pooling without affine equals the
float64 maximum, segment_mean equals a sequential fp32 sum in row order followed by one division.

The restatements follow the kernels' forms: statistics by Welford's update per row-thread and Chan's merge of the
row-threads in thread order (``stats_launch`` restates the launcher's tc / tr / grid.y); apply x*sc + sf (+ res), then
ReLU; average pooling the sum of the in-image taps in (ky, kx) order, divided by k*k, then bias, then ReLU; the global
average sequentially over hw, divided by hw.  ``mistake`` plants one deliberate error (STATS_MISTAKES ...); NOTICED_BY
names, per mistake, the case at which the host test shows it to lie outside the bound in every instance it applies to."""
import functools
from types import SimpleNamespace

import torch

from scorer_f64_inputs import EPS32, SENTINEL, compare  # noqa: F401  (one definition of the bound, shared)
from test_gpu_f16x2 import emu_pack, emu_unpack  # noqa: F401  (the AVS_F16X2 format restated on the CPU, shared)

BN_EPS = 1e-5
INSTANCES = (("f32", None), ("bf16", None), ("bf16", "c"), ("bf16", "stride"), ("bf16", "view"), ("f16x2", None))
STATS_FORMATS = ("f32", "bf16", "f16x2")        # the statistics and the global average have one instance per format

STATS_MISTAKES = ("var_e2", "unbiased", "boundary_off_by_one", "shift_no_scale", "gamma_next_channel")
APPLY_MISTAKES = ("relu_before_residual", "res_stride_ldx", "next_group_affine_last_row")
POOL_MISTAKES = ("zero_pad", "div_by_count", "bias_before_div", "origin_no_pad")
BNMAXPOOL_MISTAKES = ("pool_before_affine", "boundary_image_earlier_group")
GAP_MISTAKES = ("div_hw_plus_1", "drop_last_pixel")


def iname(fmt, narrow):
    return fmt if narrow is None else f"{fmt}-narrow-{narrow}"


# --------------------------------------------------------------------------- formats and layouts
def store(fmt, x):
    """The fp32 values the format stores for x (its own rounding; innermost extent a multiple of 8 for f16x2)."""
    x = x.float()
    if fmt == "f32":
        return x.clone()
    if fmt == "bf16":
        return x.bfloat16().float()
    return emu_unpack(emu_pack(x))


def elem_bytes(fmt):
    return 2 if fmt == "bf16" else 4


def channels(fmt, narrow, base):
    """The channel count of an instance for a case that asks for ``base`` channels: f16x2 and the bf16 instances other
    than narrow-by-c need a multiple of 8; narrow-by-c needs one that is not."""
    if fmt == "f32":
        return base
    if narrow == "c":
        return base if base % 8 else base + 4
    return (base + 7) // 8 * 8


def operand(fmt, narrow, c, which):
    """(ld, off) in elements of operand ``which`` (0 = x, 1 = y, 2 = residual): a window of c columns starting at column
    ``off`` of a matrix whose rows are ``ld`` wide, the matrix itself 256-byte aligned.  The three strides differ pairwise;
    y starts 16 bytes (f32, bf16 wide) or 32 bytes (f16x2) into its rows.  narrow "stride": ldx = c + 12; narrow "view":
    x starts 8 bytes into its rows."""
    ld = c + 8 * (which + 1)
    off = ({"f32": 4, "bf16": 8, "f16x2": 8}[fmt]) if which == 1 else 0
    if narrow == "stride" and which == 0:
        ld += 4
    if narrow == "view" and which == 0:
        off = 4
    return ld, off


def documented_alignment(fmt, narrow):
    """Bytes every activation pointer of an instance is aligned to at least (include/avsum_hip.h)."""
    return {"f32": 16, "f16x2": 32}.get(fmt, 8 if narrow else 16)


def operand_alignment(fmt, ld, off):
    """Largest power of two <= 32 dividing the byte address of every row of an operand."""
    a = 32
    while a > 1 and ((off * elem_bytes(fmt)) % a or (ld * elem_bytes(fmt)) % a):
        a //= 2
    return a


# the launchers' rules (csrc/visual.hip), restated
def stats_launch(fmt, c):
    """(tc, tr, grid.y) of avs_bn_batch_stats: tc = a power of two <= 64 channel-threads of vw channels, tr = 256 / tc."""
    vw = 8 if fmt == "f16x2" else 4
    tc = 1
    while tc < 64 and tc * vw < c:
        tc <<= 1
    return tc, 256 // tc, -(-c // (tc * vw))


def vector_instance(fmt, c, operands, k=None):
    """(element type, V, K3) of the kernel instance avs_bn_apply / avs_pool2d_nhwc / avs_bn_maxpool_nhwc pick for
    ``operands`` = [(ld, off)] (K3 only where ``k`` is given: pool2d)."""
    if fmt == "f32":
        return "float", 4, False
    if fmt == "f16x2":
        return "h2", 8, k == 3
    wide = c % 8 == 0 and all(ld % 8 == 0 and (off * 2) % 16 == 0 for ld, off in operands)
    return "bf16", 8 if wide else 4, wide and k == 3


def _seed(*key):
    """A seed from a key of ints / strings that does not depend on PYTHONHASHSEED."""
    s = 17
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
        s = (s * 131 + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# --------------------------------------------------------------------------- BatchNorm statistics
STATS_C = {"f32": (4, 8, 12, 64, 260), "bf16": (4, 8, 12, 64, 260), "f16x2": (8, 64, 520)}
STATS_REGIMES = ("normal", "mean40", "const")
TAIL_ROWS = 3           # rows after the last group: no kernel may touch them
CONST_GROUP = 5         # the group the "const" regime makes constant (tr + 1 rows)


def group_table(tr):
    """Row offsets of 7 groups for ``tr`` row-threads: a one-row group, an empty one, one smaller than the row-threads,
    another single row, tr - 1 and tr + 1 rows, and one of several trips."""
    return [0, 1, 1, 4, 5, 5 + tr - 1, 5 + 2 * tr, 5 + 2 * tr + 777]


def stats_cases(fmt):
    """(c, regime) the tests run in ``fmt``: every channel count N(0, 1); the smallest and c = 64 in all regimes."""
    cs = STATS_C[fmt]
    return [(c, r) for c in cs for r in STATS_REGIMES if r == "normal" or c in (cs[0], 64)]


@functools.lru_cache(maxsize=None)
def stats_case(fmt, c, regime):
    """x [rows, c] (stored values; the device places it in a matrix of rows c + 8 wide), gamma with both signs and an
    exact 0 in channel 1, beta.  regime "mean40": N(40, 1) per element (mean >> spread); "const": group CONST_GROUP is
    its first row repeated (variance exactly 0)."""
    tc, tr, gy = stats_launch(fmt, c)
    gr = group_table(tr)
    rows = gr[-1] + TAIL_ROWS
    g = _seed("stats", fmt, c, regime)
    x = torch.randn(rows, c, generator=g)
    if regime == "mean40":
        x = x + 40.0
    x = store(fmt, x)
    if regime == "const":
        x[gr[CONST_GROUP]:gr[CONST_GROUP + 1]] = x[gr[CONST_GROUP]]
    gamma = torch.randn(c, generator=g)
    gamma[0], gamma[1], gamma[2] = gamma[0].abs() + 0.5, 0.0, -gamma[2].abs() - 0.5
    beta = torch.randn(c, generator=g)
    return SimpleNamespace(fmt=fmt, c=c, regime=regime, tc=tc, tr=tr, grid_y=gy, group_rows=gr, rows=rows, x=x, gamma=gamma,
                           beta=beta, ldx=c + 8, label=f"{fmt} c={c} {regime}")


def eps32(eps=BN_EPS):
    """eps as the kernels see it (a C float)."""
    return torch.tensor(eps, dtype=torch.float32)


def stats_reference(x, group_rows, gamma, beta, eps=BN_EPS):
    """float64 (scale, shift) [G, c]: biased variance over the group's rows; an empty group gives zeros."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    n_groups = len(group_rows) - 1
    scale, shift = x.new_zeros(n_groups, x.shape[1]), x.new_zeros(n_groups, x.shape[1])
    for g in range(n_groups):
        xg = x[group_rows[g]:group_rows[g + 1]]
        if xg.shape[0] == 0:
            continue
        mu = xg.mean(0)
        var = ((xg - mu) ** 2).mean(0)
        scale[g] = gamma / torch.sqrt(var + eps32(eps).double())
        shift[g] = beta - mu * scale[g]
    return scale, shift


def _fma(a, b, c):
    """fmaf: the product of two fp32 is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def stats_restatement(x, group_rows, gamma, beta, tr, eps=BN_EPS, mistake=None):
    """bn_stats_kernel in fp32 on the CPU: row-thread rt takes rows r0 + rt, r0 + rt + tr, ... through Welford's update
    (with the kernel's two fmaf), row-thread 0 merges the row-threads in order by Chan's formula."""
    assert mistake is None or mistake in STATS_MISTAKES
    x = x.float()
    rows, c = x.shape
    n_groups = len(group_rows) - 1
    one = torch.ones((), dtype=torch.float32)
    scale, shift = torch.zeros(n_groups, c), torch.zeros(n_groups, c)
    if mistake == "gamma_next_channel":
        gamma, beta = gamma.roll(-1), beta.roll(-1)
    for g in range(n_groups):
        r0, r1 = int(group_rows[g]), int(group_rows[g + 1])
        if mistake == "boundary_off_by_one":
            r0, r1 = min(r0 + 1, rows), min(r1 + 1, rows)
        n = r1 - r0
        if n <= 0:
            continue
        xg = x[r0:r1]
        nf = one * float(n)
        if mistake == "var_e2":
            mu = xg.sum(0) / nf
            var = ((xg * xg).sum(0) / nf - mu * mu).clamp_min(0.0)
        else:
            trips = -(-n // tr)
            xs = torch.cat([xg, xg.new_zeros(trips * tr - n, c)]).view(trips, tr, c)
            mean, m2 = torch.zeros(tr, c), torch.zeros(tr, c)
            for t in range(trips):
                live = (t * tr + torch.arange(tr) < n)[:, None]
                d = xs[t] - mean
                mean_new = _fma(d, one / float(t + 1), mean)
                m2 = torch.where(live, _fma(d, xs[t] - mean_new, m2), m2)
                mean = torch.where(live, mean_new, mean)
            acc, mu, s2 = 0, torch.zeros(c), torch.zeros(c)
            for q in range(min(tr, n)):
                nq = (n - q + tr - 1) // tr
                na, nqf = one * float(acc), one * float(nq)
                nn = na + nqf
                d = mean[q] - mu
                mu = mu + d * (nqf / nn)
                s2 = s2 + m2[q] + d * d * (na * nqf / nn)
                acc += nq
            var = (s2 / (one * float(max(n - 1, 1)) if mistake == "unbiased" else nf)).clamp_min(0.0)
        sc = (one / torch.sqrt(var + eps32(eps))) * gamma
        scale[g] = sc
        shift[g] = beta - (mu if mistake == "shift_no_scale" else mu * sc)
    return scale, shift


@functools.lru_cache(maxsize=None)
def stats_bundle(fmt, c, regime):
    """(case, float64 (scale, shift), fp32 restatement), computed once per process; no test modifies them."""
    case = stats_case(fmt, c, regime)
    return (case, stats_reference(case.x, case.group_rows, case.gamma, case.beta),
            stats_restatement(case.x, case.group_rows, case.gamma, case.beta, case.tr))


# --------------------------------------------------------------------------- BatchNorm apply
APPLY_BASE_C = (4, 64)
APPLY_VARIANTS = ("res_relu", "inplace_res", "mgr1_relu_nores", "nogroups")
APPLY_BIG = (32769, 256)      # f32: 2 097 216 vectors, 64 past the 8192 blocks x 256 threads of one trip


def row_groups(group_rows, rows):
    """int64 [rows]: the group of each row, -1 outside every group."""
    gi = torch.full((rows,), -1, dtype=torch.int64)
    for g in range(len(group_rows) - 1):
        gi[group_rows[g]:group_rows[g + 1]] = g
    return gi


@functools.lru_cache(maxsize=None)
def apply_case(fmt, narrow, base_c, variant, big=False):
    """One avs_bn_apply call.  variant "res_relu": residual, ReLU, ldx / ldy / ldr pairwise different; "inplace_res": y is
    x, with a residual, no ReLU; "mgr1_relu_nores": max_group_rows = 1 although groups are larger (the grid-stride loop
    must still cover them), ReLU, no residual; "nogroups": groups == 0, one affine for every row.  scale / shift [G, c]
    have both signs; the rows of the empty group hold NaN, which nothing may read."""
    c = channels(fmt, narrow, base_c)
    tr = stats_launch(fmt, c)[1]
    gr = [0, APPLY_BIG[0]] if big else group_table(tr)
    rows = gr[-1] + (0 if big else TAIL_ROWS)
    g = _seed("apply", fmt, narrow, c, variant, big)
    x = store(fmt, torch.randn(rows, c, generator=g) * 2)
    has_res = variant in ("res_relu", "inplace_res")
    ox, oy, orr = operand(fmt, narrow, c, 0), operand(fmt, narrow, c, 1), operand(fmt, narrow, c, 2)
    if variant == "inplace_res":
        oy = ox
    res_wide = None
    if has_res:        # the whole residual matrix, pad columns included (SENTINEL there): a wrong row stride reads them
        res_wide = torch.full((rows, orr[0]), SENTINEL)
        res_wide[:, orr[1]:orr[1] + c] = torch.randn(rows, c, generator=g)
        res_wide = store(fmt, res_wide)
    grouped = variant != "nogroups"
    n_aff = len(gr) - 1 if grouped else 1
    scale = torch.randn(n_aff, c, generator=g)
    shift = torch.randn(n_aff, c, generator=g)
    gidx = row_groups(gr, rows) if grouped else torch.zeros(rows, dtype=torch.int64)
    if grouped:
        for e in range(n_aff):
            if gr[e] == gr[e + 1]:
                scale[e], shift[e] = float("nan"), float("nan")
    mgr = 1 if variant == "mgr1_relu_nores" else max(b - a for a, b in zip(gr[:-1], gr[1:]))
    return SimpleNamespace(fmt=fmt, narrow=narrow, c=c, variant=variant, rows=rows, group_rows=gr if grouped else None,
                           gidx=gidx, x=x, res_wide=res_wide, res=res_wide[:, orr[1]:orr[1] + c] if has_res else None,
                           scale=scale, shift=shift, relu=variant in ("res_relu", "mgr1_relu_nores"), max_group_rows=mgr,
                           ox=ox, oy=oy, ores=orr if has_res else None, inplace=variant == "inplace_res",
                           label=f"{iname(fmt, narrow)} c={c} {variant}" + (" big" if big else ""))


def apply_reference(case):
    """float64 y [rows, c] (rows outside every group: 0, not compared) and the magnitude of the terms."""
    live = case.gidx >= 0
    gi = case.gidx.clamp_min(0)
    sc, sf = case.scale.double()[gi], case.shift.double()[gi]
    x = case.x.double()
    y = x * sc + sf
    mag = x.abs() * sc.abs() + sf.abs()
    if case.res is not None:
        y = y + case.res.double()
        mag = mag + case.res.double().abs()
    if case.relu:
        y = y.clamp_min(0.0)
    y[~live] = 0.0
    return y, max(1.0, mag[live].max().item())


def apply_restatement(case, mistake=None):
    """bn_apply_kernel in fp32 on the CPU, rounded to the format at the end."""
    assert mistake is None or mistake in APPLY_MISTAKES
    live = case.gidx >= 0
    gi = case.gidx.clamp_min(0).clone()
    if mistake == "next_group_affine_last_row" and case.group_rows is not None:
        gr, n_groups = case.group_rows, len(case.group_rows) - 1
        for g in range(n_groups):
            if gr[g + 1] > gr[g]:
                nxt = (g + 1) % n_groups
                while gr[nxt + 1] == gr[nxt]:
                    nxt = (nxt + 1) % n_groups
                gi[gr[g + 1] - 1] = nxt
    y = case.x * case.scale[gi] + case.shift[gi]
    if mistake == "relu_before_residual" and case.relu:
        y = y.clamp_min(0.0)
    if case.res is not None:
        if mistake == "res_stride_ldx":
            flat = case.res_wide.reshape(-1)
            idx = case.ores[1] + torch.arange(case.rows)[:, None] * case.ox[0] + torch.arange(case.c)[None, :]
            y = y + flat[idx.clamp_max(flat.numel() - 1)]
        else:
            y = y + case.res
    if case.relu:
        y = y.clamp_min(0.0)
    y = store(case.fmt, y)
    y[~live] = 0.0
    return y


@functools.lru_cache(maxsize=None)
def apply_bundle(fmt, narrow, base_c, variant, big=False):
    case = apply_case(fmt, narrow, base_c, variant, big)
    ref, mag = apply_reference(case)
    return case, ref, mag, apply_restatement(case)


# --------------------------------------------------------------------------- pooling
POOL_KSP = ((3, 2, 1), (3, 2, 0), (3, 1, 1), (2, 2, 0), (5, 1, 2))
POOL_MAPS = ((1, 1), (2, 5), (7, 7), (17, 13))
POOL_BASE_C = {"f32": 12, "bf16": 24, "f16x2": 24}
POOL_N = 2
POOL_FLAVOURS = {"max": ("plain", "negative"), "avg": ("plain", "bias_relu")}


def pool_bases(fmt, narrow):
    """Channel counts of the pooling cases of an instance: 12 and 4 where 4 channels make a vector (fp32, bf16 narrow by
    c), 24 elsewhere.  The first is the one bn_maxpool and NOTICED_BY use."""
    return (12, 4) if fmt == "f32" or narrow == "c" else (POOL_BASE_C[fmt],)


def out_extent(h, k, s, p):
    """torch's floor rule; 1 where the padded map is smaller than the window (the window then overhangs the far edge:
    the kernel's only condition is (ho - 1) * s - p < h)."""
    return max(1, (h + 2 * p - k) // s + 1)


def torch_defines(h, w, k, p):
    return h + 2 * p >= k and w + 2 * p >= k and 2 * p <= k


@functools.lru_cache(maxsize=None)
def pool_case(fmt, narrow, base_c, mode, flavour, ksp, hw):
    """x [2, h, w, c] stored values (a channel slice on the device: x_px_stride > c); flavour "negative": every value
    <= -0.5 (a padding of 0 instead of -inf would win); "bias_relu": y = relu(avg(x) + bias) into a channel slice."""
    c = channels(fmt, narrow, base_c)
    (k, s, p), (h, w) = ksp, hw
    g = _seed("pool", fmt, narrow, c, mode, flavour, k, s, p, h, w)
    x = torch.randn(POOL_N, h, w, c, generator=g)
    if flavour == "negative":
        x = -x.abs() - 0.5
    bias = torch.randn(c, generator=g) * 0.5 if flavour == "bias_relu" else None
    return SimpleNamespace(fmt=fmt, narrow=narrow, c=c, mode=mode, flavour=flavour, k=k, s=s, p=p, h=h, w=w, n=POOL_N,
                           ho=out_extent(h, k, s, p), wo=out_extent(w, k, s, p), x=store(fmt, x), bias=bias,
                           relu=flavour == "bias_relu", ox=operand(fmt, narrow, c, 0), oy=operand(fmt, narrow, c, 1),
                           label=f"{iname(fmt, narrow)} c={c} {mode}/{flavour} k{k}s{s}p{p} {h}x{w}")


def window_taps(x, k, s, p, ho, wo, fill):
    """[(tap [n, ho, wo, c], inside [ho, wo] bool)] in (ky, kx) order: tap (ky, kx) of output (oy, ox) is input
    (oy*s - p + ky, ox*s - p + kx), ``fill`` outside the image."""
    n, h, w, c = x.shape
    hh, ww = max(p + h, (ho - 1) * s + k), max(p + w, (wo - 1) * s + k)
    canvas = x.new_full((n, hh, ww, c), fill)
    canvas[:, p:p + h, p:p + w] = x
    inside = torch.zeros(hh, ww, dtype=torch.bool)
    inside[p:p + h, p:p + w] = True
    taps = []
    for ky in range(k):
        for kx in range(k):
            ys, xs = slice(ky, ky + (ho - 1) * s + 1, s), slice(kx, kx + (wo - 1) * s + 1, s)
            taps.append((canvas[:, ys, xs], inside[ys, xs]))
    return taps


def pool_eval(case, dtype, mistake=None, x=None):
    """pool2d_kernel's arithmetic in ``dtype`` (float64: the reference; float32: the restatement before the format's
    rounding): max from -inf over the in-image taps, or the sum of the in-image taps in (ky, kx) order divided by k*k;
    then + bias, then ReLU."""
    assert mistake is None or mistake in POOL_MISTAKES
    x = (case.x if x is None else x).to(dtype)
    p = 0 if mistake == "origin_no_pad" else case.p
    if case.mode == "max":
        fill = 0.0 if mistake == "zero_pad" else float("-inf")
        a = x.new_full((case.n, case.ho, case.wo, case.c), float("-inf"))
        for tap, inside in window_taps(x, case.k, case.s, p, case.ho, case.wo, fill):
            a = torch.maximum(a, tap) if mistake == "zero_pad" else torch.where(inside[None, :, :, None], torch.maximum(a, tap), a)
    else:
        a = x.new_zeros(case.n, case.ho, case.wo, case.c)
        count = torch.zeros(case.ho, case.wo, dtype=dtype)
        for tap, inside in window_taps(x, case.k, case.s, p, case.ho, case.wo, 0.0):
            a = torch.where(inside[None, :, :, None], a + tap, a)
            count = count + inside.to(dtype)
        if mistake == "bias_before_div" and case.bias is not None:
            a = a + case.bias.to(dtype)
        div = count.clamp_min(1.0)[None, :, :, None] if mistake == "div_by_count" else torch.tensor(float(case.k * case.k), dtype=dtype)
        a = a / div
    if case.bias is not None and mistake != "bias_before_div":
        a = a + case.bias.to(dtype)
    if case.relu:
        a = a.clamp_min(0.0)
    return a


def pool_restatement(case, mistake=None):
    return store(case.fmt, pool_eval(case, torch.float32, mistake))


def pool_check(case, got, ref=None, cpu32=None):
    """(ok, err, e32, bound): equality with the float64 maximum for max pooling (a stored value), ``compare`` for the
    average."""
    ref = pool_eval(case, torch.float64) if ref is None else ref
    if case.mode == "max":
        ok = bool(torch.equal(got.double(), ref))
        return ok, 0.0 if ok else float("inf"), 0.0, 0.0
    return compare(got, ref, pool_restatement(case) if cpu32 is None else cpu32)


# --------------------------------------------------------------------------- BatchNorm apply + max pooling
BMP_IMAGES, BMP_HW = 9, (6, 10)
BMP_GROUP_IMAGES = (0, 1, 2, 2, 5, 6, 9)      # singles, an empty group, a triple
BMP_KSP = ((3, 2, 1), (2, 2, 0))


def image_groups(group_rows, n, rows_per_image, mistake=None):
    """The group of each image: the largest g < groups with group_rows[g] <= the image's first row (the kernel's binary
    search); an empty group is never the answer for an image that starts where it 'starts'."""
    out = []
    for img in range(n):
        row = img * rows_per_image
        g = 0
        for e in range(len(group_rows) - 1):
            if (group_rows[e] < row) if mistake == "boundary_image_earlier_group" else (group_rows[e] <= row):
                g = e
        out.append(g)
    return torch.tensor(out, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def bnmaxpool_case(fmt, narrow, base_c, ksp, relu, grouped=True):
    c = channels(fmt, narrow, base_c)
    (k, s, p), (h, w) = ksp, BMP_HW
    g = _seed("bnmaxpool", fmt, narrow, c, k, s, p, relu, grouped)
    x = store(fmt, torch.randn(BMP_IMAGES, h, w, c, generator=g) * 2)
    gr = [i * h * w for i in BMP_GROUP_IMAGES] if grouped else None
    n_aff = len(gr) - 1 if grouped else 1
    scale = torch.randn(n_aff, c, generator=g)
    scale[:, 0], scale[:, 1] = scale[:, 0].abs() + 0.25, -scale[:, 1].abs() - 0.25
    shift = torch.randn(n_aff, c, generator=g)
    if grouped:
        for e in range(n_aff):
            if gr[e] == gr[e + 1]:
                scale[e], shift[e] = float("nan"), float("nan")
    return SimpleNamespace(fmt=fmt, narrow=narrow, c=c, k=k, s=s, p=p, h=h, w=w, n=BMP_IMAGES, relu=relu, group_rows=gr,
                           ho=out_extent(h, k, s, p), wo=out_extent(w, k, s, p), x=x, scale=scale, shift=shift,
                           mode="max", bias=None, ox=operand(fmt, narrow, c, 0), oy=operand(fmt, narrow, c, 1),
                           label=f"{iname(fmt, narrow)} c={c} k{k}s{s}p{p} relu={int(relu)} groups={n_aff if grouped else 0}")


def bnmaxpool_eval(case, dtype, mistake=None):
    """max over the in-image taps of x*scale[g] + shift[g], then ReLU; returns (y, magnitude of the terms)."""
    assert mistake is None or mistake in BNMAXPOOL_MISTAKES
    gi = image_groups(case.group_rows, case.n, case.h * case.w, mistake) if case.group_rows is not None \
        else torch.zeros(case.n, dtype=torch.int64)
    sc, sf = case.scale.to(dtype)[gi][:, None, None, :], case.shift.to(dtype)[gi][:, None, None, :]
    x = case.x.to(dtype)
    plain = SimpleNamespace(**{**vars(case), "relu": False})
    if mistake == "pool_before_affine":
        y = pool_eval(plain, dtype) * sc + sf
    else:
        y = pool_eval(plain, dtype, x=x * sc + sf)
    mag = max(1.0, (x.abs() * sc.abs() + sf.abs()).max().item())
    return (y.clamp_min(0.0) if case.relu else y), mag


def bnmaxpool_restatement(case, mistake=None):
    return store(case.fmt, bnmaxpool_eval(case, torch.float32, mistake)[0])


# --------------------------------------------------------------------------- global average pooling
GAP_SHAPES = ((1, 1, 4), (3, 49, 4), (600, 1, 4), (600, 49, 4), (1, 64, 8), (600, 64, 8), (3, 1, 8), (1, 49, 2048),
              (3, 64, 2048), (3, 1, 2048))      # (n, hw, c): every n, hw and c of the issue; 600 x c/4 threads: 3 blocks


def gap_shapes(fmt):
    return tuple(s for s in GAP_SHAPES if fmt != "f16x2" or s[2] % 8 == 0)


@functools.lru_cache(maxsize=None)
def gap_case(fmt, n, hw, c, view=False):
    """x [n, hw, c] stored values, mean 1 so that the sum grows; view (bf16): x starts 8 bytes into its buffer."""
    g = _seed("gap", fmt, n, hw, c)
    x = store(fmt, torch.randn(n, hw, c, generator=g) + 1.0)
    return SimpleNamespace(fmt=fmt, n=n, hw=hw, c=c, x=x, view=view, ldy=c + 8, off_y=4,
                           label=f"{fmt}{'-view' if view else ''} n={n} hw={hw} c={c}")


def gap_restatement(case, mistake=None):
    """Sequential fp32 sum over hw, divided by hw; the output is fp32 in every format."""
    assert mistake is None or mistake in GAP_MISTAKES
    a = torch.zeros(case.n, case.c)
    for r in range(case.hw - (1 if mistake == "drop_last_pixel" else 0)):
        a = a + case.x[:, r]
    return a / torch.tensor(float(case.hw + (1 if mistake == "div_hw_plus_1" else 0)), dtype=torch.float32)


def gap_reference(case):
    return case.x.double().mean(1)


# --------------------------------------------------------------------------- segment mean
SEGMENT_CASES = tuple((d, tuple(seg)) for d in (1, 33) for seg in ((0, 0, 1, 1, 40, 41), tuple(range(5, 3006))))


@functools.lru_cache(maxsize=None)
def segment_case(d, seg):
    """x [rows, d] as a window of a matrix d + 3 wide; ``seg`` the row offsets (rows before seg[0] and after seg[-1]
    belong to no segment)."""
    rows = seg[-1] + 2
    g = _seed("segment", d, len(seg))
    wide = torch.full((rows, d + 3), SENTINEL)
    wide[:, :d] = torch.randn(rows, d, generator=g) + 0.5
    return SimpleNamespace(d=d, seg=seg, rows=rows, wide=wide, x=wide[:, :d], ldo=d + 5,
                           label=f"d={d} segments={len(seg) - 1}")


def segment_mean_sequential(x, seg):
    """fp32: the rows of a segment added in row order, one division; an empty segment gives zeros."""
    out = torch.zeros(len(seg) - 1, x.shape[1])
    for s, (r0, r1) in enumerate(zip(seg[:-1], seg[1:])):
        if r1 > r0:
            a = torch.zeros(x.shape[1])
            for r in range(r0, r1):
                a = a + x[r]
            out[s] = a / torch.tensor(float(r1 - r0), dtype=torch.float32)
    return out


# --------------------------------------------------------------------------- which case notices which mistake
# Per mistake: the arguments of the case constructor after (fmt[, narrow]) - the same case in every instance.
NOTICED_BY = {
    # statistics: (c, regime); c = 64 is run by every format
    "var_e2": (64, "mean40"),                       # 40^2 * eps32 against a variance of 1
    "unbiased": (64, "normal"),                     # groups of 3 rows: sqrt(3/2)
    "boundary_off_by_one": (64, "normal"),
    "shift_no_scale": (64, "mean40"),
    "gamma_next_channel": (64, "normal"),
    # apply: (base_c, variant)
    "relu_before_residual": (64, "res_relu"),
    "res_stride_ldx": (64, "res_relu"),
    "next_group_affine_last_row": (64, "res_relu"),
    # pooling: (mode, flavour, ksp, hw)
    "zero_pad": ("max", "negative", (3, 2, 1), (7, 7)),
    "div_by_count": ("avg", "plain", (3, 1, 1), (7, 7)),
    "bias_before_div": ("avg", "bias_relu", (3, 1, 1), (7, 7)),
    "origin_no_pad": ("avg", "plain", (3, 2, 1), (17, 13)),
    # bn_maxpool: (ksp, relu)
    "pool_before_affine": ((3, 2, 1), False),
    "boundary_image_earlier_group": ((3, 2, 1), False),
    # global average: (n, hw, c)
    "div_hw_plus_1": (3, 64, 2048),
    "drop_last_pixel": (3, 64, 2048),
}
