"""Cases, float64 references, restatements and the error bound of the per-instance tests of avs_gemm_nt
(test_gemm_f64_host.py on the host, test_gpu_gemm_f64.py on the device).  torch-CPU only: both build the same seeded
cases from here.

``plan`` restates, for the geometry avs_gemm_nt sets (HoWo = Wo = H = W = 1, cin = K, KW = 1, variant 0), the part of
igemm_plan (csrc/igemm.hip) that chooses the instance of igemm_kernel: (es, bn, rowb, pipe, wr, fastk, epi).  Its three
thresholds are READ from the AVS_RULE lines of igemm.hip (RULES), so a retuned rule moves the plans and fails the
host test's reach assertion instead of silently moving a case onto another instance.

The case table (CASES) is built from the rules: for every dtype, every class of reduction length (below one step, whole
steps without the pipeline, pipelined with the generic staging / with the scalar tap walk, 128-byte steps generic / tap
walk, fast64_only) on 64- and on 128-wide column tiles under each of the three epilogue forms; the row and column
counts either side of a tile; the six epilogue orders; the attention's strided batches; lda = 0; the destination
layouts; the 256-row tiles; M = 0.

Two operand sets per case: "a" - N(0, 1) with the rows of A scaled by 1, 1e-3 and 1e3 in turn, so that an error in a
small row cannot hide under the matrix maximum; "b" - small integers (|x| <= 8, bf16 <= 4), for which every partial sum
is exact in fp32 whatever the summation order (``exact_headroom``), so the result has to EQUAL the float64 product
(after one bf16 rounding for bf16).

The 256-row cases need 2048 tall tiles, half a million rows.  Their A repeats a base of TALL_PERIOD = 1021 rows (a
prime: no multiple of a tile, a wave or a store pass), built on the device by index, so the reference is 1021 rows of
float64 and every one of the rows is still compared; a row written from another row passes only if the two are a
multiple of 1021 rows apart.

The bound is per element.  With S = |alpha| * |A| @ |B|^T + |bias| in float64 and e32_i the largest error over row i of
the same expression evaluated in fp32 on the CPU:
    AVS_F32        |got - ref| <= 4 * e32_i + 8 * eps32 * S
    AVS_F32_ACC64  |got - ref| <= 8 * eps32 * S
    AVS_BF16       |got - ref| <= half a bf16 step of ref + the fp32 term
    AVS_F32_SPLIT  |got - restatement| <= the fp32 term, and |restatement - ref| <= SPLIT_C * 2^-15 * S
(restatement: hi = bf16(x), lo = bf16(x - hi), ah*bh + ah*bl + al*bh in float64).  SPLIT_C is twice the largest ratio
of the restatement over all split cases, measured on the CPU against the float64 reference (never against the kernel):
see SPLIT_C_MEASURED."""
import collections
import functools
import math
import os
import re
import zlib
from types import SimpleNamespace

import torch

F32, BF16, ACC64, SPLIT = 0, 1, 2, 3                 # AVS_F32, AVS_BF16, AVS_F32_ACC64, AVS_F32_SPLIT (avsum_hip.h)
DTYPES = (F32, BF16, ACC64, SPLIT)
DTYPE_NAMES = {F32: "f32", BF16: "bf16", ACC64: "acc64", SPLIT: "split"}
NONE, COL, ROW = 0, 1, 2                             # AVS_BIAS_*
RELU = 1                                             # AVS_ACT_RELU
EPS32 = 2.0 ** -23
TALL_PERIOD = 1021
MAGNITUDES = (1.0, 1e-3, 1e3)                         # of the rows of A in operand set "a", in turn
SPLIT_C_MEASURED = 0.4233      # largest |restatement - ref| / (2^-15 * S) over every split case and both operand sets
SPLIT_C = 2 * SPLIT_C_MEASURED
MISTAKES = ("last_step_dropped", "row_bias_by_column", "alpha_after_bias", "relu_before_bias", "b_stride_ignored",
            "tile_seam", "bf16_twice", "split_drop_al_bh")


# --------------------------------------------------------------------------- the rules, read from the source
def _source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = [d for d in sorted(os.listdir(root)) if os.path.isfile(os.path.join(root, d, "csrc", "igemm.hip"))]
    assert len(dirs) == 1, dirs
    return os.path.join(root, dirs[0], "csrc", "igemm.hip")


def read_rules(path=None):
    """{name: value} of the ``AVS_RULE g_<name> = <int>;`` lines of igemm.hip."""
    with open(path or _source()) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^AVS_RULE\s+g_(\w+)\s*=\s*(\d+)\s*;", f.read(), re.M)}


RULES = read_rules()


def plan(dtype, m, n, k, batch=1, bias_mode=NONE, act=0, alpha=1.0, lda=None, rules=None):
    """(es, bn, rowb, pipe, wr, fastk, epi) of avs_gemm_nt for these arguments, as igemm_plan chooses them (ldb and the
    batch strides small enough for the buffer window, as every case here has them)."""
    r = rules or RULES
    assert r["pipe3"] == 1
    es = 2 if dtype == BF16 else 4
    plain = bias_mode == NONE and act == 0 and alpha == 1.0
    brelu = bias_mode == COL and act == RELU and alpha == 1.0
    few_f32 = dtype == F32 and batch == 1 and -(-m // 128) * -(-n // 128) < 256
    narrow = n <= 64 or dtype == ACC64 or few_f32
    bn = 64 if narrow else 128
    can = dtype in (BF16, SPLIT) and (plain or brelu) and k * es > 128 and batch == 1
    tall = can and -(-m // 256) * -(-n // bn) >= r["tall_min_tiles"] and (narrow or k * es >= r["tall_min_k_bytes"])
    fast64_only = k % (64 // es) == 0 and k % (128 // es) != 0
    rowb = 64 if tall or fast64_only or k * es <= r["rowb_threshold_bytes"] else 128
    pipe = rowb == 64 and dtype != ACC64 and k * es > 2 * rowb
    window = (256 * (k if lda is None else lda) + k) * es < 2 ** 31
    fastk = dtype != ACC64 and window and k % (rowb // es) == 0
    return es, bn, rowb, pipe, 4 if pipe and tall else 2, fastk, "plain" if plain else "brelu" if brelu else "any"


# --------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "name dtype m n k batch bias_mode act alpha lda sa ldb sb ldc col0 sc sbias "
                                      "via_linear period")
EPILOGUES = {                      # name: (bias mode, activation, alpha)
    "plain": (NONE, 0, 1.0), "brelu": (COL, RELU, 1.0), "col": (COL, 0, 1.0), "row": (ROW, 0, 1.0),
    "scaled_brelu": (COL, RELU, 0.125), "neg_row": (ROW, 0, -1.5)}


def _case(name, dtype, m, n, k, epi="plain", batch=1, lda=None, sa=None, ldb=None, sb=None, pad=0, col0=0, sc=None,
          sbias=None, via_linear=False, period=None):
    bias_mode, act, alpha = EPILOGUES[epi]
    lda = k if lda is None else lda
    ldb = k if ldb is None else ldb
    ldc = n + pad
    assert col0 + n <= ldc
    blen = {NONE: 0, COL: n, ROW: m}[bias_mode]
    return Case(f"{DTYPE_NAMES[dtype]}-{name}-{epi}", dtype, m, n, k, batch, bias_mode, act, alpha, lda,
                (m * lda if batch > 1 else 0) if sa is None else sa, ldb, (n * ldb if batch > 1 else 0) if sb is None else sb,
                ldc, col0, (m * ldc if batch > 1 else 0) if sc is None else sc, blen if sbias is None else sbias,
                via_linear, period)


def _k_classes(dtype):
    """[(K, is the representative of its class)]: the issue's reduction lengths, in elements of this dtype."""
    f32 = [(4, False), (12, True), (16, False), (32, True), (36, False), (52, True), (48, True), (512, False), (516, True),
           (544, True), (528, False)]
    return [(k * 2, rep) for k, rep in f32] if dtype == BF16 else f32


def _build_cases():
    cases = []
    rot = ("plain", "brelu", "neg_row")      # the three epilogue forms: EPI_PLAIN, EPI_BRELU, EPI_ANY
    for dtype in DTYPES:
        # 1. every class of reduction length on 64- and on 128-wide column tiles under each epilogue form (AVS_F32
        #    reaches the wide tile batched only; AVS_F32_ACC64 has no wide tile)
        for wide in (False, True):
            if wide and dtype == ACC64:
                continue
            for i, (k, rep) in enumerate(_k_classes(dtype)):
                for epi in (rot if rep else (rot[(i + wide) % 3],)):
                    if wide:
                        cases.append(_case(f"k{k}-wide", dtype, 37, 129, k, epi, batch=2 if dtype == F32 else 1))
                    else:
                        cases.append(_case(f"k{k}", dtype, 37, 40, k, epi, ldb=k + 16 if i % 2 else None))
        # 2. rows and columns either side of a tile (AVS_F32 unbatched stays on 64-wide tiles: N = 65, 129, 200 are 2 .. 4
        #    column tiles with a tail); the six epilogues in turn
        k = 104 if dtype == BF16 else 52
        pairs = [(m, n) for m in (1, 127, 128, 129, 257) for n in (1, 63, 64, 65, 127, 128, 129, 200)]
        for i, (m, n) in enumerate(pairs):
            cases.append(_case(f"m{m}-n{n}", dtype, m, n, k, list(EPILOGUES)[i % 6], pad=(0, 3, 8)[i % 3]))
        # 3. the six epilogues on one shape with a row and a column tail
        for epi in EPILOGUES:
            cases.append(_case("epilogue-m70-n90", dtype, 70, 90, 2 * k, epi, pad=6))
        # 4. the attention's calls: heads as the batch inside the rows of one [T, heads * d] matrix (lda = e, stride_a = d),
        #    a shared B (stride_b = 0), the context's C interleaved the same way (stride_c = d < M * ldc), and a C with
        #    a gap between batch entries; bias strides of 0 and of one bias length
        d = 24 if dtype == BF16 else 12
        for heads, t in ((3, 50), (5, 21)):
            e = heads * d
            cases.append(_case(f"heads{heads}-qk", dtype, t, t, d, "plain" if heads == 3 else "neg_row", batch=heads, lda=e, sa=d,
                               ldb=e, sb=d, pad=3, sc=t * (t + 3) + 7, sbias=0 if heads == 3 else None))
            cases.append(_case(f"heads{heads}-shared-b", dtype, t, 2 * d, d, "scaled_brelu", batch=heads, lda=e, sa=d, sb=0,
                               pad=0, sc=t * 2 * d + 16, sbias=0 if heads == 5 else None))
            cases.append(_case(f"heads{heads}-ctx", dtype, t, d, d, "row", batch=heads, ldb=d, pad=e - d, sc=d, sbias=0))
        cases.append(_case("bt2-n129-gap", dtype, 130, 129, 2 * d, "col", batch=2, pad=3, sc=130 * 132 + 5))
        # 5. lda = 0: every row of A is the one row
        cases.append(_case("lda0", dtype, 70, 40, 4 * d, "neg_row", lda=0, pad=3))
        # 6. destinations: ldc = N + 3, and a column slice of a wider buffer at a column offset through ops.linear(out=)
        cases.append(_case("ldc-n+3", dtype, 130, 70, 4 * d, "brelu", pad=3))
        #    (ops.linear takes AVS_F32 and AVS_BF16; the other two get the same layout through the entry point itself)
        lin = dtype in (F32, BF16)
        cases.append(_case("out-slice", dtype, 33, 96, 4 * d, "col", pad=40, col0=16, via_linear=lin))
        cases.append(_case("out-slice-m1", dtype, 1, 40, 4 * d, "plain", pad=24, col0=8, via_linear=lin))
        # 7. M = 0: AVS_OK and nothing written
        cases.append(_case("m0", dtype, 0, 40, 4 * d, "col", pad=3))
    # 8. AVS_F32 on the 128-wide tile unbatched: 256 tiles of 128 x 128, the first size past few_f32
    cases.append(_case("m2048-n2048-k16", F32, 2048, 2048, 16, "brelu"))
    # 9. the bf16 store: 16-byte vectors only for a 16-byte-aligned C with 16-byte row strides.  Full tiles, a row tail
    #    and a column tail with col + 8 > N on the vector path; the scalar path by an odd row stride and by a C that is
    #    2-byte but not 16-byte aligned
    for tag, nfull, ntail in (("narrow", 64, 45), ("wide", 256, 141)):
        cases.append(_case(f"store-vec-full-{tag}", BF16, 256, nfull, 64, "brelu"))
        cases.append(_case(f"store-vec-tails-{tag}", BF16, 130, ntail, 64, "col", pad=3))             # ldc = N + 3: 48, 144
        cases.append(_case(f"store-odd-ldc-{tag}", BF16, 130, ntail, 64, "col", pad=2))
        cases.append(_case(f"store-odd-ldc-full-{tag}", BF16, 128, nfull, 64, "plain", pad=1))
        cases.append(_case(f"store-unaligned-c-{tag}", BF16, 130, ntail, 64, "brelu", pad=11, col0=1))   # ldc = 56, 152
        cases.append(_case(f"store-unaligned-c-full-{tag}", BF16, 128, nfull, 64, "plain", pad=8, col0=3))
    # 10. the 256-row tiles: 2048 tall tiles with a one-row last tile; on 64-wide tiles (N = 8) from three steps on, on
    #     128-wide tiles (N = 129: two column tiles, 1024 row tiles) from 1024 bytes of reduction on; generic staging
    #     and tap walk; EPI_PLAIN and EPI_BRELU.  No cheaper shape reaches wr == 4: the rule counts tiles, and
    #     N <= 64 already has the fewest columns per tile
    for dtype, ks_narrow, ks_wide in ((BF16, (80, 96), (520, 512)), (SPLIT, (52, 48), (260, 256))):
        for epi in ("plain", "brelu"):
            for k in ks_narrow:
                cases.append(_case(f"tall-n8-k{k}", dtype, 2047 * 256 + 1, 8, k, epi, pad=8, period=TALL_PERIOD))
            for k in ks_wide:
                cases.append(_case(f"tall-n129-k{k}", dtype, 1023 * 256 + 1, 129, k, epi, pad=7, period=TALL_PERIOD))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(cases)


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def case_plan(case, rules=None):
    return (case.dtype,) + plan(case.dtype, case.m, case.n, case.k, case.batch, case.bias_mode, case.act, case.alpha,
                                case.lda, rules)


def rows(case):
    """Rows of A (and of the reference) that are distinct: the base of a periodic case, else M."""
    return min(case.m, case.period) if case.period else case.m


# --------------------------------------------------------------------------- operands
def _tdt(case):
    return torch.bfloat16 if case.dtype == BF16 else torch.float32


@functools.lru_cache(maxsize=64)
def operands(case, which):
    """The operand set ``which`` ("a" random, "b" small integers) of a case.  a_buf / b_buf / bias_buf are the flat
    buffers the entry point is given (fp32 values; bf16 cases hold bf16-representable values), A [batch, rows, K],
    B [batch or 1, N, K] and bias [batch or 1, len] the logical operands in fp32.  Nothing here is modified by a test."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{which}".encode()))
    nr = max(1, 1 if case.lda == 0 else rows(case))
    nbb = case.batch if case.sb else 1
    mag = torch.tensor(MAGNITUDES)[torch.arange(nr) % 3][None, :, None]
    top = 4 if case.dtype == BF16 else 8
    if which == "a":
        a = torch.randn(case.batch, nr, case.k, generator=g) * mag
        b = torch.randn(nbb, case.n, case.k, generator=g)
    else:
        a = torch.randint(-top, top + 1, (case.batch, nr, case.k), generator=g).float()
        b = torch.randint(-top, top + 1, (nbb, case.n, case.k), generator=g).float()
    a, b = a.to(_tdt(case)).float(), b.to(_tdt(case)).float()
    a_buf = torch.zeros((case.batch - 1) * case.sa + (nr - 1) * case.lda + case.k)
    a_view = a_buf.as_strided((case.batch, nr, case.k), (case.sa, case.lda, 1))
    a_view.copy_(a)
    assert torch.equal(a_view, a), "A overlaps itself"
    b_buf = torch.zeros((nbb - 1) * case.sb + (case.n - 1) * case.ldb + case.k)
    b_view = b_buf.as_strided((nbb, case.n, case.k), (case.sb, case.ldb, 1))
    b_view.copy_(b)
    assert torch.equal(b_view, b), "B overlaps itself"
    bias = bias_buf = None
    if case.bias_mode != NONE:
        blen = case.n if case.bias_mode == COL else case.m
        nb = case.batch if case.sbias else 1
        if which == "a":
            # of the size of the products it is added to (per row for a row bias), either sign: the ReLU clips about
            # half the outputs, and the orders of alpha, bias and ReLU all give different results
            bias = torch.randn(nb, blen, generator=g) * abs(case.alpha) * math.sqrt(case.k)
            if case.bias_mode == ROW:
                bias = bias * torch.tensor(MAGNITUDES)[(torch.arange(blen) % nr if case.lda == 0 else torch.arange(blen)) % 3]
            else:
                bias = bias * 30.0     # the middle rows' products are ~ sqrt(K); the large rows' ~ 1e3 sqrt(K)
        else:
            bias = torch.randint(-2 * top, 2 * top + 1, (nb, blen), generator=g).float()
        bias_buf = bias.reshape(-1).clone()
        assert case.sbias in (0, blen)
    if case.lda == 0:
        a = a.expand(case.batch, max(1, case.m), case.k)
    return SimpleNamespace(a_buf=a_buf, b_buf=b_buf, bias_buf=bias_buf, A=a[:, :rows(case)] if case.m else a[:, :0], B=b,
                           bias=bias)


def exact_headroom(case):
    """(largest possible |partial sum| of operand set "b" in units of its step, largest |operand|): the first below
    2^24 makes every fp32 partial sum exact in any order; the second below 2^8 makes the operands exact in bf16, so
    AVS_BF16 rounds once (the output) and AVS_F32_SPLIT's lo halves are zero."""
    top = 4 if case.dtype == BF16 else 8
    step = {1.0: 1.0, 0.125: 0.125, -1.5: 0.5}[case.alpha]       # every partial sum is a multiple of it
    return (abs(case.alpha) * case.k * top * top + (2 * top if case.bias_mode != NONE else 0)) / step, top


# --------------------------------------------------------------------------- reference, restatement, bound
def _biases(case, o, dtype, mistake=None):
    """(column bias, row bias) broadcastable to [batch, rows, N] in ``dtype``; zeros where the mode has none."""
    zero = torch.zeros((), dtype=dtype)
    if case.bias_mode == COL:
        return o.bias.to(dtype)[:, None, :], zero
    if case.bias_mode == ROW:
        brow = o.bias.to(dtype)[:, :, None]
        if mistake == "row_bias_by_column":
            brow = o.bias.to(dtype)[:, torch.arange(case.n) % case.m][:, None, :]
        return zero, brow
    return zero, zero


def reference(case, which):
    """float64 act(alpha * A @ B^T + bias): [batch, rows, N]."""
    o = operands(case, which)
    bcol, brow = _biases(case, o, torch.float64)
    v = case.alpha * (o.A.double() @ o.B.double().transpose(1, 2)) + bcol + brow
    return v.clamp_min(0) if case.act == RELU else v


def magnitude(case, which):
    """S = |alpha| * |A| @ |B|^T + |bias| in float64."""
    o = operands(case, which)
    bcol, brow = _biases(case, o, torch.float64)
    return abs(case.alpha) * (o.A.double().abs() @ o.B.double().abs().transpose(1, 2)) + bcol.abs() + brow.abs()


def applies(case, mistake):
    """Does the planted mistake change what this case computes (by more than a rounding)?"""
    es, bn, rowb = case_plan(case)[1:4]
    if case.m == 0:
        return False
    many = case.m * case.n >= 64        # the data-dependent ones need a few dozen outputs to meet a clipped / cancelled one
    return {"last_step_dropped": case.k % (rowb // es) != 0,
            "row_bias_by_column": case.bias_mode == ROW and case.m > 1 and case.n > 1,
            "alpha_after_bias": case.alpha != 1.0 and case.bias_mode != NONE,
            "relu_before_bias": case.act == RELU and case.bias_mode != NONE and many,
            "b_stride_ignored": case.batch > 1 and case.sb != 0,
            # (under a ReLU the copied column shows only in rows where it or the right one is positive)
            "tile_seam": case.n > bn and (case.act != RELU or case.m >= 8),
            # (a second rounding moves a few per cent of the outputs, by at most a step: it needs a thousand of them)
            "bf16_twice": case.dtype == BF16 and case.bias_mode != NONE and case.m * case.n >= 1024,
            "split_drop_al_bh": case.dtype == SPLIT}[mistake]


def _fma(acc, alpha, b):
    """fmaf(acc, alpha, b) on fp32 tensors: the product is exact in float64, the sum rounded once to fp32 (a second
    rounding from float64 moves the result only from within 2^-29 of a tie)."""
    return (acc.double() * alpha + b.double()).float()


def restatement(case, which, mistake=None):
    """The case in the kernel's order of operations, as float64 [batch, rows, N] holding what the kernel should store:
    fp32 products summed in fp32 (AVS_F32, AVS_BF16), the fp32 sums of the reduction steps summed in float64 (AVS_F32_ACC64),
    ah*bh + ah*bl + al*bh in float64 (AVS_F32_SPLIT); then fmaf(acc, alpha, bcol), the row bias, [one bf16 rounding,]
    the ReLU - ACC64: (float)(acc64 * alpha) + bcol.
    ``mistake``: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    o = operands(case, which)
    es, bn, rowb = case_plan(case)[1:4]
    a, b = o.A, o.B
    if mistake == "last_step_dropped":
        a = a.clone()
        a[:, :, case.k // (rowb // es) * (rowb // es):] = 0
    if mistake == "b_stride_ignored":
        b = b[:1]
    bt = b.transpose(1, 2)
    bcol, brow = _biases(case, o, torch.float64 if case.dtype == SPLIT else torch.float32, mistake)
    if case.dtype == SPLIT:
        ah, bh = a.bfloat16().double(), bt.bfloat16().double()
        al, bl = (a.double() - ah).bfloat16().double(), (bt.double() - bh).bfloat16().double()
        acc = ah @ bh + ah @ bl + (0 if mistake == "split_drop_al_bh" else al @ bh)
    elif case.dtype == ACC64:
        acc = torch.zeros(case.batch, a.shape[1], case.n, dtype=torch.float64)
        step = rowb // es          # a reduction step: 16 fp32 elements, 32 past the 64-byte-step threshold
        for k0 in range(0, case.k, step):
            acc += (a[:, :, k0:k0 + step] @ bt[:, k0:k0 + step]).double()
    else:
        acc = a @ bt
    plain = case.bias_mode == NONE and case.act == 0 and case.alpha == 1.0
    bias = bcol + brow
    relu = (lambda x: x.clamp_min(0)) if case.act == RELU else (lambda x: x)
    if mistake == "alpha_after_bias":
        v = (acc + bias) * case.alpha
    elif mistake == "relu_before_bias":
        v, relu = (acc * case.alpha).clamp_min(0) + bias, (lambda x: x)
    elif mistake == "bf16_twice":
        v = (acc * case.alpha).bfloat16().float() + bias
    elif plain:
        v = acc
    elif case.dtype == SPLIT:
        v = acc * case.alpha + bcol + brow
    elif case.dtype == ACC64:
        v = (acc * case.alpha).float() + bcol + brow
    else:
        v = _fma(acc, case.alpha, bcol) + brow
    if case.dtype != SPLIT:
        v = v.float()
    if case.dtype == BF16:
        v = v.bfloat16()
    v = relu(v).double()
    if mistake == "tile_seam":
        v[:, :, bn] = v[:, :, 0]
    return v


def fp32_yardstick(case, which):
    """The same expression in fp32 on the CPU (for every dtype: plain fp32 sums, no bf16 rounding, no split)."""
    o = operands(case, which)
    bcol, brow = _biases(case, o, torch.float32)
    acc = o.A @ o.B.transpose(1, 2)
    plain = case.bias_mode == NONE and case.act == 0 and case.alpha == 1.0
    v = acc if plain else _fma(acc, case.alpha, bcol) + brow
    return (v.clamp_min(0) if case.act == RELU else v).double()


def bf16_half_step(ref):
    """Half the spacing of bf16 (8 significant bits) at |ref|, elementwise; 0 at 0."""
    mant, exp = torch.frexp(ref.abs())               # |ref| = mant * 2^exp, mant in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), exp - 9))


def fp32_term(e32, s):
    """The fp32 bound's form: 4 * e32 (the fp32 CPU evaluation's largest error in the row) + 8 * eps32 * S."""
    return 4.0 * e32 + 8.0 * EPS32 * s


@functools.lru_cache(maxsize=8)
def bundle(case, which):
    """(ref, target, bound, e32 per row, S) of a case and operand set, float64 [batch, rows, N], computed once and shared;
    a result must lie within ``bound`` of ``target``: the reference, for AVS_F32_SPLIT its restatement."""
    ref, s = reference(case, which), magnitude(case, which)
    e32 = (fp32_yardstick(case, which) - ref).abs().amax(-1, keepdim=True) if ref.numel() else ref.new_zeros(ref.shape[:2] + (1,))
    term = fp32_term(e32, s)
    if case.dtype == ACC64:
        return ref, ref, 8.0 * EPS32 * s, e32, s
    if case.dtype == BF16:
        return ref, ref, bf16_half_step(ref) + term, e32, s
    if case.dtype == SPLIT:
        return ref, restatement(case, which), term, e32, s
    return ref, ref, term, e32, s


def split_ratio(case, which):
    """max |restatement - ref| / (2^-15 * S) of a split case (0 / 0 = 0)."""
    ref, s = reference(case, which), magnitude(case, which)
    if not ref.numel():
        return 0.0
    d = (restatement(case, which) - ref).abs()
    return torch.where(d == 0, d, d / (2.0 ** -15 * s)).max().item()


def exact_result(case, which="b"):
    """What operand set "b" has to give, bit for bit: the float64 product, rounded once to bf16 for AVS_BF16."""
    ref = reference(case, which)
    if case.dtype == BF16:
        # the ReLU commutes with the rounding (monotone, keeps the sign)
        return ref.float().bfloat16().double()
    assert torch.equal(ref.float().double(), ref)
    return ref


# --------------------------------------------------------------------------- refusals
def refusals():
    """[(label, status with operands given, status with null operands, changes)]: ``changes`` are the arguments that
    differ from a valid 8 x 8 x 8 fp32 call.  With null operands the library's order of checks puts "null operand"
    (AVS_E_ARG) before the checks of K, the strides, ldc and the upper batch limit."""
    return [("k-not-16-bytes", -2, -1, dict(k=6)), ("k-not-16-bytes-bf16", -2, -1, dict(dtype=BF16, k=12, lda=16, ldb=16)),
            ("lda-not-16-bytes", -3, -1, dict(lda=10)), ("ldb-not-16-bytes", -3, -1, dict(ldb=10)),
            ("stride-a-not-16-bytes", -3, -1, dict(batch=2, sa=66, sb=64, sc=64)),
            ("stride-b-not-16-bytes", -3, -1, dict(batch=2, sa=64, sb=66, sc=64)),
            ("ldb<k", -2, -2, dict(ldb=4)), ("lda<0", -2, -2, dict(lda=-8)), ("ldc<n", -2, -1, dict(ldc=7)),
            ("batch-0", -2, -2, dict(batch=0)), ("batch-65536", -2, -1, dict(batch=65536)),
            ("bias-mode-3", -1, -1, dict(bias_mode=3)), ("bias-mode--1", -1, -1, dict(bias_mode=-1)),
            ("bias-mode-without-bias", -1, -1, dict(bias_mode=1)), ("bad-dtype", -1, -1, dict(dtype=7)),
            ("n-0", -2, -2, dict(n=0))]


def refusal_args(changes, a=None, b=None, c=None):
    """The positional arguments of avs_gemm_nt for a valid 8 x 8 x 8 call with ``changes`` applied; operands a, b, c
    (None: null pointers - whatever the status, nothing can then be launched)."""
    v = dict(dtype=F32, m=8, n=8, k=8, lda=8, sa=0, ldb=8, sb=0, ldc=8, sc=0, bias_mode=0, sbias=0, alpha=1.0, act=0, batch=1)
    v.update(changes)
    return (v["dtype"], v["m"], v["n"], v["k"], a, v["lda"], v["sa"], b, v["ldb"], v["sb"], c, v["ldc"], v["sc"], None,
            v["bias_mode"], v["sbias"], v["alpha"], v["act"], v["batch"], None)
