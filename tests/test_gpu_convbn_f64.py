"""The bf16 convolution + BatchNorm kernels of the throughput path, each on its own against float64: conv1x1_bn_kernel
(avs_conv1x1_bn_bf16, avs_conv1x1_bn_in_bf16, avs_conv1x1_affine_bf16 without and with a residual affine) and
bn_gram_affine_kernel (avs_bn_gram_affine_bf16) of csrc/convbn.hip, the bf16 instances of avs_conv2d_nhwc_bnstats and
avs_conv2d_nhwc_bnlocal of csrc/igemm.hip, and the fused stem avs_stem_conv_bn_pool_bf16 of csrc/stem.hip.  Cases,
references, restatements and the bound come from convbn_f64_inputs;
test_convbn_f64_host.py shows on the host that the bound passes the restatement and fails every planted mistake, and that
the cases reach all 12 + 4 kernel instances of convbn.hip and the three branches of ``live``.

The order of operations the restatement follows, and which these tests thereby pin (convbn.hip, the header):
  * a transformed input is a = bf16(relu(x * in_scale + in_shift)), product and sum rounded separately (avs_bn_apply's
    arithmetic: held bit for bit against avs_bn_apply here);
  * statistics from the fp32 accumulators before any rounding, var = max(E[y^2] - mean^2, 0), scale = gamma / sqrt(var +
    eps), shift = beta - mean * scale;
  * the output is t = bf16(fma(acc, scale, shift));
  * with a residual there is an INTERMEDIATE bf16 rounding: t is rounded to bf16 first, then the sum is rounded again,
    bf16(t + r), or bf16(t + (r * rs + rh)) with a residual affine; ReLU comes last.
The float64 reference has none of these roundings: relu(acc * scale + shift + residual') on the exact products.

Every output is held per (group, output channel) to 4 * e32 + 8 * EPS32 * scale (scorer_f64_inputs.compare), e32 and scale
over that group's rows of that channel; the two-pass and tile-local cases without residual and ReLU also to the moments
check, each (group, channel) against its own restatement moment (convbn_f64_inputs.compare_moments); returned (scale,
shift) directly, with scale exactly 0 where gamma is 0.  Every destination - the (scale, shift) and the map of
avs_conv2d_nhwc_bnstats and of the stem included, which are called through the C ABI for that - is pre-filled with NaN
inside its window and a sentinel in its pad columns and in the rows after the last group: the window must be finite
afterwards, the rest bit for bit untouched.  Every call runs twice into fresh destinations and must give the same bits.
Where the header promises bit identity it is asserted: conv1x1_bn_in against avs_bn_apply + conv1x1_bn, the stored d_a_out
of the Gram kernel against avs_bn_apply.

The fused stem (avs_stem_conv_bn_pool_bf16, csrc/stem.hip) reads the image avs_frames_normalize_u8 would write in bf16
(held here to bf16((v / denom - mean) / std) for all 256 byte values per channel); its (scale, shift) are held to float64
statistics of the exact products, the pooled raw map (apply = 0: the maximum where gamma >= 0, the minimum elsewhere) and
the finished map (apply = 1) per (group, channel) to the float64 pooled map; apply = 0 followed by avs_bn_apply equals
apply = 1 bit for bit.

RATIO lines (printed per check; run with -s).  Measured on an MI355X, per kernel family over all cases of this file (err
and e32 both against float64), with the check that came closest to its bound:

  family                      checks  max err/e32  closest to the bound
  conv1x1 two-pass  y         18      1.00         rpg=161 k=128 n=256 const, relu, padded, ch 168: err 1.5e-2, bound 5.9e-2
  conv1x1 two-pass  moments   13      2.36         rpg=257 k=64 n=64 mean40, mean of ch 1 (gamma 0): err 3.0e-3, bound 1.2e-2
  conv1x1 affine    y         18      1.00         rpg=130 k=72 n=200 mean40, residual, relu, ch 183: err 2.5e-2, bound 1.0e-1
  conv1x1 affine+ra y         18      1.00         rpg=1 k=8 n=8 normal, input affine, relu, ch 0: err 2.8e-3, bound 1.1e-2
  bn_gram_affine    scale     26      1.46         k=128 n=32 rpg=130 G=1 mean40, in place: err 9.5e-5, bound 3.8e-4
  bn_gram_affine    shift     26      1.50         k=128 n=32 rpg=130 G=3 mean40, in place: err 5.4e-4, bound 2.2e-3
  conv2d bnlocal    y         18      1.20         9 x 7x7, 72 -> 64, 1x1, mean40, ch 14: err 2.2e-3, bound 7.5e-3
  conv2d bnlocal    moments   12      16.5         2 x 14x14, 32 -> 128, 3x3, mean40, slope of ch 9: err 2.2e-4, bound 4.1e-4
  conv2d bnstats    raw       51      1.00         3 x 14x14, 32 -> 128, 3x3, mean40, group 1 ch 14: err 1.2e-1, bound 5.0e-1
  conv2d bnstats    scale     15      2.80         5 x 14x14, 64 -> 64, 3x3 / 2, pairs of frames, mean40: err 3.2e-4, bound 8.4e-4
  conv2d bnstats    shift     15      1.54         the same case: err 1.1e-2, bound 3.0e-2
  stem              scale     5       1.43         n=2, frames_per_group=1 (the single-colour frame): err 1.3e-2, bound 3.7e-2
  stem              shift     5       1.43         the same case: err 3.6e-3, bound 1.0e-2
  stem              y         12      1.00         n=2, frames_per_group=1, apply=1, relu=0, ch 28: err 1.8e-2, bound 7.3e-2

Every output check sits at err / e32 = 1.00 (a quarter of its bound): the restatement follows the kernels' order of
operations, so the kernels' largest error is half a bf16 step of the stored result, as the restatement's; the tile-local
form's 1.20 is one output of a mean40 channel rounding the other way.  The returned affines exceed 1 where mean >> spread:
E[y^2] - mean^2 in fp32 (the Gram kernel's C = a^T a / R - m m^T likewise) loses one rounding of a number 1600 times the
variance, in the kernel and in the restatement alike but not the same one.  The moments rows give the (moment, group,
channel) pair closest to its own bound, 4 * e32 + 8 * EPS32 + half a bf16 step of the pair over sqrt(R): the largest err /
e32 belong to pairs whose own restatement moment is nearly 0 and where one or two device outputs of a mean40 channel round
the other way (the pair at 16.5 uses 0.54 of its bound, the floor); a gamma == 0 pair's err is its e32, the rounding of
beta.  No test here takes more than 0.3 s.
"""
from types import SimpleNamespace

import pytest
import torch

import convbn_f64_inputs as cfi

pytestmark = pytest.mark.gpu

S = cfi.SENTINEL
NAN = float("nan")
TAIL_ROWS = 3


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _place(values, ld, off, dev, tail=0):
    """values [rows, c] (fp32 numbers bf16 holds) in columns [off, off + c) of a bf16 matrix ``ld`` wide with ``tail`` more
    rows; everything else holds the sentinel: (the matrix on the device, the window)."""
    rows, c = values.shape
    assert ld >= off + c
    wide = torch.full((rows + tail, ld), S)
    wide[:rows, off:off + c] = values
    buf = wide.bfloat16().to(dev)
    return buf, buf[:rows, off:off + c]


def _read(buf, before, rows, off, c):
    """The window as fp32 on the CPU, after asserting that the pad columns and the rows after the last group are bit for
    bit what they were and that the window is finite."""
    a, b = _bits(buf).clone(), _bits(before).clone()
    got = buf[:rows, off:off + c].float().cpu()
    a[:rows, off:off + c] = 0
    b[:rows, off:off + c] = 0
    assert torch.equal(a, b), "a pad column or a row after the last group was written"
    assert torch.isfinite(got).all(), "a destination element was left unwritten or is not finite"
    return got


def _ratio(family, label, name, err, e32, bound):
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO family={family!r} case={label!r} tensor={name} err={err:.3e} e32={e32:.3e} bound={bound:.3e} "
          f"err/e32={ratio:.2f}")


def _check_groups(family, label, got, ref, cpu32, groups, rpg, name="y"):
    ok, (err, e32, bound, gi, ci) = cfi.compare_groups(got, ref, cpu32, groups, rpg)
    _ratio(family, label, f"{name}[g={gi},ch={ci}]", err, e32, bound)
    assert ok, f"{family} {label} {name} group {gi} channel {ci}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"


def _check_moments(family, label, got, ref, cpu32, groups, rpg):
    ok, err, e32, bound, (mi, gi, ci) = cfi.compare_moments(got, ref, cpu32, groups, rpg)
    _ratio(family, label, f"moments[m={mi},g={gi},ch={ci}]", err, e32, bound)
    assert ok, f"{family} {label} moment {mi} group {gi} channel {ci}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"


def _check_affine(family, label, got, ref, cpu32, gamma, per_group=False):
    """Returned (scale, shift) [G, n] against float64: compare on the whole tensor, or per group over its channels (the
    stem: every channel of a group is alike, and a single-colour group's cancellation loosens only itself); scale exactly
    0 where gamma is 0."""
    for name, y, r, c in zip(("scale", "shift"), got, ref, cpu32):
        assert torch.isfinite(y).all(), (label, name)
        parts = [(f"{name}[g={g}]", y[g], r[g], c[g]) for g in range(y.shape[0])] if per_group else [(name, y, r, c)]
        for pname, yy, rr, cc in parts:
            ok, err, e32, bound = cfi.compare(yy, rr, cc)
            _ratio(family, label, pname, err, e32, bound)
            assert ok, f"{family} {label} {pname}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"
    assert (got[0][:, gamma == 0] == 0).all(), "gamma == 0: scale must be exactly 0"


def _f32(t, dev):
    return None if t is None else t.contiguous().to(dev)


# --------------------------------------------------------------------------- conv1x1_bn_kernel
def _launch_conv(ops, abi, case, xw, wd, ops_dev, yw, res):
    lib, p, st = abi.lib(), ops._p, ops._stream()
    gamma, beta, isc, ish, psc, psh, rsc, rsh = ops_dev
    ldr = res.stride(0) if res is not None else 0
    if case.form == "two_pass" and not case.xf:
        abi.check(lib.avs_conv1x1_bn_bf16(p(xw), xw.stride(0), case.k, p(wd), wd.stride(0), case.n, case.rpg, case.groups,
                                          p(gamma), p(beta), cfi.BN_EPS, p(res), ldr, int(case.relu), p(yw), yw.stride(0), st),
                  "avs_conv1x1_bn_bf16")
    elif case.form == "two_pass":
        abi.check(lib.avs_conv1x1_bn_in_bf16(p(xw), xw.stride(0), case.k, p(isc), p(ish), p(wd), wd.stride(0), case.n, case.rpg,
                                             case.groups, p(gamma), p(beta), cfi.BN_EPS, p(res), ldr, int(case.relu), p(yw),
                                             yw.stride(0), st), "avs_conv1x1_bn_in_bf16")
    else:
        abi.check(lib.avs_conv1x1_affine_bf16(p(xw), xw.stride(0), case.k, p(isc), p(ish), p(wd), wd.stride(0), case.n,
                                              case.rpg, case.groups, p(psc), p(psh), p(res), ldr, p(rsc), p(rsh),
                                              int(case.relu), p(yw), yw.stride(0), st), "avs_conv1x1_affine_bf16")


def _run_conv(dev, case):
    ops, abi = _api()
    xbuf, xw = _place(case.x, case.lin_stride, 0, dev)
    _, wd = _place(case.w, case.k + (8 if case.padded else 0), 0, dev)
    rbuf = res = None
    if case.res is not None:
        rbuf, res = _place(case.res, case.ldr, 0, dev)
    pre = case.pre if case.pre is not None else (None, None)
    ops_dev = tuple(_f32(t, dev) for t in (case.gamma, case.beta, case.isc, case.ish, pre[0], pre[1], case.rsc, case.rsh))
    outs = []
    for _ in range(2):
        ybuf, yw = _place(torch.full((case.rows, case.n), NAN), case.ldc, case.off_y, dev, TAIL_ROWS)
        before = ybuf.clone()
        _launch_conv(ops, abi, case, xw, wd, ops_dev, yw, res)
        outs.append((_read(ybuf, before, case.rows, case.off_y, case.n), _bits(ybuf)))
    assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
    assert torch.equal(_bits(xbuf), _bits(_place(case.x, case.lin_stride, 0, "cpu")[0])), "the input was written"
    if rbuf is not None:
        assert torch.equal(_bits(rbuf), _bits(_place(case.res, case.ldr, 0, "cpu")[0])), "the residual was written"
    if case.xf:     # bit for bit avs_bn_apply on x first, then the same kernel without an input affine
        grows = torch.arange(0, case.rows + 1, case.rpg, dtype=torch.int64, device=dev)
        a_dev = ops.bn_apply(xw, ops_dev[2], ops_dev[3], grows, case.rpg, None, ops.ACT_RELU)
        assert torch.equal(a_dev.float().cpu(), case.a), "avs_bn_apply is not bf16(relu(x * sc + sh))"
        plain = SimpleNamespace(**{**vars(case), "xf": False})
        ybuf, yw = _place(torch.full((case.rows, case.n), NAN), case.ldc, case.off_y, dev, TAIL_ROWS)
        _launch_conv(ops, abi, plain, a_dev, wd, ops_dev[:2] + (None, None) + ops_dev[4:], yw, res)
        assert torch.equal(_bits(ybuf), outs[0][1]), "the input affine differs from avs_bn_apply followed by the plain kernel"
    return outs[0][0]


@pytest.mark.parametrize("form", cfi.FORMS)
@pytest.mark.parametrize("si", range(len(cfi.CONV_SHAPES)), ids=[f"rpg{s[0]}-k{s[1]}-n{s[2]}-G{s[3]}" for s in cfi.CONV_SHAPES])
def test_conv1x1_bn(dev, si, form):
    """One shape of the table in one statistics form, in the regimes normal, mean40 and const; the input affine, the
    residual, ReLU and the padded strides (lin_stride = k + 8, ldb = k + 8, ldc = n + 16 with y from column 8, ldr =
    n + 8) vary with the shape, the form and the regime (convbn_f64_inputs.conv_options)."""
    for regime in cfi.REGIMES:
        case, ref, cpu32 = cfi.conv_bundle(si, form, regime)
        got = _run_conv(dev, case)
        _check_groups(f"conv1x1 {form}", case.label, got, ref, cpu32, case.groups, case.rpg)
        if cfi.has_moments(case):
            _check_moments(f"conv1x1 {form}", case.label, got, ref, cpu32, case.groups, case.rpg)
        if form == "two_pass" and not case.relu and case.res is None:
            # gamma == 0: the output is bf16(beta) in every row; a constant channel (rows_per_group 1: every channel) too
            assert (got[:, 1] == cfi.bf(case.beta[1])).all()
        if regime == "const" and not case.relu and case.res is None and form == "two_pass":
            g0 = case.const_group * case.rpg
            assert (got[g0:g0 + case.rpg, cfi.CONST_CH] == cfi.bf(case.beta[cfi.CONST_CH])).all()


# --------------------------------------------------------------------------- bn_gram_affine_kernel
def _gram_ids():
    return [f"k{k}-n{n}-rpg{r}-G{g}-{reg}-xf{int(xf)}-{st}" for k, n, r, g, reg, xf, st in cfi.gram_case_keys()]


@pytest.mark.parametrize("key", cfi.gram_case_keys(), ids=_gram_ids())
def test_bn_gram_affine(dev, key):
    """k in {64, 128}, n in {32, 96, 160}, groups of 1, 63, 64, 65 and 130 rows (the LDS tile is 64 rows), 1 and 3 groups;
    the input affine off and on; d_a_out off, into a separate buffer (lda = k + 8) and in place.  scale and shift against
    float64 statistics of the exact products; in mean40 mean^2 / variance is about 1600 in input channels 8..15."""
    ops, abi = _api()
    case, ref, cpu32 = cfi.gram_bundle(*key)
    lib, p = abi.lib(), ops._p
    _, wd = _place(case.w, case.k + 8, 0, dev)
    gamma, beta, isc, ish = (_f32(t, dev) for t in (case.gamma, case.beta, case.isc, case.ish))
    outs = []
    for _ in range(2):
        xbuf, xw = _place(case.x, case.lin_stride, 0, dev, TAIL_ROWS)
        xbefore = xbuf.clone()
        abuf = aw = abefore = None
        if case.store == "separate":
            abuf, aw = _place(torch.full((case.rows, case.k), NAN), case.lda, 0, dev, TAIL_ROWS)
            abefore = abuf.clone()
        elif case.store == "inplace":
            abuf, aw, abefore = xbuf, xw, xbefore
        scale = torch.full((case.groups + 1, case.n), NAN, device=dev)
        shift = torch.full((case.groups + 1, case.n), NAN, device=dev)
        abi.check(lib.avs_bn_gram_affine_bf16(p(xw), xw.stride(0), case.k, p(isc), p(ish), p(wd), wd.stride(0), case.n, case.rpg,
                                              case.groups, p(gamma), p(beta), cfi.BN_EPS, p(scale), p(shift), p(aw),
                                              aw.stride(0) if aw is not None else 0, ops._stream()), "avs_bn_gram_affine_bf16")
        assert torch.isnan(scale[-1]).all() and torch.isnan(shift[-1]).all(), "a row after the last group was written"
        stored = None
        if aw is not None:
            stored = _read(abuf, abefore, case.rows, 0, case.k)
        if case.store != "inplace":
            assert torch.equal(_bits(xbuf), _bits(xbefore)), "the input was written"
        outs.append((scale[:-1].cpu(), shift[:-1].cpu(), stored))
    (scale, shift, stored), again = outs
    assert torch.equal(_bits(scale), _bits(again[0])) and torch.equal(_bits(shift), _bits(again[1])), "two runs differ"
    if stored is not None:      # bit for bit avs_bn_apply's bf16(relu(x * sc + sh))
        assert torch.equal(stored, again[2])
        xbuf, xw = _place(case.x, case.lin_stride, 0, dev)
        grows = torch.arange(0, case.rows + 1, case.rpg, dtype=torch.int64, device=dev)
        a_dev = ops.bn_apply(xw, isc, ish, grows, case.rpg, None, ops.ACT_RELU)
        assert torch.equal(stored, a_dev.float().cpu()) and torch.equal(stored, case.a)
    _check_affine("bn_gram_affine", case.label, (scale, shift), ref, cpu32, case.gamma)


# --------------------------------------------------------------------------- conv2d + statistics, conv2d + tile-local BN
def _conv2d_operands(ops, dev, case):
    xd = case.x.bfloat16().to(dev)
    wd = case.wt.bfloat16().to(dev)
    return xd, wd, case.gamma.to(dev), case.beta.to(dev), ops.dtype_code(torch.bfloat16)


@pytest.mark.parametrize("shape", cfi.LOCAL_SHAPES, ids=[str(s).replace(" ", "") for s in cfi.LOCAL_SHAPES])
def test_conv2d_bnlocal(dev, shape):
    """avs_conv2d_nhwc_bnlocal in bf16: groups of 49, 64, 100 and 196 rows (tiles of 5, 4, 2 and 1 groups, a last tile with
    fewer), 1x1 and 3x3 / pad 1, stride 1 and 2; the finished output per (group, channel) and the moments check."""
    ops, _ = _api()
    for regime, with_res, relu in (("normal", False, False), ("mean40", False, False), ("const", True, True)):
        case = cfi.conv2d_case("local", shape, regime, with_res, relu)
        ge = case.ge
        xd, wd, gamma, beta, code = _conv2d_operands(ops, dev, case)
        assert ops.conv_bnlocal_tile_rows(code, *ge.geom, *ge.xs, wd.shape[1], ge.cout, ge.rpg) == 256 // ge.rpg * ge.rpg
        res = _place(case.res, ge.cout, 0, dev)[1] if with_res else None
        outs = []
        for _ in range(2):
            ybuf, _ = _place(torch.full((ge.rows, ge.cout), NAN), ge.cout, 0, dev, TAIL_ROWS)
            before = ybuf.clone()
            ops.conv2d_raw(code, *ge.geom, xd, *ge.xs, wd, wd.stride(0), ybuf, ge.cout,
                           act=ops.ACT_RELU if relu else ops.ACT_NONE, bnlocal=(ge.rpg, gamma, beta, cfi.BN_EPS, res))
            outs.append((_read(ybuf, before, ge.rows, 0, ge.cout), _bits(ybuf)))
        assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
        got, ref, cpu32 = outs[0][0], cfi.local_reference(case), cfi.local_restatement(case)
        groups = ge.rows // ge.rpg
        _check_groups("conv2d bnlocal", case.label, got, ref, cpu32, groups, ge.rpg)
        if not with_res and not relu:
            _check_moments("conv2d bnlocal", case.label, got, ref, cpu32, groups, ge.rpg)


def _spare_row_affine(groups, n, dev):
    """scale, shift [groups + 1, n] of NaN: the spare row must still be NaN after the call."""
    return torch.full((groups + 1, n), NAN, device=dev), torch.full((groups + 1, n), NAN, device=dev)


def _take_affine(scale, shift, label):
    assert torch.isnan(scale[-1]).all() and torch.isnan(shift[-1]).all(), f"{label}: a row after the last group was written"
    sc, sh = scale[:-1].cpu(), shift[:-1].cpu()
    assert torch.isfinite(sc).all() and torch.isfinite(sh).all(), f"{label}: scale / shift left unwritten or not finite"
    return sc, sh


def _bnstats_into(ops, abi, code, ge, xd, wd, ybuf, gamma, beta, groups, dev):
    """avs_conv2d_nhwc_bnstats through the C ABI into destinations of the caller (ops.conv2d_raw allocates its own)."""
    import ctypes
    lib, p = abi.lib(), ops._p
    d = abi.ConvDesc(code, *ge.geom, *ge.xs, wd.stride(0), ge.cout, ops.ACT_NONE, 1.0, 0, 0, 0)
    need = int(lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(d), ge.rpg))
    assert need > 0
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    scale, shift = _spare_row_affine(groups, ge.cout, dev)
    abi.check(lib.avs_conv2d_nhwc_bnstats(ctypes.byref(d), p(xd), p(wd), p(ybuf), ge.rpg, p(gamma), p(beta), cfi.BN_EPS,
                                          p(scale), p(shift), p(ws), need, ops._stream()), "avs_conv2d_nhwc_bnstats")
    assert (ws[need:] == 0xA5).all(), "the workspace was written past the size the library asked for"
    return _take_affine(scale, shift, "avs_conv2d_nhwc_bnstats")


@pytest.mark.parametrize("shape", cfi.STATS_SHAPES, ids=[str(s).replace(" ", "") for s in cfi.STATS_SHAPES])
def test_conv2d_bnstats(dev, shape):
    """avs_conv2d_nhwc_bnstats in bf16: groups of 64 rows and more that straddle the row tiles, the last group shorter; the
    raw output bf16(acc) per (group, channel) and (scale, shift) against float64 statistics of the unrounded products.
    Called through the C ABI, so that scale and shift are the test's own NaN-filled buffers with a spare row."""
    ops, abi = _api()
    for regime in cfi.REGIMES:
        case = cfi.conv2d_case("stats", shape, regime)
        ge = case.ge
        xd, wd, gamma, beta, code = _conv2d_operands(ops, dev, case)
        assert ops.conv_bnstats_ok(code, *ge.geom, *ge.xs, wd.shape[1], ge.cout, ge.rpg)
        offsets = cfi.stats_groups(ge.rows, ge.rpg)
        outs = []
        for _ in range(2):
            ybuf, _ = _place(torch.full((ge.rows, ge.cout), NAN), ge.cout, 0, dev, TAIL_ROWS)
            before = ybuf.clone()
            sc, sh = _bnstats_into(ops, abi, code, ge, xd, wd, ybuf, gamma, beta, len(offsets) - 1, dev)
            outs.append((_read(ybuf, before, ge.rows, 0, ge.cout), _bits(ybuf), sc, sh))
        assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(_bits(outs[0][2]), _bits(outs[1][2])) \
            and torch.equal(_bits(outs[0][3]), _bits(outs[1][3])), "two runs differ"
        via_ops = ops.conv2d_raw(code, *ge.geom, xd, *ge.xs, wd, wd.stride(0), torch.empty_like(ybuf), ge.cout,
                                 bnstats=(ge.rpg, gamma, beta, cfi.BN_EPS))
        assert torch.equal(_bits(via_ops[0]), _bits(outs[0][2])) and torch.equal(_bits(via_ops[1]), _bits(outs[0][3]))
        got, _, sc, sh = outs[0]
        assert sc.shape == (len(offsets) - 1, ge.cout)
        for g, (r0, r1) in enumerate(zip(offsets[:-1], offsets[1:])):
            _check_groups("conv2d bnstats", case.label, got[r0:r1], case.acc64[r0:r1], cfi.bf(case.acc32[r0:r1]), 1, r1 - r0,
                          name=f"raw[g={g}]")
        _check_affine("conv2d bnstats", case.label, (sc, sh),
                      cfi.ragged_stats(case.acc64, offsets, case.gamma, case.beta, torch.float64),
                      cfi.ragged_stats(case.acc32, offsets, case.gamma, case.beta, torch.float32), case.gamma)


# --------------------------------------------------------------------------- the fused stem
@pytest.mark.parametrize("denom", (1.0, 255.0))
def test_frames_normalize_bf16_every_byte_value(dev, denom):
    """avs_frames_normalize_u8 in bf16 equals bf16((v / denom - mean) / std) for all 256 byte values of every channel; the
    fourth channel and the padding are 0."""
    ops, _ = _api()
    frame = cfi.all_bytes_frame()
    outs = []
    for _ in range(2):
        out = torch.full((1, 19, 20, 4), NAN, dtype=torch.bfloat16, device=dev)
        ops.frames_normalize(frame.to(dev), torch.bfloat16, denom, cfi.STEM_MEAN, cfi.STEM_STD, 19, 20, 1, 3, out=out)
        outs.append(out.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    got = outs[0].float()
    lut = cfi.normalize_lut(denom)
    want = torch.zeros(1, 19, 20, 4)
    for c in range(3):
        want[0, 1:17, 3:19, c] = lut[c][frame[0, :, :, c].long()]
    assert torch.equal(got, want)


def _stem_into(ops, abi, dev, fd, wk, n, fpg, gd, bd, apply, relu):
    """avs_stem_conv_bn_pool_bf16 through the C ABI into the test's own destinations (ops.stem_conv_bn_pool allocates its
    own): y [n * 56 * 56 + TAIL_ROWS, 64] NaN in the map and the sentinel after it, scale / shift NaN with a spare row,
    a fresh workspace of exactly the size the library asks for.  Returns (y [n, 56, 56, 64] on the device, scale, shift)."""
    import ctypes
    lib, p = abi.lib(), ops._p
    rows = n * 56 * 56
    ybuf, _ = _place(torch.full((rows, 64), NAN), 64, 0, dev, TAIL_ROWS)
    before = ybuf.clone()
    scale, shift = _spare_row_affine(n // fpg, 64, dev)
    need = int(lib.avs_stem_workspace_bytes(n))
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    m3, s3 = (ctypes.c_float * 3)(*cfi.STEM_MEAN), (ctypes.c_float * 3)(*cfi.STEM_STD)
    abi.check(lib.avs_stem_conv_bn_pool_bf16(p(fd), n, cfi.STEM_DENOM, m3, s3, p(wk), wk.stride(0), fpg, p(gd), p(bd),
                                             cfi.BN_EPS, int(apply), int(relu), p(ybuf), p(scale), p(shift), p(ws), need,
                                             ops._stream()), "avs_stem_conv_bn_pool_bf16")
    _read(ybuf, before, rows, 0, 64)        # the map finite, the rows after it untouched
    assert (ws[need:] == 0xA5).all(), "the workspace was written past the size the library asked for"
    sc, sh = _take_affine(scale, shift, "avs_stem_conv_bn_pool_bf16")
    return ybuf[:rows].view(n, 56, 56, 64), sc, sh


@pytest.mark.parametrize("n,fpg", cfi.STEM_CASES)
def test_fused_stem(dev, n, fpg):
    """(frames, frames per group) in {(2, 1), (3, 3), (4, 2)}, one frame a single colour, gamma of both signs and a zero;
    apply in {0, 1} x relu in {0, 1}."""
    ops, abi = _api()
    from avsum_amd.cnn import _stem_weight
    case, _, _, ref_aff, cpu_aff = cfi.stem_bundle(n, fpg)
    fd = case.frames.to(dev)
    # the operand: the image avs_frames_normalize_u8 writes in bf16 is the table's
    x0 = ops.frames_normalize(fd, torch.bfloat16, cfi.STEM_DENOM, cfi.STEM_MEAN, cfi.STEM_STD, 224, 224, 0, 0)
    assert torch.equal(x0[..., :3].float().cpu().permute(0, 3, 1, 2), cfi.stem_image(case)) and (x0[..., 3] == 0).all()
    wk = _stem_weight(case.w4, 8, torch.bfloat16).to(dev)
    gd, bd = case.gamma.to(dev), case.beta.to(dev)
    rows = fpg * 56 * 56
    finished = {}
    for apply in (0, 1):
        for relu in (0, 1):
            runs = [_stem_into(ops, abi, dev, fd, wk, n, fpg, gd, bd, apply, relu) for _ in range(2)]
            (y, sc, sh), (y2, sc2, sh2) = runs
            assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(sc), _bits(sc2)) and torch.equal(_bits(sh), _bits(sh2))
            label = f"{case.label} apply={apply} relu={relu}"
            got = y.float().cpu().view(-1, 64)
            if (apply, relu) == (0, 0):
                _check_affine("stem", label, (sc, sh), ref_aff, cpu_aff, case.gamma, per_group=True)
                first = (sc, sh)
                via_ops = ops.stem_conv_bn_pool(fd, wk, cfi.STEM_DENOM, cfi.STEM_MEAN, cfi.STEM_STD, fpg, gd, bd, cfi.BN_EPS,
                                                relu=False, apply=False)
                assert torch.equal(_bits(via_ops[0]), _bits(y)) and torch.equal(_bits(via_ops[1]), _bits(sc))
            else:
                assert torch.equal(sc, first[0]) and torch.equal(sh, first[1])
            _check_groups("stem", label, got, cfi.stem_reference(n, fpg, apply, relu), cfi.stem_restatement(n, fpg, apply, relu),
                          case.groups, rows)
            finished[(apply, relu)] = y
    # apply = 0 followed by avs_bn_apply: apply = 1 bit for bit
    grows = torch.arange(0, n + 1, fpg, dtype=torch.int64, device=dev) * 56 * 56
    sc, sh = first[0].to(dev), first[1].to(dev)
    for relu in (0, 1):
        fin = ops.bn_apply(finished[(0, relu)].view(-1, 64), sc, sh, grows, rows, None, ops.ACT_RELU if relu else ops.ACT_NONE)
        assert torch.equal(_bits(fin.view(-1, 64)), _bits(finished[(1, relu)].view(-1, 64)))
