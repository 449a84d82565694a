"""The two fused attention kernels of csrc/attention.hip, each on its own against float64, through the C ABI
(avs_mhsa_flash_f32: flash_mhsa_kernel<D, 2 | 4>; avs_mhsa_flash_f16x2: flash_mhsa_h2q16_kernel<D, 4>) with no projection
GEMM between the kernel and the check.  Cases, reference, yardsticks and the bound come from mhsa_f64_inputs (see its
docstring): strided Q, K, V and ctx buffers whose other columns hold a sentinel, head dims 64, 128 and 256, T on both
sides of the key tile (32) and of the query tiles (16 / 32 per wave, 64 / 128 per workgroup) on both wave counts of the
fp32 kernel, one row of 1031 keys, and value regimes that move the running maximum (peaked, rising and falling ramps,
scores of +-250) next to the flat softmax of the module-level tests.  tests/test_mhsa_f64_host.py shows on the CPU that
the bound accepts a correct online-softmax kernel at every case and rejects nine planted mistakes.

Per case: the result within 4 * e + 8 * eps32 * scale of float64 (e = the fp32 yardstick's error), pad columns and guard
rows of ctx untouched, inputs unchanged, T = 1 exact, twin query rows and twin batch entries bit-identical, a second
launch bit-identical.

Measured on an MI355X: the largest err / e per kernel, head dim and regime over all cases of this file, err and e both
against the float64 reference (the bound allows 4 plus the floor):

    kernel  D     flat  peaked  ramp_up  ramp_down  huge  offset_v  tiny_v  equal_keys  twins
    f32     64    3.13  1.05    1.00     1.00       1.00  1.01              1.56        1.73
    f32    128    3.75  1.03    1.00     1.01       1.00  1.09              1.02        1.85
    f32    256    3.42  2.93    2.32     3.17       1.79  1.23              1.32        1.84
    f16x2   64    2.59  1.19    1.54     0.95       0.79  1.33      0.82    1.79        1.29
    f16x2  128    2.69  0.95    0.73     1.07       1.37  1.05      0.90    1.85        1.06
    f16x2  256    2.58  1.72    1.76     1.29       1.51  0.98      0.99    2.21        1.16

The flat column's largest ratios are all the row of 1031 keys (err 2.0e-7 to 2.3e-7 against e 5.5e-8 to 6.7e-8 for fp32:
far inside the bound of 1.2e-6 by its floor; at T <= 257 the flat ratios are at most 2.21).  Closest to the bound: the fp32
kernel at head dim 256 on ramp_down, T = 65, b = 1, heads = 2: err 4.9e-5, e 1.5e-5, bound 6.4e-5 (0.77 of it) - the
score is one fp32 chain of 256 products of magnitude up to 50 * 16, where the CPU's blocked sum rounds less.  No case
needed the yardstick restated in the online form.  With the lo halves of every split forced to zero (the accuracy-study
build, make fp16emu) 187 of the 201 f16x2 cases fall outside the bound, by factors of 6 to 1500 of e."""
import pytest
import torch

import mhsa_f64_inputs as mfi

pytestmark = pytest.mark.gpu

S = mfi.SENTINEL
FAMILIES = [(kind, d) for kind in mfi.KINDS for d in mfi.HEAD_DIMS]


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _launch(case, qd, kd, vd, ctx):
    """The kernel under test on device buffers laid out as mhsa_f64_inputs.buffers states."""
    ops, abi = _api()
    name = "avs_mhsa_flash_f32" if case.kind == "f32" else "avs_mhsa_flash_f16x2"
    fn = getattr(abi.lib(), name)
    abi.check(fn(ops._p(qd, case.col0), ops._p(kd, case.col0), ops._p(vd, case.col0), case.ld, case.b, case.t, case.heads,
                 case.d, ops._p(ctx, case.ldo + case.ocol0), case.ldo, ops._stream()), name)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _run_case(dev, spec):
    case, ref, yard = mfi.bundle(spec)
    qb, kb, vb, blank = mfi.buffers(case)
    qd, kd, vd = qb.to(dev), kb.to(dev), vb.to(dev)
    outs = []
    for _ in range(2):
        ctx = blank.to(dev)
        _launch(case, qd, kd, vd, ctx)
        outs.append(ctx.cpu())
    full = outs[0]
    assert torch.equal(_bits(full), _bits(outs[1])), f"{case.label}: a second launch gave other bits"
    for buf, dbuf in ((qb, qd), (kb, kd), (vb, vd)):
        assert torch.equal(_bits(dbuf.cpu()), _bits(buf)), f"{case.label}: an input was written"
    c0, e = case.ocol0, case.e
    got = full[1:1 + case.rows, c0:c0 + e]
    assert (full[0] == S).all() and (full[-1] == S).all(), f"{case.label}: a guard row of ctx was written"
    assert (full[:, :c0] == S).all() and (full[:, c0 + e:] == S).all(), f"{case.label}: a pad column of ctx was written"

    ok, err, ey, bound = mfi.check(case, got, ref, yard)
    ratio = err / ey if ey > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO kernel={case.kind} D={case.d} NW={case.nw if case.kind == 'f32' else 4} regime={case.regime} "
          f"case={case.label!r} err={err:.3e} e={ey:.3e} bound={bound:.3e} err/e={ratio:.2f}")
    assert ok, f"{case.label}: err {err:.3e} > bound {bound:.3e} (yardstick {ey:.3e}, err/e {ratio:.1f})"

    if case.t == 1:     # one key: the probability is 1 and the context is the V row
        v = case.v.reshape(case.rows, e)
        want = v if case.kind == "f32" else mfi.emu_unpack(mfi.emu_pack(v))
        assert torch.equal(_bits(got), _bits(want)), f"{case.label}: T = 1 is not the V row bit for bit"
    g4 = got.reshape(case.b, case.t, e)
    for i, j in case.twin_rows:
        assert torch.equal(_bits(g4[:, i]), _bits(g4[:, j])), f"{case.label}: twin query rows {i}, {j} differ"
    for i, j in case.twin_batches:
        assert torch.equal(_bits(g4[i]), _bits(g4[j])), f"{case.label}: twin batch entries {i}, {j} differ"
    if case.regime == "twins":
        assert case.twin_rows and (case.twin_batches or case.b < 3)
    return got


@pytest.mark.parametrize("kind,d", FAMILIES)
def test_kernel_against_float64(dev, kind, d):
    """Every short case of the family: T = 1 ... 257 at (b, heads) = (1, 2) and (4, 4) - the fp32 kernel's 2-wave and 4-wave
    instance - in every regime, strided buffers, and the contiguous layout once."""
    for spec in mfi.specs(kind, d):
        _run_case(dev, spec)


@pytest.mark.parametrize("kind,d", FAMILIES)
def test_kernel_against_float64_long_row(dev, kind, d):
    """T = 1031 (33 key tiles, the last one partial; the fp32 kernel's 4-wave instance, the f16x2 kernel's prefetch over
    many tiles): flat, peaked and both ramps."""
    for spec in mfi.long_specs(kind, d):
        _run_case(dev, spec)


@pytest.mark.parametrize("d", mfi.HEAD_DIMS)
def test_ops_wrapper_is_the_direct_call(dev, d):
    """ops.mhsa_flash(split=True / False) on contiguous inputs: bit for bit the direct calls above (split=True packs on
    the device, the direct call is fed the CPU's pack)."""
    ops, _ = _api()
    for kind, split in (("f32", False), ("f16x2", True)):
        spec = next(s for s in mfi.specs(kind, d) if not s[6])
        case = mfi.bundle(spec)[0]
        direct = _run_case(dev, spec)
        q, k, v = (x.reshape(case.rows, case.e).to(dev) for x in (case.q, case.k, case.v))
        got = ops.mhsa_flash(q, k, v, case.b, case.t, case.heads, split=split).cpu()
        assert torch.equal(_bits(got), _bits(direct)), case.label

