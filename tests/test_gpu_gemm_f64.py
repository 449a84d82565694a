"""avs_gemm_nt per instance of igemm_kernel against float64: every case of gemm_f64_inputs.CASES (the host test
test_gemm_f64_host.py asserts that they reach every instance a plain GEMM can) with both operand sets - "a" within the
per-element bound of the float64 reference (AVS_F32_SPLIT: of its float64 restatement), "b" (small integers) EQUAL to
the float64 product.  Calls go through ops.gemm_nt_batched, the out= column-slice cases through ops.linear.

The destination is a flat buffer filled with a NaN / bf16 sentinel bit pattern: one spare row, the batch entries at
their stride (pad columns, a gap between entries, or entries interleaved in the columns as the attention's context
has them), one spare row.  Every element outside [M, N] of every batch entry must come back bit-identical, the inputs
unchanged, and a second call into a fresh buffer must give identical bits.

Measured on an MI355X over all cases (operand set "a"; err / e32 is taken per row: the row's largest error over the
fp32 CPU evaluation's largest error in that row, both against float64; err / bound per element).  A row of one output
(N = 1), or of a few that a ReLU clips, has an e32 that is tiny by accident: those rows are held by the 8 eps32 S floor
and are given apart.
    AVS_F32        err / e32 4.97 (f32-k544-wide-plain), N = 1: 402.7 (f32-m129-n1-plain, err / bound 0.08);
                   err / bound 0.184 (f32-k544-wide-plain)
    AVS_F32_ACC64  err / e32 4.36 (acc64-heads5-ctx-row), N = 1: 258.0 (acc64-m128-n1-scaled_brelu, err / bound 0.04);
                   err / bound 0.188 (acc64-heads5-qk-neg_row)
    AVS_F32_SPLIT  against its restatement: err / e32 6.55 (split-tall-n8-k52-plain), N = 1: 289.7 (split-m257-n1-col,
                   err / bound 0.04), clipped: 107.5 (split-tall-n8-k52-brelu, err / bound 0.08);
                   err / bound 0.131 (split-tall-n129-k260-plain)
    AVS_BF16       err / e32 has no meaning (the error is the bf16 rounding: bf16-k8-plain sums exactly in fp32, e32 = 0);
                   err / bound 1.000, a tie of the rounding: exactly half a step (bf16-k8-wide-brelu)
The whole file runs in about 4 seconds.
"""
import ctypes

import pytest
import torch

import gemm_f64_inputs as gfi

pytestmark = pytest.mark.gpu

SENTINEL = {torch.float32: (torch.int32, 0x7FC01234), torch.bfloat16: (torch.int16, 0x7FC1)}      # NaNs no kernel produces


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _tdt(case):
    return torch.bfloat16 if case.dtype == gfi.BF16 else torch.float32


def _row_index(case, dev):
    idx = torch.arange(case.m, device=dev)
    return idx % case.period if case.period else idx


def _launch(dev, case, o):
    """One call into a fresh sentinel-filled buffer: (the buffer, its [batch, M, N] view, the mask of the elements
    outside that view)."""
    ops, _ = _api()
    tdt = _tdt(case)
    if case.period:      # the base rows repeated, on the device
        a = o.A[0].to(tdt).to(dev)[_row_index(case, dev)].contiguous()
    else:
        a = o.a_buf.to(tdt).to(dev)
    b = o.b_buf.to(tdt).to(dev)
    bias = o.bias_buf.to(dev) if o.bias_buf is not None else None
    held = [None if t is None or case.period and t is a else t.clone() for t in (a, b, bias)]
    c_off = case.ldc + case.col0
    last = c_off + (case.batch - 1) * case.sc + max(case.m - 1, 0) * case.ldc + case.n
    total = -(-last // case.ldc) * case.ldc + case.ldc
    itype, pattern = SENTINEL[tdt]
    buf = torch.full((total,), pattern, dtype=itype, device=dev).view(tdt)
    if case.via_linear:
        assert case.batch == 1 and case.lda == case.k and case.ldb == case.k and case.dtype == ops.dtype_code(tdt)
        out = buf[case.ldc:case.ldc + case.m * case.ldc].view(case.m, case.ldc)[:, case.col0:case.col0 + case.n]
        ret = ops.linear(a.view(case.m, case.k), b.view(case.n, case.k), bias, case.act, out=out, alpha=case.alpha)
        assert ret.data_ptr() == buf.data_ptr() + c_off * buf.element_size()
    else:
        ops.gemm_nt_batched(case.dtype, case.m, case.n, case.k, a, 0, case.lda, case.sa, b, 0, case.ldb, case.sb, buf, c_off,
                            case.ldc, case.sc, bias, case.bias_mode, case.sbias, case.alpha, case.act, case.batch)
    torch.cuda.synchronize(dev)
    for t, h in zip((a, b, bias), held):
        assert h is None or torch.equal(t, h), "an input changed"
    if case.period:
        assert torch.equal(a, o.A[0].to(tdt).to(dev)[_row_index(case, dev)]), "A changed"
    outside = torch.ones(total, dtype=torch.bool, device=dev)
    outside.as_strided((case.batch, case.m, case.n), (case.sc, case.ldc, 1), c_off).fill_(False)
    assert int((~outside).sum()) == case.batch * case.m * case.n, "the batch entries of C overlap"
    return buf, buf.as_strided((case.batch, case.m, case.n), (case.sc, case.ldc, 1), c_off), outside


def _run_twice(dev, case, which):
    o = gfi.operands(case, which)
    buf, got, outside = _launch(dev, case, o)
    itype, pattern = SENTINEL[_tdt(case)]
    touched = int((buf.view(itype)[outside] != pattern).sum())
    assert touched == 0, f"{case.name}/{which}: {touched} elements outside [M, N] were written"
    buf2, _, _ = _launch(dev, case, o)
    assert torch.equal(buf.view(itype), buf2.view(itype)), f"{case.name}/{which}: two calls differ"
    return got.double()


@pytest.mark.parametrize("case", gfi.CASES, ids=[c.name for c in gfi.CASES])
def test_gemm_nt_against_float64(dev, case):
    assert case.dtype in gfi.DTYPES
    idx = _row_index(case, dev)
    # (a) within the bound, element by element
    got = _run_twice(dev, case, "a")
    ref, target, bound, e32, s = (t.to(dev)[:, idx] for t in gfi.bundle(case, "a"))
    if case.m == 0:
        assert got.numel() == 0
    else:
        err = (got - target).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        row_err, row_e32 = err.amax(-1), e32[..., 0]
        ratio = torch.where(row_e32 > 0, row_err / row_e32, torch.where(row_err > 0, float("inf"), 0.0).to(row_err)).max().item()
        worst = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err))
        at = int(worst.argmax())
        print(f"RATIO dtype={gfi.DTYPE_NAMES[case.dtype]} case={case.name!r} plan={gfi.case_plan(case)[1:]} err={err.max().item():.3e} "
              f"e32={row_e32.max().item():.3e} bound={bound.reshape(-1)[at].item():.3e} err/e32={ratio:.2f} "
              f"err/bound={worst.reshape(-1)[at].item():.3f}")
        bad = int((err > bound).sum())
        assert bad == 0, (f"{case.name}: {bad} of {err.numel()} elements outside the bound, the worst at "
                          f"{tuple(int(i) for i in torch.unravel_index(torch.tensor(at), err.shape))}: err "
                          f"{err.reshape(-1)[at].item():.3e} > {bound.reshape(-1)[at].item():.3e}")
        if case.dtype == gfi.SPLIT:      # and the restatement's own distance from the float64 product
            assert bool(((got - ref).abs() <= (gfi.SPLIT_C * 2.0 ** -15) * s + bound).all())
    # (b) exact operands: equal to the float64 product (bf16: rounded once)
    got = _run_twice(dev, case, "b")
    want = gfi.exact_result(case).to(dev)[:, idx]
    wrong = int((got != want).sum())
    assert wrong == 0, f"{case.name}: {wrong} of {want.numel()} elements of the exact operand set differ"


def test_acc64_beats_the_plain_fp32_sum(dev):
    """Long sums of large same-sign terms: the fp64 sum of the reduction steps' fp32 sums is within 8 eps32 S of the exact
    product element by element, and closer to it than the fp32 running sum of AVS_F32."""
    ops, _ = _api()
    g = torch.Generator().manual_seed(4)
    m, n, k = 300, 402, 400
    a = torch.randn(m, k, generator=g) * 10 + 30
    b = torch.randn(n, k, generator=g)
    exact = a.double() @ b.double().t()
    s = a.double().abs() @ b.double().abs().t()
    got = {}
    for dtype in (gfi.ACC64, gfi.F32):
        c = torch.full((m, n), float("nan"), device=dev)
        ops.gemm_nt_batched(dtype, m, n, k, a.to(dev), 0, k, 0, b.to(dev), 0, k, 0, c, 0, n, 0)
        got[dtype] = (c.cpu().double() - exact).abs()
    assert bool((got[gfi.ACC64] <= 8.0 * gfi.EPS32 * s).all())
    assert got[gfi.ACC64].max().item() < 0.6 * got[gfi.F32].max().item()


# (the one refusal that would read a null bias were it accepted is left to the host test)
DEVICE_REFUSALS = [r for r in gfi.refusals() if r[3].get("bias_mode") != 1]


@pytest.mark.parametrize("label,status,status_null,changes", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_refusals_with_device_operands(dev, label, status, status_null, changes):
    """The status of each check with operands given (the host test makes these calls with null operands).  Every
    operand points into the middle of a zeroed buffer that any of these shapes would stay inside were it accepted."""
    _, abi = _api()
    lib = abi.lib()
    bufs = [torch.zeros(1 << 16, device=dev, dtype=torch.float32) for _ in range(3)]
    ptrs = [ctypes.c_void_p(t.data_ptr() + (1 << 17)) for t in bufs]
    assert lib.avs_gemm_nt(*gfi.refusal_args(changes, *ptrs)) == status, lib.avs_last_error()
    assert b"avs_gemm_nt" in lib.avs_last_error()
    torch.cuda.synchronize(dev)
    assert all(not t.any() for t in bufs)
