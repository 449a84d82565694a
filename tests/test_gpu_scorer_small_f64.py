"""The small kernels of the scorer's forward and backward, each on its own against float64: softmax_rows /
softmax_bwd_rows, score_head / score_head_bwd, relu_dropout_bwd, mul, transpose_padded / grad_weight and mha_batchaxis.
Inputs come from scorer_f64_inputs; pad columns are pre-filled with a sentinel and must come back untouched.  Where a
result is rounded more than once the bound is scorer_f64_inputs.compare (4 * e32 + 8 * eps32 * max(1, max|ref|), e32 = the
same formula in fp32 on the CPU); where there is one rounding per element the result must equal the fp32 formula exactly.

Measured on an MI355X, the largest err / e32 per kernel family over all cases of this file (err and e32 both against
float64): softmax pair 1.00 (softmax_rows) and 1.23 (softmax_bwd_rows); score head pair 1.00 (dz, dpre) and 15.6 (scores,
rows=5 d=65: err 1.7e-7, e32 1.1e-8, bound 1.0e-6); grad_weight 1.94; mha_batchaxis 1.48.
The scores' ratio is above 4 and the case still lies within the bound, by its floor: the CPU's fp32 sigmoid is all but
correctly rounded (e32 a third of an ulp of 0.5), the kernel's 1 / (1 + expf(-x)) rounds three times - 1.7e-7 is 1.4 ulp
of a score near 1, which is what 8 * eps32 is there to allow."""
import math

import pytest
import torch

import scorer_f64_inputs as sfi

pytestmark = pytest.mark.gpu

S = sfi.SENTINEL


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _check(family, label, name, got, ref, cpu32):
    ok, err, e32, bound = sfi.compare(got, ref, cpu32)
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO family={family!r} case={label!r} tensor={name} err={err:.3e} e32={e32:.3e} bound={bound:.3e} "
          f"err/e32={ratio:.2f}")
    assert ok, f"{family} {label} {name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"


# --------------------------------------------------------------------------- softmax pair
@pytest.mark.parametrize("n", sfi.SOFTMAX_N)
def test_softmax_rows_and_its_backward(dev, n):
    """Row lengths on both sides of one wave (64) and of one trip of the 256-thread loop, and four trips (1003); the
    backward is alpha * p * (dp - sum(p * dp)) with alpha = 1/sqrt(64) and 1, fed the fp32 probabilities of the CPU."""
    ops, _ = _api()
    x, dp = sfi.softmax_case(n)
    rows, ld = sfi.SOFTMAX_ROWS, n + 3
    xd = x.to(dev)
    ops.softmax_rows(xd, rows, n, ld)
    got = xd.cpu()
    assert (got[:, n:] == S).all()
    _check("softmax pair", f"n={n}", "softmax", got[:, :n], torch.softmax(x[:, :n].double(), -1), torch.softmax(x[:, :n], -1))
    assert (got[:, :n].double().sum(-1) - 1).abs().max().item() <= 8 * sfi.EPS32

    p = torch.full_like(x, S)
    p[:, :n] = torch.softmax(x[:, :n], -1)
    pd = p.to(dev)
    for alpha in (1.0 / math.sqrt(64), 1.0):
        dd = dp.to(dev)
        ops.softmax_bwd_rows(pd, dd, rows, n, ld, alpha)
        got = dd.cpu()
        assert (got[:, n:] == S).all() and torch.equal(pd.cpu(), p)
        _check("softmax pair", f"n={n} alpha={alpha:.3f}", "softmax_bwd", got[:, :n],
               sfi.softmax_bwd_formula(p[:, :n].double(), dp[:, :n].double(), alpha),
               sfi.softmax_bwd_formula(p[:, :n], dp[:, :n], torch.tensor(alpha, dtype=torch.float32)))


# --------------------------------------------------------------------------- score head pair
@pytest.mark.parametrize("rows", sfi.SCORE_ROWS)
@pytest.mark.parametrize("d", sfi.SCORE_D)
def test_score_head_and_its_backward(dev, rows, d):
    """scores = sigmoid(hid @ w2 + b2) with hid = relu(pre) in a buffer whose rows are 3 wider than d.  The backward
    returns dz [rows] = dL/d(hid @ w2 + b2) = dscores * s * (1 - s), and dpre [rows, d] = dz * w2 where hid > 0, else 0:
    the gradient with respect to the input of the ReLU that produced hid (scorer.0's pre-activation), not with respect
    to hid itself.  Both against float64 autograd of sigmoid(relu(pre) @ w2 + b2); the backward is fed the reference's
    scores rounded to fp32."""
    ops, _ = _api()
    pre, w2, b2, ds = sfi.score_case(rows, d)
    hid_wide = torch.relu(pre)
    hid_wide[:, d:] = S
    hid = hid_wide[:, :d]

    pre64 = pre[:, :d].double().requires_grad_(True)
    z64 = torch.relu(pre64) @ w2.double() + b2.double()
    s64 = torch.sigmoid(z64)
    dz64, dpre64 = torch.autograd.grad(s64, [z64, pre64], ds.double())
    s32 = torch.sigmoid(hid @ w2 + b2)

    hd = hid_wide.to(dev)[:, :d]
    assert hd.stride(0) == d + 3
    got = ops.score_head(hd, w2.to(dev), b2.to(dev)).cpu()
    _check("score head pair", f"rows={rows} d={d}", "scores", got, s64.detach(), s32)

    s_in = s64.detach().float()
    dz, dpre = ops.score_head_bwd(ds.to(dev), s_in.to(dev), hd, w2.to(dev))
    dz32 = ds * s_in * (1 - s_in)
    dpre32 = torch.where(hid > 0, dz32[:, None] * w2[None, :], torch.zeros(()))
    _check("score head pair", f"rows={rows} d={d}", "dz", dz.cpu(), dz64, dz32)
    _check("score head pair", f"rows={rows} d={d}", "dpre", dpre.cpu(), dpre64, dpre32)
    assert (dpre.cpu()[hid == 0] == 0).all()
    assert torch.equal(hd.cpu(), hid) and (hid_wide.to(dev)[:, d:] == S).all()


# --------------------------------------------------------------------------- element-wise gradient gates
@pytest.mark.parametrize("n", sfi.ELEMENTWISE_N)
def test_relu_dropout_bwd_and_mul_are_exact(dev, n):
    """One rounding per element: bit for bit the fp32 formula.  A zero of relu_out gives a zero gradient."""
    ops, _ = _api()
    dy, relu_out, keep = sfi.elementwise_case(n)
    dyd, rd, kd = dy.to(dev), relu_out.to(dev), keep.to(dev)
    zero = torch.zeros(())
    got = ops.relu_dropout_bwd(dyd, rd, kd).cpu()
    assert torch.equal(got, torch.where(relu_out > 0, dy * keep, zero))
    assert (got[relu_out == 0] == 0).all()
    got = ops.relu_dropout_bwd(dyd, rd).cpu()
    assert torch.equal(got, torch.where(relu_out > 0, dy, zero))
    assert (got[relu_out == 0] == 0).all()
    assert torch.equal(ops.mul(dyd, kd).cpu(), dy * keep)
    assert torch.equal(dyd.cpu(), dy) and torch.equal(rd.cpu(), relu_out) and torch.equal(kd.cpu(), keep)


# --------------------------------------------------------------------------- transposes and the weight gradient
@pytest.mark.parametrize("rows,cols", sfi.TRANSPOSE_SHAPES)
def test_transpose_padded_and_grad_weight(dev, rows, cols):
    """transpose_padded: exact, the tail up to a multiple of 4 rows zero, from a contiguous matrix and from one whose rows
    are 3 wider than cols.  grad_weight = dy^T @ x against float64, into a fresh tensor and into rows of a larger one."""
    ops, _ = _api()
    wide, x = sfi.transpose_case(rows, cols)
    dy = wide[:, :cols]
    rp = (rows + 3) // 4 * 4
    want = torch.zeros(cols, rp)
    want[:, :rows] = dy.t()
    for src in (dy.contiguous().to(dev), wide.to(dev)[:, :cols]):
        got = ops.transpose_padded(src)
        assert got.shape == (cols, rp) and torch.equal(got.cpu(), want)

    ref = dy.double().t() @ x.double()
    cpu32 = dy.t() @ x
    k = x.shape[1]
    got = ops.grad_weight(dy.contiguous().to(dev), x.to(dev))
    assert got.shape == (cols, k)
    _check("grad_weight", f"rows={rows} cols={cols}", "dW", got.cpu(), ref, cpu32)
    big = torch.full((3 * cols, k), S, device=dev)
    ret = ops.grad_weight(wide.to(dev)[:, :cols], x.to(dev), out=big[cols:2 * cols])      # (dy with its wider row stride)
    assert ret.data_ptr() == big[cols:2 * cols].data_ptr()
    assert torch.equal(big[cols:2 * cols], got)
    assert (big[:cols] == S).all() and (big[2 * cols:] == S).all()
    with pytest.raises(ValueError):
        ops.grad_weight(dy.contiguous().to(dev), x.to(dev), out=big[:cols + 1])


# --------------------------------------------------------------------------- attention over the batch axis
@pytest.mark.parametrize("t", sfi.MHA_T)
@pytest.mark.parametrize("b", sfi.MHA_B)
@pytest.mark.parametrize("e,heads", sfi.MHA_E_HEADS)
def test_mha_batchaxis_against_float64(dev, e, heads, b, t):
    """Head dimensions 16, 100, 256 and 512: a fraction of a wave, a second per-lane element that only 36 lanes have, and
    4 and 8 elements per lane; B = 1 (softmax constant 1), 2 and 5 keys.  Reference: oracle.scorer.mha_seq_first in
    float64 with an identity output projection, on an in_proj whose products are exact so that both sides see one qkv."""
    ops, _ = _api()
    x, qkv = sfi.mha_case(e, b, t)
    w64, b64 = sfi.mha_in_proj(e, torch.float64)
    assert torch.equal((x.double() @ w64.t() + b64).reshape(b * t, 3 * e), qkv.double())
    ref = sfi.mha_reference(x, e, heads, torch.float64)
    cpu32 = sfi.mha_reference(x, e, heads, torch.float32)
    got = ops.mha_batchaxis(qkv.to(dev), b, t, e, heads).cpu()
    _check("mha_batchaxis", f"E={e} heads={heads} B={b} T={t}", "ctx", got, ref, cpu32)
    if b == 1:      # one key: the context is v
        assert torch.equal(got, qkv[:, 2 * e:])


def test_mha_batchaxis_refuses_a_head_dimension_of_513(dev):
    ops, abi = _api()
    with pytest.raises(abi.AvsError, match="avs_mha_batchaxis_f32"):
        ops.mha_batchaxis(torch.zeros(1, 3 * 2052, device=dev), 1, 1, 2052, 4)
