"""Host checks of the float64 LSTM reference and of the bound the device tests hold the kernels to (no GPU):

  * oracle.scorer.lstm_recurrence equals torch.nn.LSTM(bidirectional=True).double() to float64 rounding - outputs, dL/dx
    (as dxproj @ W_ih) and dL/dW_hh (as dxproj^T . h of the step processed before);
  * scorer_f64_inputs.lstm_backward, the step-by-step backward the fp32 yardstick runs, equals float64 autograd;
  * scorer_f64_inputs.compare accepts the fp32 CPU restatement and rejects it with any one of four planted mistakes, at
    every hidden size the device tests run: the bound is neither tighter than fp32 itself nor slack enough to pass a
    wrong formula."""
import pytest
import torch

import scorer_f64_inputs as sfi
from oracle import scorer as osc

# float64 rounding: a pre-activation is a sum of (input + hidden) <= 64 products of magnitude <= 8, and 17 steps chain
# them: 2^12 roundings of 2^-53 cover it, nine orders of magnitude below fp32
F64_TOL = 2.0 ** 12 * 2.0 ** -53


def _close64(a, b):
    return (a - b).abs().max().item() <= F64_TOL * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("hidden", [5, 32])
@pytest.mark.parametrize("t_len", [1, 2, 17])
def test_reference_equals_torch_nn_lstm_in_float64(hidden, t_len):
    torch.manual_seed(100 * hidden + t_len)
    inp = 7
    lstm = torch.nn.LSTM(inp, hidden, batch_first=True, bidirectional=True).double()
    x = torch.randn(t_len, inp, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(t_len, 2 * hidden, dtype=torch.float64)
    want = lstm(x[None])[0][0]
    (want * dout).sum().backward()

    dx = torch.zeros_like(x)
    for d, sfx in enumerate(("", "_reverse")):
        w_ih, w_hh = getattr(lstm, "weight_ih_l0" + sfx).detach(), getattr(lstm, "weight_hh_l0" + sfx).detach()
        bias = (getattr(lstm, "bias_ih_l0" + sfx) + getattr(lstm, "bias_hh_l0" + sfx)).detach()
        xproj = (x.detach() @ w_ih.t() + bias).requires_grad_(True)
        h, gates, cell = osc.lstm_recurrence(xproj, w_hh, reverse=bool(d))
        assert h.shape == (t_len, hidden) and gates.shape == (t_len, 4 * hidden) and cell.shape == (t_len, hidden)
        assert _close64(h.detach(), want[:, d * hidden:(d + 1) * hidden].detach())
        # the saved tensors are what they claim: h = o * tanh(c), c = f * c_prev + i * g
        i, f, g, o = gates.detach().view(t_len, 4, hidden).unbind(1)
        assert _close64(o * torch.tanh(cell.detach()), h.detach())
        prev = torch.zeros_like(cell.detach())
        if d:
            prev[:-1] = cell.detach()[1:]
        else:
            prev[1:] = cell.detach()[:-1]
        assert _close64(f * prev + i * g, cell.detach())
        dxproj = torch.autograd.grad(h, xproj, dout[:, d * hidden:(d + 1) * hidden])[0]
        dx += dxproj @ w_ih
        h_shift = torch.zeros_like(h.detach())
        if d:
            h_shift[:-1] = h.detach()[1:]
        else:
            h_shift[1:] = h.detach()[:-1]
        assert _close64(dxproj.t() @ h_shift, getattr(lstm, "weight_hh_l0" + sfx).grad)
        # the written-out backward of the yardstick is the same function as autograd
        manual = sfi.lstm_backward(dout[:, d * hidden:(d + 1) * hidden], gates.detach(), cell.detach(), w_hh, bool(d))
        assert _close64(manual, dxproj)
    assert _close64(dx, x.grad)


def test_reference_of_an_empty_sequence():
    h, gates, cell = osc.lstm_recurrence(torch.zeros(0, 12, dtype=torch.float64), torch.zeros(12, 3, dtype=torch.float64))
    assert h.shape == (0, 3) and gates.shape == (0, 12) and cell.shape == (0, 3) and h.dtype == torch.float64


def test_case_layout_is_the_one_the_device_tests_state():
    case = sfi.lstm_case(20)
    assert (case.ndir, case.reverse_mask, case.out_col0, case.ldo) == (3, 0b010, 4, 3 * 20 + 9)
    assert case.seq_rows.tolist() == [2, 2, 3, 5, 14] and case.rows == 15 and case.in_seq.sum().item() == 12
    assert case.whh.abs().max().item() <= 1 / 20 ** 0.5
    again = sfi.lstm_case(20)
    assert torch.equal(case.xproj, again.xproj) and torch.equal(case.whh, again.whh) and torch.equal(case.dout, again.dout)
    sat = sfi.lstm_case(20, saturate=True)
    assert torch.equal(sat.xproj[:, ::3], case.xproj[:, ::3] * 30) and torch.equal(sat.xproj[:, 1::3], case.xproj[:, 1::3])
    tw = sfi.lstm_case(20, lens=(5, 0, 9, 1, 9), twins=(2, 4))
    assert torch.equal(tw.xproj[7:16], tw.xproj[17:26]) and torch.equal(tw.dout[7:16], tw.dout[17:26])


@pytest.mark.parametrize("hidden", sfi.ALL_HIDDEN)
def test_bound_accepts_fp32_and_rejects_each_planted_mistake(hidden):
    case, ref, cpu32, iso32 = sfi.lstm_bundle(hidden)
    gscale = ref.dxproj.abs().max().item()
    assert gscale > 0
    for name in ("out", "gates", "cell"):
        ok, err, e32, bound = sfi.compare(getattr(cpu32, name), getattr(ref, name), getattr(cpu32, name))
        assert ok and err == e32, (name, err, bound)
    for got in (cpu32.dxproj, iso32.dxproj):
        ok, err, e32, bound = sfi.compare(got, ref.dxproj, got, gscale)
        assert ok and err == e32 and bound < 1e-3 * gscale, (err, bound, gscale)
    # (a non-finite result is never within the bound)
    bad = cpu32.dxproj.clone()
    bad[5, 0] = float("nan")
    assert not sfi.compare(bad, ref.dxproj, cpu32.dxproj, gscale)[0]
    for mistake in sfi.MISTAKES:
        wrong = sfi.lstm_restatement(case, mistake=mistake)
        ok, err, e32, bound = sfi.compare(wrong.dxproj, ref.dxproj, cpu32.dxproj, gscale)
        assert not ok, (mistake, err, e32, bound)
        # also with the backward on its own, fed the reference's saved tensors
        wrong_iso = sfi.lstm_restatement(case, mistake=mistake, saved=(ref.gates.float(), ref.cell.float()))
        if mistake != "walk_forward":       # (the walk is the forward's: with saved tensors it only permutes the steps)
            assert not sfi.compare(wrong_iso.dxproj, ref.dxproj, iso32.dxproj, gscale)[0], mistake
    walked = sfi.lstm_restatement(case, mistake="walk_forward")
    for name in ("out", "gates", "cell"):
        assert not sfi.compare(getattr(walked, name), getattr(ref, name), getattr(cpu32, name))[0], name
