"""The ragged-batch attention of csrc/attn_train.hip on the device: each of its four kernels on its own against float64
through attn.py's launch wrappers (strided buffers whose other entries hold a sentinel, guard rows around the batch),
the forward's bits against ops.mhsa_flash(split=False) per video, batch invariance and determinism bit for bit, the
module's forward_rows / fused_backward against torch autograd through the oracle, and the memory the backward takes.
Cases, references, yardsticks and the bound come from attn_rows_inputs (see its docstring); test_attn_rows_host.py shows
on the CPU that the bound accepts a correct tiled backward at every case and rejects eight planted mistakes.

The gradient kernels are handed lse and delta derived in float64 and rounded to fp32, and are checked against float64 on
those handed values: a forward error is not charged to them.

Measured on an MI355X over all cases of this file, per output and head dim 64 / 128 / 256: the largest err / e32 (the bound
allows 4 plus the floor) and, in brackets, the largest err / bound:

    ctx    2.26 / 2.16 / 2.58   (0.27 / 0.24 / 0.63)      dq   4.23 / 3.31 / 3.47   (0.35 / 0.23 / 0.38)
    lse    2.05 / 2.21 / 3.84   (0.16 / 0.16 / 0.30)      dk   3.52 / 2.90 / 3.41   (0.38 / 0.14 / 0.33)
    delta  1.10 / 1.49 / 1.05   (0.09 / 0.08 / 0.07)      dv   3.30 / 3.57 / 3.71   (0.19 / 0.16 / 0.19)

The ratios above 4 are flat-regime cases whose errors are of the size of the bound's floor (8 eps32): every case lies
inside the bound, the closest at 0.63 of it (ctx, D = 256, the row of 1031 keys on ramp_up: one fp32 chain of 256
products per score, as in test_gpu_mhsa_f64.py)."""
import numpy as np
import pytest
import torch

import attn_rows_inputs as ari

pytestmark = pytest.mark.gpu


def _api():
    from avsum_amd import attn, ops
    return attn, ops


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Device:
    """The buffers of a case on the device, laid out as attn_rows_inputs states, and the views the wrappers take."""

    def __init__(self, dev, spec):
        _, ops = _api()
        self.b = ari.bundle(spec)
        self.case = case = self.b.case
        self.dev = dev
        self.host = [ari.wide(case, x, ari.PAD_IN) for x in (case.q, case.k, case.v)] + [ari.wide(case, case.dctx)]
        self.bufs = [x.to(dev) for x in self.host]
        self.q, self.k, self.v, self.dctx = (self.view(x) for x in self.bufs)
        self.table = ops.AttnTable(case.offsets, device=dev)

    def view(self, buf):
        return buf[:, ari.COL0:ari.COL0 + self.case.e]

    def blank(self, narrow=False, fill=None):
        """A device output buffer of SENTINEL (or an input buffer holding ``fill``) and its view."""
        buf = (ari.narrow(self.case, fill) if narrow else ari.wide(self.case, fill)).to(self.dev)
        return buf, (buf if narrow else self.view(buf))

    def taken(self, buf):
        """The kernel's block of a buffer, on the host, after checking that nothing else of it was written."""
        host = buf.cpu()
        assert ari.untouched(self.case, host), f"{self.case.label}: a pad column or guard row was written"
        return ari.inner(self.case, host)

    def inputs_unchanged(self):
        for h, d in zip(self.host, self.bufs):
            assert _same(d.cpu(), h), f"{self.case.label}: an input was written"


def _report(case, name, ok, err, e32, bound):
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO {name} case={case.label!r} err={err:.3e} e={e32:.3e} bound={bound:.3e} err/e={ratio:.2f}")
    assert ok, f"{case.label} {name}: err {err:.3e} > bound {bound:.3e} (yardstick {e32:.3e})"


# --------------------------------------------------------------------------- per kernel against float64
@pytest.mark.parametrize("d", ari.HEAD_DIMS)
def test_forward_kernel_against_float64_and_the_dense_kernels_bits(dev, d):
    """avsa_mhsa_rows_fwd_f32: ctx and lse within the bound, sentinels untouched, twins, a second launch the same bits,
    and every video's ctx bit for bit ops.mhsa_flash(split=False) on that video alone."""
    attn, ops = _api()
    for spec in ari.specs(d):
        dv = _Device(dev, spec)
        case, b = dv.case, dv.b
        outs = []
        for _ in range(2):
            (cbuf, ctx), (lbuf, lse) = dv.blank(), dv.blank(narrow=True)
            attn.mhsa_rows_fwd(dv.q, dv.k, dv.v, dv.table, case.heads, ctx=ctx, lse=lse)
            outs.append((dv.taken(cbuf), dv.taken(lbuf)))
        (ctx, lse), again = outs
        assert _same(ctx, again[0]) and _same(lse, again[1]), f"{case.label}: a second launch gave other bits"
        dv.inputs_unchanged()
        _report(case, "ctx", *ari.compare(ctx, b.ref.ctx, b.yard.ctx))
        _report(case, "lse", *ari.compare(lse, b.ref.lse, b.yard.lse))
        o = case.offsets0
        for v in range(len(case.lengths)):
            lo, hi = int(o[v]), int(o[v + 1])
            alone = ops.mhsa_flash(*(x[lo:hi].to(dev) for x in (case.q, case.k, case.v)), 1, hi - lo, case.heads, split=False)
            assert _same(alone.cpu(), ctx[lo:hi]), f"{case.label}: video {v} differs from the dense kernel's bits"
        for i, j in case.twin_seqs:
            for x in (ctx, lse):
                assert _same(x[o[i]:o[i + 1]], x[o[j]:o[j + 1]]), f"{case.label}: twin sequences {i}, {j} differ"
        for v, r, s in case.twin_rows:
            assert _same(ctx[o[v] + r], ctx[o[v] + s]) and _same(lse[o[v] + r], lse[o[v] + s])


@pytest.mark.parametrize("d", ari.HEAD_DIMS)
def test_delta_kernel_against_float64(dev, d):
    """avsa_mhsa_rows_delta_f32 on dctx and the float64 ctx rounded to fp32."""
    attn, _ = _api()
    for spec in ari.specs(d):
        dv = _Device(dev, spec)
        case, b = dv.case, dv.b
        _, ctx = dv.blank(fill=b.ctx32)
        outs = []
        for _ in range(2):
            dbuf, delta = dv.blank(narrow=True)
            attn.mhsa_rows_delta(dv.dctx, ctx, dv.table, case.heads, delta=delta)
            outs.append(dv.taken(dbuf))
        assert _same(*outs), f"{case.label}: a second launch gave other bits"
        _report(case, "delta", *ari.compare(outs[0], b.delta_ref, b.delta_yard))


@pytest.mark.parametrize("d", ari.HEAD_DIMS)
def test_gradient_kernels_against_float64(dev, d):
    """avsa_mhsa_rows_dkv_f32 and avsa_mhsa_rows_dq_f32, handed the float64 lse and delta rounded to fp32: dq, dk, dv
    within the bound, sentinels and guard rows untouched, inputs unchanged, two runs the same bits, twins."""
    attn, _ = _api()
    for spec in ari.specs(d):
        dv = _Device(dev, spec)
        case, b = dv.case, dv.b
        (_, lse), (_, delta) = dv.blank(narrow=True, fill=b.lse32), dv.blank(narrow=True, fill=b.delta32)
        runs = []
        for _ in range(2):
            (qbuf, dq), (kbuf, dk), (vbuf, dvv) = dv.blank(), dv.blank(), dv.blank()
            attn.mhsa_rows_dkv(dv.dctx, dv.q, dv.k, dv.v, lse, delta, dv.table, case.heads, dk=dk, dv=dvv)
            attn.mhsa_rows_dq(dv.dctx, dv.q, dv.k, dv.v, lse, delta, dv.table, case.heads, dq=dq)
            runs.append([dv.taken(x) for x in (qbuf, kbuf, vbuf)])
        for name, x, y in zip(("dq", "dk", "dv"), *runs):
            assert _same(x, y), f"{case.label}: a second run of {name} gave other bits"
        dv.inputs_unchanged()
        for name, result in ari.check_grads(b, *runs[0]).items():
            _report(case, name, *result)
        o = case.offsets0
        for i, j in case.twin_seqs:
            for x in runs[0]:
                assert _same(x[o[i]:o[i + 1]], x[o[j]:o[j + 1]]), f"{case.label}: twin sequences {i}, {j} differ"


# --------------------------------------------------------------------------- batch invariance
def _pipeline(dev, q, k, v, dctx, offsets, heads):
    """fwd -> delta -> dK/dV -> dQ on contiguous rows, everything the device computed: (ctx, lse, dq, dk, dv) on the host."""
    attn, ops = _api()
    table = ops.AttnTable(offsets, device=dev)
    q, k, v, dctx = (x.contiguous().to(dev) for x in (q, k, v, dctx))
    ctx, lse = attn.mhsa_rows_fwd(q, k, v, table, heads)
    dq, dk, dvv = attn.mhsa_rows_bwd(dctx, q, k, v, ctx, lse, table, heads)
    return [x.cpu() for x in (ctx, lse, dq, dk, dvv)]


@pytest.mark.parametrize("d", ari.HEAD_DIMS)
def test_a_video_has_the_same_bits_alone_and_in_the_batch(dev, d):
    for spec in ((d, ari.LENGTHS, "flat"), (d, ari.TWIN_LENGTHS, "twins"), (d, ari.LENGTHS, "peaked")):
        case = ari.bundle(spec).case
        o = case.offsets0
        whole = _pipeline(dev, case.q, case.k, case.v, case.dctx, o, case.heads)
        again = _pipeline(dev, case.q, case.k, case.v, case.dctx, o, case.heads)
        for name, x, y in zip(("ctx", "lse", "dq", "dk", "dv"), whole, again):
            assert _same(x, y), f"{case.label}: a second run of the batch gave other bits of {name}"
        for v in range(len(case.lengths)):
            lo, hi = int(o[v]), int(o[v + 1])
            alone = _pipeline(dev, *(x[lo:hi] for x in (case.q, case.k, case.v, case.dctx)), [0, hi - lo], case.heads)
            for name, x, y in zip(("ctx", "lse", "dq", "dk", "dv"), whole, alone):
                assert _same(x[lo:hi], y), f"{case.label}: {name} of video {v} differs between batch and alone"
        for i, j in case.twin_seqs:
            for x in whole:
                assert _same(x[o[i]:o[i + 1]], x[o[j]:o[j + 1]])


# --------------------------------------------------------------------------- the module
def _close(a, r, name):
    """The criterion of tests/test_gpu_models.py::test_mhsa_backward."""
    err = (a.cpu() - r).abs().max().item()
    assert err <= 1e-4 * max(r.abs().max().item(), 1e-2), (name, err, r.abs().max().item())


def _oracle(m, x, offsets, gout, h):
    """torch autograd through oracle.scorer.mhsa_forward, per video, the gradients summed: (out, dx, {name: grad})."""
    from oracle import scorer as osc
    sd = {k_: v_.detach().cpu().clone().requires_grad_(True) for k_, v_ in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = torch.cat([osc.mhsa_forward(sd, xr[lo:hi][None], h)[0] for lo, hi in zip(offsets[:-1], offsets[1:])])
    ref.backward(gout)
    return ref.detach(), xr.grad, {k_: v_.grad for k_, v_ in sd.items()}


def _node(out, name):
    """The autograd node called ``name`` at or just behind ``out`` (a view may stand between them)."""
    node = out.grad_fn
    for _ in range(3):
        if type(node).__name__ == name:
            return node
        node = node.next_functions[0][0]
    raise AssertionError(f"no {name} behind the output, its grad_fn is {type(out.grad_fn).__name__}")


MODULE_LENGTHS = (5, 40, 33, 130, 1)


@pytest.mark.parametrize("e,h", [(128, 2), (512, 2), (1024, 4)])
def test_module_forward_rows_against_the_oracle(dev, e, h):
    """forward_rows on a ragged batch: the output and the gradients of x and all 8 parameters against torch autograd
    through the oracle applied per video; then the parameters frozen, then the input without grad."""
    from avsum_amd.models.attention import MultiHeadSelfAttention
    _, ops = _api()
    torch.manual_seed(13)
    m = MultiHeadSelfAttention(e, h)
    offsets = np.concatenate([[0], np.cumsum(MODULE_LENGTHS)])
    rows = int(offsets[-1])
    x = torch.randn(rows, e, generator=torch.Generator().manual_seed(e + h))
    gout = torch.randn(rows, e, generator=torch.Generator().manual_seed(3))
    ref, dx, grads = _oracle(m, x, offsets, gout, h)
    md = m.to(dev)
    xd = x.to(dev).requires_grad_(True)
    got = md.forward_rows(xd, offsets)
    assert got.requires_grad and got.shape == (rows, e)
    _close(got.detach(), ref, "out")
    got.backward(gout.to(dev))
    _close(xd.grad, dx, "x")
    for name, prm in md.named_parameters():
        _close(prm.grad, grads[name], name)
    # a table built once gives the same bits as host offsets; no grad: the same forward
    table = ops.AttnTable(offsets, device=dev)
    with torch.no_grad():
        plain = md.forward_rows(x.to(dev), table)
    assert not plain.requires_grad and _same(plain.cpu(), got.detach().cpu())
    # input without grad: the parameter gradients alone
    first = {name: prm.grad.clone() for name, prm in md.named_parameters()}
    for prm in md.parameters():
        prm.grad = None
    md.forward_rows(x.to(dev), table).backward(gout.to(dev))
    for name, prm in md.named_parameters():
        assert _same(prm.grad.cpu(), first[name].cpu()), name
    # parameters frozen: the input gradient alone
    for prm in md.parameters():
        prm.grad = None
        prm.requires_grad_(False)
    xd2 = x.to(dev).requires_grad_(True)
    md.forward_rows(xd2, table).backward(gout.to(dev))
    assert _same(xd2.grad.cpu(), xd.grad.cpu()) and all(prm.grad is None for prm in md.parameters())
    _close(xd2.grad, dx, "x (frozen parameters)")


def test_module_forward_rows_refusals(dev):
    from avsum_amd.models.attention import MultiHeadSelfAttention
    m = MultiHeadSelfAttention(64, 2).to(dev)                         # head dim 32: the batched-GEMM path is dense-only
    x = torch.zeros(10, 64, device=dev)
    with pytest.raises(ValueError, match="head dim 32"):
        m.forward_rows(x, [0, 4, 10])
    m = MultiHeadSelfAttention(128, 2).to(dev)
    x = torch.zeros(10, 128, device=dev)
    for offsets, word in (([0, 4, 9], "x_rows has 10 rows"), ([1, 4, 10], "cover rows 1"), ([0, 4, 4, 10], "at least 1")):
        with pytest.raises(ValueError, match=word):
            m.forward_rows(x, offsets)
    with pytest.raises(ValueError, match="x_rows must be"):
        m.forward_rows(x[None], [0, 10])


@pytest.mark.parametrize("e,h,b,t", [(128, 2, 3, 45), (1024, 4, 2, 130)])
def test_module_dense_fused_backward(dev, e, h, b, t):
    """fused_backward = True: forward(x) and its gradients are forward_rows on uniform offsets bit for bit, and pass the
    criterion against the oracle.  The default False keeps today's path: its outputs and its saved tensors."""
    from avsum_amd.models.attention import MultiHeadSelfAttention
    torch.manual_seed(13)
    m = MultiHeadSelfAttention(e, h)
    assert m.fused_backward is False
    x = torch.randn(b, t, e, generator=torch.Generator().manual_seed(t + e))
    gout = torch.randn(b, t, e, generator=torch.Generator().manual_seed(3))
    offsets = np.arange(b + 1) * t
    ref, dx, grads = _oracle(m, x.reshape(b * t, e), offsets, gout.reshape(b * t, e), h)
    md = m.to(dev)

    def run(fn, xin):
        for prm in md.parameters():
            prm.grad = None
        xd = xin.to(dev).requires_grad_(True)
        out = fn(xd)
        out.backward(gout.to(dev).reshape(out.shape))
        return out, [out.detach().cpu().reshape(b * t, e), xd.grad.cpu().reshape(b * t, e)] + \
            [prm.grad.cpu().clone() for prm in md.parameters()]

    _, rows = run(lambda xd: md.forward_rows(xd, offsets), x.reshape(b * t, e))
    md.fused_backward = True
    out, dense = run(md, x)
    assert out.shape == (b, t, e) and _node(out, "_MHSARowsFunctionBackward") is not None
    for i, (a_, b_) in enumerate(zip(dense, rows)):
        assert _same(a_, b_), f"tensor {i}: the dense fused path differs from forward_rows on uniform offsets"
    _close(dense[0], ref, "out")
    _close(dense[1], dx, "x")
    for (name, _), g in zip(md.named_parameters(), dense[2:]):
        _close(g, grads[name], name)
    with torch.no_grad():                                             # without autograd: today's forward
        assert _same(md(x.to(dev)).cpu(), md._forward(x.to(dev))[0].cpu())
    # the default: _MHSAFunction, its nine saved tensors, today's outputs
    md.fused_backward = False
    out = md(x.to(dev).requires_grad_(True))
    saved = _node(out, "_MHSAFunctionBackward").saved_tensors
    assert [tuple(s.shape) for s in saved] == [(b * t, e)] * 4 + [(e, e)] * 3 + [(e,), (e, e)]
    want, (x2, q, k, att) = md._forward(x.to(dev), keep=True)
    assert _same(out.detach().cpu(), want.cpu())
    for s, w in zip(saved[:4], (x2, q, k, att)):
        assert _same(s.cpu(), w.cpu())


# --------------------------------------------------------------------------- memory
def test_backward_memory_stays_below_one_score_matrix(dev):
    """E = 256, H = 4 (D = 64), one sequence of T = 2048: [H, T, T] fp32 is 67 MB and the unfused backward holds five of
    them.  The rise of the allocator's peak across forward_rows(...).sum().backward() stays below ONE, and nothing that
    is saved for the backward has T * T entries."""
    from avsum_amd.models.attention import MultiHeadSelfAttention
    _, ops = _api()
    e, h, t = 256, 4, 2048
    torch.manual_seed(5)
    m = MultiHeadSelfAttention(e, h).to(dev)
    table = ops.AttnTable([0, t], device=dev)
    x = torch.randn(t, e, device=dev).requires_grad_(True)
    m.forward_rows(x, table).sum().backward()                         # (first use: the allocator's pools, the libraries)
    x.grad = None
    for prm in m.parameters():
        prm.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m.forward_rows(x, table)
    saved = _node(out, "_MHSARowsFunctionBackward").saved_tensors
    assert all(s.numel() < t * t for s in saved) and sum(s.numel() for s in saved) <= 5 * t * e + t * h + 4 * e * e
    out.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    one = h * t * t * 4
    print(f"peak rise {rise / 2 ** 20:.1f} MiB; one [H, T, T] fp32 buffer {one / 2 ** 20:.1f} MiB")
    assert rise < one
    assert x.grad is not None and torch.isfinite(x.grad).all()
