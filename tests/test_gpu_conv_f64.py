"""avs_conv2d_nhwc and avs_conv2d_nhwc_split per instance of igemm_kernel against float64: every case of
conv_f64_inputs.CASES (the host test test_conv_f64_host.py asserts that they reach every instance the two entry points
can launch but the ones listed there with a reason) with both operand sets - "a" within the per-element bound of the
float64 reference (AVS_F32_SPLIT, AVS_F16X2: of their float64 restatement) on EVERY element, "b" (small integers) EQUAL
to the float64 convolution.  Calls go through ops.conv2d_raw and ops.conv2d_split; AVS_F16X2 outputs are decoded with the format's plain-torch
restatement (f16x2_format.emu_unpack), not with the library's kernel.

The destination is a flat buffer filled with a NaN bit pattern: one spare pixel row, the n * Ho * Wo pixels at their
stride (the output a channel slice of them), one spare row.  Every element outside the slice must come back
bit-identical, the inputs unchanged, and a second call into a fresh buffer must give identical bits.

Measured on an MI355X over all cases (operand set "a"; the largest err / bound over the elements of a case, the bound
per element):
    AVS_F32        0.193 (f32-grid-lin-1x1-c8-n40-r64-odd-plain)
    AVS_F32_ACC64  0.223 (acc64-grid-sp-1x2-c8-n40-r64-odd-plain)
    AVS_F32_SPLIT  against its restatement: 0.156 (split-7x7-s2-p3-c16-brelu)
    AVS_F16X2      against its restatement: 0.576 (f16x2-1x1-c8-gen-plain: a sum of 8 products, where
                   the output's own packing step is most of the bound)
    AVS_BF16       1.000, a tie of the rounding: exactly half a step (bf16-grid-lin-1x1-c80-n40-r64-odd-brelu)
The whole file (793 tests) runs in about 5 seconds; the slowest case takes 0.2 seconds (the 2048 x 2048 AVS_F32 output
and the half a million rows of a 256-row-tile case), the first one 0.8 (it loads the library).
"""
import ctypes

import pytest
import torch

import conv_f64_inputs as cfi

pytestmark = pytest.mark.gpu

SENTINEL = {torch.float32: (torch.int32, 0x7FC01234), torch.bfloat16: (torch.int16, 0x7FC1)}      # NaNs no kernel produces


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _tdt(case):
    return torch.bfloat16 if case.dtype == cfi.BF16 else torch.float32


def _ref_rows(case, dev):
    """Row of the reference (the base frames of a periodic case) for every output row."""
    ho, wo = cfi.extent(case)
    r = torch.arange(case.n * ho * wo, device=dev)
    return r if not case.period else (r // (ho * wo)) % case.period * (ho * wo) + r % (ho * wo)


def _sentinel_buffer(tdt, rows, ld, dev):
    itype, pattern = SENTINEL[tdt]
    return torch.full(((rows + 2) * ld,), pattern, dtype=itype, device=dev).view(tdt)


def _launch(dev, case, o):
    """One call into fresh sentinel-filled buffers: [(buffer, its [M, columns] view, the mask of the elements outside)]
    per destination."""
    ops, _ = _api()
    tdt = _tdt(case)
    ho, wo = cfi.extent(case)
    m = case.n * ho * wo
    x = o.x_buf.to(tdt).to(dev)
    if case.period:      # the base frames repeated, on the device
        frame = torch.arange(case.n, device=dev) % case.period
        x = x[frame].contiguous()
    w = o.w_buf.to(tdt).to(dev)
    wsel = ops.weights_kstep32(w) if case.w_layout == cfi.W_KSTEP32 else w
    bias = o.bias.to(dev) if o.bias is not None else None
    held = [t.clone() if t is not None and t.numel() < 2 ** 24 else None for t in (x, wsel, bias)]
    x_img, x_row, x_px, x_off = cfi.strides(case)
    has_bias, act, alpha = cfi.EPILOGUES[case.epi]
    dests = []
    if case.split:
        n_split, relu_cols, ypad2, yc2 = case.split
        for cols, pad, c0 in ((n_split, case.ypad, case.yc0), (case.cout - n_split, ypad2, yc2)):
            dests.append((_sentinel_buffer(tdt, m, cols + pad, dev), cols, cols + pad, c0))
        xv = x.reshape(-1).as_strided((case.n, case.h, case.w, case.cin), (x_img, x_row, x_px, 1), x_off)
        views = [buf.as_strided((case.n, ho, wo, cols), (ho * wo * ld, wo * ld, ld, 1), ld + c0) for buf, cols, ld, c0 in dests]
        ops.conv2d_split(xv, wsel, views[0], n_split, views[1], bias, act, w_layout=case.w_layout, relu_cols=relu_cols)
    else:
        ld = case.cout + case.ypad
        dests.append((_sentinel_buffer(tdt, m, ld, dev), case.cout, ld, case.yc0))
        ops.conv2d_raw(case.dtype, case.n, case.h, case.w, case.cin, case.kh, case.kw, case.sh, case.sw, case.ph, case.pw, ho, wo,
                       case.cout, x, x_img, x_row, x_px, wsel, case.kh * case.kw * case.cin, dests[0][0], ld, bias, act, alpha,
                       x_off=x_off, y_off=ld + case.yc0, w_layout=case.w_layout, variant=case.variant)
    torch.cuda.synchronize(dev)
    for t, h in zip((x, wsel, bias), held):
        assert h is None or torch.equal(t, h), "an input changed"
    if case.period:
        assert torch.equal(x, o.x_buf.to(tdt).to(dev)[frame]), "the input changed"
    out = []
    for buf, cols, ld, c0 in dests:
        outside = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
        outside.as_strided((m, cols), (ld, 1), ld + c0).fill_(False)
        out.append((buf, buf.as_strided((m, cols), (ld, 1), ld + c0), outside))
    return out


def _run_twice(dev, case, which):
    o = cfi.operands(case, which)
    first = _launch(dev, case, o)
    itype, pattern = SENTINEL[_tdt(case)]
    for buf, view, outside in first:
        touched = int((buf.view(itype)[outside] != pattern).sum())
        assert touched == 0, f"{case.name}/{which}: {touched} elements outside the output slice were written"
    for (buf, _, _), (buf2, _, _) in zip(first, _launch(dev, case, o)):
        assert torch.equal(buf.view(itype), buf2.view(itype)), f"{case.name}/{which}: two calls differ"
    got = [view.contiguous() for _, view, _ in first]
    if case.dtype == cfi.F16X2:
        got = [cfi.emu_unpack(g) for g in got]      # the format's plain-torch restatement, not the library's kernel
    return torch.cat(got, 1).double()


def _where(case, at, shape):
    ho, wo = cfi.extent(case)
    row, ch = divmod(at, shape[1])
    return row // (ho * wo), row % (ho * wo) // wo, row % wo, ch


@pytest.mark.parametrize("case", cfi.CASES, ids=[c.name for c in cfi.CASES])
def test_conv_against_float64(dev, case):
    idx = _ref_rows(case, dev)
    plan = cfi.case_plan(case)[1:]
    # (a) within the bound, element by element
    got = _run_twice(dev, case, "a")
    if case.n == 0:
        assert got.numel() == 0
        return
    ref, target, bound, e32, s = (t.to(dev)[idx] for t in cfi.bundle(case, "a"))
    err = (got - target).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    worst = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err))
    at = int(worst.argmax())
    flat = lambda t: t.reshape(-1)[at].item()
    print(f"RATIO dtype={cfi.DTYPE_NAMES[case.dtype]} case={case.name!r} plan={plan} err={err.max().item():.3e} "
          f"e32={e32.max().item():.3e} bound={flat(bound):.3e} err/bound={flat(worst):.3f}")
    bad = int((err > bound).sum())
    assert bad == 0, (f"{case.name} plan {plan}: {bad} of {err.numel()} elements outside the bound, the worst at (frame, y, x, channel) = "
                      f"{_where(case, at, err.shape)}: got {flat(got)!r}, ref {flat(target)!r}, err {flat(err):.3e} > bound {flat(bound):.3e}")
    if case.dtype in (cfi.SPLIT, cfi.F16X2):      # and the restatement's own distance from the float64 convolution
        const = cfi.SPLIT_C if case.dtype == cfi.SPLIT else cfi.F16X2_C
        assert bool(((got - ref).abs() <= const * cfi.restatement_unit(case) * s + bound).all()), case.name
    del ref, target, bound, e32, s, err, worst
    # (b) exact operands: equal to the float64 convolution (bf16: rounded once)
    got = _run_twice(dev, case, "b")
    want = cfi.exact_result(case).to(dev)[idx]
    wrong = got != want
    at = int(wrong.reshape(-1).to(torch.uint8).argmax())
    assert not bool(wrong.any()), (f"{case.name} plan {plan}: {int(wrong.sum())} of {want.numel()} elements of the exact operand set differ, "
                                   f"the first at (frame, y, x, channel) = {_where(case, at, want.shape)}: got "
                                   f"{got.reshape(-1)[at].item()!r}, ref {want.reshape(-1)[at].item()!r}")


@pytest.mark.parametrize("label,status,has_bias,changes", cfi.refusals(), ids=[r[0] for r in cfi.refusals()])
def test_refusals_with_device_operands(dev, label, status, has_bias, changes):
    """The refusals of conv_geometry and of AVS_F16X2's epilogues with operands given (the host test makes these calls
    with null operands): the status, and a NaN-filled output that stays as it was.  Every operand is a zeroed buffer
    larger than any of these shapes would read or write were it accepted."""
    _, abi = _api()
    lib = abi.lib()
    x, w = (torch.zeros(1 << 18, device=dev) for _ in range(2))
    bias = torch.zeros(1 << 10, device=dev)
    y = torch.full((1 << 18,), float("nan"), device=dev)
    d = abi.ConvDesc(*cfi.desc_fields(**changes))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    got = lib.avs_conv2d_nhwc(ctypes.byref(d), ptr(x), ptr(w), ptr(bias) if has_bias else None, ptr(y), None)
    assert got == status, lib.avs_last_error()
    assert b"avs_conv2d_nhwc" in lib.avs_last_error()
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(y).all()) and not x.any() and not w.any()


def test_the_split_entry_point_refuses_what_it_does_not_take(dev):
    """avs_conv2d_nhwc_split: AVS_F16X2 only, 0 < n_split < cout and relu_cols in multiples of 8; nothing written."""
    _, abi = _api()
    lib = abi.lib()
    x, w = (torch.zeros(1 << 16, device=dev) for _ in range(2))
    y, y2 = (torch.full((1 << 16,), float("nan"), device=dev) for _ in range(2))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    base = dict(kh=1, kw=1, ph=0, pw=0, cout=72, y_px_stride=40)
    for dtype, n_split, ld2, relu_cols, status in ((cfi.F32, 40, 32, 0, cfi.E_UNSUPPORTED), (cfi.F16X2, 0, 72, 0, cfi.E_SHAPE),
                                                   (cfi.F16X2, 72, 8, 0, cfi.E_SHAPE), (cfi.F16X2, 36, 40, 0, cfi.E_SHAPE),
                                                   (cfi.F16X2, 40, 24, 0, cfi.E_SHAPE), (cfi.F16X2, 40, 32, 4, cfi.E_SHAPE),
                                                   (cfi.F16X2, 40, 32, 80, cfi.E_SHAPE)):
        d = abi.ConvDesc(*cfi.desc_fields(dtype=dtype, **base))
        got = lib.avs_conv2d_nhwc_split(ctypes.byref(d), ptr(x), ptr(w), None, ptr(y), n_split, ptr(y2), ld2, relu_cols, None)
        assert got == status, (dtype, n_split, ld2, relu_cols, lib.avs_last_error())
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(y2).all())
