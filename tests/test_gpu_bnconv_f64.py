"""avs_conv2d_nhwc_bnstats, _bnstats_xin, _bnlocal and _affine per instance of igemm_kernel (and the two instances of
igemm_h2_local224_kernel) against float64: every case of bnconv_f64_inputs.CASES - the host test test_bnconv_f64_host.py
asserts that they reach every instance these entry points can launch for AVS_F16X2 (and AVS_F32 / AVS_F32_SPLIT under the
statistics epilogue) - held on EVERY element / (group, channel) to the bounds that module states.  The tile-local and
given-affine forms go through ops.conv2d_raw / ops.conv2d_affine; the statistics forms through the C ABI, because the test
owns their workspace and their (scale, shift) tables.  Outputs are decoded with the formats' plain-torch restatements, not
with the library's kernels.

Destinations are flat buffers filled with a NaN bit pattern: one spare pixel row, the pixels at their stride (the output a
channel slice of them), one spare row; the statistics workspace is exactly the queried size plus a guard region, the
(scale, shift) tables have a guard row.  Everything outside the windows must come back bit-identical, every input
unchanged (the raw input of the input-affine form and the residual included), and a second call into fresh buffers must
give identical bits.  The input-affine form must give the bits of avs_bn_apply followed by the plain statistics form; the
224-row tile and the 256-row tile (AVS_TILE_256) of the same shape must agree within their bounds.  (GROUPW against the
general instance needs the study build: test_gpu_group_aligned.py.)

Measured on an MI355X (per form, dtype and family: checks, the largest err / e32 - err against the check's target, e32 the
restatement's own distance from the float64 reference, which for the raw output of AVS_F32_SPLIT / AVS_F16X2 is the
dropped lo * lo product alone - and the check closest to its bound, err / bound):
    affine   f16x2  grid    y          24     1.61   0.422 (f16x2-affine-grid-lin-c40-n128-odd-rpg64-normal)
    affine   f16x2  groups  y          32     1.21   0.369 (f16x2-affine-1x1-c136-m495-t128-rpg192-normal)
    bnlocal  f16x2  grid    moments     7     4.55   0.015 (f16x2-bnlocal-grid-tap9-c16-n64-fk-rpg64-const)
    bnlocal  f16x2  grid    y          14     1.00   0.473 (f16x2-bnlocal-grid-ns-c40-n64-odd-rpg64-mean40)
    bnlocal  f16x2  groups  moments    18    19.20   0.053 (f16x2-bnlocal-local-bare-1x1-s1-rpg42-const)
    bnlocal  f16x2  groups  y          30     1.01   0.793 (f16x2-bnlocal-local-3x3-s2-rpg256-mean40)
    stats    f16x2  grid    raw        52   350.28   0.632 (f16x2-stats-grid-sp-1x2-c8-n72-r64-odd-rpg100-normal)
    stats    f16x2  grid    scale      52     2.64   0.827 (f16x2-stats-grid-ns-3x3-c64-n72-r128-fk-rpg65-mean40)
    stats    f16x2  grid    shift      52     2.87   0.717 (f16x2-stats-grid-ns-1x1-c8-n40-r64-odd-rpg65-mean40)
    stats    f16x2  groups  raw        23   173.00   0.655 (f16x2-stats-groups-3x3-n8-rpg300-const)
    stats    f16x2  groups  scale      23     1.32   0.410 (f16x2-stats-groups-1x1-n64-rpg600-mean40)
    stats    f16x2  groups  shift      23     1.52   0.342 (f16x2-stats-groups-1x1-n128-rpg196-mean40)
    stats    f16x2  tall    raw         8     8.72   0.352 (f16x2-stats-tall-3x3-c32-n72-f3-rpg189-const)
    stats    f16x2  tall    scale       8     1.49   0.165 (f16x2-stats-tall-3x3-c16-n8-f2-xin-rpg126-const)
    stats    f16x2  tall    shift       8     2.51   0.408 (f16x2-stats-tall-3x3-c16-n8-f2-xin-rpg126-const)
    stats    f32    grid    raw        36     3.65   0.840 (f32-stats-grid-sp-3x3-c40-n72-r64-odd-rpg65-mean40)
    stats    f32    grid    scale      36     3.14   0.842 (f32-stats-grid-sp-3x3-c64-n40-r128-fk-rpg65-mean40)
    stats    f32    grid    shift      36     3.69   0.838 (f32-stats-grid-ns-3x3-c64-n40-r128-fk-rpg65-mean40)
    stats    f32    groups  raw        20     3.04   0.425 (f32-stats-groups-1x1-n8-rpg64-mean40)
    stats    f32    groups  scale      20     2.22   0.938 (f32-stats-groups-1x1-n128-rpg196-mean40)
    stats    f32    groups  shift      20     2.09   0.884 (f32-stats-groups-1x1-n128-rpg196-mean40)
    stats    split  grid    raw        48     0.26   0.478 (split-stats-grid-ns-3x3-c40-n40-r64-odd-rpg65-mean40)
    stats    split  grid    scale      48     2.49   0.976 (split-stats-grid-ns-3x3-c64-n40-r128-fk-rpg65-mean40)
    stats    split  grid    shift      48     2.50   0.963 (split-stats-grid-ns-3x3-c64-n40-r128-fk-rpg65-mean40)
    stats    split  groups  raw        20     0.12   0.264 (split-stats-rows256-3x3-rpg100-mean40)
    stats    split  groups  scale      20     1.93   0.770 (split-stats-groups-1x1-n8-rpg64-mean40)
    stats    split  groups  shift      20     2.07   0.770 (split-stats-groups-1x1-n8-rpg64-mean40)
(the scale / shift figures of the mean40 channels of AVS_F32 / AVS_F32_SPLIT were taken with their e32 pooled per group; it is
now pooled over the table, which only lowers them).  The smallest group the tile-local form takes, 37 rows (six groups per
tile, a wave in three groups), passes.  The whole file (346 tests) runs in 4.0 seconds; the slowest case takes 0.9 seconds,
the first one (it loads the library), the next 0.37 (the cin = 144 input-affine case over half a million rows) and 0.22.
"""
import ctypes
import time

import pytest
import torch

import bnconv_f64_inputs as bfi
import conv_f64_inputs as cfi

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC01234           # a NaN no kernel produces (int32 lanes; the byte buffers of AVS_F16P8 take its low byte)
GUARD = 256                     # 4-byte lanes behind the statistics workspace


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _filled(lanes, dev):
    return torch.full((lanes,), NAN_BITS, dtype=torch.int32, device=dev)


def _ptr(t, offset_bytes=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _stage(dev, case):
    """The operands of a case on the device (the periodic cases' frames and affine rows built by index)."""
    ops, abi = _api()
    o, c, lay = bfi.operands(case), case.conv, bfi.layout(case)
    groups = bfi.groups_of(case)
    x = o.x_buf.to(dev)
    if case.x_p8:
        x = x.reshape(o.x_base.shape[0], -1)
    if c.period:
        x = x[torch.arange(c.n, device=dev) % c.period].contiguous()
    w = o.w_buf.to(dev)
    s = dict(x=x, w=ops.weights_kstep32(w) if c.w_layout == cfi.W_KSTEP32 else w, gamma=o.gamma.to(dev), beta=o.beta.to(dev))
    if case.xin is not None:
        aff = torch.arange(groups, device=dev) % bfi.AFF_PERIOD if c.period else torch.arange(groups, device=dev)
        s["in_scale"], s["in_shift"] = o.isc.to(dev)[aff].contiguous(), o.ish.to(dev)[aff].contiguous()
    if case.res is not None:
        s["residual"] = o.res_buf.to(dev)
    if case.res_affine:
        s["res_scale"], s["res_shift"] = o.rsc.to(dev), o.rsh.to(dev)
    if case.form == "affine":
        given = bfi.reference(case).given
        s["scale"], s["shift"] = given[0].to(dev), given[1].to(dev)
    return s


def _desc(abi, case):
    c = case.conv
    ho, wo = cfi.extent(c)
    x_img, x_row, x_px, _ = cfi.strides(c)
    return abi.ConvDesc(c.dtype, c.n, c.h, c.w, c.cin, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, ho, wo, c.cout, x_img, x_row, x_px,
                        c.kh * c.kw * c.cin, c.cout + c.ypad, bfi.RELU if case.relu else 0, 1.0, c.w_layout, c.variant,
                        abi.X_F16P8 if case.x_p8 else 0)


def _launch(dev, case, s):
    """One call into fresh NaN-filled destinations: {name: (buffer, mask of the lanes / bytes outside the window)} and the
    decoded results."""
    ops, abi = _api()
    lib = abi.lib()
    c = case.conv
    ho, wo = cfi.extent(c)
    m, groups = bfi.rows_of(case), bfi.groups_of(case)
    ld = c.cout + c.ypad
    x_off = cfi.strides(c)[3]
    dests = {}
    if case.y_p8:
        ybuf = torch.full(((m + 2) * 3 * c.cout,), NAN_BITS & 0xFF, dtype=torch.uint8, device=dev)
        outside = torch.ones_like(ybuf, dtype=torch.bool)
        outside[3 * c.cout:(m + 1) * 3 * c.cout] = False
    else:
        ybuf = _filled((m + 2) * ld, dev)
        outside = torch.ones_like(ybuf, dtype=torch.bool)
        outside.as_strided((m, c.cout), (ld, 1), ld + c.yc0).fill_(False)
    dests["y"] = (ybuf, outside)
    res = None
    if case.res == "h2":
        res = s["residual"][:, :c.cout]
    scale = shift = None
    if case.form == "stats":
        need = lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(_desc(abi, case)), case.rpg)
        assert need == bfi.case_plan(case).ws_bytes and need % 4 == 0
        ws = _filled(need // 4 + GUARD, dev)
        guard = torch.zeros_like(ws, dtype=torch.bool)
        guard[need // 4:] = True
        dests["ws"] = (ws, guard)
        for name in ("scale", "shift"):
            t = _filled((groups + 1) * c.cout, dev)
            row = torch.zeros_like(t, dtype=torch.bool)
            row[groups * c.cout:] = True
            dests[name] = (t, row)
        entry = "bnstats" if case.xin is None else "bnstats_xin"
        a = dict(x=_ptr(s["x"], x_off * 4), w=_ptr(s["w"]), y=_ptr(ybuf, (ld + c.yc0) * 4), gamma=_ptr(s["gamma"]), beta=_ptr(s["beta"]),
                 scale=_ptr(dests["scale"][0]), shift=_ptr(dests["shift"][0]), ws=_ptr(ws), in_scale=_ptr(s.get("in_scale")),
                 in_shift=_ptr(s.get("in_shift")))
        args = bfi.entry_args(entry, a, case.rpg, ws_bytes=need, in_relu=int(bool(case.xin)),
                              stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        st = getattr(lib, bfi.ENTRY_POINTS[entry])(ctypes.byref(_desc(abi, case)), *args)
        assert st == 0, (case.name, st, lib.avs_last_error())
        scale = dests["scale"][0].view(torch.float32)[:groups * c.cout].view(groups, c.cout)
        shift = dests["shift"][0].view(torch.float32)[:groups * c.cout].view(groups, c.cout)
    elif case.form == "bnlocal":
        x_img, x_row, x_px, _ = cfi.strides(c)
        ops.conv2d_raw(c.dtype, c.n, c.h, c.w, c.cin, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, ho, wo, c.cout, s["x"], x_img, x_row, x_px,
                       s["w"], c.kh * c.kw * c.cin, ybuf.view(torch.float32), ld, act=bfi.RELU if case.relu else 0, x_off=x_off,
                       y_off=ld + c.yc0, bnlocal=(case.rpg, s["gamma"], s["beta"], bfi.BN_EPS, res), w_layout=c.w_layout,
                       variant=c.variant)
    else:
        x_img, x_row, x_px, _ = cfi.strides(c)
        y = ops.P8(ybuf[3 * c.cout:], (m, c.cout)) if case.y_p8 else ybuf.view(torch.float32)[ld + c.yc0:]
        if case.res == "p8":
            res = ops.P8(s["residual"], (m, c.cout))
        ops.conv2d_affine(c.dtype, c.n, c.h, c.w, c.cin, c.sh, c.sw, ho, wo, c.cout, s["x"], x_img, x_row, x_px, s["w"], c.cin, y,
                          ld, case.rpg, s["scale"], s["shift"], residual=res, relu=case.relu,
                          res_affine=(s["res_scale"], s["res_shift"]) if case.res_affine else None, w_layout=c.w_layout,
                          variant=c.variant)
    torch.cuda.synchronize(dev)
    if case.y_p8:
        got = bfi.emu_p8_unpack(ybuf[3 * c.cout:(m + 1) * 3 * c.cout].cpu(), (m, c.cout)).to(dev)
    else:
        got = ybuf.view(torch.float32).as_strided((m, c.cout), (ld, 1), ld + c.yc0).contiguous()
        if c.dtype == bfi.F16X2:
            got = bfi.emu_unpack(got)
    return dests, SimpleResult(got.double(), scale, shift)


class SimpleResult:
    def __init__(self, y, scale, shift):
        self.y, self.scale, self.shift = y, scale, shift


def _run_twice(dev, case):
    s = _stage(dev, case)
    held = {k: v.clone() for k, v in s.items()}
    dests, got = _launch(dev, case, s)
    for name, (buf, outside) in dests.items():
        pattern = NAN_BITS & 0xFF if buf.dtype == torch.uint8 else NAN_BITS
        touched = int((buf[outside] != pattern).sum())
        assert touched == 0, f"{case.name}: {touched} lanes outside the window of {name} were written"
    for k in s:
        assert torch.equal(s[k], held[k]), f"{case.name}: the input {k} changed"
    dests2, _ = _launch(dev, case, s)
    for name in dests:
        assert torch.equal(dests[name][0], dests2[name][0]), f"{case.name}: two calls differ in {name}"
    return s, dests, got


def _held(dev, name, case, got, target, bound, idx, what):
    """Every element of got within bound of target[idx]; prints the RATIO line of the check closest to its bound."""
    target, bound = target.to(dev)[idx], bound.to(dev)[idx]
    err = (got.double() - target).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    worst = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err))
    at = int(worst.argmax())
    flat = lambda t: t.reshape(-1)[at].item()
    e32 = (getattr(bfi.bundle(case).rs, name).double() - bfi.bundle(case).ref.__dict__[what]).abs().max().item()
    print(f"RATIO form={case.form} check={name} case={case.name!r} err={err.max().item():.3e} e32={e32:.3e} "
          f"bound={flat(bound):.3e} err/bound={flat(worst):.3f} err/e32={err.max().item() / e32 if e32 else float('inf'):.2f}")
    bad = int((err > bound).sum())
    assert bad == 0, (f"{case.name} {name}: {bad} of {err.numel()} outside the bound, the worst at (row or group, channel) = "
                      f"{divmod(at, err.shape[1])}: got {flat(got)!r}, ref {flat(target)!r}, err {flat(err):.3e} > bound {flat(bound):.3e}")


@pytest.mark.parametrize("case", bfi.CASES, ids=[c.name for c in bfi.CASES])
def test_bnconv_against_float64(dev, case):
    t0 = time.perf_counter()
    s, dests, got = _run_twice(dev, case)
    b = bfi.bundle(case)
    hrow, hgroup = bfi.device_maps(case, dev)
    if case.form == "stats":
        _held(dev, "raw", case, got.y, *b.raw, hrow, "acc")
        if b.raw_slack is not None:
            ref, slack, bound = b.ref.acc.to(dev)[hrow], b.raw_slack.to(dev)[hrow], b.raw[1].to(dev)[hrow]
            assert bool(((got.y - ref).abs() <= slack + bound).all()), case.name
        _held(dev, "scale", case, got.scale, *b.scale, hgroup, "scale")
        _held(dev, "shift", case, got.shift, *b.shift, hgroup, "shift")
        gamma0 = (bfi.operands(case).gamma == 0).to(dev)
        assert bool((got.scale[:, gamma0] == 0).all()), f"{case.name}: scale is not exactly 0 where gamma is 0"
    else:
        _held(dev, "y", case, got.y, *b.y, hrow, "y")
        if bfi.has_moments(case):
            ok, err, e32, bound, where = bfi.compare_moments(got.y.cpu(), b.ref.y, b.rs.y, bfi.layout(case).groups, case.rpg)
            print(f"RATIO form={case.form} check=moments case={case.name!r} err={err:.3e} e32={e32:.3e} bound={bound:.3e} "
                  f"err/bound={err / bound:.3f} err/e32={err / e32 if e32 else float('inf'):.2f}")
            assert ok, (case.name, "moments", err, bound, where)
    if case.xin is not None:        # the bits of avs_bn_apply followed by the plain statistics form
        ops, _ = _api()
        c = case.conv
        m = bfi.rows_of(case)
        rows = torch.tensor(list(range(0, m, case.rpg)) + [m], dtype=torch.int64, device=dev)
        applied = s["x"].clone().view(-1, c.cin)
        ops.bn_apply(applied, s["in_scale"], s["in_shift"], rows, case.rpg, None, ops.ACT_RELU if case.xin else ops.ACT_NONE, applied,
                     code=c.dtype)
        plain = case._replace(xin=None)
        dests2, _ = _launch(dev, plain, dict(s, x=applied))
        for name in ("y", "scale", "shift"):
            assert torch.equal(dests[name][0], dests2[name][0]), f"{case.name}: {name} differs from avs_bn_apply + the plain form"
    torch.cuda.synchronize(dev)
    print(f"SECONDS case={case.name!r} {time.perf_counter() - t0:.3f}")


def test_the_224_row_tile_agrees_with_the_256_row_tile(dev):
    pairs = [(c, bfi.CASE_BY_NAME[c.name.replace("local224", "t256")]) for c in bfi.CASES if "-local224-" in c.name]
    assert len(pairs) == 4
    for small, tall in pairs:
        assert bfi.case_plan(small).local224 and not bfi.case_plan(tall).local224 and bfi.operands(small).x_buf.shape == bfi.operands(tall).x_buf.shape
        # (the two cases are seeded by name: run the 256-row tile on the 224-row case's operands)
        twin = small._replace(conv=small.conv._replace(variant=bfi.TILE_256))
        assert not bfi.case_plan(twin).local224
        ya = _launch(dev, small, _stage(dev, small))[1].y
        yb = _launch(dev, twin, _stage(dev, small))[1].y
        target, bound = (t.to(dev) for t in bfi.bundle(small).y)
        assert bool(((ya - yb).abs() <= 2.0 * bound).all()), small.name
        assert bool(((yb - target).abs() <= bound).all()), small.name


@pytest.mark.parametrize("label,entry,status,changes,kw", bfi.refusals(), ids=[r[0] for r in bfi.refusals()])
def test_refusals_with_device_operands(dev, label, entry, status, changes, kw):
    """The refusals of the four entry points with device buffers larger than any of these shapes would touch were it
    accepted: the documented status, and destinations that come back bit-identical."""
    _, abi = _api()
    lib = abi.lib()
    f = bfi.desc_fields(**changes)
    n, h, w, cin, ho, wo, cout = f[1], f[2], f[3], f[4], f[11], f[12], f[13]
    rpg = kw.get("rpg", 64)
    m = n * ho * wo
    ldr = kw.get("ldr", cout)
    lanes = dict(x=n * h * w * cin, w=cout * f[17], y=(m + 1) * max(f[18], cout), gamma=cout, beta=cout, residual=(m + 1) * max(ldr, cout))
    groups = m // max(rpg, 1) + 2
    for name in ("scale", "shift", "res_scale", "res_shift"):
        lanes[name] = groups * cout
    lanes["in_scale"] = lanes["in_shift"] = groups * cin
    d = abi.ConvDesc(*f)
    ws = lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(d), rpg) if entry.startswith("bnstats") else 0
    lanes["ws"] = max(ws, 0) // 4 + GUARD
    dest = {"y", "ws"} | ({"scale", "shift"} if entry.startswith("bnstats") else set())
    bufs = {name: (_filled(lanes[name] + 64, dev) if name in dest else torch.zeros(lanes[name] + 64, dtype=torch.int32, device=dev))
            for name in bfi.POINTERS[entry]}
    a = {name: _ptr(t) for name, t in bufs.items()}
    for name in kw.get("null", ()):
        a[name] = None
    for name in kw.get("misalign", ()):
        a[name] = _ptr(bufs[name], 8)
    args = bfi.entry_args(entry, a, rpg, ldr=ldr, ws_bytes=max(ws, 0) - (1 if kw.get("ws_short") else 0))
    got = getattr(lib, bfi.ENTRY_POINTS[entry])(ctypes.byref(d), *args)
    assert got == status, (got, lib.avs_last_error())
    torch.cuda.synchronize(dev)
    for name, t in bufs.items():
        assert bool((t == (NAN_BITS if name in dest else 0)).all()), f"{label}: {name} was written"
