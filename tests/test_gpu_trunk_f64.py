"""Every step of the ResNet-50 trunk against float64, with BatchNorm parameters that differ per layer, take both signs
and hold an exact zero (trunk_f64_inputs.randomize_bn).  Every other trunk test runs resnet50_trunk()'s defaults (weight
1, bias 0), under which a step that is handed another layer's parameters, a stacked vector in the wrong order or no beta
gives the same bits (test_trunk_f64_host.py states that, and that the bars used here catch each such mistake).

The runner is recorded from outside (no product change): its _conv and _gram_pair and the two fused-stem wrappers of ops
are wrapped for one forward; a recorder clones its inputs BEFORE the call (the Gram steps and the declined nine-tap path
finish their input in place) and the input, the output and a returned (scale, shift) after it.

  end to end   features against the float64 trace: 5e-4 * max(1, max|ref|), the project's trunk bar
               (test_resnet50_trunk_f16x2), for AVS_F16X2 and exact fp32, batch and folded BatchNorm.  Per step the
               error of its finished output against the trace is printed, so that a failure names the step.
  forced       per step, the float64 reference computed from the DEVICE's own captured inputs of that step (error does
               not travel through 53 BatchNorms), weights = the trunk's own state dict by the step's name (AVS_F16X2: what
               the format keeps of them, emu_unpack(emu_pack(w))), a raw input finished in float64 with the captured
               (scale, shift).  TOL = 1e-5 (AVS_F16X2) / 2e-5 (exact fp32), the kernel bars of test_gpu_f16x2.py;
               amp = max(1, max |gamma| / sqrt(var + eps) * max|raw|):
                 finished   TOL * max(amp, max|ref|)
                 deferred   raw output: TOL * max(1, max|raw|); (scale, shift) against float64 statistics of the stored raw
                            output: scale 2e-5 relative (exactly 0 where gamma is 0), shift 2e-5 * max(1, max|raw| max|scale|)
                 p8         the finished bound + 2^-18 |ref| + 2^-24 (the format's resolution, test_gpu_f16p8.py)
                 fused AVS_F16X2 stem   test_fused_stem_f16x2's bars for random frames (pooled raw map: max where
                            gamma >= 0, min elsewhere)
                 an input finished in place: TOL * max(1, max|.|) against relu(scale * before + shift)

Measured on one MI355X (largest error / bound per case, and the step where it occurred):
  case                                        end to end (of its bar)             forced: largest error / bound, step (checks)
  f16x2, 8 frames in fours                    8.92e-5 (0.178)                     0.663  layer1.0.conv1+downsample, downsample (108)
  f16x2, 3 frames, per-frame groups           2.63e-5 (0.053)                     0.277  layer1.0.conv1+downsample, downsample (108)
  f16x2, groups [0, 4, 5]                     2.37e-5 (0.047)                     0.098  layer3.2.conv2 (53)
  f16x2, fours, one switch off                8.69e-5 .. 9.55e-5 (0.174 .. 0.191; the largest: fused_stem off)
  exact fp32, groups [0, 4]                   1.55e-5 (0.031)                     0.065  layer4.0.conv2 (53)
  exact fp32, 4 per-frame groups              8.98e-6 (0.018)                     0.064  layer3.5.conv2 (53)
  folded, fp32 / f16x2, 4 frames              5.89e-7 (0.001) / 1.37e-6 (0.003)
  fp32-split, fours / 4 per-frame groups      2.416e-4 / 1.409e-4: the bars are 3 times these, 7.25e-4 / 4.23e-4
  Inception-v3, fp32 / f16x2                  4.25e-7 (0.004) / 1.30e-6 (0.013) of 1e-4
The per-step error against the trace (not forced) grows to 4.6e-4 of a map's largest value by layer 4 in the f16x2 cases
and to 8e-5 in exact fp32 - the conditioning of 53 batch-normalised layers, which the forced comparison leaves out.
No step failed: the runner's hand-offs are right.

bf16 is NOT tested here.  Measured against the float64 trace: relative L2 6.2e-2 / 3.1e-2, 1 - cosine 1.9e-3 / 4.9e-4
(fours / per-frame).  Bars of 3 times that (0.19, 0.09) are not 10 times below the planted mistakes in the same metric
(relative L2 from 0.004 - one flipped sign in the last BatchNorm - to 0.17; test_trunk_f64_host.py), so the case could not
tell a wiring mistake from bf16 rounding and was left out.  The bf16 convolution + BatchNorm kernels are held to float64
one kernel at a time, per (group, channel), in test_gpu_convbn_f64.py.

The folded cases run on dark frames (trunk_f64_inputs.frames): with synthetic running statistics the trunk does not
normalise and full-range frames carry layer 4 to 2e6, past the 65504 at which AVS_F16X2 saturates by design.
"""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import trunk_f64_inputs as tfi

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _ops():
    from avsum_amd import ops
    return ops


# --------------------------------------------------------------------------- recording one forward
def _clone(t):
    ops = _ops()
    if t is None:
        return None
    if isinstance(t, ops.P8):
        return ops.P8(t.data.clone(), t.shape)
    if isinstance(t, (tuple, list)):
        return tuple(_clone(v) for v in t)
    return t.clone()


def _same_bits(a, b):
    ops = _ops()
    a, b = (v.data if isinstance(v, ops.P8) else v for v in (a, b))
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def record_forward(runner, frames_dev, groups):
    """(features, records in launch order) of one forward with every step's operands cloned around its call."""
    ops = _ops()
    records = []
    conv, pair = runner._conv, runner._gram_pair
    stem_h2, stem_bf16 = ops.stem_conv_pool_h2, ops.stem_conv_bn_pool

    def rec_conv(st, w, x, x_aff, groups_, residual=None, res_aff=None):
        r = SimpleNamespace(kind="conv", st=st, x_before=_clone(x), x_aff=_clone(x_aff), residual=_clone(residual),
                            res_aff=_clone(res_aff))
        out, aff = conv(st, w, x, x_aff, groups_, residual, res_aff)
        r.out, r.aff, r.x_after = _clone(out), _clone(aff), _clone(x)
        records.append(r)
        return out, aff

    def rec_pair(st, w, x, x_aff, gmax):
        r = SimpleNamespace(kind="pair", st=st, x_before=_clone(x), x_aff=_clone(x_aff))
        t, idn = pair(st, w, x, x_aff, gmax)
        r.out, r.out_down, r.x_after = _clone(t), _clone(idn), _clone(x)
        records.append(r)
        return t, idn

    def rec_stem(fn):
        def f(frames_u8, *a, **k):
            r = SimpleNamespace(kind="stem", frames=frames_u8.clone())
            y, sc, sh = fn(frames_u8, *a, **k)
            r.out, r.aff = _clone(y), (_clone(sc), _clone(sh))
            records.append(r)
            return y, sc, sh
        return f

    runner._conv, runner._gram_pair = rec_conv, rec_pair
    ops.stem_conv_pool_h2, ops.stem_conv_bn_pool = rec_stem(stem_h2), rec_stem(stem_bf16)
    try:
        feat = runner.forward(frames_dev, groups)
    finally:
        del runner._conv, runner._gram_pair          # (instance attributes over the class's methods)
        ops.stem_conv_pool_h2, ops.stem_conv_bn_pool = stem_h2, stem_bf16
    steps = runner.plan(frames_dev.shape[0], groups)
    assert [r.st.name for r in records if r.kind != "stem"] == [s.name for s in steps if not s.form.startswith("stem_")]
    for r in records:
        if r.kind == "stem":
            r.st = steps[0]
            assert r.st.form.startswith("stem_")
    assert len(records) == len(steps)
    return feat, records


def _vals(t, h2):
    """The fp32 values of a stored tensor, on its device."""
    ops = _ops()
    if isinstance(t, ops.P8):
        return ops.f16p8_unpack(t)
    return ops.f16x2_unpack(t.contiguous()) if h2 else t.float()


def _v64(t, h2):
    return _vals(t, h2).cpu().double()


# --------------------------------------------------------------------------- float64 arithmetic of one step
def _sd_keys(name):
    """torchvision's step name -> (convolution weight key, BatchNorm prefix) of the nn.Sequential trunk's state dict."""
    if name == "conv1":
        return "0.weight", "1."
    layer, block, part = name.split(".")
    p = f"{int(layer[5:]) + 3}.{block}."
    if part == "downsample":
        return p + "downsample.0.weight", p + "downsample.1."
    return p + part + ".weight", p + "bn" + part[4:] + "."


def _gid(groups, n):
    return torch.bucketize(torch.arange(n), torch.tensor(groups[1:-1], dtype=torch.int64), right=True)


def _affine(a, aff, gid, relu):
    """a NHWC (or [rows, C] of n frames) float64, aff = (scale, shift) [groups, C]."""
    sc, sh = (v.cpu().double()[gid] for v in aff)
    shape = a.shape
    y = a.reshape(len(gid), -1, shape[-1]) * sc[:, None, :] + sh[:, None, :]
    return (torch.relu(y) if relu else y).reshape(shape)


def _conv64(a, w, stride, pad):
    return F.conv2d(a.permute(0, 3, 1, 2), w, None, stride, pad).permute(0, 2, 3, 1).contiguous()


def _stats(raw, groups):
    """(mean, biased variance) [groups, C] of a float64 NHWC map over each group's frames."""
    parts = [raw[a:b].reshape(-1, raw.shape[-1]) for a, b in zip(groups[:-1], groups[1:])]
    return torch.stack([p.mean(0) for p in parts]), torch.stack([p.var(0, unbiased=False) for p in parts])


def _weight(sd, key, h2):
    w = sd[key].float()
    if h2:   # what AVS_F16X2 keeps of a weight (an element's hi + lo does not depend on where its run of 8 starts)
        w = tfi.emu_unpack(tfi.emu_pack(w.reshape(-1, 8))).reshape(w.shape)
    return w.double()


class _Report:
    """Collects error / bound per check; the test asserts at its end so that every step gets printed."""

    def __init__(self, case):
        self.case, self.rows, self.failed = case, [], []

    def check(self, step, what, err, bound):
        err, bound = float(err), float(bound)
        ok = math.isfinite(err) and err <= bound
        self.rows.append((err / bound if bound > 0 else (0.0 if err == 0 else math.inf), step, what))
        if not ok:
            self.failed.append(f"{step} {what}: {err:.3e} > {bound:.3e}")

    def worst(self):
        return max(self.rows) if self.rows else (0.0, "-", "-")


def _check_output(rep, st, what, got, ref, tol, amp, p8):
    bound = tol * max(amp, ref.abs().max().item())
    d = (got - ref).abs()
    if p8:   # elementwise: the format's resolution on top
        lim = bound + 2.0 ** -18 * ref.abs() + 2.0 ** -24
        i = (d / lim).argmax()
        rep.check(st.name, what, d.flatten()[i], lim.flatten()[i])
    else:
        rep.check(st.name, what, d.max(), bound)


def _bn_ref(raw, groups, gid, gamma, beta):
    mean, var = _stats(raw, groups)
    scale = gamma / torch.sqrt(var + EPS)
    shift = beta - mean * scale
    amp = max(1.0, scale.abs().max().item() * raw.abs().max().item())
    return _affine(raw, (scale, shift), gid, False), scale, shift, amp


def _check_affine(rep, st, aff, stored_raw, raw_ref, groups, gamma, beta, bar=2e-5):
    """A returned (scale, shift) against float64 statistics of the device's own stored raw output (test_conv_bnstats_f16x2)."""
    mean, var = _stats(stored_raw, groups)
    sc_own = gamma / torch.sqrt(var + EPS)
    sh_own = beta - mean * sc_own
    sc, sh = (v.cpu().double() for v in aff)
    nz = gamma != 0
    rep.check(st.name, "scale", ((sc - sc_own).abs()[:, nz] / sc_own.abs()[:, nz]).max(), bar)
    rep.check(st.name, "scale where gamma = 0", sc[:, ~nz].abs().max() if (~nz).any() else 0.0, 0.0)
    ynorm = raw_ref.abs().max().item() * sc_own.abs().max().item()
    rep.check(st.name, "shift", (sh - sh_own).abs().max(), bar * max(1.0, ynorm))


def _input(rep, r, h2, gid, tol):
    """The step's input in float64 (a raw input finished with the captured affine); checks an input stored in place."""
    xb = _v64(r.x_before, h2)
    if r.st.inp == "raw":
        assert r.x_aff is not None, r.st.name
        a = _affine(xb, r.x_aff, gid, True)
    else:
        assert r.x_aff is None, r.st.name
        a = xb
    if not _same_bits(r.x_before, r.x_after):
        assert r.st.inp == "raw", f"{r.st.name}: a finished input was overwritten"
        rep.check(r.st.name, "input finished in place", (_v64(r.x_after, h2) - a).abs().max(), tol * max(1.0, a.abs().max().item()))
    return a


def forced_checks(rep, records, sd, h2, groups, tol):
    n = groups[-1]
    gid = _gid(groups, n)
    for r in records:
        st = r.st
        if r.kind == "stem":
            assert st.form == "stem_f16x2"
            gamma, beta = sd["1.weight"].double(), sd["1.bias"].double()
            x = tfi.preprocess(r.frames.cpu().numpy())
            raw = F.conv2d(x, sd["0.weight"].double(), None, 2, 3).permute(0, 2, 3, 1)
            _, sc_ref, sh_ref, _ = _bn_ref(raw, groups, gid, gamma, beta)
            sc, sh = (v.cpu().double() for v in r.aff)
            nz = gamma != 0
            rep.check("conv1", "scale", ((sc - sc_ref).abs()[:, nz] / sc_ref.abs()[:, nz]).max(), 2e-5)
            rep.check("conv1", "scale where gamma = 0", sc[:, ~nz].abs().max(), 0.0)
            ynorm = raw.abs().max().item() * sc_ref.abs().max().item()
            rep.check("conv1", "shift", (sh - sh_ref).abs().max(), 2e-5 * max(1.0, ynorm))
            sgn = torch.sign(gamma + (gamma == 0)).view(1, 64, 1, 1)
            pooled = (F.max_pool2d(raw.permute(0, 3, 1, 2) * sgn, 3, 2, 1) * sgn).permute(0, 2, 3, 1)
            rep.check("conv1", "pooled raw map", (_v64(r.out, True) - pooled).abs().max(), tol * max(1.0, raw.abs().max().item()))
            continue
        a = _input(rep, r, h2, gid, tol)
        if r.kind == "pair":
            for part, out, relu in (("conv1", r.out, True), ("downsample", r.out_down, False)):
                wkey, bnp = _sd_keys(f"layer1.0.{part}")
                raw = _conv64(a, _weight(sd, wkey, h2), 1, 0)
                ref, _, _, amp = _bn_ref(raw, groups, gid, sd[bnp + "weight"].double(), sd[bnp + "bias"].double())
                ref = torch.relu(ref) if relu else ref
                _check_output(rep, st, part, _v64(out, h2).reshape(ref.shape), ref, tol, amp, False)
            continue
        wkey, bnp = _sd_keys(st.name)
        gamma, beta = sd[bnp + "weight"].double(), sd[bnp + "bias"].double()
        geom = st.geom[0]
        stem = st.block < 0
        if stem:   # the pre-padded 4-channel image [n,230,232,4]; the reduction's fourth channel and eighth pixel are zeros
            raw = _conv64(a[..., :3], _weight(sd, wkey, h2), 2, 0)[:, :112, :112].contiguous()
        else:
            raw = _conv64(a, _weight(sd, wkey, h2), geom[6], geom[8])
        if st.out == "deferred":
            assert r.aff is not None and r.residual is None
            got = _v64(r.out, h2)
            rep.check(st.name, "raw output", (got - raw).abs().max(), tol * max(1.0, raw.abs().max().item()))
            _check_affine(rep, st, r.aff, got, raw, groups, gamma, beta)
            continue
        assert r.aff is None
        ref, _, _, amp = _bn_ref(raw, groups, gid, gamma, beta)
        assert (r.residual is not None) == (st.res != "none") and (r.res_aff is not None) == (st.res == "deferred"), st.name
        if r.residual is not None:
            res = _v64(r.residual, h2).reshape(ref.shape)
            ref = ref + (_affine(res, r.res_aff, gid, False) if r.res_aff is not None else res)
        if not st.name.endswith("downsample"):
            ref = torch.relu(ref)
        if stem:
            ref = F.max_pool2d(ref.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        p8 = isinstance(r.out, _ops().P8)
        assert p8 == (st.out == "p8"), st.name
        _check_output(rep, st, "output", _v64(r.out, h2).reshape(ref.shape), ref, tol, amp, p8)


def unforced_errors(case, records, trace, h2, groups, dev):
    """Prints, per step, the error of its finished output against the float64 trace (relative to the largest value)."""
    gid = _gid(groups, groups[-1])
    worst = (0.0, "-")
    for r in records:
        st = r.st
        outs = [(st.name, r.out, getattr(r, "aff", None))]
        if r.kind == "pair":
            outs = [("layer1.0.conv1", r.out, None), ("layer1.0.downsample", r.out_down, None)]
        for name, out, aff in outs:
            key = "maxpool" if name == "conv1" else name.rsplit(".", 1)[0] if name.endswith("conv3") else name
            ref = trace[key].to(dev).permute(0, 2, 3, 1)
            got = _vals(out, h2).reshape(ref.shape)
            if aff is not None:
                sc, sh = (v.float()[gid.to(dev)].view(ref.shape[0], 1, 1, -1) for v in aff)
                got = got * sc + sh
                got = got if name.endswith("downsample") else torch.relu(got)
            err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
            worst = max(worst, (err, name))
            print(f"[{case}] {name:28s} {st.form:10s} in {st.inp:8s} out {st.out:8s} vs trace {err:.2e}")
    return worst


# --------------------------------------------------------------------------- the cases
def _run(dev, case, groups, bn_mode="batch", forced=True, switch=None, bar=tfi.TRUNK_BAR, **mode):
    """One runner on tfi.frames(n) in BatchNorm groups `groups`: end to end against the float64 trace, per step forced."""
    from avsum_amd.cnn import ResNet50Runner
    n = groups[-1]
    trunk = tfi.make_trunk(running=bn_mode == "folded")
    sd = tfi.state_dict(trunk, torch.float32)
    ref, trace = tfi.trace(tfi.SEED, groups, bn_mode)
    runner = ResNet50Runner(trunk.to(dev), torch.float32, bn_mode, **mode)
    if switch is not None:
        base = runner.plan(n, groups)
        setattr(runner, *switch)
        assert runner.plan(n, groups) != base, f"{switch[0]} changes no step at this layout"
    h2 = runner.h2
    fd = torch.from_numpy(tfi.frames(n, bn_mode)).to(dev)
    feat, records = record_forward(runner, fd, groups)
    feat = feat.cpu().double()
    assert torch.equal(feat, runner.forward(fd, groups).cpu().double())       # recording changes nothing; deterministic
    w_err, w_step = unforced_errors(case, records, trace, h2, groups, dev)
    scale = max(1.0, ref.abs().max().item())
    e2e = (feat - ref).abs().max().item()
    rep = _Report(case)
    if forced:
        forced_checks(rep, records, sd, h2, groups, 1e-5 if h2 else 2e-5)
    ratio, step, what = rep.worst()
    print(f"[{case}] end to end {e2e / scale:.2e} of the largest feature = {e2e / (bar * scale):.3f} of the bar "
          f"(largest per-step error vs trace {w_err:.2e} at {w_step}); forced: largest error / bound {ratio:.3f} at {step} ({what}), "
          f"{len(rep.rows)} checks")
    assert not rep.failed, "\n".join(rep.failed)
    assert torch.isfinite(feat).all() and e2e <= bar * scale, (e2e / scale, w_step)
    return records


def test_f16x2_eight_frames_in_fours(dev):
    """The defaults at the reference's micro-batches: fused stem, Gram pair, nine-tap input BatchNorm, 3-byte block outputs,
    packed clusters with two groups sharing a tile."""
    records = _run(dev, "f16x2 [0,4,8]", [0, 4, 8], f32_split="f16x2")
    forms = {r.st.form for r in records}
    assert {"stem_f16x2", "gram_pair", "gram", "stats", "cluster", "local"} <= forms
    assert any(r.st.packed for r in records) and any(r.st.out == "p8" for r in records)
    assert any(r.st.res == "deferred" for r in records) and any(r.st.inp == "raw" and r.st.form == "stats" for r in records)


def test_f16x2_three_frames_per_frame_groups(dev):
    _run(dev, "f16x2 [0,1,2,3]", [0, 1, 2, 3], f32_split="f16x2")


def test_f16x2_ragged_groups(dev):
    records = _run(dev, "f16x2 [0,4,5]", [0, 4, 5], f32_split="f16x2")
    assert {r.st.form for r in records} == {"split"}


@pytest.mark.parametrize("switch", [("pack_groups", False), ("bn_cluster", False), ("fold_input_bn", False), ("p8_blocks", ()),
                                    ("defer_bn_apply", False), ("defer_res_apply", False), ("fused_stem", False)],
                         ids=lambda s: s[0])
def test_f16x2_one_switch_off(dev, switch):
    _run(dev, f"f16x2 [0,4,8] {switch[0]} off", [0, 4, 8], forced=False, switch=switch, f32_split="f16x2")


@pytest.mark.parametrize("groups", [[0, 4], [0, 1, 2, 3, 4]], ids=["one_group", "per_frame"])
def test_exact_fp32(dev, groups):
    records = _run(dev, f"fp32 {groups}", groups)
    assert {r.st.form for r in records} == {"split"}


@pytest.mark.parametrize("mode", [{}, {"f32_split": "f16x2"}], ids=["fp32", "f16x2"])
def test_folded_running_statistics(dev, mode):
    """bn_mode="folded" with running statistics that differ per layer (dark frames: tfi.frames)."""
    records = _run(dev, f"folded {'f16x2' if mode else 'fp32'} [0,4]", [0, 4], bn_mode="folded", forced=False, **mode)
    assert {r.st.form for r in records} == {"folded"}


@pytest.mark.parametrize("groups", sorted(tfi.F32_SPLIT_BARS), ids=["per_frame", "in_fours"])
def test_fp32_split(dev, groups):
    """AVS_F32_SPLIT end to end, at its measured bar (trunk_f64_inputs.F32_SPLIT_BARS; the host test holds every planted
    mistake 10 of these bars away).  bf16 has no case: see the module docstring."""
    records = _run(dev, f"fp32-split {list(groups)}", list(groups), forced=False, bar=tfi.F32_SPLIT_BARS[groups], f32_split=True)
    assert "stats" in {r.st.form for r in records}


def test_inception_v3_signed_gamma(dev):
    """Inception-v3 (eval-mode BatchNorm folded into the weights) with test_inception_v3_fp32's running statistics and biases
    and BatchNorm weights of both signs with an exact zero, against inception_v3_forward in float64; that test's bar."""
    from avsum_amd.cnn import InceptionV3Runner
    net, frames = tfi.inception_case()
    ref = tfi.inception_f64(net, frames)
    fd = torch.from_numpy(frames).to(dev)
    net = net.to(dev)
    scale = max(1.0, ref.abs().max().item())
    for name, mode in (("fp32", {}), ("f16x2", {"f32_split": "f16x2"})):
        got = InceptionV3Runner(net, torch.float32, **mode).forward(fd).cpu().double()
        err = (got - ref).abs().max().item()
        print(f"[inception {name}] {err / scale:.2e} of the largest feature = {err / (1e-4 * scale):.3f} of the bar")
        assert torch.isfinite(got).all() and err <= 1e-4 * scale, name
