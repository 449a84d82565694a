"""Host side of the per-step trunk tests (test_gpu_trunk_f64.py): the float64 trace is what it claims to be, and the
end-to-end bar of the device tests - the project's trunk bar, 5e-4 of the largest feature - separates a correct trunk
from every planted wiring mistake (trunk_f64_inputs.MISTAKES) at every BatchNorm group layout the device tests use.

Both are CONDITIONS on the inputs, asserted here on the float64 oracle: (a) the fp32 CPU restatement of the trunk lies
within the bar of the float64 features (a correct fp32-class implementation can pass), (b) every planted mistake moves the
features by at least 10 bars.  A layout's error is the largest over its groups, so (b) holds for a layout as soon as it
holds for ONE of its groups against the layout's bar: the mistakes are evaluated on the layouts' common groups only
(frames 0-3 as one group, frame 0 alone) and the printed figures are lower bounds of the layouts' own.

Figures (seed 24; err = max|d| / max(1, max|ref|), the bar is 5e-4; [a:b] = the frames of the probed group):
  fp32 restatement vs float64: batch 1.4e-5 (layouts with a 4-frame group), 7.6e-6 (per-frame layouts); folded 4.0e-7
  planted mistake                                   batch [0:4]          batch [0:1]          folded [0:1]
                                                    err   L2    cos      err   L2    cos      err   L2    cos
  layer3.2: bn1 and bn2 swapped                     0.254 0.143 0.9898   0.097 0.061 0.9981   0.161 0.165 0.9886
  bn2 of layer1.1 and layer1.2 swapped              0.262 0.164 0.9867   0.108 0.064 0.9979   0.058 0.054 0.9995
  bn3 of layer4.1 and layer4.2 swapped              0.297 0.148 0.9891   0.199 0.107 0.9943   0.784 0.738 0.7174
  stem gamma replaced by |gamma|                    0.271 0.160 0.9872   0.109 0.064 0.9980   0.041 0.040 1.0000
  beta of layer2.0.downsample dropped               0.233 0.138 0.9905   0.091 0.060 0.9982   0.009 0.009 1.0000
  one gamma sign flipped in layer4.2.bn3            0.058 0.004 1.0000   0.008 0.000 1.0000   0.536 0.062 0.9981
  one gamma sign flipped in layer1.0.bn1            0.243 0.138 0.9905   0.101 0.059 0.9983   0.011 0.009 1.0000
  layer1.0.conv1+downsample parameters swapped      0.268 0.165 0.9864   0.110 0.062 0.9981   0.041 0.041 0.9992
(L2 = largest per-frame relative L2, cos = smallest per-frame cosine.)  The smallest margin is 16 bars (batch, per-frame
groups: one flipped sign among layer4.2's 2048 outputs).  A single flipped sign in the last BatchNorm moves one feature
of 2048: relative L2 and cosine do not see it, which is why a mode that can only be held to those metrics (bf16) cannot
be given a wiring test by them.
The fp32-split case of the device tests has a measured bar of its own (trunk_f64_inputs.F32_SPLIT_BARS, up to 7.25e-4):
condition (b) is asserted against it as well.
With the container's default BatchNorm parameters the four permutations among them leave the features bit-identical:
the gap these tests close."""
import collections

import pytest
import torch
import torch.nn as nn

import trunk_f64_inputs as tfi
from oracle import cnn as ocnn

# the BatchNorm group layouts of test_gpu_trunk_f64.py (frame offsets; the frames are tfi.frames(n), a common prefix)
LAYOUTS = ([0, 4, 8], [0, 1, 2, 3], [0, 4, 5], [0, 4], [0, 1, 2, 3, 4])
assert all(list(k) in LAYOUTS for k in tfi.F32_SPLIT_BARS)
# the groups every planted mistake is evaluated on, and the layouts each of them speaks for
PROBES = {(0, 4): ([0, 4, 8], [0, 4, 5], [0, 4]), (0, 1): ([0, 1, 2, 3], [0, 1, 2, 3, 4])}


def _metrics(got, ref):
    """(max error relative to the largest feature, largest per-frame relative L2, smallest per-frame cosine)."""
    got, ref = got.double(), ref.double()
    l2 = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1).min().item()
    return tfi.rel_err(got, ref), l2, cos


def test_fp32_trace_is_the_forward_bit_for_bit():
    sd = tfi.state_dict(tfi.make_trunk(running=True), torch.float32)
    x = tfi.preprocess(tfi.frames(2), torch.float32)
    names = None
    for mode in ("batch", "folded"):
        with torch.no_grad():
            feat, tr = ocnn.resnet50_trunk_trace(sd, x, mode)
            ref = ocnn.resnet50_trunk_forward(sd, x, mode)
        assert feat.dtype == torch.float32 and torch.equal(feat, ref), mode
        names = list(tr)
    # torchvision's names, in forward order: 53 convolutions (raw + finished), the pooled stem map, 16 block outputs
    assert names[:3] == ["conv1.raw", "conv1", "maxpool"] and names[3:5] == ["layer1.0.conv1.raw", "layer1.0.conv1"]
    assert names[-1] == "layer4.2" and len(names) == 2 * 53 + 1 + 16
    assert "layer2.0.downsample" in names and "layer2.1.downsample" not in names
    assert tr["layer4.2"].shape == (2, 2048, 7, 7) and tr["maxpool"].shape == (2, 64, 56, 56)
    assert (tr["layer3.1.conv2"] >= 0).all() and (tr["layer3.1.conv3"] < 0).any() and (tr["layer2.0.downsample"] < 0).any()


def test_float64_trace_of_one_block_against_torch_modules():
    """layer2.0 (stride 2, a downsample) of the float64 trace against nn.Conv2d / nn.BatchNorm2d(train).double() composed by
    hand from the same state dict, on small maps (the trunk is fully convolutional)."""
    sd = tfi.state_dict(tfi.make_trunk())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 3, 96, 96, generator=g, dtype=torch.float64) * 50
    with torch.no_grad():
        feat, tr = ocnn.resnet50_trunk_trace(sd, x)
    assert feat.dtype == torch.float64 and all(v.dtype == torch.float64 for v in tr.values())

    def conv(key, cin, cout, k, s, p):
        m = nn.Conv2d(cin, cout, k, s, p, bias=False).double()
        m.weight.data.copy_(sd[key])
        return m

    def bn(prefix, c):
        m = nn.BatchNorm2d(c).double().train()
        m.weight.data.copy_(sd[prefix + "weight"])
        m.bias.data.copy_(sd[prefix + "bias"])
        return m

    xin = tr["layer1.2"]
    with torch.no_grad():
        r1 = conv("5.0.conv1.weight", 256, 128, 1, 1, 0)(xin)
        t1 = torch.relu(bn("5.0.bn1.", 128)(r1))
        r2 = conv("5.0.conv2.weight", 128, 128, 3, 2, 1)(t1)
        t2 = torch.relu(bn("5.0.bn2.", 128)(r2))
        t3 = bn("5.0.bn3.", 512)(conv("5.0.conv3.weight", 128, 512, 1, 1, 0)(t2))
        td = bn("5.0.downsample.1.", 512)(conv("5.0.downsample.0.weight", 256, 512, 1, 2, 0)(xin))
        out = torch.relu(t3 + td)
    for name, ref in (("layer2.0.conv1.raw", r1), ("layer2.0.conv1", t1), ("layer2.0.conv2.raw", r2), ("layer2.0.conv2", t2),
                      ("layer2.0.conv3", t3), ("layer2.0.downsample", td), ("layer2.0", out)):
        assert tr[name].shape == ref.shape, name
        assert (tr[name] - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), name
    assert (sd["5.0.bn1.weight"] < 0).any() and sd["5.0.bn1.weight"][0] == 0 and (tr["layer2.0.conv1"][:, 0] ==
                                                                                torch.relu(sd["5.0.bn1.bias"][0])).all()


def test_randomize_bn_rule():
    trunk = tfi.make_trunk(running=True)
    seen = set()
    for m in trunk.modules():
        if isinstance(m, nn.BatchNorm2d):
            w = m.weight.detach()
            assert w[0] == 0 and ((w[1:].abs() >= 0.5) & (w[1:].abs() <= 1.5)).all()
            assert (m.running_var >= 0.5).all() and (m.running_var <= 1.5).all() and m.running_mean.abs().max() > 0
            seen.add(tuple(w[:8].tolist()))
    assert len(seen) == 53                                           # every BatchNorm its own parameters
    allw = torch.cat([m.weight.detach()[1:] for m in trunk.modules() if isinstance(m, nn.BatchNorm2d)])
    assert 0.13 < (allw < 0).float().mean().item() < 0.17
    plain = tfi.make_trunk(randomized=False)
    assert all(torch.equal(a, b) for a, b in zip((p for n, p in trunk.named_parameters() if p.dim() == 4),
                                                 (p for n, p in plain.named_parameters() if p.dim() == 4)))


@pytest.mark.parametrize("bn_mode", ["batch", "folded"])
def test_bar_passes_fp32_and_catches_every_planted_mistake(bn_mode):
    running = bn_mode == "folded"
    sd64 = tfi._sd64(tfi.SEED, running)
    sd32 = tfi.state_dict(tfi.make_trunk(running=running), torch.float32)
    x = tfi.preprocess(tfi.frames(tfi.MAX_FRAMES, bn_mode))
    # (a) the fp32 restatement within the bar, per layout
    scale = {}
    for groups in LAYOUTS:
        ref, _ = tfi.trace(tfi.SEED, groups, bn_mode)
        n = groups[-1]
        f32 = tfi.features(sd32, x[:n].float(), groups if bn_mode == "batch" else None, bn_mode)
        err = tfi.rel_err(f32, ref)
        scale[tuple(groups)] = max(1.0, ref.abs().max().item())
        print(f"\n[{bn_mode}] groups {groups}: fp32 restatement vs float64 {err:.2e} of the largest feature ({scale[tuple(groups)]:.3f})")
        assert err <= tfi.TRUNK_BAR, groups
    # (b) every planted mistake at least 10 bars away, per layout (through one of its groups)
    for (a, b), layouts in PROBES.items():
        if bn_mode == "folded" and (a, b) != (0, 1):
            continue      # folded BatchNorm is per frame: frame 0 is part of every layout
        ref, _ = tfi.trace(tfi.SEED, [0, b], bn_mode)
        ref = ref[a:b]
        for name, plant, _ in tfi.MISTAKES:
            got = tfi.features(plant(sd64), x[a:b], [0, b - a], bn_mode)
            err, l2, cos = _metrics(got, ref)
            print(f"[{bn_mode}] frames [{a}:{b}] {name}: max err {err:.3f}, relative L2 {l2:.3f}, cosine {cos:.4f}")
            abs_err = (got - ref).abs().max().item()
            for groups in (LAYOUTS if bn_mode == "folded" else layouts):
                assert abs_err >= 10.0 * tfi.TRUNK_BAR * scale[tuple(groups)], (name, groups)
                if bn_mode == "batch" and tuple(groups) in tfi.F32_SPLIT_BARS:   # the measured bar of the fp32-split case too
                    assert abs_err >= 10.0 * tfi.F32_SPLIT_BARS[tuple(groups)] * scale[tuple(groups)], (name, groups)


def test_default_parameters_hide_the_permutations():
    """The gap: with the container's default BatchNorm parameters (what every other trunk test runs) a permutation of
    whole parameter sets changes no bit of the features; with randomize_bn each of them is visible (the test above)."""
    sd = tfi.state_dict(tfi.make_trunk(randomized=False), torch.float32)
    x = tfi.preprocess(tfi.frames(1), torch.float32)
    ref = tfi.features(sd, x, [0, 1])
    swaps = [(name, plant) for name, plant, swap in tfi.MISTAKES if swap]
    assert len(swaps) == 4
    for name, plant in swaps:
        assert torch.equal(tfi.features(plant(collections.OrderedDict(sd)), x, [0, 1]), ref), name


def test_inception_signed_gamma_fp32_within_the_bar():
    """The device test's Inception inputs (test_inception_v3_fp32's randomisation + randomize_bn's signed weights): the fp32
    CPU restatement must lie within that test's bar, 1e-4 of the largest feature, of the float64 result."""
    net, frames = tfi.inception_case()
    x = torch.cat([ocnn.preprocess_inception(f) for f in frames])
    with torch.no_grad():
        ref = tfi.inception_f64(net, frames)
        f32 = ocnn.inception_v3_forward(net.state_dict(), x)
    err = tfi.rel_err(f32, ref)
    print(f"\nInception-v3, signed gamma: fp32 restatement vs float64 {err:.2e} of the largest feature ({ref.abs().max().item():.3f})")
    assert torch.isfinite(ref).all() and ref.abs().max().item() > 1e-2 and err <= 1e-4
