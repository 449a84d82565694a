"""Inputs and float64 references of the per-step ResNet-50 trunk tests (test_trunk_f64_host.py on the host,
test_gpu_trunk_f64.py on the device).  torch-CPU only: both files build the same seeded trunk and frames from here.

Every other trunk-level test takes its weights from ``resnet50_trunk()``, whose BatchNorm weights are all 1 and biases
all 0: a step of the runner that is handed another layer's (gamma, beta), a stacked parameter vector in the wrong order
or no beta at all then gives the same bits.  ``randomize_bn`` gives every BatchNorm its own parameters, of both signs and
with one channel exactly 0 (what pretrained weights look like to the code: per-layer values, some negative, some near
0); ``MISTAKES`` plants the wiring errors, as functions from one state dict to another, that the bars of the device
tests have to notice (checked on the host, on the float64 oracle).

The float64 trace of a layout is the concatenation of its groups' traces (a BatchNorm group never sees another group),
cached per (seed, group, bn_mode), so that layouts that share a group share its trace.  The features are kept in float64; the per-step
intermediates are kept in fp32 (2^-24 relative: they only serve the printed per-step diagnostics, figures of 1e-6 and
more) - a float64 trace of 8 frames is 1.7 GB."""
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import cnn as ocnn
from test_gpu_f16x2 import emu_pack, emu_unpack  # noqa: F401  (the AVS_F16X2 format restated on the CPU, shared)

SEED = 24            # torch.manual_seed of the convolution weights (test_resnet50_trunk_f16x2's)
FRAME_SEED = 5
MAX_FRAMES = 8
TRUNK_BAR = 5e-4     # the project's trunk bar: |features - reference| <= 5e-4 * max(1, max|reference|)
# AVS_F32_SPLIT (products on the bf16 matrix cores, ~2^-15 each) has no bar of the project's with these parameters: 3 times
# the error measured on one MI355X against the float64 trace (2.416e-4 at 8 frames in fours, 1.409e-4 at 4 per-frame
# groups, the same bits run to run), the factor for other summation orders.  Same scale as TRUNK_BAR, per layout.
F32_SPLIT_BARS = {(0, 4, 8): 7.25e-4, (0, 1, 2, 3, 4): 4.23e-4}


# --------------------------------------------------------------------------- the trunk and its inputs
def randomize_bn(trunk, seed, running=False):
    """Every BatchNorm of ``trunk`` (any module tree) in place: weight = +-U(0.5, 1.5), negative with probability 0.15,
    channel 0 exactly 0; bias = N(0, 0.5); running=True: running_mean = N(0, 0.1), running_var = U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in trunk.modules():
            if not isinstance(m, torch.nn.BatchNorm2d):
                continue
            c = m.num_features
            mag = torch.rand(c, generator=g) + 0.5
            sign = torch.where(torch.rand(c, generator=g) < 0.15, -1.0, 1.0)
            gamma = mag * sign
            gamma[0] = 0.0
            m.weight.copy_(gamma)
            m.bias.copy_(torch.randn(c, generator=g) * 0.5)
            if running:
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return trunk


def make_trunk(seed=SEED, randomized=True, running=False):
    """The seeded container on the CPU: resnet50_trunk()'s convolution weights, BatchNorm by randomize_bn (randomized=False:
    the container's defaults, weight 1 / bias 0 / running statistics 0 and 1)."""
    from avsum_amd.cnn import resnet50_trunk
    torch.manual_seed(seed)
    trunk = resnet50_trunk()
    return randomize_bn(trunk, seed, running) if randomized else trunk


def frames(n, bn_mode="batch"):
    """The first n of the 8 seeded uint8 frames [n,224,224,3] (a prefix: layouts of different length share frames).
    batch: the full range 0..255.  folded: their lowest bit, 0 / 1 (a dark frame; normalised without / 255 that is
    -2.1 / +2.2, the range of a standardised picture).  Running statistics that are not the activations' own - any
    synthetic ones - do not normalise: this trunk then gains a factor of ~2000 from the stem to layer 4 (measured on the
    float64 oracle), which full-range frames (normalised values to 1100) carry to 2e6, past the 65504 at which the
    AVS_F16X2 storage saturates by design (test_pack_unpack_bit_exact).  Dark frames keep every activation below 2e4."""
    assert 0 < n <= MAX_FRAMES
    fr = np.random.default_rng(FRAME_SEED).integers(0, 256, (MAX_FRAMES, 224, 224, 3), dtype=np.uint8)[:n]
    return fr & 1 if bn_mode == "folded" else fr


def preprocess(fr, dtype=torch.float64):
    """(x - mean) / std without / 255 in fp32, as the reference rounds it (features/extractors.py:133-139) -> [n,3,224,224]."""
    return torch.cat([ocnn.preprocess_frame(f) for f in fr]).to(dtype)


def state_dict(trunk, dtype=torch.float64):
    return OrderedDict((k, v.detach().cpu().to(dtype).clone() if v.is_floating_point() else v.detach().cpu().clone())
                       for k, v in trunk.state_dict().items())


def group_bounds(n, groups):
    groups = list(range(n + 1)) if groups is None else [int(v) for v in groups]
    assert groups[0] == 0 and groups[-1] == n
    return list(zip(groups[:-1], groups[1:]))


def features(sd, x, groups, bn_mode="batch"):
    """resnet50_trunk_forward group by group, in the dtype of sd and x."""
    with torch.no_grad():
        return torch.cat([ocnn.resnet50_trunk_forward(sd, x[a:b], bn_mode) for a, b in group_bounds(x.shape[0], groups)])


def rel_err(got, ref):
    """max|got - ref| relative to max(1, max|ref|): the scale of the trunk bar."""
    return (got.double() - ref.double()).abs().max().item() / max(1.0, ref.abs().max().item())


# --------------------------------------------------------------------------- cached float64 traces
@functools.lru_cache(maxsize=None)
def _sd64(seed, running):
    return state_dict(make_trunk(seed, True, running))


@functools.lru_cache(maxsize=None)
def _group_trace(seed, a, b, bn_mode, running):
    with torch.no_grad():
        feat, tr = ocnn.resnet50_trunk_trace(_sd64(seed, running), preprocess(frames(b, bn_mode)[a:b]), bn_mode)
    return feat, OrderedDict((k, v.float()) for k, v in tr.items() if not k.endswith(".raw"))


def trace(seed, groups, bn_mode="batch"):
    """(float64 features [n,2048], {torchvision name: finished output, NCHW fp32}) of the randomised trunk on
    frames(n, bn_mode) in BatchNorm groups ``groups`` (frame offsets); folded: with randomised running statistics.
    The groups' traces are cached per process (one copy, whatever the layouts that share them)."""
    groups = [int(v) for v in groups]
    running = bn_mode == "folded"
    # (folded BatchNorm is per frame whatever the groups: per-frame pieces are shared by every layout)
    bounds = group_bounds(groups[-1], groups if bn_mode == "batch" else None)
    parts = [_group_trace(seed, a, b, bn_mode, running) for a, b in bounds]
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p[0] for p in parts]), OrderedDict((k, torch.cat([p[1][k] for p in parts])) for k in parts[0][1])


# --------------------------------------------------------------------------- planted wiring mistakes
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def _swap_bn(a, b):
    def f(sd):
        sd = OrderedDict(sd)
        for k in _BN_KEYS:
            sd[a + k], sd[b + k] = sd[b + k], sd[a + k]
        return sd
    return f


def _edit(key, fn):
    def f(sd):
        sd = OrderedDict(sd)
        sd[key] = fn(sd[key].clone())
        return sd
    return f


def _flip(key, channel):
    def fn(t):
        assert t[channel] != 0
        t[channel] = -t[channel]
        return t
    return _edit(key, fn)


def _pair_swapped(sd):
    """layer1.0's shared Gram step takes conv1's and the downsample's BatchNorm parameters stacked [bn1 | downsample]
    next to the weights stacked the same way: here the parameters are stacked the other way round."""
    sd = OrderedDict(sd)
    for k in _BN_KEYS:
        cat = torch.cat([sd["4.0.downsample.1." + k], sd["4.0.bn1." + k]])
        n1 = sd["4.0.bn1." + k].numel()
        sd["4.0.bn1." + k], sd["4.0.downsample.1." + k] = cat[:n1].clone(), cat[n1:].clone()
    return sd


# (name, state dict -> state dict, "swap": a permutation of whole parameter sets, invisible with default parameters)
MISTAKES = (
    ("layer3.2: bn1 and bn2 swapped", _swap_bn("6.2.bn1.", "6.2.bn2."), True),
    ("bn2 of layer1.1 and layer1.2 swapped", _swap_bn("4.1.bn2.", "4.2.bn2."), True),
    ("bn3 of layer4.1 and layer4.2 swapped", _swap_bn("7.1.bn3.", "7.2.bn3."), True),
    ("stem gamma replaced by |gamma|", _edit("1.weight", torch.abs), False),
    ("beta of layer2.0.downsample dropped", _edit("5.0.downsample.1.bias", torch.zeros_like), False),
    ("one gamma sign flipped in layer4.2.bn3", _flip("7.2.bn3.weight", 5), False),
    ("one gamma sign flipped in layer1.0.bn1", _flip("4.0.bn1.weight", 5), False),
    ("layer1.0.conv1+downsample: stacked parameters in swapped order", _pair_swapped, True),
)


# --------------------------------------------------------------------------- Inception-v3
def inception_case():
    """(Inception3 on the CPU, uint8 frames [2,299,299,3]): test_inception_v3_fp32's randomisation (running statistics, bias)
    and randomize_bn's signed weights (zero channel included) on top."""
    from avsum_amd.cnn import Inception3
    torch.manual_seed(23)
    net = Inception3()
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                gamma = (torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.15, -1.0, 1.0)
                gamma[0] = 0.0
                m.weight.copy_(gamma)
    return net, np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)


def inception_f64(net, fr):
    x = torch.cat([ocnn.preprocess_inception(f) for f in fr]).double()
    with torch.no_grad():
        return ocnn.inception_v3_forward(state_dict(net), x)
