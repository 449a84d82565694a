"""AVS_F16X2 input affine of the nine-tap convolution + statistics form (avs_conv2d_nhwc_bnstats_xin): the BatchNorm + ReLU
of the layer before applied while the kernel stages its input, instead of an apply pass over that input in HBM.

The arithmetic per element is the apply pass's (join, multiply, add, ReLU, split), only run in another kernel, so every
comparison here is bit for bit: outputs, folded statistics and the trunk's features.  The nine-tap form runs on the
256-row tiles, which the library takes for layers of at least 2048 such tiles: the shapes below are sized for that."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from avsum_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(dev, frames, hw, cin, cout, fpg, seed):
    """Raw input (f16x2), packed 3x3 weights, BatchNorm parameters of the output, an input affine [groups, cin]."""
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = frames * hw * hw
    rpg = fpg * hw * hw
    groups = (rows + rpg - 1) // rpg
    x = ops.f16x2_pack(torch.randn(frames, hw, hw, cin, device=dev, generator=g) * 2.0 + 0.3)
    w = torch.randn(cout, 9 * cin, device=dev, generator=g) * (2.0 / (9 * cin)) ** 0.5
    wk = ops.weights_kstep32(ops.f16x2_pack(w))
    # both signs of the input scale (a negative gamma) and of the shift; the output BatchNorm's gamma too
    in_scale = (torch.rand(groups, cin, device=dev, generator=g) + 0.25) * torch.where(
        torch.rand(groups, cin, device=dev, generator=g) < 0.3, -1.0, 1.0)
    in_shift = torch.randn(groups, cin, device=dev, generator=g) * 0.5
    gamma = (torch.rand(cout, device=dev, generator=g) + 0.5) * torch.where(
        torch.rand(cout, device=dev, generator=g) < 0.3, -1.0, 1.0)
    beta = torch.randn(cout, device=dev, generator=g)
    return x, wk, rpg, in_scale.contiguous(), in_shift.contiguous(), gamma.contiguous(), beta.contiguous()


def _conv(dev, x, wk, frames, hw, cin, cout, rpg, gamma, beta, x_affine=None):
    ops = _ops()
    code = ops.dtype_code(torch.float32, "f16x2")
    geom = (frames, hw, hw, cin, 3, 3, 1, 1, 1, 1, hw, hw, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    y = torch.full((frames, hw, hw, cout), float("nan"), device=dev)
    aff = ops.conv2d_raw(code, *geom, x, *xs, wk, wk.stride(0), y, cout, bnstats=(rpg, gamma, beta, 1e-5), w_layout=1,
                         x_affine=x_affine)
    return y, aff


# (frames, map, cin = cout): enough rows for 2048 256-row tiles - layer 1's 64-channel 3x3 at 56 x 56, layer 2's
# 128-channel one at 28 x 28
SHAPES = [(168, 56, 64), (672, 28, 128)]


@pytest.mark.parametrize("shape", SHAPES, ids=["c64", "c128"])
@pytest.mark.parametrize("fpg", [1, 2, 3, 4])
def test_nine_tap_input_affine_equals_apply_then_conv(dev, shape, fpg):
    """avs_bn_apply (+ ReLU, in place) then the nine-tap convolution + statistics == the input-affine form on the raw
    input: the same output bits, the same folded (scale, shift); the raw input is left as it was."""
    ops = _ops()
    frames, hw, cin = shape
    cout = cin
    x, wk, rpg, isc, isf, gamma, beta = _case(dev, frames, hw, cin, cout, fpg, 11 * fpg + cin)
    x_raw = x.clone()
    y, aff = _conv(dev, x, wk, frames, hw, cin, cout, rpg, gamma, beta, x_affine=(isc, isf, True))
    assert aff is not None, "the nine-tap form declined a shape it is built for"
    assert torch.equal(_bits(x), _bits(x_raw))
    rows = torch.arange(0, frames // fpg + 1, dtype=torch.int64, device=dev) * rpg
    x2d = x.view(-1, cin)
    ops.bn_apply(x2d, isc, isf, rows, rpg, None, ops.ACT_RELU, x2d, code=ops.dtype_code(torch.float32, "f16x2"))
    y_ref, aff_ref = _conv(dev, x, wk, frames, hw, cin, cout, rpg, gamma, beta)
    assert torch.equal(_bits(y), _bits(y_ref))
    assert torch.equal(_bits(aff[0]), _bits(aff_ref[0])) and torch.equal(_bits(aff[1]), _bits(aff_ref[1]))


def test_nine_tap_input_affine_without_relu(dev):
    """in_relu = 0: the affine alone (the apply pass with ACT_NONE)."""
    ops = _ops()
    frames, hw, cin = SHAPES[0]
    x, wk, rpg, isc, isf, gamma, beta = _case(dev, frames, hw, cin, cin, 4, 5)
    y, aff = _conv(dev, x, wk, frames, hw, cin, cin, rpg, gamma, beta, x_affine=(isc, isf, False))
    assert aff is not None
    rows = torch.arange(0, frames // 4 + 1, dtype=torch.int64, device=dev) * rpg
    x2d = x.view(-1, cin)
    ops.bn_apply(x2d, isc, isf, rows, rpg, None, ops.ACT_NONE, x2d, code=ops.dtype_code(torch.float32, "f16x2"))
    y_ref, aff_ref = _conv(dev, x, wk, frames, hw, cin, cin, rpg, gamma, beta)
    assert torch.equal(_bits(y), _bits(y_ref))
    assert torch.equal(_bits(aff[0]), _bits(aff_ref[0])) and torch.equal(_bits(aff[1]), _bits(aff_ref[1]))


def test_input_affine_declines_other_shapes(dev):
    """Shapes that do not take the nine-tap form (too few rows for the 256-row tiles, a stride of 2) are declined
    before anything is launched: the output stays untouched."""
    ops = _ops()
    code = ops.dtype_code(torch.float32, "f16x2")
    x, wk, rpg, isc, isf, gamma, beta = _case(dev, 8, 56, 64, 64, 4, 3)
    y, aff = _conv(dev, x, wk, 8, 56, 64, 64, rpg, gamma, beta, x_affine=(isc, isf, True))
    assert aff is None and torch.isnan(y).all()
    geom = (8, 56, 56, 64, 3, 3, 2, 2, 1, 1, 28, 28, 64)
    y2 = torch.full((8, 28, 28, 64), float("nan"), device=dev)
    aff = ops.conv2d_raw(code, *geom, x, 56 * 56 * 64, 56 * 64, 64, wk, wk.stride(0), y2, 64,
                         bnstats=(4 * 784, gamma, beta, 1e-5), w_layout=1, x_affine=(isc[:2].contiguous(), isf[:2].contiguous(), True))
    assert aff is None and torch.isnan(y2).all()


def _frames(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


@pytest.mark.parametrize("groups", ["gf4", "gf1", "gf4_tail"])
def test_trunk_fold_input_bn_on_off_equal(dev, groups, monkeypatch):
    """The whole AVS_F16X2 trunk with fold_input_bn on and off: equal features.  168 frames fill layer 1's 3x3 layers
    with 256-row tiles (its conv1 -> conv2 pairs take the input affine); layer 2's fall back to the apply pass at this
    size.  A shorter tail group (not uniform) takes the unfused sequence either way."""
    from avsum_amd import ops
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(31)
    trunk = resnet50_trunk().to(dev)
    n = 168 if groups != "gf4_tail" else 166
    gf = [0] + list(range(4 if groups != "gf1" else 1, n, 4 if groups != "gf1" else 1)) + [n]
    fd = torch.from_numpy(_frames(n, 7)).to(dev)
    taken = []
    raw = ops.conv2d_raw

    def spy(*a, **k):
        r = raw(*a, **k)
        if k.get("x_affine") is not None:
            taken.append(r is not None)
        return r

    monkeypatch.setattr(ops, "conv2d_raw", spy)
    r = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2")
    on = r.forward(fd, gf).cpu()
    assert torch.equal(on, r.forward(fd, gf).cpu())
    if groups != "gf4_tail":
        assert sum(taken) == 4, taken   # layer 1 blocks 1-2, twice
    else:
        assert not taken
    r.fold_input_bn = False
    taken.clear()
    off = r.forward(fd, gf).cpu()
    assert not taken
    assert torch.isfinite(on).all()
    assert torch.equal(_bits(on), _bits(off))


def test_trunk_fold_input_bn_ragged_groups(dev):
    """Ragged groups (4 + 1 frames) still run with the switch on, equal to the switch off, and reproducibly."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(21)
    trunk = resnet50_trunk().to(dev)
    fd = torch.from_numpy(_frames(5, 1)).to(dev)
    r = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2")
    a = r.forward(fd, [0, 4, 5]).cpu()
    assert torch.equal(a, r.forward(fd, [0, 4, 5]).cpu())
    r.fold_input_bn = False
    assert torch.equal(_bits(a), _bits(r.forward(fd, [0, 4, 5]).cpu()))
