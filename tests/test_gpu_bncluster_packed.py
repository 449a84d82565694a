"""The packed form of the clustered tile-local BatchNorm (avs_conv2d_nhwc_bncluster with AVS_CLUSTER_PACKED): tiles of 224
consecutive rows instead of one 196-row tile per 14x14 map, so a 4-frame group (784 rows) is 3.5 tiles, two groups are 7 full
tiles and the tile in the middle holds rows of both groups, the boundary at its row 112.

Same construction and bar as test_gpu_f16x2.py::test_conv_bncluster_f16x2: float64 arithmetic on the unpacked operands,
<= TOL * amp; the output pre-filled with NaN and finite afterwards; three runs bit-identical; no exchange wait ran out; and
agreement with the unpacked clustered form to 2 * TOL * amp (the two sum a group's statistics in different fixed orders)."""
import numpy as np
import pytest
import torch

from test_gpu_f16x2 import TOL, _bn_reference, _conv_operands, _conv_ref, emu_pack, emu_unpack

pytestmark = pytest.mark.gpu


def _ops():
    from avsum_amd import ops
    return ops


_PACKED_CASES = [   # frames, hw (in), cin, cout, k, stride, frames per group, residual, relu, offset
    (8, 14, 64, 256, 1, 1, 4, True, True, 0.3),       # 2 groups = 7 tiles, the shared tile, two column tiles
    (8, 14, 64, 256, 1, 1, 4, True, True, 40.0),      # mean >> spread: the centred statistics across segments
    (12, 14, 64, 128, 3, 1, 4, False, True, 0.3),     # 3 groups = 10.5 tiles: the last tile half used; taps cross frame borders inside a tile
    (8, 28, 64, 128, 1, 2, 4, False, False, 0.3),     # the strided 1x1 down to 14x14, no ReLU
    (8, 28, 64, 128, 1, 1, 4, False, True, 0.3),      # 28x28 maps: groups of 3136 rows = 14 full tiles, no shared tile
    (320, 14, 64, 256, 1, 1, 4, False, True, 0.3),    # 280 row tiles x 2 = 560 workgroups > the 512 resident at once: the dispatch-order mapping
]


@pytest.mark.parametrize("cfg", _PACKED_CASES)
def test_conv_bncluster_packed_f16x2(dev, cfg):
    ops = _ops()
    frames, hw, cin, cout, k, s, gf, with_res, relu, offset = cfg
    pad = k // 2
    xp, wp, xv, wv = _conv_operands(frames, hw, hw, cin, cout, k, k, sum(cfg[:6]), offset)
    raw = _conv_ref(xv, wv, s, pad)
    ho = raw.shape[1]
    rpg = gf * ho * ho
    cluster = rpg // 196          # what the unpacked form calls the group: tiles of 196 rows
    raw = raw.reshape(-1, cout)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    resp = emu_pack(torch.randn(raw.shape[0], cout, generator=g)) if with_res else None
    ref = _bn_reference(raw, rpg, gamma, beta, emu_unpack(resp).double() if with_res else None, relu)
    geom = (frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    code = ops.dtype_code(torch.float32, "f16x2")
    assert ops.conv_bncluster_ok(code, *geom, *xs, wp.shape[1], cout, rpg, cluster, packed=True)
    xd, wd = xp.to(dev), wp.to(dev)
    gd, bd, rd = gamma.to(dev), beta.to(dev), resp.to(dev) if with_res else None
    amp = max(1.0, (1.0 / torch.sqrt(raw.reshape(-1, rpg, cout).var(1, unbiased=False) + 1e-5)).max().item() *
              raw.abs().max().item())

    def run(packed):
        y = torch.full((frames, ho, ho, cout), float("nan"), device=dev)
        ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                       bnlocal=(rpg, gd, bd, 1e-5, rd), cluster=cluster, packed=packed)
        return y

    outs = [run(True) for _ in range(3)]
    assert ops.cluster_exchange_errors(dev) == 0
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    got = ops.f16x2_unpack(outs[0]).cpu().double().view(-1, cout)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"\npacked vs float64: {err:.3e} (bar {TOL * amp:.3e})")
    assert err <= TOL * amp
    unpacked = ops.f16x2_unpack(run(False)).cpu().double().view(-1, cout)
    assert ops.cluster_exchange_errors(dev) == 0
    d = (unpacked - got).abs().max().item()
    print(f"packed vs unpacked: {d:.3e} (bar {2 * TOL * amp:.3e})")
    assert d <= 2 * TOL * amp


def test_resnet50_trunk_f16x2_packed_groups(dev):
    """The whole trunk, f16x2, 8 frames in groups of 4, with ResNet50Runner.pack_groups on and off: each run deterministic
    and within the f16x2 mode's bar of the fp32 GPU mode; the plan says which form ran."""
    ops = _ops()
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(24)
    trunk = resnet50_trunk().to(dev)
    fd = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (8, 224, 224, 3), dtype=np.uint8)).to(dev)
    groups = [0, 4, 8]
    g32 = ResNet50Runner(trunk, torch.float32, "batch").forward(fd, groups).cpu()
    scale = max(1.0, g32.abs().max().item())
    r = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2")
    assert r.pack_groups is True
    for pack in (True, False):
        r.pack_groups = pack
        cl = [st for st in r.plan(8, groups) if st.form == "cluster"]
        assert len(cl) == 20 and all(st.packed == pack for st in cl)
        got = r.forward(fd, groups).cpu()
        assert torch.equal(got, r.forward(fd, groups).cpu())
        assert ops.cluster_exchange_errors(dev) == 0
        err = (got - g32).abs().max().item()
        print(f"\n[pack_groups {pack}] f16x2 vs GPU fp32 {err / scale:.2e} (relative to the largest feature)")
        assert torch.isfinite(got).all() and err < 5e-4 * scale
