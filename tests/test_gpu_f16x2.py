"""AVS_F16X2 - the fast parity-grade arithmetic of the CNN trunk (values stored as fp16 hi | lo runs, products as
three fp16 MFMAs, outputs split once where they are produced, centred two-round BatchNorm statistics): kernel-level
parity against float64 arithmetic on the same operands, through the C-ABI.

The format is restated here on the CPU (``emu_pack`` / ``emu_unpack``: hi = fp16(x), lo = fp16(x - hi), runs of 8) so
that the GPU conversion kernels are checked bit for bit and every other test builds its operands independently of
them.  Tolerances: a product drops lo*lo (2^-22 relative) and the sum is an fp32 MFMA accumulation, so results sit
within ~1e-6 of the float64 value relative to the output scale (asserted at 1e-5; the exact-fp32 mode's own bar in
test_gpu_kernels.py is 2e-5, AVS_F32_SPLIT's 1e-4, bf16's 1.2e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f16x2_format import emu_pack, emu_unpack  # noqa: F401  (the format restated on the CPU; other modules import it from here)

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _ops():
    from avsum_amd import ops
    return ops


def test_pack_unpack_bit_exact(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g) * s for s in (1.0, 1e-3, 1e-6, 300.0, 7e4)] +
                  [torch.tensor([0.0, -0.0, 65504.0, -65504.0, 1e9, -1e9, 6e-8, 2.0 ** -24])]).reshape(-1, 8)
    ref = emu_pack(x)
    got = ops.f16x2_pack(x.to(dev)).cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    back = ops.f16x2_unpack(got.to(dev)).cpu()
    assert torch.equal(back, emu_unpack(ref))
    inside = x.abs() <= 65504
    # 22 significant bits, absolute floor from the fp16 denormals (2^-25), saturation beyond 65504
    assert ((back - x).abs()[inside] <= x.abs()[inside] * 2.0 ** -21 + 2.0 ** -25).all()
    assert (back[~inside].abs() <= 65504 + 32).all()


def _conv_operands(n, h, w, cin, cout, kh, kw, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g) + offset
    wt = torch.randn(cout, kh, kw, cin, generator=g) / (cin * kh * kw) ** 0.5
    xp, wp = emu_pack(x), emu_pack(wt.reshape(cout, -1))
    xv, wv = emu_unpack(xp).double(), emu_unpack(wp).double().reshape(cout, kh, kw, cin)
    return xp, wp, xv, wv


def _conv_ref(xv, wv, stride, pad):
    return F.conv2d(xv.permute(0, 3, 1, 2), wv.permute(0, 3, 1, 2), None, stride, pad).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("cfg", [
    (2, 14, 14, 64, 64, 1, 1, 1, 0), (2, 14, 14, 64, 96, 3, 3, 1, 1), (3, 15, 15, 32, 48, 3, 3, 2, 1),
    (2, 16, 16, 128, 256, 1, 1, 2, 0), (1, 17, 17, 128, 192, 1, 7, 1, (0, 3)), (2, 12, 12, 48, 64, 5, 5, 1, 2),
    (2, 9, 9, 80, 192, 3, 3, 1, 0), (1, 35, 35, 288, 384, 3, 3, 2, 0), (2, 28, 28, 16, 32, 1, 1, 1, 0),
    (3, 9, 9, 8, 24, 3, 3, 1, 1), (40, 14, 14, 256, 256, 3, 3, 1, 1), (2, 8, 8, 1024, 136, 1, 1, 1, 0),
])
@pytest.mark.parametrize("tall", [0, 2])
def test_conv2d_f16x2(dev, cfg, tall):
    """Plain convolution (both weight layouts; the library's own tile choice and the 256-row tiles forced on per call:
    avs_conv_desc.variant = AVS_TILE_256)."""
    ops = _ops()
    n, h, w, cin, cout, kh, kw, stride, pad = cfg
    xp, wp, xv, wv = _conv_operands(n, h, w, cin, cout, kh, kw, h * 13 + cin)
    ref = _conv_ref(xv, wv, stride, pad)
    ho, wo = ref.shape[1], ref.shape[2]
    scale = max(1.0, ref.abs().max().item())
    outs = []
    for layout in (0, 1):
        if layout == 1 and (kh * kw * cin) % 16:
            continue
        wd = wp.to(dev)
        wsel = ops.weights_kstep32(wd) if layout else wd
        out = torch.empty((n, ho, wo, cout), device=dev)
        ops.conv2d(xp.to(dev), wsel, kh, kw, stride, pad, out, split="f16x2", w_layout=layout, variant=tall)
        outs.append(out)
        got = ops.f16x2_unpack(out).cpu().double()
        assert (got - ref).abs().max().item() <= TOL * scale
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))   # same products, same order


def test_conv2d_f16x2_stem_geometry(dev):
    """The ResNet stem as the trunk runs it: uint8 frames -> avs_frames_normalize_u8 (f16x2 image, 4 channels, padded)
    -> 7x7/2 convolution reading 8-pixel runs (cin = 32 slots per kernel row, 7 rows)."""
    from avsum_amd.cnn import RESNET_MEAN, RESNET_STD, ResNet50Runner, _stem_weight
    ops = _ops()
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, (3, 224, 224, 3), dtype=np.uint8))
    img = ops.frames_normalize(frames.to(dev), torch.float32, 1.0, RESNET_MEAN, RESNET_STD, 230, 232, 3, 3,
                               code=ops.dtype_code(torch.float32, "f16x2"))
    mean, std = torch.tensor(RESNET_MEAN), torch.tensor(RESNET_STD)
    xn = (frames.float() / 1.0 - mean) / std                      # (x - mean) / std WITHOUT / 255 (extractors.py:133-139)
    ref_img = torch.zeros(3, 230, 232, 4)
    ref_img[:, 3:227, 3:227, :3] = xn
    ref_p = emu_pack(ref_img.reshape(3, 230, 232 * 4)).reshape(3, 230, 232, 4)   # runs of 8 slots = two pixels
    assert torch.equal(img.cpu().view(torch.int32), ref_p.view(torch.int32))
    g = torch.Generator().manual_seed(9)
    w4 = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    wp = emu_pack(_stem_weight(w4, 8, torch.float32))
    geom, xs, wrs = ResNet50Runner._stem_geom(3)
    y = torch.empty((3, 112, 112, 64), device=dev)
    ops.conv2d_raw(ops.dtype_code(torch.float32, "f16x2"), *geom, img, *xs, wp.to(dev), wrs, y, 64, algo_k=147)
    xv = emu_unpack(ref_p.reshape(3, 230, 232 * 4)).reshape(3, 230, 232, 4)[..., :3].double()
    wv = emu_unpack(wp).reshape(64, 7, 8, 4)[:, :, :7, :3].double()
    ref = F.conv2d(xv.permute(0, 3, 1, 2), wv.permute(0, 3, 1, 2), None, 2, 0).permute(0, 2, 3, 1)[:, :112, :112]
    got = ops.f16x2_unpack(y).cpu().double()
    assert (got - ref).abs().max().item() <= TOL * ref.abs().max().item()


def _group_stats(raw, rpg, gamma, beta, eps):
    rows, c = raw.shape
    groups = (rows + rpg - 1) // rpg
    sc, sh = torch.empty(groups, c, dtype=torch.float64), torch.empty(groups, c, dtype=torch.float64)
    for gi in range(groups):
        blk = raw[gi * rpg:(gi + 1) * rpg]
        mean, var = blk.mean(0), blk.var(0, unbiased=False)
        sc[gi] = gamma.double() / torch.sqrt(var + eps)
        sh[gi] = beta.double() - mean * sc[gi]
    return sc, sh


@pytest.mark.parametrize("cfg", [
    (12, 56, 64, 256, 1, 1, 1, 0.0),     # layer1 conv3 shape: tiles straddle groups (3136 % 256 != 0)
    (12, 56, 64, 64, 3, 1, 1, 0.0),      # 64-wide tile, spatial taps
    (8, 28, 128, 128, 3, 2, 4, 0.0),     # stride 2, 4-frame groups
    (5, 14, 1024, 256, 1, 1, 5, 0.0),    # ONE group for the whole call (980 rows)
    (7, 14, 64, 128, 3, 1, 2, 0.0),      # 392-row groups, a shorter last group (7 frames in pairs)
    (6, 28, 64, 64, 1, 1, 1, 300.0),     # mean >> spread: E[y^2] - E[y]^2 would cancel, the centred sums do not
    (4, 16, 32, 128, 3, 1, 1, 50.0),
])
def test_conv_bnstats_f16x2(dev, cfg):
    """Convolution + BatchNorm batch statistics from the epilogue (two-round centred sums per tile, Chan's merge over
    the tiles of a group) against float64 statistics of the float64 convolution; deterministic."""
    ops = _ops()
    frames, hw, cin, cout, k, s, gf, offset = cfg
    pad = k // 2
    xp, wp, xv, wv = _conv_operands(frames, hw, hw, cin, cout, k, k, sum(cfg[:6]), offset)
    if offset:   # a weight column sum far from zero so that the OUTPUT mean is large against its spread
        wv = wv.abs()
        wp = emu_pack(wv.float().reshape(cout, -1))
        wv = emu_unpack(wp).double().reshape(cout, k, k, cin)
    ref = _conv_ref(xv, wv, s, pad)
    ho = ref.shape[1]
    rpg = gf * ho * ho
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    raw = ref.reshape(-1, cout)
    sc_ref, sh_ref = _group_stats(raw, rpg, gamma, beta, 1e-5)
    res = []
    for _ in range(2):
        y = torch.empty((frames, ho, ho, cout), device=dev)
        sc, sh = ops.conv2d(xp.to(dev), wp.to(dev), k, k, s, pad, y, bnstats=(rpg, gamma.to(dev), beta.to(dev), 1e-5),
                            split="f16x2")
        res.append((y, sc, sh))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    y, sc, sh = res[0]
    got = ops.f16x2_unpack(y).cpu().double().reshape(-1, cout)
    assert (got - raw).abs().max().item() <= TOL * max(1.0, raw.abs().max().item())
    # the variance is what is hard: relative error of scale = 0.5 * relative error of (var + eps).  The statistics
    # ALGORITHM is judged on the kernel's own output (float64 statistics of the values it stored): 2e-5.  Against the
    # float64 convolution the fp32 accumulation error e of the outputs themselves enters through 2 cov(y, e) / var:
    # with |y| ~ 2000 against a spread of 1 (the offset cases) that is a few 1e-5 more.
    sc_own, sh_own = _group_stats(got, rpg, gamma, beta, 1e-5)
    assert ((sc.cpu().double() - sc_own).abs() / sc_own.abs()).max().item() < 2e-5
    ynorm = raw.abs().max().item() * sc_ref.abs().max().item()
    assert (sh.cpu().double() - sh_own).abs().max().item() < 2e-5 * max(1.0, ynorm)
    loose = 2e-5 if not offset else 2e-4
    assert ((sc.cpu().double() - sc_ref).abs() / sc_ref.abs()).max().item() < loose
    assert (sh.cpu().double() - sh_ref).abs().max().item() < loose * max(1.0, ynorm)


def test_bnstats_f16x2_declines_small_groups(dev):
    ops = _ops()
    xp, wp, _, _ = _conv_operands(4, 7, 7, 64, 64, 1, 1, 1)
    y = torch.empty((4, 7, 7, 64), device=dev)
    one = torch.ones(64, device=dev)
    assert ops.conv2d(xp.to(dev), wp.to(dev), 1, 1, 1, 0, y, bnstats=(49, one, one, 1e-5), split="f16x2") is None


def _bn_reference(raw, rpg, gamma, beta, res, relu):
    ref = torch.empty_like(raw)
    for gi in range(raw.shape[0] // rpg):
        blk = raw[gi * rpg:(gi + 1) * rpg]
        mean, var = blk.mean(0), blk.var(0, unbiased=False)
        ref[gi * rpg:(gi + 1) * rpg] = (blk - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
    if res is not None:
        ref = ref + res
    return torch.relu(ref) if relu else ref


# (frames, hw in, cin, cout, kernel, stride, frames per BatchNorm group, residual, relu, input offset)
_LOCAL_CASES = [
    (11, 14, 256, 1024, 1, 1, 1, True, True, 0.3),   # 196 rows: one group per tile
    (11, 14, 256, 256, 3, 1, 1, False, True, 0.3),   # 3x3 taps, 196-row groups
    (7, 14, 1024, 256, 1, 1, 1, False, False, 0.3),  # long reduction
    (13, 8, 128, 128, 3, 1, 1, True, True, 0.3),     # 64-row groups: four per tile, the tile exactly full
    (6, 10, 128, 64, 1, 1, 1, False, True, 0.3),     # 100-row groups: two per tile; 64-wide tile
    (9, 7, 2048, 512, 1, 1, 1, False, True, 0.3),    # 49-row groups: five per tile, last tile 4 groups
    (9, 7, 512, 2048, 1, 1, 1, True, True, 0.3),     # layer4 conv3: 49-row groups, residual
    (8, 7, 512, 512, 3, 2, 4, False, True, 0.3),     # stride 2 to 4x4 maps, 4-frame groups of 64 rows
    (8, 28, 256, 512, 1, 2, 1, False, False, 0.3),   # strided downsample to 14x14, no ReLU
    (10, 7, 512, 128, 1, 1, 1, True, True, 40.0),    # mean >> spread
    (12, 14, 64, 64, 3, 1, 1, False, True, 0.3),     # 43-row..: 196-row groups on the 64-wide tile, spatial
    (5, 28, 256, 256, 3, 2, 1, False, True, 0.3),    # 3x3 / 2 down to 14x14: 196-row groups, strided taps with padding
    (6, 10, 128, 128, 1, 1, 2, True, True, 0.3),     # two-frame groups of 200 rows
    (6, 10, 64, 128, 3, 1, 2, True, False, 40.0),    # ... 3x3, mean >> spread, no ReLU
]


@pytest.mark.parametrize("cfg", _LOCAL_CASES)
def test_conv_bnlocal_f16x2(dev, cfg):
    """Convolution + the whole batch-statistics BatchNorm (+ residual, + ReLU) in one launch on f16x2 operands against
    float64 arithmetic; deterministic."""
    ops = _ops()
    frames, hw, cin, cout, k, s, gf, with_res, relu, offset = cfg
    pad = k // 2
    xp, wp, xv, wv = _conv_operands(frames, hw, hw, cin, cout, k, k, sum(cfg[:6]), offset)
    raw = _conv_ref(xv, wv, s, pad)
    ho = raw.shape[1]
    rpg = gf * ho * ho
    raw = raw.reshape(-1, cout)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    resp = emu_pack(torch.randn(raw.shape[0], cout, generator=g)) if with_res else None
    ref = _bn_reference(raw, rpg, gamma, beta, emu_unpack(resp).double() if with_res else None, relu)
    geom = (frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    code = ops.dtype_code(torch.float32, "f16x2")
    assert ops.conv_bnlocal_tile_rows(code, *geom, *xs, wp.shape[1], cout, rpg) == 256 // rpg * rpg
    xd, wd = xp.to(dev), wp.to(dev)
    # normalised values: |scale| up to gamma / sqrt(var) amplifies the convolution's 1e-6 by the same factor
    amp = max(1.0, (1.0 / torch.sqrt(raw.reshape(-1, rpg, cout).var(1, unbiased=False) + 1e-5)).max().item() *
              raw.abs().max().item())
    # groups of 193..224 rows have a tile of their own (224 rows, the waves split the columns: AVS_TILE_224, what the
    # library picks for them); AVS_TILE_256 keeps them on the general 256-row tile.  Same convolution, another summation
    # order of the statistics: both are held to the float64 bar
    from avsum_amd import _abi
    fits = 192 < rpg <= 224 and cout % 128 == 0
    for variant in ((_abi.TILE_AUTO, _abi.TILE_224, _abi.TILE_256) if fits else (_abi.TILE_AUTO,)):
        outs = []
        for _ in range(2):
            y = torch.empty((frames, ho, ho, cout), device=dev)
            ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                           bnlocal=(rpg, gamma.to(dev), beta.to(dev), 1e-5, resp.to(dev) if with_res else None),
                           variant=variant)
            outs.append(y)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        got = ops.f16x2_unpack(outs[0]).cpu().double().view(-1, cout)
        assert (got - ref).abs().max().item() <= TOL * amp, variant
        if variant == _abi.TILE_AUTO:
            auto = outs[0]
        elif variant == _abi.TILE_224:
            assert torch.equal(auto.view(torch.int32), outs[0].view(torch.int32))   # the library's own choice
    if not fits:
        y = torch.empty((frames, ho, ho, cout), device=dev)
        with pytest.raises(RuntimeError, match="AVS_TILE_224"):
            ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_NONE,
                           bnlocal=(rpg, gamma.to(dev), beta.to(dev), 1e-5, None), variant=_abi.TILE_224)


_CLUSTER_CASES = [   # frames, hw (in), cin, cout, k, stride, frames per group, residual, relu, offset
    (8, 14, 1024, 256, 1, 1, 4, False, True, 0.3),    # layer 3 conv1 with the reference's 4-frame micro-batches
    (8, 14, 256, 256, 3, 1, 4, False, True, 0.3),     # ... conv2 (3x3, spatial taps)
    (8, 14, 256, 1024, 1, 1, 4, True, True, 0.3),     # ... conv3 + residual, 8 column tiles
    (12, 28, 512, 1024, 1, 2, 4, False, False, 0.3),  # the strided downsample to 14x14, no ReLU
    (6, 14, 256, 256, 1, 1, 2, True, True, 40.0),     # two-frame groups (a video's tail), mean >> spread
    (9, 14, 128, 128, 3, 1, 3, False, True, 0.3),     # three-frame groups
    (70, 14, 256, 256, 1, 1, 7, True, True, 0.3),     # more tiles than one round of the chip's slots would order trivially
    (8, 28, 512, 256, 1, 1, 16, False, True, 0.3),    # 28 x 28 maps: a frame = 4 tiles of 196 rows, 4-frame groups = clusters of 16
    (6, 28, 128, 128, 3, 1, 4, False, True, 0.3),     # ... one-frame groups of 4 tiles, 3x3 taps across the tile borders
]


@pytest.mark.parametrize("cfg", _CLUSTER_CASES)
def test_conv_bncluster_f16x2(dev, cfg):
    """avs_conv2d_nhwc_bncluster: convolution + the whole batch-statistics BatchNorm (+ residual, + ReLU) in one launch for
    groups of several 14x14 maps - one 224-row tile per frame, the tiles of a group exchange (mean, centred sum of squares)
    as tagged 8-byte granules and merge them by Chan's update in tile order - against float64 arithmetic
    (features/extractors.py:48: micro-batches of 4 frames; train-mode BatchNorm of the trunk, :29,65).
    Deterministic run to run (the exchange carries values, never partial sums in arrival order); no wait ran out."""
    ops = _ops()
    frames, hw, cin, cout, k, s, gf, with_res, relu, offset = cfg
    pad = k // 2
    xp, wp, xv, wv = _conv_operands(frames, hw, hw, cin, cout, k, k, sum(cfg[:6]), offset)
    raw = _conv_ref(xv, wv, s, pad)
    ho = raw.shape[1]
    # gf = tiles per group: 14 x 14 maps are one tile each (gf frames per group), 28 x 28 maps four tiles of 196 rows
    tiles_per_frame = (ho * ho) // 196
    rpg = gf * 196
    assert rpg % (ho * ho) == 0 or (ho * ho) % rpg == 0
    raw = raw.reshape(-1, cout)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    resp = emu_pack(torch.randn(raw.shape[0], cout, generator=g)) if with_res else None
    ref = _bn_reference(raw, rpg, gamma, beta, emu_unpack(resp).double() if with_res else None, relu)
    geom = (frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    code = ops.dtype_code(torch.float32, "f16x2")
    assert tiles_per_frame in (1, 4)
    assert ops.conv_bncluster_ok(code, *geom, *xs, wp.shape[1], cout, rpg, gf)
    if gf < 16:
        assert not ops.conv_bncluster_ok(code, *geom, *xs, wp.shape[1], cout, rpg, gf + 1)      # not whole tiles
    xd, wd = xp.to(dev), wp.to(dev)
    amp = max(1.0, (1.0 / torch.sqrt(raw.reshape(-1, rpg, cout).var(1, unbiased=False) + 1e-5)).max().item() *
              raw.abs().max().item())
    outs = []
    for _ in range(3):
        y = torch.full((frames, ho, ho, cout), float("nan"), device=dev)
        ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                       bnlocal=(rpg, gamma.to(dev), beta.to(dev), 1e-5, resp.to(dev) if with_res else None), cluster=gf)
        outs.append(y)
    assert ops.cluster_exchange_errors(dev) == 0
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    got = ops.f16x2_unpack(outs[0]).cpu().double().view(-1, cout)
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= TOL * amp
    # the same group statistics as the unfused sequence (convolution + statistics, then the apply pass) to rounding
    y2 = torch.empty((frames, ho, ho, cout), device=dev)
    aff = ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y2, cout, bnstats=(rpg, gamma.to(dev), beta.to(dev), 1e-5))
    assert aff is not None
    rows = torch.arange(0, raw.shape[0] // rpg + 1, dtype=torch.int64, device=dev) * rpg
    y2d = y2.view(-1, cout)
    ops.bn_apply(y2d, aff[0], aff[1], rows, rpg, resp.to(dev) if with_res else None, ops.ACT_RELU if relu else ops.ACT_NONE,
                 y2d, code=code)
    assert (ops.f16x2_unpack(y2).cpu().double().view(-1, cout) - got).abs().max().item() <= 2 * TOL * amp


def test_elementwise_f16x2(dev):
    """avs_bn_apply (+ residual, + ReLU), avs_bn_maxpool_nhwc, avs_pool2d_nhwc, avs_global_avgpool_nhwc,
    avs_bn_batch_stats on f16x2 tensors against float64 arithmetic on the unpacked values."""
    ops = _ops()
    code = ops.dtype_code(torch.float32, "f16x2")
    g = torch.Generator().manual_seed(8)
    n, h, c = 5, 12, 64
    xp = emu_pack(torch.randn(n, h, h, c, generator=g) * 3 + 1)
    rp = emu_pack(torch.randn(n, h, h, c, generator=g))
    xv, rv = emu_unpack(xp).double(), emu_unpack(rp).double()
    groups = [0, 2, 3, 5]
    grow = torch.tensor([v * h * h for v in groups], dtype=torch.int64, device=dev)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    sc, sh = ops.bn_batch_stats(xp.to(dev).view(-1, c), grow, gamma.to(dev), beta.to(dev), 1e-5, code=code)
    ref_sc = torch.stack([gamma.double() / torch.sqrt(xv[a:b].reshape(-1, c).var(0, unbiased=False) + 1e-5)
                          for a, b in zip(groups[:-1], groups[1:])])
    ref_sh = torch.stack([beta.double() - xv[a:b].reshape(-1, c).mean(0) * s for (a, b), s in
                          zip(zip(groups[:-1], groups[1:]), ref_sc)])
    assert (sc.cpu().double() - ref_sc).abs().max().item() < 1e-5
    assert (sh.cpu().double() - ref_sh).abs().max().item() < 1e-5
    gid = torch.tensor([0, 0, 1, 2, 2])
    yref = torch.relu(xv * sc.cpu().double()[gid][:, None, None, :] + sh.cpu().double()[gid][:, None, None, :] + rv)
    y = ops.bn_apply(xp.to(dev).view(-1, c), sc, sh, grow, 2 * h * h, rp.to(dev).view(-1, c), ops.ACT_RELU, code=code)
    got = ops.f16x2_unpack(y).cpu().double().view(n, h, h, c)
    assert (got - yref).abs().max().item() < 2e-6 * yref.abs().max().item()
    # bn + relu + maxpool 3x3/2 pad 1 in one pass; plain max / average pooling; global average
    pooled = torch.empty((n, 6, 6, c), device=dev)
    ops.bn_maxpool(xp.to(dev), sc, sh, grow, True, 3, 2, 1, pooled, code=code)
    act = torch.relu(xv * sc.cpu().double()[gid][:, None, None, :] + sh.cpu().double()[gid][:, None, None, :])
    pref = F.max_pool2d(act.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert (ops.f16x2_unpack(pooled).cpu().double() - pref).abs().max().item() < 2e-6 * pref.abs().max().item()
    mp = torch.empty((n, 6, 6, c), device=dev)
    ops.pool2d(xp.to(dev), "max", 3, 2, 1, mp, code=code)
    assert torch.equal(ops.f16x2_unpack(mp).cpu().double(), F.max_pool2d(xv.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
    ga = ops.global_avgpool(xp.to(dev), code=code).cpu().double()
    assert (ga - xv.mean((1, 2))).abs().max().item() < 1e-5


def _frames(n, seed, h=224, w=224):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("gsize", [1, 2, 4])
def test_resnet50_trunk_f16x2(dev, gsize):
    """The whole trunk in the f16x2 mode (tile-local BatchNorm on the 14x14 / 7x7 layers, epilogue statistics + apply
    on the others) against the fp32 oracle on the CPU and against the exact-fp32 GPU mode; deterministic."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    from oracle import cnn as ocnn
    torch.manual_seed(24)
    trunk = resnet50_trunk()
    frames = _frames(8, 5)
    sd = {k: v.clone() for k, v in trunk.state_dict().items()}
    with torch.no_grad():
        x = torch.cat([ocnn.preprocess_frame(f) for f in frames])
        ref = torch.cat([ocnn.resnet50_trunk_forward(sd, x[i:i + gsize]) for i in range(0, 8, gsize)])
    trunk = trunk.to(dev)
    fd = torch.from_numpy(frames).to(dev)
    groups = list(range(0, 9, gsize))
    r = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2")
    got = r.forward(fd, groups).cpu()
    assert torch.equal(got, r.forward(fd, groups).cpu())
    g32 = ResNet50Runner(trunk, torch.float32, "batch").forward(fd, groups).cpu()
    scale = max(1.0, ref.abs().max().item())
    e_oracle, e_gpu32 = (got - ref).abs().max().item(), (got - g32).abs().max().item()
    e_32_oracle = (g32 - ref).abs().max().item()
    print(f"\n[gsize {gsize}] f16x2 vs oracle {e_oracle / scale:.2e}, vs GPU fp32 {e_gpu32 / scale:.2e}; "
          f"GPU fp32 vs oracle {e_32_oracle / scale:.2e} (relative to the largest feature)")
    # the fp32 features of this trunk are themselves conditioned to a few 1e-4 (test_resnet50_trunk_equal_groups)
    assert e_oracle < 5e-4 * scale and e_gpu32 < 5e-4 * scale


def test_resnet50_trunk_f16x2_ragged_groups(dev):
    """Groups of unequal size (4 + 1 frames) take the unfused sequence (avs_bn_batch_stats + avs_bn_apply on f16x2)."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(21)
    trunk = resnet50_trunk().to(dev)
    fd = torch.from_numpy(_frames(5, 1)).to(dev)
    got = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2").forward(fd, [0, 4, 5]).cpu()
    ref = ResNet50Runner(trunk, torch.float32, "batch").forward(fd, [0, 4, 5]).cpu()
    assert (got - ref).abs().max().item() < 5e-4 * max(1.0, ref.abs().max().item())


def test_low_contrast_frames_f16x2_vs_fp32(dev):
    """Near-constant frames (black, white, +-1 grey level of noise, letterbox bars, a faint ramp): the stem's convolution
    output is then almost constant per channel (mean^2 >> variance; inputs reach ~1100 because the reference does not
    divide by 255), which is where statistics of the E[y^2] - E[y]^2 form cancel.  The f16x2 mode takes centred
    two-round sums.  Such frames are ill-conditioned for ANY arithmetic (interior pixels are identical, BatchNorm divides
    by the little variance the borders leave, 53 times), so the bar is relative: against the fp32 ORACLE on the CPU the
    f16x2 mode must not be materially worse than the exact-fp32 GPU mode is on the same frame."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    from oracle import cnn as ocnn
    torch.manual_seed(3)
    trunk = resnet50_trunk()
    sd = {k: v.clone() for k, v in trunk.state_dict().items()}
    trunk = trunk.to(dev)
    rng = np.random.default_rng(0)
    frames = np.zeros((6, 224, 224, 3), dtype=np.uint8)
    frames[1] = 255
    frames[2] = 128 + rng.integers(0, 2, (224, 224, 3))            # +-1 grey level of noise
    frames[3, 40:184] = rng.integers(100, 104, (144, 224, 3))      # letterbox bars around a low-contrast picture
    frames[4] = np.linspace(0, 8, 224, dtype=np.float32)[None, :, None].astype(np.uint8)   # a faint ramp
    frames[5] = rng.integers(0, 256, (224, 224, 3))                # an ordinary frame for scale
    with torch.no_grad():
        oracle = torch.cat([ocnn.resnet50_trunk_forward(sd, ocnn.preprocess_frame(f)) for f in frames])
    fd = torch.from_numpy(frames).to(dev)
    got = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2").forward(fd).cpu()
    g32 = ResNet50Runner(trunk, torch.float32, "batch").forward(fd).cpu()
    assert torch.isfinite(got).all() and torch.isfinite(g32).all()
    bad = []
    for i in range(6):
        scale = max(1.0, oracle[i].abs().max().item())
        e_h2 = (got[i] - oracle[i]).abs().max().item() / scale
        e_32 = (g32[i] - oracle[i]).abs().max().item() / scale
        print(f"\nframe {i}: f16x2 vs oracle {e_h2:.2e}, exact fp32 (GPU) vs oracle {e_32:.2e}, "
              f"f16x2 vs exact fp32 (GPU) {(got[i] - g32[i]).abs().max().item() / scale:.2e} (of the largest feature)")
        if e_h2 > 3.0 * max(e_32, 1e-4) or e_32 > 1e-3:   # (the exact mode's Welford statistics pass holds too)
            bad.append(i)
    assert not bad, bad


@pytest.mark.parametrize("rpg,k,n,xf,with_res,ra", [
    (3136, 64, 256, True, True, False),     # layer1 conv3: raw conv2 output in, identity residual
    (3136, 64, 256, False, False, False),   # layer1 downsample: finished input, no residual, no ReLU
    (784, 128, 512, True, True, True),      # layer2 conv3 of the first block: the residual is the RAW downsample output
    (784, 128, 512, True, True, False),
    (196, 64, 96, True, False, False),      # odd sizes: 196-row groups, 96 outputs (one 128-wide tile, partly used)
    (100, 128, 64, False, True, False),     # 64-wide tile, groups of 100 rows (a wave's rows straddle groups)
])
def test_gram_statistics_and_affine_pass_f16x2(dev, rpg, k, n, xf, with_res, ra):
    """avs_bn_gram_affine_f16x2 (statistics of y = a . w^T from the second moments of a, the input's BatchNorm + ReLU
    applied and stored in place) + avs_conv2d_nhwc_affine (one streaming pass) against float64; deterministic."""
    ops = _ops()
    code = ops.dtype_code(torch.float32, "f16x2")
    groups = 5
    rows = groups * rpg
    g = torch.Generator().manual_seed(rpg + k + n)
    xp = emu_pack(torch.randn(rows, k, generator=g) * 2 + 0.5)
    wp = emu_pack(torch.randn(n, k, generator=g) / k ** 0.5)
    gamma, beta = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    isc, ish = torch.rand(groups, k, generator=g) + 0.5, torch.randn(groups, k, generator=g) * 0.5
    xv, wv = emu_unpack(xp).double(), emu_unpack(wp).double()
    gid = torch.arange(rows) // rpg
    if xf:
        a32 = torch.relu(torch.addcmul(ish[gid], emu_unpack(xp), isc[gid]))      # fp32, like the kernel (fmaf)
        a_st = emu_unpack(emu_pack(a32)).double()
    else:
        a_st = xv
    yref = a_st @ wv.t()
    sc_ref, sh_ref = _group_stats(yref, rpg, gamma, beta, 1e-5)
    xd, wd = xp.to(dev), wp.to(dev)
    res = []
    for _ in range(2):
        xin = xd.clone()
        sc, sh = ops.bn_gram_affine_h2(xin, wd, rpg, gamma.to(dev), beta.to(dev), 1e-5,
                                       (isc.to(dev), ish.to(dev)) if xf else None, store_input=xf)
        res.append((xin, sc, sh))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    xin, sc, sh = res[0]
    if xf:   # the finished activation, in place (a fused multiply-add against torch's: one rounding of difference)
        a_gpu = ops.f16x2_unpack(xin).cpu().double()
        assert (a_gpu - a_st).abs().max().item() <= 1e-6 * max(1.0, a_st.abs().max().item())
        a_st = a_gpu
        yref = a_st @ wv.t()
        sc_ref, sh_ref = _group_stats(yref, rpg, gamma, beta, 1e-5)
    assert ((sc.cpu().double() - sc_ref).abs() / sc_ref.abs()).max().item() < 2e-5
    ynorm = yref.abs().max().item() * sc_ref.abs().max().item()
    assert (sh.cpu().double() - sh_ref).abs().max().item() < 2e-5 * max(1.0, ynorm)
    # the streaming pass with the kernel's own affine
    resp = emu_pack(torch.randn(rows, n, generator=g)) if with_res else None
    rsc = (torch.rand(groups, n, generator=g) + 0.5) if ra else None
    rsh = torch.randn(groups, n, generator=g) if ra else None
    out_ref = yref * sc.cpu().double()[gid] + sh.cpu().double()[gid]
    if with_res:
        r = emu_unpack(resp).double()
        out_ref = out_ref + (r * rsc.double()[gid] + rsh.double()[gid] if ra else r)
    relu = with_res or xf
    if relu:
        out_ref = torch.relu(out_ref)
    # both weight layouts and both tiles (short reductions take the 128-row tile by rule, AVS_TILE_256 / AVS_TILE_128 force
    # one): no statistics in this form, so every variant gives the same bits
    from avsum_amd import _abi
    outs = []
    for layout, variant in ((0, _abi.TILE_AUTO), (1, _abi.TILE_AUTO), (1, _abi.TILE_256), (0, _abi.TILE_128)):
        y = torch.empty((rows, n), device=dev)
        wsel = ops.weights_kstep32(wd) if layout else wd
        ops.conv2d_affine(code, rows, 1, 1, k, 1, 1, 1, 1, n, xin, k, k, k, wsel, k, y, n, rpg, sc, sh,
                          resp.to(dev) if with_res else None, relu, (rsc.to(dev), rsh.to(dev)) if ra else None,
                          w_layout=layout, variant=variant)
        outs.append(y)
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    got = ops.f16x2_unpack(outs[0]).cpu().double()
    assert (got - out_ref).abs().max().item() <= TOL * max(1.0, out_ref.abs().max().item())


def test_affine_pass_long_reduction_every_variant(dev):
    """avs_conv2d_nhwc_affine with AVS_TILE_128 and a reduction longer than the 64-byte-step rule (K = 1024) used
    to return AVS_OK without launching anything.  The tile variant is a hint: every variant must write the same bits, and
    they must be the convolution's."""
    ops = _ops()
    from avsum_amd import _abi
    code = ops.dtype_code(torch.float32, "f16x2")
    rpg, groups, k, n = 196, 3, 1024, 256
    rows = rpg * groups
    g = torch.Generator().manual_seed(17)
    xp = emu_pack(torch.randn(rows, k, generator=g))
    wp = emu_pack(torch.randn(n, k, generator=g) / k ** 0.5)
    sc, sh = torch.rand(groups, n, generator=g) + 0.5, torch.randn(groups, n, generator=g)
    gid = torch.arange(rows) // rpg
    ref = torch.relu(emu_unpack(xp).double() @ emu_unpack(wp).double().t() * sc.double()[gid] + sh.double()[gid])
    outs = []
    for variant in (_abi.TILE_AUTO, _abi.TILE_128, _abi.TILE_256):
        y = torch.full((rows, n), float("nan"), device=dev)
        ops.conv2d_affine(code, rows, 1, 1, k, 1, 1, 1, 1, n, xp.to(dev), k, k, k, wp.to(dev), k, y, n, rpg, sc.to(dev),
                          sh.to(dev), None, True, None, w_layout=0, variant=variant)
        outs.append(y)
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    got = ops.f16x2_unpack(outs[0]).cpu().double()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= TOL * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("n,fpg,kind", [(6, 1, "random"), (8, 4, "random"), (3, 3, "random"), (4, 1, "low_contrast")])
def test_fused_stem_f16x2(dev, n, fpg, kind):
    """avs_stem_conv_pool_f16x2 (uint8 frames -> conv1 7x7/2 with the normalisation folded into the operands -> centred
    statistics of bn1 -> the pooled RAW map) against (i) float64 on the reference's formula ((x - mean) / std without /255,
    zero padding of the NORMALISED input, features/extractors.py:126-140 + children()[0:4]) and (ii) the unfused HIP
    sequence it replaces (avs_frames_normalize_u8 -> avs_conv2d_nhwc_bnstats -> avs_bn_maxpool_nhwc).
    Bars: statistics <= 2e-5, values <= 1e-5 of the scale (the f16x2 bars of this file); deterministic."""
    import torch.nn.functional as F
    ops = _ops()
    from avsum_amd.cnn import RESNET_MEAN, RESNET_STD, _stem_weight
    g = torch.Generator().manual_seed(140 + n)
    if kind == "random":
        frames = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=g)
    else:   # black / white / grey +- 1 level / letterbox: the stem's output is almost constant per channel
        frames = torch.zeros((n, 224, 224, 3), dtype=torch.uint8)
        frames[1] = 255
        frames[2] = 128
        frames[2, ::2, 1::2] = 129
        frames[3, 40:180] = torch.randint(0, 256, (140, 224, 3), dtype=torch.uint8, generator=g)
    w4 = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5
    gamma = torch.randn(64, generator=g)                      # both signs
    beta = torch.randn(64, generator=g) * 0.5
    fd, gd, bd = frames.to(dev), gamma.to(dev), beta.to(dev)
    wimg = ops.stem_h2_operands(w4.to(dev), 1.0, RESNET_MEAN, RESNET_STD)
    y, sc, sh = ops.stem_conv_pool_h2(fd, wimg, fpg, gd, bd, 1e-5)
    y2, sc2, sh2 = ops.stem_conv_pool_h2(fd, wimg, fpg, gd, bd, 1e-5)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(sc, sc2) and torch.equal(sh, sh2)
    assert y.shape == (n, 56, 56, 64) and sc.shape == (n // fpg, 64)
    # (i) float64 on the fp32 normalised input (the reference's own rounding of x) and the fp32 weights
    mean = torch.tensor(RESNET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(RESNET_STD).view(1, 3, 1, 1)
    x = ((frames.permute(0, 3, 1, 2).float() - mean) / std)
    raw = F.conv2d(x.double(), w4.double(), None, 2, 3)                              # [n,64,112,112]
    rg = raw.view(n // fpg, fpg, 64, 112, 112)
    m = rg.mean((1, 3, 4), keepdim=True)
    v = rg.var((1, 3, 4), unbiased=False, keepdim=True)
    scale_ref = gamma.double().view(1, 1, 64, 1, 1) / torch.sqrt(v + 1e-5)
    shift_ref = beta.double().view(1, 1, 64, 1, 1) - m * scale_ref
    rel = ((sc.cpu().double() - scale_ref.view(-1, 64)).abs() / scale_ref.view(-1, 64).abs()).max().item()
    # (the variance of a constant frame's channel is carried by its border pixels alone: ill-conditioned for any arithmetic)
    assert rel < (2e-5 if kind == "random" else 2e-4), rel
    ynorm = raw.abs().max().item() * scale_ref.abs().max().item()
    assert (sh.cpu().double() - shift_ref.view(-1, 64)).abs().max().item() < (2e-5 if kind == "random" else 2e-4) * max(1.0, ynorm)
    sgn = torch.sign(gamma + (gamma == 0)).double().view(1, 64, 1, 1)
    pooled = (F.max_pool2d(raw * sgn, 3, 2, 1) * sgn).permute(0, 2, 3, 1)         # max where gamma >= 0, min elsewhere
    got = ops.f16x2_unpack(y).cpu().double()
    assert (got - pooled).abs().max().item() <= TOL * max(1.0, raw.abs().max().item())
    # (ii) the unfused HIP sequence: same statistics to rounding; finished maps agree
    code = ops.dtype_code(torch.float32, "f16x2")
    x0 = ops.frames_normalize(fd, torch.float32, 1.0, RESNET_MEAN, RESNET_STD, 230, 232, 3, 3, code=code)
    wk = ops.f16x2_pack(_stem_weight(w4, 8, torch.float32).to(dev))
    rawd = torch.empty((n, 112, 112, 64), dtype=torch.float32, device=dev)
    geom, xs = (n, 230, 112, 32, 7, 1, 2, 1, 0, 0, 112, 112, 64), (230 * 232 * 4, 232 * 4, 8)
    scu, shu = ops.conv2d_raw(code, *geom, x0, *xs, wk, wk.stride(0), rawd, 64, bnstats=(fpg * 112 * 112, gd, bd, 1e-5))
    assert ((sc - scu).abs() / scu.abs()).max().item() < (4e-5 if kind == "random" else 4e-4)
    rows = torch.arange(0, n + 1, fpg, dtype=torch.int64, device=dev) * 112 * 112
    yu = ops.bn_maxpool(rawd, scu, shu, rows, True, 3, 2, 1, torch.empty((n, 56, 56, 64), device=dev), code=code)
    gidx = (torch.arange(n) // fpg).to(dev)
    fin = torch.relu(ops.f16x2_unpack(y) * sc[gidx].view(n, 1, 1, 64) + sh[gidx].view(n, 1, 1, 64))
    fu = ops.f16x2_unpack(yu)
    bar = (2e-5 if kind == "random" else 5e-4) * max(1.0, fu.abs().max().item())
    assert (fin - fu).abs().max().item() <= bar


@pytest.mark.parametrize("n,h,cin,couts,pool_cout", [(3, 17, 768, (192, 160, 160), 192), (2, 35, 192, (64, 48, 64), 32),
                                                     (2, 8, 1280, (320, 384, 448), 0),
                                                     # 288 stacked columns on enough rows for the 256 x 96 tiles, the split
                                                     # inside the first of them
                                                     (150, 35, 64, (64, 128, 96), 0)])
def test_conv_split_two_destinations(dev, n, h, cin, couts, pool_cout):
    """avs_conv2d_nhwc_split: several 1x1 convolutions that read one input as ONE contraction over their stacked filters - the
    first head into its channel slice of a wider buffer, the others (and, with relu_cols, a head without bias / ReLU) into a
    temporary - bit for bit the separate avs_conv2d_nhwc launches (an Inception block's heads, features/extractors.py:26,73-90)."""
    ops = _ops()
    g = torch.Generator().manual_seed(n + h + cin)
    x = emu_pack(torch.randn(n, h, h, cin, generator=g)).to(dev)
    ws = [emu_pack(torch.randn(c, cin, generator=g) / cin ** 0.5).to(dev) for c in couts + ((pool_cout,) if pool_cout else ())]
    bs = [torch.randn(c, generator=g).to(dev) for c in couts]
    cat = torch.full((n, h, h, couts[0] + 40), float("nan"), device=dev)        # the first head's slice of a concatenation
    ref_tmp = []
    ops.conv2d(x, ws[0], 1, 1, 1, 0, cat[..., :couts[0]], bs[0], ops.ACT_RELU, split="f16x2")
    ref_first = cat[..., :couts[0]].clone()
    for w_, b_ in zip(ws[1:len(couts)], bs[1:]):
        y = torch.empty((n, h, h, w_.shape[0]), device=dev)
        ops.conv2d(x, w_, 1, 1, 1, 0, y, b_, ops.ACT_RELU, split="f16x2")
        ref_tmp.append(y)
    if pool_cout:
        y = torch.empty((n, h, h, pool_cout), device=dev)
        ops.conv2d(x, ws[-1], 1, 1, 1, 0, y, None, ops.ACT_NONE, split="f16x2")   # raw: bias + ReLU follow a pooling
        ref_tmp.append(y)
    wst = torch.cat(ws).contiguous()                                            # packed rows stack as they are
    bst = torch.cat(bs + ([torch.zeros(pool_cout, device=dev)] if pool_cout else [])).contiguous()
    cat2 = torch.full_like(cat, float("nan"))
    tmp = torch.full((n, h, h, sum(couts[1:]) + pool_cout), float("nan"), device=dev)
    ops.conv2d_split(x, wst, cat2[..., :couts[0]], couts[0], tmp, bst, ops.ACT_RELU,
                     relu_cols=(sum(couts) if pool_cout else 0))
    assert torch.equal(cat2[..., :couts[0]].contiguous().view(torch.int32), ref_first.view(torch.int32))
    assert torch.isnan(cat2[..., couts[0]:]).all()                              # nothing beyond the slice was touched
    o = 0
    for y in ref_tmp:
        c = y.shape[3]
        assert torch.equal(tmp[..., o:o + c].contiguous().view(torch.int32), y.view(torch.int32)), o
        o += c


@pytest.mark.parametrize("cfg", [
    (3, 17, 17, 128, 192, 1, 7, 1, (0, 3)), (2, 17, 17, 160, 160, 7, 1, 1, (3, 0)), (5, 35, 35, 64, 96, 3, 3, 1, 1),
    (2, 35, 35, 96, 96, 3, 3, 2, 0), (2, 19, 19, 80, 192, 3, 3, 1, 0), (2, 9, 9, 768, 288, 1, 1, 1, 0),
    (1, 13, 13, 24, 104, 3, 3, 1, 1),
])
def test_conv_bias_relu_96_column_tiles(dev, cfg):
    """The bias + ReLU convolutions whose cout leaves a 128-wide column tile mostly empty (96, 160, 192, 288: most of
    Inception-v3, features/extractors.py:26,83) run on 256 x 96 tiles where the rows allow it (forced here per call with
    AVS_TILE_256; AVS_TILE_128 keeps the 128 x 128 tiles): the same products in the same order - bit for bit the same
    outputs, both weight layouts, ragged last tiles, a channel-slice destination - and the double-precision reference."""
    ops = _ops()
    n, h, w, cin, cout, kh, kw, stride, pad = cfg
    xp, wp, xv, wv = _conv_operands(n, h, w, cin, cout, kh, kw, h * 7 + cout)
    g = torch.Generator().manual_seed(cout)
    bias = torch.randn(cout, generator=g)
    ref = torch.relu(_conv_ref(xv, wv, stride, pad) + bias.double())
    ho, wo = ref.shape[1], ref.shape[2]
    scale = max(1.0, ref.abs().max().item())
    outs = []
    for variant in (1, 2):                       # AVS_TILE_128, AVS_TILE_256
        for layout in (0, 1):
            if layout == 1 and (kh * kw * cin) % 16:
                continue
            wd = wp.to(dev)
            wsel = ops.weights_kstep32(wd) if layout else wd
            buf = torch.full((n, ho, wo, cout + 24), float("nan"), device=dev)
            out = buf[..., 8:8 + cout]
            ops.conv2d(xp.to(dev), wsel, kh, kw, stride, pad, out, bias.to(dev), ops.ACT_RELU, split="f16x2", w_layout=layout,
                       variant=variant)
            assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + cout:]).all()
            outs.append(out.contiguous())
    got = ops.f16x2_unpack(outs[0]).cpu().double()
    assert (got - ref).abs().max().item() <= TOL * scale
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))


@pytest.mark.parametrize("cfg", [
    (1024, 17, 128, 192, 1, 7, 0), (1024, 17, 160, 160, 7, 1, 32), (512, 35, 64, 96, 3, 3, 48), (2048, 8, 384, 384, 1, 3, 0),
    (2048, 8, 448, 384, 3, 3, 64), (900, 17, 192, 192, 7, 1, 0),
])
def test_conv_bias_relu_shifted_row_form(dev, cfg):
    """Stride-1 'same' bias + ReLU convolutions (Inception-v3's 1x7 / 7x1 / 3x3 / 1x3 layers, features/extractors.py:26,83) on
    enough rows for the 256-row tiles take the shifted-row form by rule: a channel block of the tile's pixels and its halo is
    fetched once and serves every tap from shifted LDS rows (block-major / tap-minor reduction order).  Against the classic
    tap walk (AVS_TILE_256 keeps it) to rounding on the whole tensor - frame borders, tiles that straddle frames, an input
    that is a channel slice of a wider tensor - and against the float64 reference on the first frames; twice the same bits."""
    ops = _ops()
    n, h, cin, cout, kh, kw, xoff = cfg
    g = torch.Generator().manual_seed(h * 31 + cin + kh)
    wide = ops.f16x2_pack(torch.randn(n, h, h, cin + xoff, generator=g).to(dev))
    x = wide[..., xoff // 2:xoff // 2 + cin] if xoff else wide
    wt = torch.randn(cout, kh * kw * cin, generator=g) / (kh * kw * cin) ** 0.5
    wp = ops.f16x2_pack(wt.to(dev))
    bias = torch.randn(cout, generator=g).to(dev)
    pad = (kh // 2, kw // 2)
    outs = []
    for variant in (0, 0, 2):
        y = torch.empty((n, h, h, cout), device=dev)
        ops.conv2d(x, ops.weights_kstep32(wp), kh, kw, 1, pad, y, bias, ops.ACT_RELU, split="f16x2", w_layout=1, variant=variant)
        outs.append(y)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    a, b = ops.f16x2_unpack(outs[0]), ops.f16x2_unpack(outs[2])
    scale = max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= 4e-6 * scale          # two fp32 summation orders of the same products
    m = 3
    xv = ops.f16x2_unpack(x[:m].contiguous()).cpu().double()
    wv = ops.f16x2_unpack(wp).cpu().double().reshape(cout, kh, kw, cin)
    ref = torch.relu(_conv_ref(xv, wv, 1, pad) + bias.cpu().double())
    assert (a[:m].cpu().double() - ref).abs().max().item() <= TOL * max(1.0, ref.abs().max().item())
