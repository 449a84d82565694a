"""Layers 1-2 without per-value group lookups: the paths the library takes where BatchNorm groups align to the kernels'
units, against the general paths they replace.  Every comparison is bit for bit.

* avs_conv2d_nhwc_affine: groups that are whole numbers of 64 rows run an instantiation in which a wave holds ONE group's
  affine.  The reference is the same entry point with every group cut in two (rows_per_group / 2 is no multiple of 64, so the
  general epilogue runs) and every scale / shift / residual-affine row given twice: the same affine per value.
* avs_conv2d_nhwc_bnstats_xin: groups of at least 384 rows take the input affine from an LDS table of the tile's two groups.
  The reference is avs_bn_apply in place followed by the plain nine-tap form.
* ResNet50Runner.forward: reproducible run to run on whole 4- and 3-frame groups.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 64


def _ops():
    from avsum_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _signed(shape, dev, g):
    """Scales of both signs (a negative gamma), away from zero."""
    return ((torch.rand(shape, device=dev, generator=g) + 0.5) *
            torch.where(torch.rand(shape, device=dev, generator=g) < 0.3, -1.0, 1.0)).contiguous()


# (rows_per_group, its general-path divisor, rows): 64 - neighbouring waves of one tile lie in different groups (and the last
# 128-row tile is half empty); 192 x 5 - boundaries inside tiles, the last tile partial; 3136 x 3 - layer 1's frame
GROUPS = [(64, 32, 7 * 64), (192, 96, 5 * 192), (3136, 1568, 3 * 3136)]
# (cout, variant): 128-row tiles (the rule for K <= 128 and wide outputs), the 256-row tile forced, the narrow 256-row tile
TILES = [(256, "TILE_AUTO"), (256, "TILE_256"), (64, "TILE_AUTO")]
RESIDUALS = ["none", "h2", "p8", "raw"]


@pytest.fixture(scope="module")
def affine_inputs(dev):
    """Per (rows, cout): input, weights, the largest residual - built once, never written."""
    ops = _ops()
    cache = {}

    def get(rows, n):
        if (rows, n) not in cache:
            g = torch.Generator(device=dev).manual_seed(rows + n)
            x = ops.f16x2_pack(torch.randn(rows, K, device=dev, generator=g) * 2 + 0.5)
            w = ops.f16x2_pack(torch.randn(n, K, device=dev, generator=g) / K ** 0.5)
            r = torch.randn(rows, n, device=dev, generator=g) * 2
            cache[(rows, n)] = (x, w, ops.f16x2_pack(r), ops.f16p8_pack(r))
        return cache[(rows, n)]
    return get


@pytest.mark.parametrize("tile", TILES, ids=["n256_t128", "n256_t256", "n64"])
@pytest.mark.parametrize("grp", GROUPS, ids=["rpg64", "rpg192", "rpg3136"])
def test_affine_wave_in_one_group_equals_general_epilogue(dev, affine_inputs, grp, tile):
    ops = _ops()
    from avsum_amd import _abi
    code = ops.dtype_code(torch.float32, "f16x2")
    rpg, rpg_ref, rows = grp
    n, variant = tile[0], getattr(_abi, tile[1])
    assert rpg % 64 == 0 and rpg_ref % 64 != 0 and rpg % rpg_ref == 0
    rep = rpg // rpg_ref
    groups = rows // rpg
    x, w, res_h2, res_p8 = affine_inputs(rows, n)
    g = torch.Generator(device=dev).manual_seed(rpg + n)
    sc, sh = _signed((groups, n), dev, g), torch.randn(groups, n, device=dev, generator=g).contiguous()
    rsc, rsh = _signed((groups, n), dev, g), torch.randn(groups, n, device=dev, generator=g).contiguous()
    assert (sc < 0).any() and (rsc < 0).any()

    def twice(t):
        return t.repeat_interleave(rep, dim=0).contiguous()

    def run(group_rows, a, b, residual, relu, res_affine, p8_out):
        if p8_out:
            y = ops.P8.empty((rows, n), dev)
            y.data.fill_(0xff)                       # (fp16 0xffff is a NaN)
        else:
            y = torch.full((rows, n), float("nan"), device=dev)
        ops.conv2d_affine(code, rows, 1, 1, K, 1, 1, 1, 1, n, x, K, K, K, w, K, y, n, group_rows, a, b, residual, relu,
                          res_affine, variant=variant)
        return y.data if p8_out else _bits(y)

    for kind in RESIDUALS:
        residual = {"none": None, "h2": res_h2, "p8": res_p8, "raw": res_h2}[kind]
        before = None if residual is None else (residual.data if kind == "p8" else residual).clone()
        for relu in (True, False):
            got = run(rpg, sc, sh, residual, relu, (rsc, rsh) if kind == "raw" else None, kind == "p8")
            ref = run(rpg_ref, twice(sc), twice(sh), residual, relu, (twice(rsc), twice(rsh)) if kind == "raw" else None,
                      kind == "p8")
            assert torch.equal(got, ref), (kind, relu)
            if kind != "p8":   # every value was written (the prefill is NaN)
                assert torch.isfinite(ops.f16x2_unpack(got.view(torch.float32))).all(), (kind, relu)
            else:
                assert torch.isfinite(ops.f16p8_unpack(ops.P8(got, (rows, n)))).all(), relu
        if residual is not None:
            assert torch.equal(before, residual.data if kind == "p8" else residual), kind


# ---- the nine-tap input transform ----

def _xin_case(dev, frames, hw, cin, fpg, seed):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(seed)
    rpg = fpg * hw * hw
    groups = (frames + fpg - 1) // fpg
    x = ops.f16x2_pack(torch.randn(frames, hw, hw, cin, device=dev, generator=g) * 2.0 + 0.3)
    w = torch.randn(cin, 9 * cin, device=dev, generator=g) * (2.0 / (9 * cin)) ** 0.5
    wk = ops.weights_kstep32(ops.f16x2_pack(w))
    isc = _signed((groups, cin), dev, g)
    isf = (torch.randn(groups, cin, device=dev, generator=g) * 0.5).contiguous()
    gamma = _signed((cin,), dev, g)
    beta = torch.randn(cin, device=dev, generator=g).contiguous()
    return x, wk, rpg, groups, isc, isf, gamma, beta


def _xin_conv(dev, x, wk, frames, hw, cin, rpg, gamma, beta, x_affine=None):
    ops = _ops()
    code = ops.dtype_code(torch.float32, "f16x2")
    geom = (frames, hw, hw, cin, 3, 3, 1, 1, 1, 1, hw, hw, cin)
    y = torch.full((frames, hw, hw, cin), float("nan"), device=dev)
    aff = ops.conv2d_raw(code, *geom, x, hw * hw * cin, hw * cin, cin, wk, wk.stride(0), y, cin,
                         bnstats=(rpg, gamma, beta, 1e-5), w_layout=1, x_affine=x_affine)
    return y, aff


# (frames, map, channels, frames per group, in_relu): every case fills at least 2048 256-row tiles (the nine-tap form's rule)
XIN_CASES = [
    pytest.param(169, 56, 64, 1, True, id="partial_last_tile"),        # 169 x 3136 rows: the last tile holds 64 of them
    pytest.param(168, 56, 64, 2, True, id="boundary_at_row_128"),      # 6272-row groups: row 128 of every second tile
    pytest.param(2048, 16, 64, 1, True, id="rpg256_keeps_lookups"),    # 256 < 384 rows: the per-row transform
    pytest.param(168, 56, 64, 1, False, id="two_groups_no_relu"),
    pytest.param(672, 28, 128, 1, True, id="c128_rpg784"),             # layer 2's smallest group that takes the table
]


@pytest.mark.parametrize("frames,hw,cin,fpg,relu", XIN_CASES)
def test_input_transform_equals_apply_then_conv(dev, frames, hw, cin, fpg, relu):
    ops = _ops()
    x, wk, rpg, groups, isc, isf, gamma, beta = _xin_case(dev, frames, hw, cin, fpg, 7 * frames + hw + fpg)
    x_raw = x.clone()
    y, aff = _xin_conv(dev, x, wk, frames, hw, cin, rpg, gamma, beta, x_affine=(isc, isf, relu))
    assert aff is not None, "the nine-tap form declined a shape it is built for"
    assert torch.equal(_bits(x), _bits(x_raw))
    rows = torch.arange(0, groups + 1, dtype=torch.int64, device=dev) * rpg
    x2d = x.view(-1, cin)
    ops.bn_apply(x2d, isc, isf, rows, rpg, None, ops.ACT_RELU if relu else ops.ACT_NONE, x2d,
                 code=ops.dtype_code(torch.float32, "f16x2"))
    y_ref, aff_ref = _xin_conv(dev, x, wk, frames, hw, cin, rpg, gamma, beta)
    assert torch.equal(_bits(y), _bits(y_ref))
    assert torch.isfinite(ops.f16x2_unpack(y)).all()
    assert torch.equal(_bits(aff[0]), _bits(aff_ref[0])) and torch.equal(_bits(aff[1]), _bits(aff_ref[1]))


# ---- the trunk ----

@pytest.mark.parametrize("n,fpg", [(8, 4), (6, 3)])
def test_trunk_is_reproducible_on_whole_groups(dev, n, fpg):
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(5)
    trunk = resnet50_trunk().to(dev)
    fd = torch.from_numpy(np.random.default_rng(n).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)).to(dev)
    r = ResNet50Runner(trunk, torch.float32, "batch", f32_split="f16x2")
    gf = list(range(0, n + 1, fpg))
    runs = [r.forward(fd, gf).clone() for _ in range(3)]
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[0]), _bits(runs[2]))
