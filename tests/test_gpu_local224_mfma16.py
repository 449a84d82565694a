"""The 224-row convolution + BatchNorm kernel (csrc/local224.hip) at the reduction lengths where pairing two 64-byte steps
into one v_mfma_f32_16x16x32_f16 can go wrong: one step (tail only), exactly one pair, a pair plus a tail, nine-tap
reductions whose pairs straddle taps (odd step counts, border masks), and the same through the clustered and the packed
exchange.  All maps are 14x14 (or four 7x7 maps per group) with 128 output columns: one column tile, 196-row tiles, the
packed case seven 224-row tiles with the shared one in the middle.

The library takes reductions of more than 128 bytes only (include/avsum_hip.h: avs_conv2d_nhwc_bnlocal / _bncluster refuse
"a reduction of at most 128 bytes"), so one or two steps - 1x1 with 16 or 32 input channels - never reach the kernel: for
those cases the test holds the library to that refusal, and the shortest reductions that do run stand next to them (three
steps: one pair plus the tail; four steps: pairs only; the clustered form at three steps).

Construction and bar are those of test_gpu_f16x2.py: float64 arithmetic on the unpacked operands, <= TOL * amp; the output
pre-filled with NaN and finite afterwards; three runs bit-identical; no exchange wait ran out."""
import pytest
import torch

from test_gpu_f16x2 import TOL, _bn_reference, _conv_operands, _conv_ref, emu_pack, emu_unpack

pytestmark = pytest.mark.gpu


def _ops():
    from avsum_amd import ops
    return ops


_CASES = [   # form, frames, hw (in), cin, kernel, frames per group, residual, relu, offset  (steps = k * k * cin / 16)
    ("local", 3, 14, 16, 1, 1, False, True, 0.3),      # 1 step: the tail alone (refused: 64 bytes)
    ("local", 3, 14, 32, 1, 1, True, False, 0.3),      # 2 steps: exactly one pair (refused: 128 bytes)
    ("local", 3, 14, 48, 1, 1, False, True, 40.0),     # 3 steps: one pair plus the tail; mean >> spread
    ("local", 3, 14, 64, 1, 1, True, False, 0.3),      # 4 steps: pairs only, the shortest such reduction that runs
    ("local", 3, 14, 16, 3, 1, False, True, 0.3),      # 9 steps: every pair straddles a tap, border masks
    ("local", 3, 14, 48, 3, 1, True, True, 0.3),       # 27 steps
    ("local", 8, 7, 80, 1, 4, False, True, 0.3),       # 5 steps: 4-frame groups of 7x7 maps, one 196-row tile each
    ("cluster", 4, 14, 16, 1, 2, True, False, 40.0),   # the clustered form, 2-frame groups, residual (refused: 64 bytes)
    ("cluster", 4, 14, 48, 1, 2, True, False, 40.0),   # ... at three steps; mean >> spread
    ("packed", 8, 14, 48, 1, 4, True, True, 0.3),      # the packed form: 7 tiles, one shared at its row 112
]


@pytest.mark.parametrize("cfg", _CASES)
def test_local224_step_pairing(dev, cfg):
    ops = _ops()
    from avsum_amd import _abi
    form, frames, hw, cin, k, gf, with_res, relu, offset = cfg
    cout, pad = 128, k // 2
    xp, wp, xv, wv = _conv_operands(frames, hw, hw, cin, cout, k, k, frames + hw + cin + k + gf, offset)
    raw = _conv_ref(xv, wv, 1, pad)
    ho = raw.shape[1]
    assert ho == hw
    rpg = gf * ho * ho
    raw = raw.reshape(-1, cout)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    resp = emu_pack(torch.randn(raw.shape[0], cout, generator=g)) if with_res else None
    ref = _bn_reference(raw, rpg, gamma, beta, emu_unpack(resp).double() if with_res else None, relu)
    geom = (frames, hw, hw, cin, k, k, 1, 1, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    code = ops.dtype_code(torch.float32, "f16x2")
    runs = k * k * cin * 4 > 128              # the library's rule: a reduction of more than 128 bytes
    if form == "local":
        assert rpg == 196
        kw = dict(variant=_abi.TILE_224)      # an error unless the 224-row tile takes the call
    else:
        assert ops.conv_bncluster_ok(code, *geom, *xs, wp.shape[1], cout, rpg, gf, packed=form == "packed") == runs
        kw = dict(cluster=gf, packed=form == "packed")
    xd, wd = xp.to(dev), wp.to(dev)
    gd, bd, rd = gamma.to(dev), beta.to(dev), resp.to(dev) if with_res else None
    if not runs:
        y = torch.empty((frames, ho, ho, cout), device=dev)
        with pytest.raises(RuntimeError, match="more than 128 bytes"):
            ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_NONE, bnlocal=(rpg, gd, bd, 1e-5, rd), **kw)
        return
    amp = max(1.0, (1.0 / torch.sqrt(raw.reshape(-1, rpg, cout).var(1, unbiased=False) + 1e-5)).max().item() *
              raw.abs().max().item())
    outs = []
    for _ in range(3):
        y = torch.full((frames, ho, ho, cout), float("nan"), device=dev)
        ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                       bnlocal=(rpg, gd, bd, 1e-5, rd), **kw)
        outs.append(y)
    if form != "local":
        assert ops.cluster_exchange_errors(dev) == 0
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    got = ops.f16x2_unpack(outs[0]).cpu().double().view(-1, cout)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"\n{form} cin {cin} k {k}: {err:.3e} (bar {TOL * amp:.3e})")
    assert err <= TOL * amp
