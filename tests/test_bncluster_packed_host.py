"""The packed clustered BatchNorm (AVS_CLUSTER_PACKED) as the host sees it: the library's host-only answers with and
without the variant bit, and the packed flag on the ResNet-50 plan.  No GPU."""
import ctypes

import pytest
import torch

from test_gpu_f16x2 import _CLUSTER_CASES


def _ask(frames, hw, cin, cout, k, s, rpg, cluster, packed):
    """avs_conv2d_bncluster_workspace_bytes for a square convolution with 'same' padding."""
    from avsum_amd import _abi, ops
    pad = k // 2
    ho = (hw + 2 * pad - k) // s + 1
    d = _abi.ConvDesc(ops.dtype_code(torch.float32, "f16x2"), frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout,
                      hw * hw * cin, hw * cin, cin, k * k * cin, cout, ops.ACT_NONE, 1.0, 0,
                      _abi.CLUSTER_PACKED if packed else 0)
    return int(_abi.lib().avs_conv2d_bncluster_workspace_bytes(ctypes.byref(d), int(rpg), int(cluster))), ho


@pytest.mark.parametrize("cfg", _CLUSTER_CASES)
def test_unpacked_answers_unchanged(cfg):
    """Without the bit: one granule per lane and tile of rows_per_group / cluster rows, and a cluster count that does not
    give whole tiles is refused - as before the bit existed."""
    from avsum_amd import _abi
    frames, hw, cin, cout, k, s, gf = cfg[:7]
    rpg = gf * 196
    got, ho = _ask(frames, hw, cin, cout, k, s, rpg, gf, False)
    assert got == 64 + (frames * ho * ho // 196) * (cout // 128) * 4 * 64 * 8
    if gf < 16:
        assert _ask(frames, hw, cin, cout, k, s, rpg, gf + 1, False)[0] == _abi.E_UNSUPPORTED


@pytest.mark.parametrize("frames,hw,cin,cout,k,s,gf", [
    (8, 14, 64, 256, 1, 1, 4), (12, 14, 64, 128, 3, 1, 4), (8, 28, 64, 128, 1, 2, 4), (8, 28, 64, 128, 1, 1, 4),
    (320, 14, 64, 256, 1, 1, 4), (16, 14, 1024, 256, 1, 1, 8),
])
def test_packed_workspace(frames, hw, cin, cout, k, s, gf):
    """With the bit: two granules per lane and tile of 224 consecutive rows (the last tile may be short)."""
    ho = (hw + 2 * (k // 2) - k) // s + 1
    rpg = gf * ho * ho
    got, _ = _ask(frames, hw, cin, cout, k, s, rpg, rpg // 196, True)
    tiles = (frames * ho * ho + 223) // 224
    assert got == 64 + tiles * (cout // 128) * 4 * 2 * 64 * 8


@pytest.mark.parametrize("gf", [1, 2, 3, 5, 6, 7])
def test_packed_declines_other_groups(gf):
    """Groups whose rows are not 0 or 112 (mod 224) - 1-3 and 5-7 frames of 14x14, 392 rows among them - are declined with
    the bit (the caller keeps the unpacked form, which takes 2-7)."""
    from avsum_amd import _abi
    rpg = gf * 196
    assert rpg % 224 not in (0, 112)
    frames = gf * 2
    assert _ask(frames, 14, 256, 256, 1, 1, rpg, max(gf, 2), True)[0] == _abi.E_UNSUPPORTED
    if gf >= 2:
        assert _ask(frames, 14, 256, 256, 1, 1, rpg, gf, False)[0] > 0


def test_packed_declines_what_the_unpacked_form_declines():
    from avsum_amd import _abi
    assert _ask(8, 14, 64, 192, 1, 1, 784, 4, True)[0] == _abi.E_UNSUPPORTED      # cout not a multiple of 128
    assert _ask(8, 14, 64, 256, 1, 1, 784, 5, True)[0] == _abi.E_UNSUPPORTED      # cluster does not give whole 196-row tiles
    assert _ask(10, 14, 64, 256, 1, 1, 784, 4, True)[0] == _abi.E_UNSUPPORTED     # rows not whole groups
    assert _ask(8, 14, 64, 256, 1, 1, 784, 4, True)[0] > 0


def _runner():
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(0)
    return ResNet50Runner(resnet50_trunk(), torch.float32, f32_split="f16x2")


def test_plan_carries_the_packed_flag():
    r = _runner()
    gf4 = list(range(0, 17, 4))
    cl = [s for s in r.plan(16, gf4) if s.form == "cluster"]
    assert len(cl) == 20 and all(s.packed for s in cl)
    assert not any(s.packed for s in r.plan(16, gf4) if s.form != "cluster")
    assert not any(s.packed for s in r.plan(16, None))                    # one-frame groups
    assert not any(s.packed for s in r.plan(16, gf4, bn_cluster=False))
    r.pack_groups = False                                                 # (in the plan cache key)
    cl = [s for s in r.plan(16, gf4) if s.form == "cluster"]
    assert len(cl) == 20 and not any(s.packed for s in cl)
    assert r._w is None     # no weights were packed
