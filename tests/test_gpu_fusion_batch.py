"""Batched fusion on the GPU (ops.FusionTables / ops.fusion_batch / features.fusion.fuse_batch): every pair of a ragged
batch against the per-pair kernels (bit for bit) and against the CPU oracle."""
import numpy as np
import pytest
import torch

import fusion_batch_inputs as fbi
from oracle import fusion as ofu

pytestmark = pytest.mark.gpu


def _run(pairs, dev, gap=0, target_length=None, keep_cost=True):
    from avsum_amd import ops
    vcat, acat, table = fbi.layout(pairs, gap)
    tb = ops.FusionTables(table, dev)
    res = ops.fusion_batch(tb, vcat.to(dev), acat.to(dev), target_length, keep_cost)
    return tb, {k: t.cpu() for k, t in res.items()}


def _pair_results(tb, res, p):
    """(cost [n, m] or None, path [L, 2], L, total, rowcount [n], fused rows) of pair p, on the host."""
    n, m = int(tb.n[p]), int(tb.m[p])
    ln = int(res["path_len"][p])
    assert 1 <= ln <= n + m - 1
    c0, p0, r0 = int(tb.cell_off[p]), int(res["path_offsets"][p]), int(res["row_offsets"][p])
    assert p0 == int(tb.path_off[p]) and r0 == int(tb.row_off[p])
    cost = res["cost"][c0:c0 + n * m].reshape(n, m) if "cost" in res else None
    o0, o1 = int(res["out_offsets"][p]), int(res["out_offsets"][p + 1])
    return cost, res["path"][p0:p0 + ln], ln, res["total"][p], res["rowcount"][r0:r0 + n], res["fused"][o0:o1]


def _check_against_per_pair_kernels(pairs, dev):
    from avsum_amd import ops
    tb, res = _run(pairs, dev)
    for p, (v, a) in enumerate(pairs):
        cost, path, ln, total, rowcount, fused = _pair_results(tb, res, p)
        vd = v.to(dev)
        want_cost = ops.cdist(vd, a.to(dev))
        assert torch.equal(cost, want_cost.cpu()), p
        wpath, wlen, wtotal = ops.dtw_path(want_cost)
        wl = int(wlen.item())
        assert ln == wl and torch.equal(path, wpath[:wl].cpu()), p
        assert torch.equal(total, wtotal.cpu()[0]), p
        uniq, counts = np.unique(wpath[:wl, 0].cpu().numpy(), return_counts=True)     # interpolate_features' weights
        assert np.array_equal(rowcount.numpy(), counts) and np.array_equal(uniq, np.arange(v.shape[0]))
        want = ops.gather_scale(vd, torch.from_numpy(uniq.astype(np.int64)).to(dev),
                                torch.from_numpy((counts / counts.sum()).astype(np.float64)).to(dev))
        assert torch.equal(fused, want.cpu()), p


def test_bitwise_against_per_pair_kernels_d24(dev):
    # D = 24 is no multiple of the cost kernel's 32-wide k step; the three size classes interleave in the tables
    _check_against_per_pair_kernels(fbi.walk_batch(fbi.BATCH_D24, 24), dev)


def test_bitwise_against_per_pair_kernels_d512(dev):
    _check_against_per_pair_kernels(fbi.walk_batch(fbi.BATCH_D512, 512), dev)


def test_against_oracle(dev):
    pairs, refs = fbi.walk_batch(fbi.BATCH_D24, 24), fbi.oracle_batch("d24")
    tb, res = _run(pairs, dev, target_length=40)
    assert res["out_offsets"].tolist() == np.concatenate([[0], np.cumsum([min(n, 40) for n, _ in fbi.BATCH_D24])]).tolist()
    for p, ((v, a), (ocost, opath)) in enumerate(zip(pairs, refs)):
        cost, path, ln, total, rowcount, fused = _pair_results(tb, res, p)
        assert np.array_equal(path.numpy(), opath), p
        err = np.abs(cost.numpy() - ocost).max() / max(np.abs(ocost).max(), 1e-300)
        assert err <= 1e-12, (p, err)
        want = ofu.interpolate_features(v, opath, 40)
        assert fused.shape == (min(v.shape[0], 40), 24) and torch.equal(fused, want), p


def test_tie_order(dev):
    """Rows from {0, 1, 2}: the squared distances are exact integers, so the cost equals the oracle's bit for bit and
    the path, full of exact ties, is decided by the tie order alone (up, then left, then diagonal)."""
    pairs, refs = fbi.tie_batch(), fbi.oracle_batch("tie")
    tb, res = _run(pairs, dev)
    for p, (ocost, opath) in enumerate(refs):
        cost, path, ln, _, _, _ = _pair_results(tb, res, p)
        assert np.array_equal(cost.numpy(), ocost), p
        assert ln == len(opath) and np.array_equal(path.numpy(), opath), p


def test_position_independence_and_determinism(dev):
    d24 = fbi.walk_batch(fbi.BATCH_D24, 24)
    target = d24[10]                                   # (130, 97)
    assert tuple(target[0].shape) == (130, 24) and tuple(target[1].shape) == (97, 24)
    first = (target, d24[2], d24[0], d24[8])
    last = (d24[11], d24[3], d24[7], d24[12], target)  # other neighbours, and unused rows between the pairs
    tb1, r1 = _run(first, dev)
    tb2, r2 = _run(last, dev, gap=3)
    assert tb2.v_row0[4] != tb1.v_row0[0] and tb2.cell_off[4] != tb1.cell_off[0]
    for x, y in zip(_pair_results(tb1, r1, 0), _pair_results(tb2, r2, 4)):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))
    _, r3 = _run(last, dev, gap=3)
    for k in r2:
        if k == "cost" or k == "path":      # between the pairs' slots these buffers hold whatever the allocator gave
            continue
        assert torch.equal(r2[k], r3[k]), k
    for p in range(len(last)):
        for x, y in zip(_pair_results(tb2, r2, p), _pair_results(tb2, r3, p)):
            assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


def test_many_small_pairs(dev):
    pairs, refs = fbi.small_batch(), fbi.oracle_batch("small")
    assert len(pairs) == 3000
    tb, res = _run(pairs, dev, keep_cost=False)
    assert tb.class_count == [3000, 0, 0]
    path_all, fused_all = res["path"].numpy(), res["fused"]
    lens = res["path_len"].numpy()
    assert lens.tolist() == [len(path) for _, path in refs]
    for p, ((v, a), (_, opath)) in enumerate(zip(pairs, refs)):
        n = v.shape[0]
        p0, r0 = int(tb.path_off[p]), int(tb.row_off[p])
        assert np.array_equal(path_all[p0:p0 + lens[p]], opath), p
        assert np.array_equal(res["rowcount"][r0:r0 + n].numpy(), np.bincount(opath[:, 0], minlength=n)), p
        assert torch.equal(fused_all[r0:r0 + n], ofu.interpolate_features(v, opath, n)), p


def test_no_host_synchronisation(dev):
    from avsum_amd import ops
    vcat, acat, table = fbi.layout(fbi.walk_batch(fbi.BATCH_D24, 24)[5:11])
    tb = ops.FusionTables(table, dev)
    vd, ad = vcat.to(dev), acat.to(dev)
    ops.fusion_batch(tb, vd, ad, 40)                 # (the target length's output offsets are uploaded once, here)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = ops.fusion_batch(tb, vd, ad, keep_cost=True)
        res40 = ops.fusion_batch(tb, vd, ad, 40)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert res["fused"].shape[0] == tb.rows and res40["fused"].shape[0] == sum(min(n, 40) for n in tb.n.tolist())
    assert int(res["path_len"].min()) >= 1


def test_refusals(dev):
    from avsum_amd import ops
    v, a = torch.zeros((10, 8), device=dev), torch.zeros((12, 8), device=dev)
    tb = ops.FusionTables([(0, 10, 0, 12)], dev)
    with pytest.raises(ValueError, match="6400"):
        ops.FusionTables([(0, 3, 0, 3), (3, 6401, 3, 5)], dev)
    for empty in ((0, 0, 0, 4), (0, 4, 0, 0)):
        with pytest.raises(ValueError, match="empty"):
            ops.FusionTables([(0, 3, 0, 3), empty], dev)
    with pytest.raises(ValueError, match="device"):
        ops.fusion_batch(tb, v.cpu(), a)
    with pytest.raises(ValueError, match="device"):
        ops.fusion_batch(tb, v, a.cpu())
    with pytest.raises(ValueError, match="float32"):
        ops.fusion_batch(tb, v.double(), a.double())
    with pytest.raises(ValueError, match="columns"):
        ops.fusion_batch(tb, v, torch.zeros((12, 9), device=dev))
    with pytest.raises(ValueError, match="rows"):       # a pair that reaches past the end of v
        ops.fusion_batch(tb, v[:9], a)
    from avsum_amd.features import fusion
    with pytest.raises(ValueError):
        fusion.fuse_batch([torch.zeros(0, 8)], [torch.zeros(3, 8)], 5)


def test_host_list_api(dev):
    from avsum_amd.features import fusion
    import features.fusion as root_fusion
    assert root_fusion.fuse_batch is fusion.fuse_batch and root_fusion.fuse_batch_device is fusion.fuse_batch_device
    d24 = fbi.walk_batch(fbi.BATCH_D24, 24)
    pairs = [d24[2], d24[11], d24[8]]                  # (33,31), (257,40), (5,9)
    got = fusion.fuse_batch([v for v, _ in pairs], [a.numpy() for _, a in pairs], 40)
    assert len(got) == 3
    for (v, a), g in zip(pairs, got):
        want = fusion.interpolate_features(v, fusion.compute_optimal_path(fusion.compute_dtw(v, a)), 40)
        assert not g.is_cuda and g.dtype == torch.float32 and torch.equal(g, want)
    # the device form, one set of offsets for both sides (the configs[2] layout: as many audio rows as visual rows)
    sq = fbi.walk_batch(fbi.BATCH_D512, 512)
    vcat, acat = torch.cat([v for v, _ in sq]).to(dev), torch.cat([a for _, a in sq]).to(dev)
    fused, off = fusion.fuse_batch_device(vcat, acat, [0, 200, 400, 600])
    assert fused.is_cuda and off.tolist() == [0, 200, 400, 600]
    for p, (v, a) in enumerate(sq):
        want = fusion.interpolate_features(v, fusion.compute_optimal_path(fusion.compute_dtw(v, a)), 200)
        assert torch.equal(fused[200 * p:200 * (p + 1)].cpu(), want)
