"""Kernel temporal segmentation on the GPU (ops.kts_gram / kts_segment, features.kts.kts_batch_device): the Gram matrix
within the derived fp64 bound of the exact one, and everything after it - scatter tables, dynamic programme, model
selection, backtrack, shot table - equal to the numpy oracle run on the device's own K, the costs bit for bit."""
import numpy as np
import pytest
import torch

import kts_inputs as kin

pytestmark = pytest.mark.gpu


def _strided(x, dev):
    """x fp32 [N, D] on the device as a view with row pitch D + 3 that starts one element into its buffer."""
    n, d = x.shape
    base = torch.full((n * (d + 3) + 1,), 7.0, dtype=torch.float32, device=dev)
    view = base[1:].view(n, d + 3)[:, :d]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == d + 3
    return view


def _blocks(plan, gram):
    flat = gram.cpu().numpy()
    return [flat[plan.k_offsets[v]:plan.k_offsets[v + 1]].reshape(int(plan.n[v]), int(plan.n[v]))
            for v in range(plan.nvideos)]


def _expected(plan, blocks, select):
    """The tables kts_segment must give, from the numpy oracle on the given K blocks."""
    from avsum_amd.features.kts import cpd_auto_host
    nv, cap = plan.nvideos, plan.shot_cap
    cps_all = np.full(cap, -1, dtype=np.int64)
    costs, scores = np.zeros(cap), np.zeros(cap)
    totals, shots = np.zeros((nv, 4), dtype=np.int64), []
    for v in range(nv):
        cps, c, s, flag = cpd_auto_host(blocks[v], int(plan.ncp[v]), plan.vmax, plan.lmin, select)
        c0 = int(plan.cost_offsets[v])
        assert c.shape == (int(plan.m_max[v]) + 1,)
        cps_all[c0:c0 + cps.size] = cps
        costs[c0:c0 + c.size], scores[c0:c0 + c.size] = c, s
        totals[v] = (cps.size, plan.n[v], plan.m_max[v], flag)
        shots += plan.shots_of(v, cps)
    table = np.zeros((cap, 2), dtype=np.int64)
    table[:len(shots)] = shots
    return {"change_points": cps_all, "shot_offsets": kin.offsets_of(totals[:, 0] + 1), "shots": table, "totals": totals,
            "costs": costs, "scores": scores}


def _assert_equal(out, want):
    for name in ("change_points", "shot_offsets", "shots", "totals"):
        got = out[name].cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want[name]), name
    for name in ("costs", "scores"):                       # as fp64 bit patterns
        got = out[name].cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want[name].view(np.int64)), name


# --------------------------------------------------------------------------- the Gram matrix
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("d", [1, 20, 67])
def test_gram_is_within_the_fp64_bound_symmetric_and_batch_independent(dev, d, stride):
    from avsum_amd import ops
    lengths = kin.gram_lengths(stride)
    assert stride == 1 or all(n % 3 for n in lengths)
    off = kin.offsets_of(lengths)
    x = kin.random_features(int(off[-1]), d, seed=20 + d)
    plan = ops.KtsTables(off, stride, device=dev)
    assert plan.n.tolist() == list(kin.GRAM_SAMPLES)
    blocks = _blocks(plan, ops.kts_gram(plan, _strided(x, dev)))
    for v, k in enumerate(blocks):
        xs = x[off[v]:off[v + 1]:stride]
        a = np.abs(xs.astype(np.float64))
        err, bound = np.abs(k - kin.exact_gram(xs)), d * 2.0 ** -52 * (a @ a.T)
        print(f"video {v}: max |K - K_exact| = {err.max():.3e}, least slack = {(bound - err).min():.3e}")
        assert (err <= bound).all()
        assert np.array_equal(k.view(np.int64), k.T.view(np.int64))           # symmetric to the bit
        alone = ops.KtsTables([0, lengths[v]], stride, device=dev)
        again = _blocks(alone, ops.kts_gram(alone, _strided(x[off[v]:off[v + 1]], dev)))[0]
        assert np.array_equal(again.view(np.int64), k.view(np.int64))         # the same alone as inside the batch


def test_gram_of_integer_features_is_exact(dev):
    from avsum_amd import ops
    lengths = kin.gram_lengths(3)
    off = kin.offsets_of(lengths)
    x = kin.integer_features(int(off[-1]), 67)
    plan = ops.KtsTables(off, 3, device=dev)
    for v, k in enumerate(_blocks(plan, ops.kts_gram(plan, _strided(x, dev)))):
        x64 = x[off[v]:off[v + 1]:3].astype(np.float64)
        assert np.array_equal(k, x64 @ x64.T)


# --------------------------------------------------------------------------- everything after K, bit for bit
@pytest.fixture(scope="module")
def dp_batch(dev):
    """The batch n = 1, 2, 9, 33, 160, 1100 at stride 1 and the device's own K, downloaded once."""
    from avsum_amd import ops
    x, lengths = kin.dp_batch()
    feats = torch.from_numpy(x).to(dev)
    plans = {lmin: ops.KtsTables(kin.offsets_of(lengths), 1, list(kin.DP_NCP), 1.0, lmin, device=dev) for lmin in (1, 3)}
    gram = ops.kts_gram(plans[1], feats)
    return {"plans": plans, "gram": gram, "blocks": _blocks(plans[1], gram), "lengths": lengths}


@pytest.mark.parametrize("select", ["auto", "fixed"])
@pytest.mark.parametrize("lmin", [1, 3])
def test_segmentation_equals_the_oracle_on_the_device_gram(dp_batch, lmin, select):
    from avsum_amd import ops
    plan = dp_batch["plans"][lmin]
    assert plan.m_max.tolist() == ([0, 1, 8, 32, 159, 12] if lmin == 1 else [0, 0, 2, 10, 52, 12])
    out = ops.kts_segment(plan, dp_batch["gram"], select)
    want = _expected(plan, dp_batch["blocks"], select)
    _assert_equal(out, want)
    assert not want["totals"][:, 3].any()
    if select == "auto" and lmin == 1:       # the planted structure is what comes out
        c0 = plan.cost_offsets
        for v, segs in kin.DP_PLANTED.items():
            m = int(want["totals"][v, 0])
            assert want["change_points"][c0[v]:c0[v] + m].tolist() == np.cumsum(segs)[:-1].tolist()


def test_tie_order_on_constant_features(dev):
    """Features of ones: K = D exactly, every J is exactly 0 and every segmentation ties; the smallest t wins."""
    from avsum_amd.features.kts import kts_batch_device
    feats = torch.ones((23 + 40, 8), dtype=torch.float32, device=dev)
    result = kts_batch_device(feats, [0, 23, 63], stride=1, ncp=4, lmin=3, select="fixed")
    assert (result.gram == 8.0).all()
    host = result.host()
    assert host[0]["change_points"].tolist() == [3, 6, 9, 12] == host[1]["change_points"].tolist()
    assert host[0]["shots"] == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 23)]
    assert (result.scores == 0.0).all()
    _assert_equal({k: getattr(result, k) for k in ("change_points", "shot_offsets", "shots", "totals", "costs", "scores")},
                  _expected(result.plan, _blocks(result.plan, result.gram), "fixed"))


def test_largest_configuration(dev):
    """One video of 2048 samples: both LDS rows full, the upper triangle of 32 x 32 Gram tiles, more rows than a workgroup has threads."""
    from avsum_amd.features.kts import kts_batch_device
    x = kin.planted((700, 600, 748), 32, seed=4)
    result = kts_batch_device(torch.from_numpy(x).to(dev), [0, 2048], stride=1, ncp=3)
    plan = result.plan
    assert plan.max_n == 2048 and plan.m_max.tolist() == [3] and plan.ntiles == 32 * 33 // 2
    want = _expected(plan, _blocks(plan, result.gram), "auto")
    _assert_equal({k: getattr(result, k) for k in want}, want)
    assert result.host()[0]["change_points"].tolist() == [700, 1300]
    assert result.host()[0]["shots"] == [(0, 700), (700, 1300), (1300, 2048)]


# --------------------------------------------------------------------------- end to end
E2E_SEGMENTS = ((150, 300, 232), (90, 60, 120, 97), (240, 203))


@pytest.fixture(scope="module")
def e2e(dev):
    from avsum_amd.features.kts import kts_batch_device, kts_host
    videos = [kin.planted(segs, 64, seed=30 + v) for v, segs in enumerate(E2E_SEGMENTS)]
    lengths = [len(x) for x in videos]
    off = kin.offsets_of(lengths)
    feats = torch.from_numpy(np.concatenate(videos)).to(dev)
    result = kts_batch_device(feats, off, stride=15, ncp=8)
    return {"videos": videos, "lengths": lengths, "offsets": off, "result": result, "feats": feats,
            "host": [kts_host(x, 15, 8) for x in videos]}


def test_end_to_end_equals_kts_host(e2e):
    """Against numpy's own K: legitimate because the planted cost gaps (asserted) dwarf the 1e-13 differences of K."""
    got = e2e["result"].host()
    assert [len(h["shots"]) for h in got] == [3, 4, 2]
    for v, (cps, shots, costs, flag) in enumerate(e2e["host"]):
        ordered = np.sort(costs)
        assert ordered[1] - ordered[0] >= 2e-3, (v, ordered[:3])
        assert cps.tolist() == [b // 15 for b in np.cumsum(E2E_SEGMENTS[v])[:-1]]
        assert got[v]["change_points"].tolist() == cps.tolist() and got[v]["shots"] == shots and got[v]["flag"] == flag == 0
        assert got[v]["costs"].shape == costs.shape and np.allclose(got[v]["costs"], costs, rtol=0, atol=1e-10)
        assert shots[-1][1] == e2e["lengths"][v]


def test_keyshot_summaries_take_the_kts_result(e2e, dev):
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device, keyshot_summary_host
    from avsum_amd.pipeline import FrameScoringPipeline
    off, result = e2e["offsets"], e2e["result"]
    rows = np.random.default_rng(9).random((2, int(off[-1])), dtype=np.float32)
    scores = torch.from_numpy(rows).to(dev)
    lists = result.shot_lists()
    # half of a video: the planted segments are long, at the default 0.15 none of them would fit
    on_device = keyshot_summaries_device(scores, off, result, ratio=0.5)
    from_lists = FrameScoringPipeline.summarize_device(scores, off, lists, ratio=0.5)
    nshots = sum(len(s) for s in lists)
    assert on_device.plan.shot_cap == result.shot_cap and on_device.shots is result.shots
    assert torch.equal(on_device.mask, from_lists.mask) and torch.equal(on_device.totals, from_lists.totals)
    assert torch.equal(on_device.optimum, from_lists.optimum)
    assert torch.equal(on_device.picked[:, :nshots], from_lists.picked[:, :nshots])
    assert on_device.host() == from_lists.host()
    mask, optimum = on_device.mask.cpu().numpy(), on_device.optimum.cpu().numpy()
    for k in range(2):
        for v in range(3):
            _, want_mask, want_opt = keyshot_summary_host(rows[k, off[v]:off[v + 1]], lists[v], e2e["lengths"][v], 0.5)
            assert np.array_equal(mask[k, off[v]:off[v + 1]], want_mask) and optimum[k, v] == want_opt
    assert all(mask[k, off[v]:off[v + 1]].any() for k in range(2) for v in range(3))
    with pytest.raises(ValueError, match="other video offsets"):
        keyshot_summaries_device(scores, [0, int(off[-1])], result)
    again = FrameScoringPipeline.segment_device(e2e["feats"], off, stride=15, ncp=8)
    assert torch.equal(again.shots, result.shots) and torch.equal(again.costs, result.costs)


def test_a_nan_row_flags_its_video_alone(e2e, dev):
    from avsum_amd.features.kts import kts_batch_device
    off, clean = e2e["offsets"], e2e["result"]
    feats = e2e["feats"].clone()
    feats[int(off[1]) + 45, 3] = float("nan")                  # frame 45 = sample 3 of video 1
    result = kts_batch_device(feats, off, stride=15, ncp=8)
    totals = result.totals.cpu().numpy()
    assert totals[:, 3].tolist() == [0, 1, 0] and totals[1, 0] == 0
    got, want = result.host(), clean.host()
    assert got[1]["shots"] == [(0, e2e["lengths"][1])] and got[1]["change_points"].size == 0 and got[1]["flag"] == 1
    plan = result.plan
    for v in (0, 2):
        assert got[v]["shots"] == want[v]["shots"] and got[v]["change_points"].tolist() == want[v]["change_points"].tolist()
        assert np.array_equal(got[v]["costs"].view(np.int64), want[v]["costs"].view(np.int64))
        a, b = int(plan.k_offsets[v]), int(plan.k_offsets[v + 1])
        assert torch.equal(result.gram[a:b].view(torch.int64), clean.gram[a:b].view(torch.int64))
    assert result.shot_offsets.cpu().tolist() == [0, 3, 4, 6]


# --------------------------------------------------------------------------- argument checks
def test_arguments_are_checked_before_any_launch(dev):
    from avsum_amd import ops
    from avsum_amd.features.kts import kts_batch_device
    feats = torch.zeros((40, 6), dtype=torch.float32, device=dev)
    plan = ops.KtsTables([0, 17, 40], 2, device=dev)
    gram = torch.zeros(plan.k_entries, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="kts_batch_device"):
        kts_batch_device(feats.cpu(), [0, 17, 40])
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram(plan, feats.cpu())
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram(plan, feats.double())
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram(plan, feats[:39])                                  # the offsets end at 40
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram(plan, feats.t().contiguous().t())                  # column stride 40
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram(ops.KtsTables([0, 17, 40], 2, device="cpu"), feats)
    with pytest.raises(ValueError, match="kts_gram"):
        ops.kts_gram([0, 17, 40], feats)
    with pytest.raises(ValueError, match="KtsTables"):
        kts_batch_device(feats, [0, 17, 41, 40])
    with pytest.raises(ValueError, match="kts_segment"):
        ops.kts_segment(plan, gram.cpu())
    with pytest.raises(ValueError, match="kts_segment"):
        ops.kts_segment(plan, gram.float())
    with pytest.raises(ValueError, match="kts_segment"):
        ops.kts_segment(plan, gram[:-1])
    with pytest.raises(ValueError, match="select"):
        ops.kts_segment(plan, gram, select="best")
