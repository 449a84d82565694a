"""Pins the oracle (CPU restatement) against the golden fixtures generated from the reference's own classes and
functions by tests/golden/make_golden.py."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import fusion as ofu, scorer as osc, selection as osel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _sd(z, prefix="sd_"):
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def test_scorer_small_golden():
    z = np.load(os.path.join(GOLD, "scorer_small.npz"))
    sd = _sd(z)
    assert len(sd) == 28
    for name in ("b1", "b3", "t1"):
        out = osc.av_bilstm_forward(sd, torch.from_numpy(z[name + "_visual"]), torch.from_numpy(z[name + "_audio"]))
        ref = torch.from_numpy(z[name + "_out"])
        assert out.shape == ref.shape  # squeeze rules: [37], [3,11], []
        assert (out - ref).abs().max().item() < 1e-6


def _hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_scorer_full_golden_and_construction_order():
    """The mirror class built under the same seed must reproduce the reference's parameters bit for bit
    (same sub-modules, same construction order) and the same 28 state-dict keys."""
    from avsum_amd.models.av_model import AVBiLSTMModel
    z = np.load(os.path.join(GOLD, "scorer_full.npz"))
    torch.manual_seed(int(z["seed"]))
    m = AVBiLSTMModel().eval()
    sd = m.state_dict()
    assert sorted(sd.keys()) == list(z["keys"])
    assert sum(p.numel() for p in m.parameters()) == int(z["n_params"]) == 9667713
    assert _hash(sd) == str(z["sd_sha256"])
    v = torch.randn(1, 300, 4096, generator=torch.Generator().manual_seed(int(z["input_seed"])))
    out = osc.av_bilstm_forward(sd, v, torch.zeros(1, 300, 296))
    assert (out - torch.from_numpy(z["out"])).abs().max().item() < 1e-6


@pytest.mark.parametrize("t_len", [1800, 5000])
def test_scorer_long_golden(t_len):
    """configs[1] / configs[3] sequence lengths: the oracle's recurrences over 1800 and 5000 steps against the scores the
    reference class (models/av_model.py:6-46) produced for the same seeded parameters and input."""
    from avsum_amd.models.av_model import AVBiLSTMModel
    z = np.load(os.path.join(GOLD, "scorer_long.npz"))
    torch.manual_seed(int(z["seed"]))
    sd = AVBiLSTMModel().eval().state_dict()
    assert _hash(sd) == str(z["sd_sha256"])
    v = torch.randn(1, t_len, 4096, generator=torch.Generator().manual_seed(int(z[f"t{t_len}_input_seed"])))
    out = osc.av_bilstm_forward(sd, v, torch.zeros(1, t_len, 296))
    ref = torch.from_numpy(z[f"t{t_len}_out"])
    assert out.shape == ref.shape == (t_len,)
    assert (out - ref).abs().max().item() < 1e-6


def test_mhsa_long_golden():
    """MultiHeadSelfAttention(1024, 4) at T = 5000 (models/attention.py:15-25): 64 stored output rows of the reference
    class + the absolute sum of the whole output."""
    from avsum_amd.models.attention import MultiHeadSelfAttention
    z = np.load(os.path.join(GOLD, "mhsa_long.npz"))
    torch.manual_seed(int(z["seed"]))
    sd = MultiHeadSelfAttention(1024, 4).eval().state_dict()
    assert _hash(sd) == str(z["sd_sha256"])
    x = torch.randn(1, int(z["t"]), 1024, generator=torch.Generator().manual_seed(int(z["input_seed"])))
    out = osc.mhsa_forward(sd, x, 4)
    assert (out[0, z["rows"]] - torch.from_numpy(z["out_rows"])).abs().max().item() < 1e-6
    assert abs(float(out.double().abs().sum()) / float(z["out_abs_sum"]) - 1) < 1e-6


def test_mhsa_golden_and_keys():
    from avsum_amd.models.attention import MultiHeadSelfAttention
    z = np.load(os.path.join(GOLD, "mhsa_small.npz"))
    sd = _sd(z)
    torch.manual_seed(99)
    assert sorted(MultiHeadSelfAttention(64, 4).state_dict().keys()) == sorted(sd.keys())
    out = osc.mhsa_forward(sd, torch.from_numpy(z["x"]), 4)
    assert (out - torch.from_numpy(z["out"])).abs().max().item() < 1e-6


def test_fusion_metrics_golden():
    z = np.load(os.path.join(GOLD, "fusion_metrics.npz"))
    v, a = torch.from_numpy(z["v"]), torch.from_numpy(z["a"])
    cost = ofu.compute_dtw(v, a)
    assert cost.dtype == np.float64 and np.array_equal(cost, z["cost"])
    interp = ofu.interpolate_features(v, z["path"], 3)
    assert str(interp.dtype) == str(z["interp_dtype"]) and np.array_equal(interp.numpy(), z["interp"])
    al = osel.align_shots([(0, 50), (60, 200), (10, 11)], z["ann"], 30)
    assert np.array_equal(al.numpy(), z["align"])
    assert osel.compute_temporal_f1([(0, 10), (20, 30)], [(5, 15), (20, 25)], 30) == float(z["tf1"])
    assert abs(float(z["tf1"]) - 0.5714285665) < 1e-9  # SURVEY A.10 probe


def test_against_reference_classes_directly():
    """The oracle against what the reference's classes and functions computed when they were run directly
    (tests/golden/make_golden.py imports them and stores their inputs, parameters and outputs: reference_classes.npz)."""
    z = np.load(os.path.join(GOLD, "reference_classes.npz"))
    sd = _sd(z)
    for b, t in ((1, 50), (4, 9), (2, 1)):
        v, a = torch.from_numpy(z[f"fwd_{b}x{t}_visual"]), torch.from_numpy(z[f"fwd_{b}x{t}_audio"])
        ref = torch.from_numpy(z[f"fwd_{b}x{t}_out"])
        out = osc.av_bilstm_forward(sd, v, a)
        assert out.shape == ref.shape and (out - ref).abs().max().item() < 1e-6
    # backward: torch autograd through the restatement == autograd through the reference module
    vg, ag = torch.from_numpy(z["bwd_visual"]), torch.from_numpy(z["bwd_audio"])
    params = {k: p.clone().requires_grad_(True) for k, p in sd.items()}
    ones = torch.ones(13, 16)
    grads = torch.autograd.grad(osc.av_bilstm_forward_train(params, vg, ag, ones, ones).sum(), list(params.values()),
                                allow_unused=True)
    assert sorted(params) == sorted(k[len("grad_"):] for k in z.files if k.startswith("grad_"))
    for (k, p), gr in zip(params.items(), grads):
        want = torch.from_numpy(z["grad_" + k])
        got = gr if gr is not None else torch.zeros_like(p)
        assert (got - want).abs().max().item() < 1e-6, k
    x = torch.from_numpy(z["mhsa_x"])
    assert (osc.mhsa_forward(_sd(z, "mhsa_sd_"), x, 6) - torch.from_numpy(z["mhsa_out"])).abs().max().item() < 1e-6
    vv, aa = torch.from_numpy(z["dtw_v"]), torch.from_numpy(z["dtw_a"])
    assert np.array_equal(ofu.compute_dtw(vv, aa), z["dtw_cost"])
    _, path = ofu.dtw_path(ofu.compute_dtw(vv, aa))
    assert np.array_equal(np.asarray(path), z["dtw_path"])
    assert torch.equal(ofu.interpolate_features(vv, path, 9), torch.from_numpy(z["interp"]))
    segs = ([(0, 10), (20, 30)], [(5, 15), (20, 25)])
    assert osel.compute_temporal_f1(*segs, 30) == float(z["temporal_f1"]) == float(z["shot_f1"])
    # the metric block of scripts/evaluate.py:21-42 (its model loop needs .cuda(); restated lines only)
    rng = np.random.default_rng(0)
    preds = [rng.random(40).astype(np.float32) for _ in range(3)]
    tgts = [rng.random(40).astype(np.float32) for _ in range(3)]
    from scipy.stats import kendalltau, spearmanr
    f1 = []
    for p, t in zip(preds, tgts):
        bp, bt = (p > np.mean(p)).astype(int), (t > np.mean(t)).astype(int)
        tp = np.logical_and(bp, bt).sum()
        pr, rc = tp / bp.sum(), tp / bt.sum()
        f1.append(2 * (pr * rc) / (pr + rc + 1e-8))
    got = osel.evaluate_metrics(preds, tgts)
    assert got["f1"] == np.mean(f1)
    assert got["spearman"] == np.mean([spearmanr(p, t).correlation for p, t in zip(preds, tgts)])
    assert got["kendall"] == np.mean([kendalltau(p, t).correlation for p, t in zip(preds, tgts)])


def test_dtw_path_is_optimal_bruteforce():
    """Pins the exact-DTW restatement (fastdtw itself is absent): on small matrices the returned path must be
    a valid warping path whose cost equals the minimum over ALL warping paths, and ties follow up/left/diag."""
    rng = np.random.default_rng(5)

    def all_paths(n, m):
        def rec(i, j):
            if i == n - 1 and j == m - 1:
                yield [(i, j)]
                return
            for di, dj in ((1, 0), (0, 1), (1, 1)):
                if i + di < n and j + dj < m:
                    for rest in rec(i + di, j + dj):
                        yield [(i, j)] + rest
        return rec(0, 0)

    for n, m in ((1, 1), (1, 5), (4, 1), (4, 5), (5, 4)):
        c = rng.random((n, m))
        total, path = ofu.dtw_path(c)
        best = min(sum(c[i, j] for i, j in p) for p in all_paths(n, m))
        assert abs(total - best) < 1e-12
        assert abs(sum(c[i, j] for i, j in path) - total) < 1e-12
        assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n - 1, m - 1)
        d = np.diff(path, axis=0)
        assert ((d >= 0) & (d <= 1)).all() and (d.sum(1) >= 1).all()
    # all-zero costs: every predecessor ties; "up" (i-1, j) is preferred at every cell, so walking back from
    # (2,2) climbs column 2 first: the path runs along row 0, then down the last column
    _, p = ofu.dtw_path(np.zeros((3, 3)))
    assert p.tolist() == [[0, 0], [0, 1], [0, 2], [1, 2], [2, 2]]
