"""Batched evaluation on the GPU (ops.segment_mean_mask / ops.eval_counts / evaluation.metrics.*_device /
scripts.evaluate.evaluate_batch / FrameScoringPipeline.select_device): numpy's mean bit for bit, the ten integers
against the brute-force oracle exactly, the metrics against SciPy and against the per-video evaluate()."""
import warnings

import numpy as np
import pytest
import torch

import eval_batch_inputs as ebi

pytestmark = pytest.mark.gpu


def _quiet_reference(fn, *args):
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_segment_mean_mask_is_numpy_bitwise(dev, dtype):
    from avsum_amd import ops
    lens = [1, 7, 8, 9, 127, 128, 129, 255, 8192, 8193]
    rng = np.random.default_rng(3)
    x = (rng.random(3 + sum(lens) + 5) - 0.3).astype(dtype)
    x[3 + 1 + 7 + 8:3 + 1 + 7 + 8 + 9] = dtype(0.125)        # a constant segment: nothing exceeds its mean
    off = 3 + np.concatenate([[0], np.cumsum(lens)])          # unaligned: the first segment starts at element 3
    mean, mask = ops.segment_mean_mask(torch.from_numpy(x).to(dev), off.tolist())
    mean, mask = mean.cpu().numpy(), mask.cpu().numpy()
    assert mean.dtype == dtype and mask.dtype == np.uint8 and mask.shape == x.shape
    want_mask = np.zeros(x.shape, dtype=np.uint8)
    for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
        want = np.mean(x[a:b])
        assert mean[v].tobytes() == want.tobytes(), (lens[v], mean[v], want)
        want_mask[a:b] = x[a:b] > want
    assert np.array_equal(mask, want_mask)
    assert mask[:3].sum() == 0 and mask[-5:].sum() == 0      # rows outside every segment
    # offsets already on the device give the same
    mean2, mask2 = ops.segment_mean_mask(torch.from_numpy(x).to(dev), torch.from_numpy(off).to(dev))
    assert mean2.cpu().numpy().tobytes() == mean.tobytes() and np.array_equal(mask2.cpu().numpy(), mask)


def _counts(pairs, dev, first=0):
    from avsum_amd import ops
    pred, target, off = ebi.layout(pairs, first)
    tb = ops.EvalTables(off, dev)
    return ops.eval_counts(tb, torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev))


@pytest.mark.parametrize("tdtype", ["float32", "float64"])
def test_counts_equal_brute_force(dev, tdtype):
    pairs = list(ebi.count_batch(tdtype))
    got = _counts(pairs, dev, first=5)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(pairs), 10)
    got = got.cpu().numpy()
    want = ebi.count_batch_oracle(tdtype)
    for v, (t, levels, kind) in enumerate(ebi.COUNT_BATCH):
        assert got[v].tolist() == want[v].tolist(), (t, levels, kind)
    # the special videos are what they claim to be: all pairs tied in y / in x, and equal signed zeros
    tied, const = ebi.COUNT_BATCH.index((300, 5, "tied_target")), ebi.COUNT_BATCH.index((301, 81, "const_pred"))
    assert got[tied, ebi.EY] == 300 * 300 and got[tied, ebi.NTGT] == 0 and got[tied, ebi.S2] == 0
    assert got[const, ebi.EX] == 301 * 301 and got[const, ebi.NPRED] == 0
    # V = 1 alone, and a second call on the same input: identical bytes
    for v in (0, 7):
        assert _counts([pairs[v]], dev).cpu().numpy().tolist() == [want[v].tolist()]
    assert _counts(pairs, dev, first=5).cpu().numpy().tobytes() == got.tobytes()


def test_metrics_equal_reference_on_count_batch(dev):
    from avsum_amd.evaluation.metrics import binary_f1, metrics_from_counts, summarize_scores, summarize_scores_device
    from scipy.stats import kendalltau, spearmanr
    pairs = list(ebi.count_batch("float32"))
    per = metrics_from_counts(_counts(pairs, dev).cpu().numpy())
    for v, (p, t) in enumerate(pairs):
        f1 = _quiet_reference(binary_f1, p, t)
        rho = _quiet_reference(lambda: spearmanr(p, t).correlation)
        tau = _quiet_reference(lambda: kendalltau(p, t).correlation)
        assert np.array_equal(per["f1"][v], f1, equal_nan=True), v
        for mine, ref in ((per["spearman"][v], rho), (per["kendall"][v], tau)):
            assert np.isnan(mine) == np.isnan(ref), v
            assert np.isnan(ref) or abs(mine - ref) <= 1e-12, v
    # the summary over the videos without a NaN, and NaN in the same places with them
    plain = [pr for pr, (_, _, kind) in zip(pairs, ebi.COUNT_BATCH) if kind not in ("tied_target", "const_pred")]
    for sub in (plain, pairs):
        pred, target, off = ebi.layout(sub)
        got = summarize_scores_device(torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev), off)
        want = _quiet_reference(summarize_scores, sub)
        assert set(got) == set(want) == {"f1", "spearman", "kendall"}
        for key in want:
            assert np.isnan(got[key]) == np.isnan(want[key]), key
            assert np.isnan(want[key]) or abs(got[key] - want[key]) <= 1e-12, key
        assert np.array_equal(got["f1"], want["f1"], equal_nan=True)


def test_long_videos(dev):
    """T = 5000 and T = 8193 (float64 targets): the pair sums against SciPy-derived values, the masks against numpy."""
    from avsum_amd.evaluation.metrics import binary_f1, metrics_from_counts
    from scipy.stats import kendalltau, spearmanr
    pairs = list(ebi.long_videos())
    got = _counts(pairs, dev).cpu().numpy()
    per = metrics_from_counts(got)
    for v, (p, t) in enumerate(pairs):
        s2, ex, ey = ebi.scipy_pair_sums(p, t)
        mx, my = p > np.mean(p), t > np.mean(t)
        assert got[v, [ebi.T_, ebi.S2, ebi.EX, ebi.EY]].tolist() == [len(p), s2, ex, ey]
        assert got[v, [ebi.NPRED, ebi.NTGT, ebi.TP]].tolist() == [mx.sum(), my.sum(), (mx & my).sum()]
        assert per["f1"][v] == binary_f1(p, t)
        assert abs(per["spearman"][v] - spearmanr(p, t).correlation) <= 1e-12
        assert abs(per["kendall"][v] - kendalltau(p, t).correlation) <= 1e-12


class _Videos:
    """Seeded synthetic dataset in the reference's item form: ({"visual": [T, 4096], "audio": [T, 296]}, scores [T])."""

    def __init__(self, lengths, seed):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for t in lengths:
            feats = {"visual": torch.randn(t, 4096, generator=g), "audio": torch.randn(t, 296, generator=g)}
            scores = torch.floor(torch.rand(t, generator=g) * 5) / 5          # float32, five levels: ties
            self.items.append((feats, scores))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_evaluate_batch_equals_evaluate(dev):
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.evaluate import evaluate, evaluate_batch
    torch.manual_seed(7)
    model = AVBiLSTMModel().eval().to(dev)
    data = _Videos([20, 400, 137, 256, 57, 301], seed=17)
    want = evaluate(model, data)
    got = evaluate_batch(model, data)
    assert set(got) == set(want) == {"f1", "spearman", "kendall"}
    print("evaluate:", want, "evaluate_batch:", got)
    assert np.isfinite(want["f1"]) and got["f1"] == want["f1"]
    assert abs(got["spearman"] - want["spearman"]) <= 1e-12
    assert abs(got["kendall"] - want["kendall"]) <= 1e-12


def test_select_device_equals_select(dev):
    from avsum_amd.pipeline import FrameScoringPipeline
    lens = [1, 5, 300, 129, 2000]
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    rng = np.random.default_rng(9)
    scores = torch.from_numpy(rng.random(off[-1]).astype(np.float32)).to(dev)
    sel = FrameScoringPipeline.select(scores, off)
    mask = FrameScoringPipeline.select_device(scores, off)
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (off[-1],)
    mask = mask.cpu().numpy()
    for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.array_equal(np.flatnonzero(mask[a:b]), sel[v]), v
