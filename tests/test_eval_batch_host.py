"""Batched evaluation on the host: numpy's reduction order written out and pinned to the installed numpy, the host finish
(metrics_from_counts) on brute-force counts against binary_f1 and SciPy, the table builder (ops.EvalTables on
device="cpu") and the argument checks of the C entries (they return before any launch).  No GPU needed."""
import warnings

import numpy as np
import pytest

import eval_batch_inputs as ebi

ARG, SHAPE = -1, -2   # AVS_E_ARG, AVS_E_SHAPE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_order_mean_is_np_mean_bitwise(dtype):
    """The order the segment-mean kernel implements IS the installed numpy's, float32 and float64."""
    for n in list(range(1, 301)) + [8191, 8192, 8193, 16385, 20000]:
        for seed in range(3):
            a = (np.random.default_rng([seed, n]).random(n) - 0.3).astype(dtype)
            got, want = ebi.mean_numpy_order(a), np.mean(a)
            assert got.dtype == want.dtype == dtype and got.tobytes() == want.tobytes(), (n, seed)


def test_numpy_mean_is_not_the_rounded_mean():
    """Why the order matters: numpy's fp32 mean differs from the correctly rounded one often enough to move a mask."""
    differ = 0
    for seed in range(200):
        a = np.random.default_rng(seed).random(1800).astype(np.float32)
        differ += np.mean(a) != np.float32(a.astype(np.float64).sum() / 1800)
    assert differ > 0


def _reference(pred, target):
    from avsum_amd.evaluation.metrics import binary_f1
    from scipy.stats import kendalltau, spearmanr
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        return binary_f1(pred, target), spearmanr(pred, target).correlation, kendalltau(pred, target).correlation


HOST_CASES = [(2, 5, None, np.float32), (3, 81, None, np.float32), (65, 5, None, np.float64), (65, 81, "zeros", np.float32),
              (1800, 81, None, np.float32), (1800, 5, None, np.float64), (65, 5, "tied_target", np.float32),
              (65, 81, "const_pred", np.float32)]


@pytest.mark.parametrize("t,levels,kind,tdtype", HOST_CASES)
def test_metrics_from_brute_force_counts(t, levels, kind, tdtype):
    from avsum_amd.evaluation.metrics import metrics_from_counts
    pred, target = ebi.video(21, t, levels, tdtype=tdtype, kind=kind)
    if t > 3 and kind is None:
        assert len(np.unique(pred)) < t and len(np.unique(target)) < t     # ties on both sides
    counts = ebi.brute_counts(pred, target)
    assert counts[ebi.T_] == t and counts[ebi.S2] % 2 == 0 and (counts[ebi.EX] - t) % 2 == 0
    got = metrics_from_counts(counts[None, :])
    f1, rho, tau = _reference(pred, target)
    assert got["f1"].dtype == np.float64 and got["f1"].shape == (1,)
    assert np.array_equal(got["f1"][0], f1, equal_nan=True)
    for mine, ref in ((got["spearman"][0], rho), (got["kendall"][0], tau)):
        assert np.isnan(mine) == np.isnan(ref)
        if not np.isnan(ref):
            assert abs(mine - ref) <= 1e-12
    if kind == "tied_target":
        assert np.isnan(got["f1"][0]) and np.isnan(got["spearman"][0]) and np.isnan(got["kendall"][0])
    if kind == "const_pred":
        assert np.isnan(got["f1"][0]) and np.isnan(got["spearman"][0]) and np.isnan(got["kendall"][0])


def test_summary_has_nan_where_summarize_scores_has():
    from avsum_amd.evaluation.metrics import metrics_from_counts, summarize_scores
    for kinds in ((None, None), (None, "tied_target"), ("const_pred", None)):
        pairs = [ebi.video(31 + k, 65 + k, 5, kind=kind) for k, kind in enumerate(kinds)]
        with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
            warnings.simplefilter("ignore")
            want = summarize_scores(pairs)
        per = metrics_from_counts(ebi.brute_counts_batch(pairs))
        for key in ("f1", "spearman", "kendall"):
            got = np.mean(per[key])
            assert np.isnan(got) == np.isnan(want[key]), (kinds, key)
            if not np.isnan(got):
                assert abs(got - want[key]) <= 1e-12


def test_metrics_from_counts_refuses_other_tables():
    from avsum_amd.evaluation.metrics import metrics_from_counts
    with pytest.raises(ValueError):
        metrics_from_counts(np.zeros((3, 9), dtype=np.int64))
    with pytest.raises(ValueError):
        metrics_from_counts(np.zeros((3, 10), dtype=np.float64))
    assert metrics_from_counts(np.zeros((0, 10), dtype=np.int64))["f1"].shape == (0,)


def test_scipy_pair_sums_agree_with_brute_force():
    """The SciPy-derived S2 / E_x / E_y the long GPU videos are checked against, on a video short enough for the table."""
    pred, target = ebi.video(41, 700, 5, tdtype=np.float64)
    c = ebi.brute_counts(pred, target)
    assert ebi.scipy_pair_sums(pred, target) == (c[ebi.S2], c[ebi.EX], c[ebi.EY])


def test_tables_tiles_and_max_t():
    from avsum_amd import ops
    assert ops.EVAL_TILE == ebi.TILE and ops.EVAL_CHUNK == ebi.CHUNK
    # five videos after 7 rows of filler: 2, 256, 257, 1800 and 3 rows
    off = [7, 9, 265, 522, 2322, 2325]
    tb = ops.EvalTables(off, "cpu")
    assert tb.nvideos == 5 and tb.rows == 2325 and tb.max_t == 1800
    assert tb.lengths.tolist() == [2, 256, 257, 1800, 3]
    assert tb.ntiles == 1 + 1 + 2 + 8 + 1 and tb.tiles.dtype == np.int32 and tb.tiles.shape == (13, 2)
    assert tb.tiles.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1]] + [[3, k] for k in range(8)] + [[4, 0]]
    assert tb.offsets_t.dtype.is_floating_point is False and tb.offsets_t.tolist() == off
    assert tb.tiles_t.numpy().tolist() == tb.tiles.tolist()
    # every row of every video is owned by exactly one thread of one tile
    for v, t in enumerate(tb.lengths):
        tiles = tb.tiles[tb.tiles[:, 0] == v][:, 1]
        assert tiles.tolist() == list(range(-(-int(t) // ebi.TILE)))


def test_tables_refusals_and_empty_batch():
    from avsum_amd import ops
    ops.EvalTables([0, 2, 32770], "cpu")                                  # T = 2 and T = 32768 are the limits
    for bad, word in (([0, 1], "at least 2"), ([0, 5, 5], "at least 2"), ([0, 32769], "32768"), ([0, 10, 8], "decrease"),
                      ([(1 << 31) - 10, (1 << 31) + 10], "2^31"), ([-2, 5], "negative"), ([], "V + 1")):
        with pytest.raises(ValueError, match=word.replace("^", r"\^").replace("+", r"\+")):
            ops.EvalTables(bad, "cpu")
    empty = ops.EvalTables([0], "cpu")
    assert empty.nvideos == 0 and empty.rows == 0 and empty.ntiles == 0 and empty.max_t == 0 and empty.tiles.shape == (0, 2)


def test_ops_refuse_host_tensors():
    import torch
    from avsum_amd import ops
    from avsum_amd.evaluation.metrics import select_mask_device
    tb = ops.EvalTables([0, 4], "cpu")
    x = torch.zeros(4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.eval_counts(tb, x, x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.segment_mean_mask(x, [0, 4])
    with pytest.raises(ValueError, match="no CPU fallback"):
        select_mask_device(x, [0, 4])
    with pytest.raises(ValueError, match="EvalTables"):
        ops.eval_counts([0, 4], x, x)
    assert {"EvalTables", "eval_counts", "segment_mean_mask"} <= set(ops.__all__)


def test_evaluate_batch_refuses_other_target_dtypes():
    import torch
    from avsum_amd.scripts.evaluate import evaluate_batch

    class Model:
        def eval(self):
            return self

    feats = {"visual": torch.zeros(4, 8), "audio": torch.zeros(4, 3)}
    for dtype, name in ((torch.int64, "int64"), (torch.float16, "float16")):
        with pytest.raises(ValueError, match=name):
            evaluate_batch(Model(), [(feats, torch.zeros(4, dtype=dtype))])
    with pytest.raises(ValueError, match="mix"):
        evaluate_batch(Model(), [(feats, torch.zeros(4)), (feats, torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="empty"):
        evaluate_batch(Model(), [])


def test_entries_validate_before_launch():
    from avsum_amd import _abi
    lib = _abi.lib()
    fake = 1 << 20   # a 16-byte aligned non-null address; never read, the calls return before any HIP call
    # mean + mask: (x, elem_bytes, rows, offsets, nseg, mean, mask)
    assert lib.avs_segment_mean_mask(fake, 2, 10, fake, 1, fake, fake, None) == ARG and b"elem_bytes" in lib.avs_last_error()
    assert lib.avs_segment_mean_mask(fake, 4, -1, fake, 1, fake, fake, None) == SHAPE
    assert lib.avs_segment_mean_mask(fake, 4, 10, fake, -1, fake, fake, None) == SHAPE
    assert lib.avs_segment_mean_mask(None, 4, 10, fake, 1, fake, fake, None) == ARG and b"null" in lib.avs_last_error()
    assert lib.avs_segment_mean_mask(fake, 8, 10, None, 1, fake, fake, None) == ARG
    assert lib.avs_segment_mean_mask(fake, 8, 10, fake, 1, None, fake, None) == ARG
    assert lib.avs_segment_mean_mask(fake, 8, 10, fake, 1, fake, None, None) == ARG
    assert lib.avs_segment_mean_mask(None, 4, 0, None, 0, None, None, None) == 0          # nothing to do

    # pair counts: (pred, target, target_bytes, rows, offsets, nseg, tiles, ntiles, max_t, counts)
    def pairs(pred=fake, target=fake, tbytes=4, rows=100, off=fake, nseg=2, tiles=fake, ntiles=2, max_t=50, counts=fake):
        return lib.avs_rank_pair_counts(pred, target, tbytes, rows, off, nseg, tiles, ntiles, max_t, counts, None)
    assert pairs(tbytes=2) == ARG
    assert pairs(rows=-1) == SHAPE and pairs(rows=1 << 31) == SHAPE and pairs(nseg=-1) == SHAPE
    assert pairs(ntiles=1) == SHAPE                                    # every video has at least one tile
    assert pairs(max_t=32769) == SHAPE and b"32768" in lib.avs_last_error()
    assert pairs(max_t=0) == SHAPE and pairs(rows=1) == SHAPE
    for name in ("pred", "target", "off", "tiles", "counts"):
        assert pairs(**{name: None}) == ARG, name
    assert pairs(pred=None, target=None, off=None, tiles=None, counts=None, rows=0, nseg=0, ntiles=0, max_t=0) == 0

    # fold: (counts, mask_pred, mask_target, rows, offsets, nseg, max_t, out)
    def fold(counts=fake, mx=fake, my=fake, rows=100, off=fake, nseg=2, max_t=50, out=fake):
        return lib.avs_eval_fold(counts, mx, my, rows, off, nseg, max_t, out, None)
    assert fold(rows=-1) == SHAPE and fold(rows=1 << 31) == SHAPE and fold(nseg=-1) == SHAPE
    assert fold(max_t=32769) == SHAPE and fold(max_t=0) == SHAPE and fold(rows=1) == SHAPE
    for name in ("counts", "mx", "my", "off", "out"):
        assert fold(**{name: None}) == ARG, name
    assert fold(counts=None, mx=None, my=None, off=None, out=None, rows=0, nseg=0, max_t=0) == 0
