"""Selection rule and metrics: scripts/evaluate.py:21-42 and evaluation/metrics.py:1-9 of the
reference.  The host forms are numpy / SciPy as the reference has them; the ``*_device`` forms take concatenated device
vectors and give the same selection bit for bit (the kernels sum in numpy's order) and the same metrics from exact
integer pair counts, with one download for the whole batch."""
import numpy as np


def compute_temporal_f1(pred_shots, gt_shots, total_frames):
    overlap = sum(max(0, min(p_end, g_end) - max(p_start, g_start))
                  for p_start, p_end in pred_shots for g_start, g_end in gt_shots)
    precision = overlap / sum(p_end - p_start for p_start, p_end in pred_shots)
    recall = overlap / sum(g_end - g_start for g_start, g_end in gt_shots)
    return 2 * (precision * recall) / (precision + recall + 1e-8)


def select_frames(pred):
    """np.flatnonzero(pred > pred.mean()) — the reference's selection rule (scripts/evaluate.py:26)."""
    pred = np.asarray(pred)
    return np.flatnonzero(pred > np.mean(pred))


def segments_from_indices(idx):
    idx = np.asarray(idx)
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1)
    starts = np.concatenate([[idx[0]], idx[cut + 1]])
    ends = np.concatenate([idx[cut] + 1, [idx[-1] + 1]])
    return [(int(s), int(e)) for s, e in zip(starts, ends)]


def binary_f1(pred, target):
    bp = (pred > np.mean(pred)).astype(int)
    bt = (target > np.mean(target)).astype(int)
    tp = np.logical_and(bp, bt).sum()
    precision = tp / bp.sum()
    recall = tp / bt.sum()
    return 2 * (precision * recall) / (precision + recall + 1e-8)


def summarize_scores(pairs):
    """Mean over videos of the mean-threshold F1, Spearman and Kendall correlations (scripts/evaluate.py:21-42).
    Like the reference it does not guard a constant prediction (NaN precision / correlation)."""
    from scipy.stats import kendalltau, spearmanr
    f1 = [binary_f1(p, t) for p, t in pairs]
    rho = [spearmanr(p, t).correlation for p, t in pairs]
    tau = [kendalltau(p, t).correlation for p, t in pairs]
    return {"f1": np.mean(f1), "spearman": np.mean(rho), "kendall": np.mean(tau)}


# --------------------------------------------------------------------------- batched device forms
def metrics_from_counts(counts):
    """Per-video ``f1``, ``spearman`` and ``kendall`` (float64 arrays [V]) from the int64 [V, 10] table of
    ops.eval_counts (columns ops.EVAL_COLUMNS), with the reference's expressions: binary_f1's on the mask sums, SciPy's
    tau-b on C - D = S2 / 2 and the tied-pair counts (E - T) / 2, Pearson's r of the doubled average ranks for
    Spearman.  NaN where the reference gives NaN: an empty mask (0 / 0), all pairs tied in x or y, a zero rank
    variance."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != 10 or c.dtype != np.int64:
        raise ValueError(f"metrics_from_counts: expected an int64 [V, 10] table, got {c.dtype} {c.shape}")
    t, n_pred, n_tgt, tp, s2, e_x, e_y, s_xy, s_xx, s_yy = (c[:, k] for k in range(10))
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = tp / n_pred
        recall = tp / n_tgt
        f1 = 2 * (precision * recall) / (precision + recall + 1e-8)
        tot = t * (t - 1) // 2
        xtie, ytie = (e_x - t) // 2, (e_y - t) // 2
        tau = (s2 // 2) / np.sqrt(tot - xtie) / np.sqrt(tot - ytie)
        tau = np.where((xtie == tot) | (ytie == tot), np.nan, np.minimum(1.0, np.maximum(-1.0, tau)))
        sr = t * (t + 1)                      # the sum of the doubled ranks, whatever the ties
        vx, vy = t * s_xx - sr * sr, t * s_yy - sr * sr
        rho = (t * s_xy - sr * sr) / np.sqrt(vx.astype(np.float64) * vy.astype(np.float64))
        rho = np.where((vx == 0) | (vy == 0), np.nan, np.minimum(1.0, np.maximum(-1.0, rho)))
    return {"f1": f1.astype(np.float64), "spearman": rho.astype(np.float64), "kendall": tau.astype(np.float64)}


def _as_tables(offsets, device):
    from .. import ops
    return offsets if isinstance(offsets, ops.EvalTables) else ops.EvalTables(offsets, device)


def summarize_scores_device(pred, target, offsets):
    """summarize_scores for V videos held as concatenated device vectors: ``pred`` float32 [R], ``target`` float32 or
    float64 [R] (its own dtype: converting it would move ties and the threshold), ``offsets`` the host row offsets
    [V + 1] or a prepared ops.EvalTables.  Four launches and one download, whatever V is.  Same dict as
    summarize_scores: f1 equal, the correlations the same rational expressions evaluated once in float64."""
    from .. import ops
    counts = ops.eval_counts(_as_tables(offsets, pred.device), pred, target).cpu().numpy()
    per_video = metrics_from_counts(counts)
    return {k: np.mean(per_video[k]) for k in ("f1", "spearman", "kendall")}


def select_mask_device(scores, offsets):
    """uint8 device mask [R]: mask[r] = 1 where select_frames of r's video selects r (scores > np.mean(scores), numpy's
    own fp32 mean bit for bit).  ``scores`` float32 / float64 device vector, ``offsets`` host sequence or int64 device
    tensor [V + 1].  Nothing is downloaded."""
    from .. import ops
    return ops.segment_mean_mask(scores, offsets)[1]
