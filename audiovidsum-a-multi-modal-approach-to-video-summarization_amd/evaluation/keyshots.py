"""Keyshot summaries: whole shots chosen by a 0/1 knapsack under a length budget, and the F1 of such a summary against
each annotator's - the standard product and the standard evaluation on TVSum and SumMe.  The reference has neither
(it only has ``pred > mean``); its segment metric compute_temporal_f1 on disjoint segments is the F1 used.

The definitions, which the numpy oracle below and the kernels of csrc/summary.hip share to the bit, for one score row
and one video of n frames with shots (s_i, e_i), i = 0 .. S - 1:

  q(x)      = rint(clamp(x, 0, 1) * 2^32) as int64: fp32 widened to fp64, an exact product, round half to even; NaN and
              negative values give 0, values above 1 give 2^32
  sum_i     = the int64 sum of q(score[r]) over s_i <= r < e_i (exact: any order)
  w_i       = e_i - s_i;  val_i = float64(sum_i) / float64(w_i), one IEEE division
  C         = int(floor(float64(n) * float64(ratio)))
  row_-1[w] = 0 for w = 0 .. C;  cand = row_{i-1}[w - w_i] + val_i where w >= w_i
  take_i[w] = w >= w_i and cand > row_{i-1}[w] (STRICTLY);  row_i[w] = cand if take_i[w] else row_{i-1}[w]
  backtrack : w = C; for i = S - 1 .. 0: if take_i[w], shot i is picked and w -= w_i;  optimum = row_{S-1}[C]
  F1        = 2 (p r) / (p + r + 1e-8), p = tp / n_pred, r = tp / n_user on the frame masks (NaN for an empty summary)

The host functions are pure numpy and importable without the kernel library."""
import numpy as np

_Q_SCALE = 4294967296.0     # 2^32


def quantise_scores(scores):
    """q(x) of the definitions, elementwise: int64 array of the shape of ``scores`` (taken as fp32)."""
    x = np.asarray(scores, dtype=np.float32).astype(np.float64)
    x = np.where(x > 0.0, x, 0.0)            # NaN fails the comparison: 0
    x = np.where(x < 1.0, x, 1.0)
    return np.rint(x * _Q_SCALE).astype(np.int64)


def summary_capacity(n, ratio=0.15):
    """C of the definitions: the frames a summary of a video of ``n`` frames may hold."""
    return int(np.floor(np.float64(n) * np.float64(ratio)))


def knapsack_host(sums, lengths, capacity):
    """The recurrence and the backtrack of the definitions for one problem: ``sums`` int64 [S] (the quantised score sums
    of the shots), ``lengths`` [S] (their weights), ``capacity`` C.  Returns (picked bool [S], optimum float64)."""
    sums = np.asarray(sums, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if sums.size != lengths.size:
        raise ValueError("knapsack_host: one sum and one length per shot")
    cap = int(capacity)
    if cap < 0:
        raise ValueError(f"knapsack_host: negative capacity {capacity}")
    row = np.zeros(cap + 1, dtype=np.float64)
    take = np.zeros((sums.size, cap + 1), dtype=bool)
    for i, (total, w) in enumerate(zip(sums, lengths)):
        w = int(w)
        if w < 1 or w > cap:                 # never taken
            continue
        cand = row[:cap + 1 - w] + np.float64(total) / np.float64(w)
        better = cand > row[w:]
        take[i, w:] = better
        row = row.copy()
        row[w:][better] = cand[better]
    picked = np.zeros(sums.size, dtype=bool)
    w = cap
    for i in range(sums.size - 1, -1, -1):
        if take[i, w]:
            picked[i] = True
            w -= int(lengths[i])
    return picked, np.float64(row[cap])


def check_shots(shots, n, what="keyshot_summary_host"):
    """``shots`` as an int64 [S, 2] array, refused with a ValueError unless every (start, end) lies inside 0 .. n with
    start < end and the shots ascend without overlap."""
    arr = np.asarray(list(shots), dtype=np.int64).reshape(-1, 2)
    if arr.size and ((arr[:, 0] < 0).any() or (arr[:, 1] > n).any() or (arr[:, 0] >= arr[:, 1]).any()):
        raise ValueError(f"{what}: every shot needs 0 <= start < end <= {int(n)}")
    if arr.shape[0] > 1 and (arr[1:, 0] < arr[:-1, 1]).any():
        raise ValueError(f"{what}: the shots must ascend and must not overlap")
    return arr


def keyshot_summary_host(scores, shots, n, ratio=0.15):
    """The keyshot summary of ONE video: ``scores`` fp32 [n], ``shots`` its [(start, end)] list.  Returns (picked bool
    [S], mask uint8 [n], optimum float64) by the definitions above."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    if scores.size != n:
        raise ValueError(f"keyshot_summary_host: {scores.size} scores for a video of {n} frames")
    arr = check_shots(shots, n)
    prefix = np.concatenate([[0], np.cumsum(quantise_scores(scores), dtype=np.int64)])
    sums = prefix[arr[:, 1]] - prefix[arr[:, 0]]
    picked, optimum = knapsack_host(sums, arr[:, 1] - arr[:, 0], summary_capacity(n, ratio))
    mask = np.zeros(n, dtype=np.uint8)
    for s, e in arr[picked]:
        mask[s:e] = 1
    return picked, mask, optimum


def f1_from_overlap(counts):
    """float64 F1 of the shape of counts[..., 0] from int64 overlap counts [..., 3] = (tp, n_pred, n_user), with the
    reference's expression (compute_temporal_f1 on disjoint segment lists, bit for bit); NaN where that gives NaN."""
    c = np.asarray(counts)
    if c.shape[-1:] != (3,) or c.dtype != np.int64:
        raise ValueError(f"f1_from_overlap: expected an int64 [..., 3] table, got {c.dtype} {c.shape}")
    tp, n_pred, n_user = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = tp / n_pred
        recall = tp / n_user
        return np.asarray(2 * (precision * recall) / (precision + recall + 1e-8), dtype=np.float64)


# --------------------------------------------------------------------------- device forms
class KeyshotResult:
    """What keyshot_summaries_device leaves on the device for K score rows and V videos: ``mask`` uint8 [K, N] (1 = the
    frame is in the summary), ``picked`` uint8 [K, shot_cap] (per shot of the shot table), ``optimum`` float64 [K, V],
    ``totals`` int64 [K, V, 3] = (shots picked, frames picked, capacity), with ``plan`` (the ops.SummaryTables) and the
    shot table it was computed from (``shot_offsets``, ``shots``).  Nothing has been read back; host() is the one
    download."""

    def __init__(self, plan, shot_offsets, shots, out):
        self.plan, self.shot_offsets, self.shots = plan, shot_offsets, shots
        self.mask, self.picked, self.optimum, self.totals = out["mask"], out["picked"], out["optimum"], out["totals"]
        self._host = None

    def host(self):
        """Per score row and per video the list of picked (start, end) tuples, video-relative: ONE download, kept."""
        if self._host is None:
            import torch
            nv, cap, k = self.plan.nvideos, self.plan.shot_cap, self.picked.shape[0]
            flat = torch.cat([self.shot_offsets, self.shots.reshape(-1), self.picked.reshape(-1).to(torch.int64)])
            flat = flat.cpu().numpy()
            off, shots, picked = flat[:nv + 1], flat[nv + 1:nv + 1 + 2 * cap].reshape(cap, 2), flat[nv + 1 + 2 * cap:]
            picked = picked.reshape(k, cap).astype(bool)
            if off[nv] > cap:
                raise RuntimeError(f"keyshot_summaries_device: {int(off[nv])} shots exceed the capacity {cap}")
            self._host = [[[(int(s), int(e)) for s, e in shots[off[v]:off[v + 1]][row[off[v]:off[v + 1]]]]
                           for v in range(nv)] for row in picked]
        return self._host


def _upload_shot_lists(shot_lists, lengths, device):
    """Host shot lists, one per video, validated and uploaded ONCE in the layout of ops.shot_tables: (shot_offsets int64
    [V + 1], shots int64 [shot_cap, 2], shot_cap), shot_cap = the total number of shots (1 when there is none: a
    buffer needs a row)."""
    import torch
    if len(shot_lists) != len(lengths):
        raise ValueError(f"keyshot_summaries_device: {len(shot_lists)} shot lists for {len(lengths)} videos")
    arrays = [check_shots(s, int(n), f"keyshot_summaries_device: video {v}")
              for v, (s, n) in enumerate(zip(shot_lists, lengths))]
    counts = np.array([a.shape[0] for a in arrays], dtype=np.int64)
    total = int(counts.sum())
    cap = max(total, 1)
    packed = np.zeros(len(lengths) + 1 + 2 * cap, dtype=np.int64)
    np.cumsum(counts, out=packed[1:len(lengths) + 1])
    if total:
        packed[len(lengths) + 1:len(lengths) + 1 + 2 * total] = np.concatenate(arrays).reshape(-1)
    packed_t = torch.from_numpy(packed).to(device)
    return packed_t[:len(lengths) + 1], packed_t[len(lengths) + 1:].view(cap, 2), cap


def keyshot_summaries_device(scores, video_offsets, shots, ratio=0.15):
    """The keyshot summary of every (score row, video) of a ragged batch in two launches, nothing read back.
    ``scores``: fp32 device [N] (one row) or [K, N]; ``video_offsets``: the host frame offsets [V + 1].  ``shots``: a
    features.shots.ShotBatchResult or a features.kts.KtsResult (the segments of kernel temporal segmentation) - its
    device tables are used as they are, nothing is downloaded, shot_cap is its plan's - or a list with one host list [(start, end)] per video (video-relative, inside the video, ascending, not
    overlapping), uploaded once.  Returns a KeyshotResult (its tensors keep the row dimension, K = 1 for a vector)."""
    import torch
    from .. import ops
    from ..features.kts import KtsResult
    from ..features.shots import ShotBatchResult
    from ..ragged import RaggedOffsets
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise ValueError("keyshot_summaries_device: scores must be a device tensor (there is no CPU fallback)")
    if isinstance(shots, (ShotBatchResult, KtsResult)):
        cap = shots.shot_cap if isinstance(shots, KtsResult) else shots.plan
        plan = ops.SummaryTables(video_offsets, ratio, cap, scores.device)
        if not np.array_equal(plan.offsets, shots.plan.offsets):
            raise ValueError("keyshot_summaries_device: the shots were detected for other video offsets")
        shot_offsets, shot_table = shots.shot_offsets, shots.shots
    else:
        lengths = RaggedOffsets(video_offsets, "keyshot_summaries_device", device="cpu").lengths
        shot_offsets, shot_table, cap = _upload_shot_lists(list(shots), lengths, scores.device)
        plan = ops.SummaryTables(video_offsets, ratio, cap, scores.device)
    sums = ops.shot_value_sums(plan, scores, shot_offsets, shot_table)
    return KeyshotResult(plan, shot_offsets, shot_table, ops.knapsack_batch(plan, sums, shot_offsets, shot_table))


def keyshot_f1_device(pred_scores, user_scores, video_offsets, shots, ratio=0.15, reduce="mean"):
    """The summary F1 of a prediction against U annotators for every video: one knapsack batch of K = U + 1 score rows
    (row 0 the prediction), the overlap counts, ONE download of the int64 [V, U, 3] table.  ``pred_scores`` fp32 device
    [N], ``user_scores`` fp32 device [U, N]; ``video_offsets`` and ``shots`` as keyshot_summaries_device; ``reduce``:
    "mean" over the annotators (TVSum) or "max" (SumMe).  Returns (per-video F1 float64 [V], its mean over the videos);
    NaN where the reference's expression gives NaN (an empty summary)."""
    import torch
    from .. import ops
    if reduce not in ("mean", "max"):
        raise ValueError(f"keyshot_f1_device: reduce must be 'mean' or 'max', got {reduce!r}")
    for name, t, ndim in (("pred_scores", pred_scores, 1), ("user_scores", user_scores, 2)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != ndim:
            raise ValueError(f"keyshot_f1_device: {name} must be a float32 device tensor of rank {ndim}")
    if user_scores.shape[1] != pred_scores.shape[0] or user_scores.shape[0] < 1:
        raise ValueError(f"keyshot_f1_device: user_scores must be [U >= 1, {pred_scores.shape[0]}], got "
                         f"{list(user_scores.shape)}")
    result = keyshot_summaries_device(torch.cat([pred_scores.unsqueeze(0), user_scores]), video_offsets, shots, ratio)
    counts = ops.mask_overlap_counts(result.plan, result.mask[0], result.mask[1:]).cpu().numpy()
    f1 = f1_from_overlap(counts)
    per_video = np.mean(f1, axis=1) if reduce == "mean" else np.max(f1, axis=1)
    return per_video, np.mean(per_video)
