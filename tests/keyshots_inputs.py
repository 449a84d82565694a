"""Inputs shared by test_keyshots_host.py and test_gpu_keyshots.py: seeded ragged batches of scores and shot lists at the
smallest shapes that reach each way the knapsack kernel can go wrong, and the host pipeline the device forms must equal."""
import numpy as np

RATIO = 0.15


def tiling_shots(n, seed, lo, hi, first=0):
    """[(start, end)] shots of lo .. hi frames that tile first .. n (the last one takes what is left)."""
    rng = np.random.default_rng(seed)
    shots, s = [], first
    while s < n:
        e = min(n, s + int(rng.integers(lo, hi + 1)))
        shots.append((s, e))
        s = e
    return shots


def batch_videos():
    """(lengths, shot lists) of the five videos of the main batch:
      40    no shots at all (S = 0)
      47    one shot of the whole video: w = 47 > C = 7, never taken
      430   C = 64: C + 1 = 65 cells cross a 64-bit take word; some frames belong to no shot
      6830  C = 1024: C + 1 = 1025 cells cross the 1024-thread stride; about 200 shots of 15 .. 60 frames
      700   C = 105 and one shot of weight exactly 105, the rest small"""
    lengths = [40, 47, 430, 6830, 700]
    gappy = [s for i, s in enumerate(tiling_shots(430, 11, 5, 40)) if i % 5 != 2]
    shots = [[], [(0, 47)], gappy, tiling_shots(6830, 12, 15, 60), [(0, 105)] + tiling_shots(700, 13, 4, 20, first=105)]
    return lengths, shots


def full_lds_videos():
    """(lengths, shot lists): 54 606 frames with 40 shots, and 54 613 frames - the longest video whose capacity at
    ratio 0.15, 8191, still fits - with 40 shots: (nearly) every cell of the knapsack kernel's two LDS rows is in use."""
    lengths = [54606, 54613]
    shots = []
    for n, seed in zip(lengths, (21, 22)):
        cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), size=39, replace=False))
        bounds = [0] + [int(c) for c in cuts] + [n]
        shots.append(list(zip(bounds[:-1], bounds[1:])))
    return lengths, shots


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def score_rows(n, seed):
    """fp32 [3, n]: row 0 random in [0, 1), row 1 constant 0.5 (every comparison of the knapsack a tie), row 2 random in
    [-0.5, 1.5) - values outside [0, 1] - with a NaN."""
    rng = np.random.default_rng(seed)
    rows = np.empty((3, n), dtype=np.float32)
    rows[0] = rng.random(n, dtype=np.float32)
    rows[1] = 0.5
    rows[2] = rng.random(n, dtype=np.float32) * 2.0 - 0.5
    rows[2, n // 3] = np.nan
    return rows


def user_rows(n, users, seed):
    """fp32 [users, n] annotator scores: smooth bumps plus noise, so that summaries overlap only in part."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    rows = [0.5 + 0.4 * np.sin(t / rng.uniform(20, 90) + rng.uniform(0, 6)) + 0.1 * rng.standard_normal(n)
            for _ in range(users)]
    return np.clip(np.stack(rows), 0.0, 1.0).astype(np.float32)


def host_summaries(rows, lengths, shots, ratio=RATIO):
    """keyshot_summary_host for every (row, video): dict of mask uint8 [K, N], optimum float64 [K, V], totals int64
    [K, V, 3], picked (list per row of list per video of bool [S]) and segments (the picked (start, end) lists)."""
    from avsum_amd.evaluation.keyshots import keyshot_summary_host, summary_capacity
    off = offsets_of(lengths)
    k, nv = rows.shape[0], len(lengths)
    out = {"mask": np.zeros((k, off[-1]), dtype=np.uint8), "optimum": np.zeros((k, nv), dtype=np.float64),
           "totals": np.zeros((k, nv, 3), dtype=np.int64), "picked": [], "segments": []}
    for r in range(k):
        out["picked"].append([])
        out["segments"].append([])
        for v, (n, sh) in enumerate(zip(lengths, shots)):
            picked, mask, optimum = keyshot_summary_host(rows[r, off[v]:off[v + 1]], sh, n, ratio)
            out["mask"][r, off[v]:off[v + 1]] = mask
            out["optimum"][r, v] = optimum
            out["totals"][r, v] = (int(picked.sum()), int(mask.sum()), summary_capacity(n, ratio))
            out["picked"][-1].append(picked)
            out["segments"][-1].append([s for s, p in zip(sh, picked) if p])
    return out


def host_f1(pred_segments, user_segments, lengths, reduce):
    """Per-video F1 of the host pipeline: compute_temporal_f1 on the picked segment lists of the prediction against every
    user's (NaN where a summary is empty: the reference divides by zero there), reduced over the users."""
    from avsum_amd.evaluation.metrics import compute_temporal_f1

    def one(p, g, n):
        try:
            return compute_temporal_f1(p, g, n)
        except ZeroDivisionError:
            return float("nan")

    table = np.array([[one(pred_segments[v], user[v], n) for user in user_segments]
                      for v, n in enumerate(lengths)], dtype=np.float64)
    return (np.mean(table, axis=1) if reduce == "mean" else np.max(table, axis=1)), table
