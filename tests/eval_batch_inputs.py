"""Inputs and host oracles of the batched evaluation tests (test_eval_batch_host.py, test_gpu_eval_batch.py):
numpy's reduction order written out, the O(T^2) brute-force pair counts, and seeded (pred, target) videos with ties."""
import functools

import numpy as np

PW_BLOCK = 128      # numpy's pairwise-sum leaf size
NP_BUFSIZE = 8192   # elements numpy's reduction hands to the pairwise sum at a time
TILE = 256          # rows per workgroup of the pair-count kernel (ops.EVAL_TILE)
CHUNK = 1024        # columns staged through LDS per step of the pair-count kernel (ops.EVAL_CHUNK)

# column order of the int64 [V, 10] table
T_, NPRED, NTGT, TP, S2, EX, EY, SXY, SXX, SYY = range(10)


# --------------------------------------------------------------------------- numpy's order of np.mean
def _pw(a):
    """numpy's pairwise sum of one buffer, every addition rounded in a.dtype."""
    n = a.shape[0]
    if n < 8:
        res = a.dtype.type(-0.0)
        for v in a:
            res = res + v
        return res
    if n <= PW_BLOCK:
        r = a[:8].copy()
        for i in range(8, n - n % 8, 8):
            r = r + a[i:i + 8]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[n - n % 8:]:
            res = res + v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pw(a[:n2]) + _pw(a[n2:])


def mean_numpy_order(a):
    """np.mean of a contiguous 1-D float32 / float64 array, addition by addition: buffers of 8192 elements are summed
    pairwise and their sums added left to right; the mean is sum / n in the element type."""
    a = np.ascontiguousarray(a)
    ty = a.dtype.type
    n = a.shape[0]
    total = _pw(a[:NP_BUFSIZE]) if n else ty(0.0)
    for s in range(NP_BUFSIZE, n, NP_BUFSIZE):
        total = total + _pw(a[s:s + NP_BUFSIZE])
    with np.errstate(invalid="ignore"):
        return ty(total / ty(n))


# --------------------------------------------------------------------------- brute-force counts
def brute_counts(pred, target):
    """The ten integers of one video, O(T^2) numpy (int64 [10])."""
    x, y = np.asarray(pred), np.asarray(target)
    t = x.shape[0]
    mx, my = x > np.mean(x), y > np.mean(y)
    dx = np.sign(x[:, None] - x[None, :]).astype(np.int64) if t <= 2048 else None
    out = np.zeros(10, dtype=np.int64)
    if dx is not None:
        lx, ex = (x[None, :] < x[:, None]).sum(1), (x[None, :] == x[:, None]).sum(1)
        ly, ey = (y[None, :] < y[:, None]).sum(1), (y[None, :] == y[:, None]).sum(1)
        s = (dx * np.sign(y[:, None] - y[None, :]).astype(np.int64)).sum(1)
    else:   # row blocks keep the [T, T] temporaries small
        lx, ex, ly, ey, s = (np.zeros(t, dtype=np.int64) for _ in range(5))
        for a in range(0, t, 512):
            xa, ya = x[a:a + 512, None], y[a:a + 512, None]
            lx[a:a + 512], ex[a:a + 512] = (x[None, :] < xa).sum(1), (x[None, :] == xa).sum(1)
            ly[a:a + 512], ey[a:a + 512] = (y[None, :] < ya).sum(1), (y[None, :] == ya).sum(1)
            s[a:a + 512] = (np.sign(xa - x[None, :]).astype(np.int64) * np.sign(ya - y[None, :]).astype(np.int64)).sum(1)
    rx, ry = 2 * lx + ex + 1, 2 * ly + ey + 1     # doubled average ranks
    out[:] = (t, mx.sum(), my.sum(), (mx & my).sum(), s.sum(), ex.sum(), ey.sum(), (rx * ry).sum(), (rx * rx).sum(),
              (ry * ry).sum())
    return out


def brute_counts_batch(pairs):
    return np.stack([brute_counts(p, t) for p, t in pairs]) if pairs else np.zeros((0, 10), dtype=np.int64)


# --------------------------------------------------------------------------- videos
def video(seed, t, levels=81, pred_levels=None, tdtype=np.float32, kind=None):
    """(pred float32 [t] in (0, 1) with repeated values, target [t] quantised to `levels` values)."""
    rng = np.random.default_rng([seed, t])
    pl = pred_levels if pred_levels is not None else max(2, t // 2)
    pred = ((rng.integers(0, pl, t) + 0.5) / pl).astype(np.float32)
    # the target follows the prediction loosely, so the correlations are neither 0 nor 1
    raw = 0.6 * pred.astype(np.float64) + 0.4 * rng.random(t)
    target = (np.floor(raw * levels) / levels).astype(tdtype)
    if kind == "tied_target":
        target[:] = tdtype(0.25)
    elif kind == "const_pred":
        pred[:] = np.float32(0.5)
    elif kind == "zeros":       # both signs of zero among the values: -0.0 == 0.0 under IEEE comparison
        pred = (pred - np.float32(0.5)).astype(np.float32)
        pred[::3] = np.float32(0.0)
        pred[1::3] = np.float32(-0.0)
        target = (target - tdtype(0.5)).astype(tdtype)
        target[::4] = tdtype(-0.0)
        target[2::4] = tdtype(0.0)
    return pred, target


def layout(pairs, first=0):
    """(pred concatenated float32 [R], target concatenated, offsets int64 [V + 1]); `first` rows of filler come first."""
    tdtype = pairs[0][1].dtype if pairs else np.float32
    lens = [len(p) for p, _ in pairs]
    offsets = first + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pred = np.concatenate([np.full(first, 7.0, np.float32)] + [p for p, _ in pairs]).astype(np.float32)
    target = np.concatenate([np.full(first, -7.0, tdtype)] + [t for _, t in pairs]).astype(tdtype)
    return pred, target, offsets


# the GPU count batch: every T at which the pair-count kernel takes another path (tile and LDS chunk boundaries), the
# smallest videos, 5 and 81 target levels, an all-tied target, a constant prediction and signed zeros
COUNT_BATCH = [(2, 5, None), (3, 81, None), (TILE - 1, 5, None), (TILE, 81, None), (TILE + 1, 5, None),
               (CHUNK - 1, 81, None), (CHUNK + 1, 5, None), (1800, 81, None), (300, 5, "tied_target"),
               (301, 81, "const_pred"), (77, 81, "zeros"), (CHUNK, 5, "zeros")]


@functools.lru_cache(maxsize=None)
def count_batch(tdtype_name="float32"):
    tdtype = np.dtype(tdtype_name).type
    return tuple(video(11 + k, t, lv, tdtype=tdtype, kind=kind) for k, (t, lv, kind) in enumerate(COUNT_BATCH))


@functools.lru_cache(maxsize=None)
def count_batch_oracle(tdtype_name="float32"):
    ref = brute_counts_batch(list(count_batch(tdtype_name)))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def long_videos():
    """T = 5000 (the longest of the configs) and T = 8193 (one element past numpy's 8192 buffer), float64 targets."""
    return (video(5, 5000, 81, tdtype=np.float64), video(6, 8193, 5, tdtype=np.float64))


def scipy_pair_sums(pred, target):
    """(S2, E_x, E_y) from SciPy's own tie counts and tau-b, without an O(T^2) table: S2 = 2 (C - D)."""
    from scipy.stats import kendalltau
    x, y = np.asarray(pred), np.asarray(target)
    t = x.shape[0]
    ex = int((np.unique(x, return_counts=True)[1].astype(np.int64) ** 2).sum())
    ey = int((np.unique(y, return_counts=True)[1].astype(np.int64) ** 2).sum())
    tot = t * (t - 1) // 2
    tau = kendalltau(x, y).correlation
    cmd = tau * np.sqrt(float(tot - (ex - t) // 2)) * np.sqrt(float(tot - (ey - t) // 2))
    return 2 * int(np.rint(cmd)), ex, ey
