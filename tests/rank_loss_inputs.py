"""Seeded cases, float64 references, planted mistakes and DERIVED bounds of the per-shot targets and the pairwise ranking
loss (libavsum_loss.so, avsum_amd/loss.py, ops.RankTables): shared by test_rank_loss_host.py and test_gpu_rank_loss.py.

The main ragged batch has the video lengths [1, 2, 257, 1025, 300]: no pair; one pair; one row past the 256-row tile; one
row past the 1024-row LDS chunk (and five tiles); a video whose targets are quantised to 5 levels, so ties abound.  A
second batch holds a video whose targets are ALL tied (P = 0 with many rows).  One case of T = 4097 stands alone (two
tiles past 4096, five LDS chunks).  Scores lie in (0, 1), like sigmoid outputs, with some exact duplicates.

References are computed once per process (lru_cache) and never modified by the tests.

THE BOUNDS.  u = 2^-53 (float64 rounding unit), w = 2^-24 (fp32 rounding unit: one rounding to nearest is within
w * |value|).  The device evaluates the float64 definition, so it differs from rank_loss_host (math.fsum: the exactly
rounded sum) in three ways only:

  (a) the pair terms: x = -scale * d_ij is the SAME float64 product on both sides (d_ij is exact); exp and log1p come from
      two maths libraries, each documented to 2 ulp or better in float64, and softplus / sigma add one rounding each (an
      addition, a division).  A term is within TERM_ULPS = 16 ulp = 32 u relative of the host's: 2 * (2 + 2) for the two
      functions on the two sides, doubled for slack in the documented figures - a constant, not a fit.
  (b) summation order: a row's partial is a sequential sum of at most T terms, the fold adds at most ceil(T / 256) of them
      per thread and 8 tree levels: every term passes through fewer than 2 T additions, each within u relative of its
      partial sum.  For terms of one sign the sum is within 2 T u relative; for signed terms within 2 T u * sum |term|.
  (c) one division by P (u relative) and the final cast to fp32 (w relative).

So, with L and g the host's float64 values:

  loss_bound(L, T)       = L * (w + (2 T + 32 + 2) u)                     (the terms are non-negative)
  grad_bound(g, T, P, s) = |g| * (w + 2 u) + (s / P) * T * (2 T + 32) u   (a row has at most T terms of size < 1)

The hinge gradient is an integer over an integer: (float)(c / P) on both sides, bit for bit, no bound.  The hinge loss
takes loss_bound too (its terms margin - d_ij are the same float64 differences on both sides; (a) does not apply, and the
bound is not narrowed for it).
"""
import functools

import numpy as np

U = 2.0 ** -53
W = 2.0 ** -24
TERM_ULPS = 16

LENGTHS = [1, 2, 257, 1025, 300]
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
QUANTISED = 4                       # the video of LENGTHS whose targets take 5 levels
TIED_LENGTHS = [5, 40, 3]           # the second batch: video 1 is all tied
TIED_OFFSETS = np.concatenate([[0], np.cumsum(TIED_LENGTHS)]).astype(np.int64)
LARGE_T = 4097
KINDS = ("logistic", "hinge")
SCALE, MARGIN = 1.5, 0.1            # (a scale other than 1: it must reach the loss and the gradient)
SENTINEL = -7.5


def loss_bound(value, t):
    return abs(value) * (W + (2 * t + 2 * TERM_ULPS + 2) * U)


def grad_bound(value, t, pairs, scale):
    return abs(value) * (W + 2 * U) + (scale / max(pairs, 1)) * t * (2 * t + 2 * TERM_ULPS) * U


def _scores_targets(rng, t, levels=None):
    """Scores in (0, 1) as fp32 with every 7th a copy of its predecessor's predecessor; targets U(1, 5) as fp32, or
    ``levels`` equally spaced values."""
    s = (rng.random(t) * 0.98 + 0.01).astype(np.float32)
    s[2::7] = s[0:t - 2:7][:len(s[2::7])]
    y = (rng.random(t) * 4 + 1).astype(np.float32)
    if levels:
        y = (np.floor(rng.random(t) * levels) / levels).astype(np.float32)
    return s, y


@functools.lru_cache(maxsize=None)
def main_batch():
    rng = np.random.default_rng(20261)
    parts = [_scores_targets(rng, t, 5 if v == QUANTISED else None) for v, t in enumerate(LENGTHS)]
    s, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    s.setflags(write=False)
    y.setflags(write=False)
    return s, y


@functools.lru_cache(maxsize=None)
def tied_batch():
    rng = np.random.default_rng(20262)
    parts = [_scores_targets(rng, t) for t in TIED_LENGTHS]
    s, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    y[TIED_OFFSETS[1]:TIED_OFFSETS[2]] = np.float32(2.5)
    s.setflags(write=False)
    y.setflags(write=False)
    return s, y


@functools.lru_cache(maxsize=None)
def large_case():
    s, y = _scores_targets(np.random.default_rng(20263), LARGE_T)
    y[::3] = np.float32(3.0)             # a third of the rows tied
    s.setflags(write=False)
    y.setflags(write=False)
    return s, y


def batch(name):
    """(scores, targets, offsets) of "main", "tied" or "large"."""
    if name == "main":
        return (*main_batch(), OFFSETS)
    if name == "tied":
        return (*tied_batch(), TIED_OFFSETS)
    return (*large_case(), np.array([0, LARGE_T], dtype=np.int64))


@functools.lru_cache(maxsize=None)
def host_reference(name, kind):
    """rank_loss_host of a batch: (losses float64 [V], g float64 [R], P int64 [V]), computed once, read-only."""
    from avsum_amd.loss import rank_loss_host
    s, y, off = batch(name)
    out = rank_loss_host(s, y, off, kind, SCALE, MARGIN)
    for a in out:
        a.setflags(write=False)
    return out


def brute_force_pairs(y):
    """#{(i, j): y_i > y_j} by a double loop over Python floats."""
    y = [float(v) for v in y]
    return sum(1 for a in y for b in y if a > b)


def dense_torch_loss(scores, targets, offsets, kind, scale, margin):
    """The dense [T, T] float64 torch formulation on the CPU: (losses with autograd attached, the leaf they hang on)."""
    import torch
    s = torch.tensor(np.asarray(scores, dtype=np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(targets, dtype=np.float32))
    losses = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        d = s[a:b, None] - s[None, a:b]
        pair = y[a:b, None] > y[None, a:b]
        term = torch.nn.functional.softplus(-scale * d) if kind == "logistic" else torch.clamp(margin - d, min=0.0)
        count = pair.sum()
        losses.append((term * pair).sum() / count if count > 0 else (s[a:b] * 0.0).sum())
    return torch.stack(losses), s


RANK_PLANTED = ("ge", "t_squared", "sign")


def floor_tiles(lengths, tile=256):
    """The planted tile table: floor(T / tile) tiles per video instead of ceil - it drops row 256 of a 257-row video."""
    return [(v, k) for v, t in enumerate(lengths) for k in range(int(t) // tile)]


def rows_covered(tiles, lengths, tile=256):
    """How often each row of each video is owned by a (video, row tile) entry: a list of int arrays."""
    seen = [np.zeros(int(t), dtype=np.int64) for t in lengths]
    for v, k in tiles:
        seen[v][k * tile:(k + 1) * tile] += 1
    return seen


# --------------------------------------------------------------------------- per-shot targets
FPS_VALUES = (30, 29.97, 25, 24, 23.976)
ANN_BINS = 37                       # 74 seconds of 2-second annotation bins


@functools.lru_cache(maxsize=None)
def annotations(seed=20264, bins=ANN_BINS):
    a = (np.random.default_rng(seed).random(bins) * 4 + 1).astype(np.float32)
    a.setflags(write=False)
    return a


def shot_case(fps, bins=ANN_BINS):
    """Shots of one video at ``fps``: a ragged partition of the frames the annotations cover (cuts on and off bin
    edges), then a shot whose END bin runs past the annotations (clipped), then one that STARTS past them (an empty
    slice: NaN and the flag)."""
    frames = int(bins * 2 * fps)
    cuts = sorted({int(round(c)) for c in (0.4 * fps, 2 * fps, 6 * fps - 1, 6 * fps, 17.3 * fps, 40 * fps, 40 * fps + 1,
                                           61.9 * fps) if round(c) < frames - 3})
    bounds = [0] + cuts + [frames - 3]
    shots = list(zip(bounds[:-1], bounds[1:]))
    shots.append((frames - 3, frames + int(9 * fps)))
    shots.append((frames + int(4 * fps), frames + int(9 * fps)))
    return shots


VIDEO_FPS = (30.0, 29.97, 23.976)
VIDEO_BINS = (37, 11, 52)


def shot_batch():
    """Three videos with their own frame rates and annotation lengths: (annotations fp32, ann_offsets, shots int64
    [S, 2], shot_offsets, fps [3]).  Videos 0 and 2 hold an empty slice (flag), video 1 does not."""
    ann = [annotations(20265 + v, b) for v, b in enumerate(VIDEO_BINS)]
    lists = [shot_case(f, b) for f, b in zip(VIDEO_FPS, VIDEO_BINS)]
    lists[1] = lists[1][:-1]
    shots = np.array([s for l in lists for s in l], dtype=np.int64).reshape(-1, 2)
    return (np.concatenate(ann), np.concatenate([[0], np.cumsum(VIDEO_BINS)]).astype(np.int64), shots,
            np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64), np.array(VIDEO_FPS))
