"""Inputs and CPU references shared by test_fusion_batch_host.py and test_gpu_fusion_batch.py (not a test module).

Random-walk rows: both sides of a pair are noisy samples of one random walk at sorted random positions, so the DTW path
warps in both directions (up to tens of cells per row or column); plain Gaussian rows give near-diagonal paths."""
import functools

import numpy as np
import torch

from oracle import fusion as ofu

SEED = 7
BATCH_D24 = ((700, 300), (1, 1), (33, 31), (1, 7), (1500, 1100), (9, 1), (2, 2), (64, 65), (5, 9), (65, 64), (130, 97),
             (257, 40), (40, 257))
BATCH_D512 = ((200, 200),) * 3
TIE_SHAPES = ((33, 31), (64, 65), (130, 97), (700, 300))


def walk_pair(rng, n, m, d):
    base = np.cumsum(rng.standard_normal((2 * max(n, m), d)), 0).astype(np.float32)
    v = base[np.sort(rng.integers(0, len(base), n))]
    a = base[np.sort(rng.integers(0, len(base), m))] + (0.05 * rng.standard_normal((m, d))).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)), torch.from_numpy(np.ascontiguousarray(a, np.float32))


@functools.lru_cache(maxsize=None)
def walk_batch(shapes, d):
    """The pairs of `shapes`, drawn in order from one generator seeded SEED.  Cached: treat the tensors as read-only."""
    rng = np.random.default_rng(SEED)
    return tuple(walk_pair(rng, n, m, d) for n, m in shapes)


@functools.lru_cache(maxsize=None)
def tie_batch():
    """D = 8 rows drawn from {0, 1, 2}: squared distances are exact integers and the paths are full of exact ties."""
    rng = np.random.default_rng(SEED)
    return tuple((torch.from_numpy(rng.integers(0, 3, (n, 8)).astype(np.float32)),
                  torch.from_numpy(rng.integers(0, 3, (m, 8)).astype(np.float32))) for n, m in TIE_SHAPES)


@functools.lru_cache(maxsize=None)
def small_batch(count=3000, d=16):
    rng = np.random.default_rng(SEED)
    return tuple(walk_pair(rng, int(rng.integers(1, 13)), int(rng.integers(1, 13)), d) for _ in range(count))


def oracle_pair(v, a):
    """(cost float64 [n, m], path int64 [L, 2]) of the CPU oracle."""
    cost = ofu.compute_dtw(v, a)
    return cost, ofu.compute_optimal_path(cost)


@functools.lru_cache(maxsize=None)
def oracle_batch(name):
    """The oracle's (cost, path) of every pair of a named batch, computed once per session."""
    pairs = {"d24": lambda: walk_batch(BATCH_D24, 24), "d512": lambda: walk_batch(BATCH_D512, 512), "tie": tie_batch,
             "small": small_batch}[name]()
    return tuple(oracle_pair(v, a) for v, a in pairs)


def cost_reversed(v, a):
    """The cost matrix with the squared differences summed in DESCENDING k order, in float64."""
    v64, a64 = v.numpy().astype(np.float64), a.numpy().astype(np.float64)
    acc = np.zeros((v64.shape[0], a64.shape[0]))
    for k in range(v64.shape[1] - 1, -1, -1):
        t = v64[:, k:k + 1] - a64[None, :, k]
        acc += t * t
    return np.sqrt(acc)


def layout(pairs, gap=0, d=None):
    """Concatenate the pairs' rows (`gap` unused rows before every pair): (V, A, [(v_row0, n, a_row0, m)])."""
    d = pairs[0][0].shape[1] if d is None else d
    vs, as_, table, rv, ra = [], [], [], 0, 0
    for i, (v, a) in enumerate(pairs):
        if gap:
            vs.append(torch.full((gap, d), float(i + 1)))
            as_.append(torch.full((gap + 1, d), -float(i + 1)))
            rv, ra = rv + gap, ra + gap + 1
        table.append((rv, v.shape[0], ra, a.shape[0]))
        vs.append(v)
        as_.append(a)
        rv, ra = rv + v.shape[0], ra + a.shape[0]
    return torch.cat(vs).contiguous(), torch.cat(as_).contiguous(), table
