"""Seeded inputs shared by the kernel-temporal-segmentation tests (test_kts_host.py, test_gpu_kts.py)."""
import numpy as np


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def planted(lengths, d, noise=0.02, seed=3):
    """fp32 [sum(lengths), d]: per segment one random unit vector plus noise * N(0, 1) per row."""
    rng = np.random.default_rng(seed)
    rows = []
    for length in lengths:
        c = rng.standard_normal(d)
        rows.append(c / np.linalg.norm(c) + noise * rng.standard_normal((length, d)))
    return np.concatenate(rows).astype(np.float32)


def integer_features(n, d, seed=1):
    """fp32 [n, d] of integers -3 .. 3: every partial sum of a Gram entry is an integer far below 2^53."""
    return np.random.default_rng(seed).integers(-3, 4, (n, d)).astype(np.float32)


def random_features(n, d, seed=5):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


# the ragged batch of the Gram tests: samples n = 1, 2, 17, 65 at stride 1 and 3 (frame counts no multiples of 3)
GRAM_SAMPLES = (1, 2, 17, 65)


def gram_lengths(stride):
    """Frame counts N with ceil(N / stride) = GRAM_SAMPLES and, for stride 3, N % 3 != 0."""
    return [n if stride == 1 else stride * (n - 1) + 1 + (v % 2) for v, n in enumerate(GRAM_SAMPLES)]


# the ragged batch of the bit-for-bit tests: stride 1, planted structure in the last three videos
DP_SAMPLES = (1, 2, 9, 33, 160, 1100)
DP_NCP = (None, None, 8, 32, 159, 12)
DP_PLANTED = {3: (7, 12, 5, 9), 4: (40, 23, 64, 33), 5: (300, 250, 130, 220, 200)}


def dp_batch(d=24):
    """(features fp32 [sum n, d], lengths): random rows in the first three videos, planted segments in the others."""
    parts = []
    for v, n in enumerate(DP_SAMPLES):
        parts.append(planted(DP_PLANTED[v], d, seed=10 + v) if v in DP_PLANTED else random_features(n, d, seed=10 + v))
        assert parts[-1].shape[0] == n
    return np.concatenate(parts), list(DP_SAMPLES)


def exact_gram(x):
    """K[i, j] = math.fsum of the exact fp64 products: the correctly rounded Gram matrix of fp32 rows x [n, d]."""
    import math
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x64.shape[0]
    out = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        prod = x64[i][None, :] * x64[i:]            # exact: 24-bit x 24-bit significands
        for j in range(i, n):
            out[i, j] = out[j, i] = math.fsum(prod[j - i])
    return out
