"""Kernel temporal segmentation (KTS; Potapov et al., ECCV 2014: cpd_nonlin + cpd_auto) with the linear kernel: the
change points the TVSum / SumMe protocol cuts a video into before the keyshot knapsack (evaluation/keyshots.py) chooses
whole segments.  The reference has neither.  KTS runs on the frame features subsampled by ``stride``.

The definitions, which the numpy oracle below and the kernels of csrc/kts.hip share to the bit, for one video with N
feature rows x_r (fp32, width D), a stride >= 1 and a minimum segment length lmin >= 1:

  n        = ceil(N / stride);  sample i = row i * stride, i = 0 .. n - 1;  1 <= n <= 2048
  K[i,j]   = sum_d float64(x_i[d]) * float64(x_j[d])   (each product is exact; the ORDER of the sum is not pinned: the
             device's K agrees with any other fp64 evaluation to D * 2^-53 * (|X||X|^T)[i,j], is symmetric to the bit and
             depends on the video alone - everything below is defined on a GIVEN K)
  K1[0]    = 0;  K1[r+1] = K1[r] + K[r,r]              (sequential, r ascending)
  C        = np.cumsum(K, axis=0);  R = np.cumsum(C, axis=1)   (both strictly sequential);  K2 = zeros [n+1, n+1],
             K2[1:,1:] = R
  J(t,l)   = (K1[l] - K1[t]) - (((K2[l,l] + K2[t,t]) - K2[l,t]) - K2[t,l]) / float64(l - t)   for 0 <= t < l <= n
             (the scatter of the samples t .. l-1; exactly these operations in this order, one IEEE division)
  m_max    = max(0, min(ncp, n // lmin - 1))           (ncp defaults to n - 1)
  I_0[l]   = J(0,l)                                    for 1 <= l <= n   (the cells below lmin are never read for k >= 1)
  I_k[l]   = min over t = k*lmin .. l-lmin of (I_{k-1}[t] + J(t,l)),  p_k[l] = the SMALLEST such t attaining it,
             for k = 1 .. m_max, l = (k+1)*lmin .. n   (no other cell is ever read)
  score[k] = I_k[n];  pen[0] = 0;  pen[k] = (vmax*k / (2.0*n)) * (np.log(float64(n)/k) + 1.0)   (computed on the HOST,
             it depends on n, k and vmax only, and uploaded with the plan)
  cost[k]  = score[k] / float64(n) + pen[k];  m_best = the smallest k attaining the least cost   (select="auto"),
             m_best = m_max                                                                      (select="fixed")
  backtrack: cur = n; for k = m_best .. 1: cp[k-1] = p_k[cur]; cur = cp[k-1]     (sample indices, ascending)
  shots    : b_0 = 0, b_j = cp[j-1] * stride, b_{m_best+1} = N  ->  (b_j, b_{j+1}), video-relative FRAME rows
  flag     : 1 iff K2[n,n] is not finite (any NaN / Inf in K reaches it); then m_best = 0, one shot (0, N), NaN costs

The published cpd_auto runs cpd_nonlin twice; the rows k <= m_best of both runs are the same, so one programme with p
kept gives the same result.  The published lmax is not offered (its default never binds).

The host functions are pure numpy and importable without torch and without the kernel library."""
import numpy as np

from .._header import load as _load_header     # (re and ctypes only: still no torch, no kernel library)

KTS_MAX_SAMPLES = _load_header().constants["AVS_KTS_MAX_SAMPLES"]   # 2048, shared with csrc/kts.hip


def kts_penalties(n, m_max, vmax=1.0):
    """float64 [m_max + 1]: pen[k] of the definitions for k = 0 .. m_max change points among n samples."""
    pen = np.zeros(int(m_max) + 1, dtype=np.float64)
    ks = np.arange(1, int(m_max) + 1, dtype=np.float64)
    pen[1:] = (np.float64(vmax) * ks / (2.0 * np.float64(n))) * (np.log(np.float64(n) / ks) + 1.0)
    return pen


def _square(K, what):
    K = np.asarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1] or K.shape[0] < 1:
        raise ValueError(f"{what}: K must be a square matrix of at least one row, got shape {K.shape}")
    return K


def scatter_tables_host(K):
    """(K1 float64 [n + 1], K2 float64 [n + 1, n + 1], Jt float64 [n + 1, n + 1] with Jt[l, t] = J(t, l) where t < l -
    the other cells are never read - and the flag) of the definitions for one kernel matrix ``K`` [n, n]."""
    K = _square(K, "scatter_tables_host")
    n = K.shape[0]
    K1 = np.zeros(n + 1, dtype=np.float64)
    for r in range(n):
        K1[r + 1] = K1[r] + K[r, r]
    K2 = np.zeros((n + 1, n + 1), dtype=np.float64)
    with np.errstate(all="ignore"):
        K2[1:, 1:] = np.cumsum(np.cumsum(K, axis=0), axis=1)
        d = np.diag(K2)
        l, t = np.arange(n + 1).reshape(-1, 1), np.arange(n + 1).reshape(1, -1)
        Jt = (K1[l] - K1[t]) - (((d[l] + d[t]) - K2) - K2.T) / (l - t).astype(np.float64)
    return K1, K2, Jt, int(not np.isfinite(K2[n, n]))


def _programme(Jt, m, lmin):
    """scores float64 [m + 1] and p int64 [m + 1, n + 1] of the definitions on a given Jt, m <= n // lmin - 1 stages."""
    n = Jt.shape[0] - 1
    prev = np.full(n + 1, np.inf)
    prev[1:] = Jt[1:, 0]
    scores = np.zeros(m + 1, dtype=np.float64)
    scores[0] = prev[n]
    p = np.zeros((m + 1, n + 1), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(1, m + 1):
            cur = np.full(n + 1, np.inf)
            lo = k * lmin
            for l in range(lo + lmin, n + 1):
                c = prev[lo:l - lmin + 1] + Jt[l, lo:l - lmin + 1]
                a = int(np.argmin(c))
                cur[l], p[k, l] = c[a], a + lo
            scores[k], prev = cur[n], cur
    return scores, p


def _backtrack(p, m, n):
    cps, cur = np.zeros(m, dtype=np.int64), n
    for k in range(m, 0, -1):
        cps[k - 1] = cur = int(p[k, cur])
    return cps


def max_change_points(n, ncp=None, lmin=1):
    """m_max of the definitions."""
    ncp = n - 1 if ncp is None else int(ncp)
    if ncp < 0 or int(lmin) < 1:
        raise ValueError(f"kts: ncp must be >= 0 and lmin >= 1, got ncp = {ncp}, lmin = {lmin}")
    return max(0, min(ncp, n // int(lmin) - 1))


def cpd_nonlin_host(K, m, lmin=1):
    """The fixed-m form: (change_points int64 [m], scores float64 [m + 1]) for exactly ``m`` change points of segments
    no shorter than ``lmin`` on the kernel matrix ``K``; scores[k] = the least total scatter with k change points."""
    K = _square(K, "cpd_nonlin_host")
    n, m = K.shape[0], int(m)
    if m < 0 or m > max_change_points(n, None, lmin):
        raise ValueError(f"cpd_nonlin_host: {m} change points of segments >= {lmin} do not fit {n} samples")
    scores, p = _programme(scatter_tables_host(K)[2], m, int(lmin))
    return _backtrack(p, m, n), scores


def cpd_auto_host(K, ncp=None, vmax=1.0, lmin=1, select="auto"):
    """(change_points int64 [m_best], costs float64 [m_max + 1], scores float64 [m_max + 1], flag) of the definitions
    on the kernel matrix ``K``: the number of change points is the smallest of least penalised cost (select="auto") or
    m_max (select="fixed").  A flagged K gives no change point and NaN costs."""
    if select not in ("auto", "fixed"):
        raise ValueError(f"cpd_auto_host: select must be 'auto' or 'fixed', got {select!r}")
    K = _square(K, "cpd_auto_host")
    n = K.shape[0]
    m_max = max_change_points(n, ncp, lmin)
    _, _, Jt, flag = scatter_tables_host(K)
    if flag:
        nan = np.full(m_max + 1, np.nan)
        return np.zeros(0, dtype=np.int64), nan, nan.copy(), 1
    scores, p = _programme(Jt, m_max, int(lmin))
    with np.errstate(all="ignore"):
        costs = scores / np.float64(n) + kts_penalties(n, m_max, vmax)
    m_best = m_max if select == "fixed" else int(np.argmin(costs))
    return _backtrack(p, m_best, n), costs, scores, 0


def shots_from_change_points(change_points, n_frames, stride):
    """The [(start, end)] list in frame rows of the definitions."""
    b = [0] + [int(c) * int(stride) for c in change_points] + [int(n_frames)]
    return list(zip(b[:-1], b[1:]))


def kts_host(features, stride=15, ncp=None, vmax=1.0, lmin=1, select="auto"):
    """KTS of ONE video on the host: ``features`` fp32 [N, D].  Returns (change_points int64 (sample indices), shots
    [(start, end)] in frame rows, costs float64 [m_max + 1], flag); K is numpy's X64 @ X64.T of the subsampled rows."""
    x = np.asarray(features, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] < 1 or int(stride) < 1:
        raise ValueError(f"kts_host: features must be [N >= 1, D] and stride >= 1, got {x.shape}, stride {stride}")
    x64 = x[::int(stride)].astype(np.float64)
    if x64.shape[0] > KTS_MAX_SAMPLES:
        raise ValueError(f"kts_host: {x64.shape[0]} samples, above the limit {KTS_MAX_SAMPLES}")
    with np.errstate(all="ignore"):
        K = x64 @ x64.T
    cps, costs, _, flag = cpd_auto_host(K, ncp, vmax, lmin, select)
    return cps, shots_from_change_points(cps, x.shape[0], stride), costs, flag


# --------------------------------------------------------------------------- device form
class KtsResult:
    """What kts_batch_device leaves on the device for V videos: ``plan`` (the ops.KtsTables), ``gram`` (the packed fp64
    K), ``change_points`` int64 [shot_cap] (per video slot, -1 after the m_best entries), ``shot_offsets`` int64 [V + 1]
    and ``shots`` int64 [shot_cap, 2] (video-relative frame rows: the table evaluation.keyshots.keyshot_summaries_device
    consumes where it lies), ``shot_cap`` (the plan's), ``costs`` / ``scores`` float64 [shot_cap], ``totals`` int64
    [V, 4] = (m_best, n, m_max, flag).  Nothing has been read back; host() is the one download."""

    def __init__(self, plan, gram, out):
        self.plan, self.gram, self.shot_cap = plan, gram, plan.shot_cap
        self.change_points, self.shot_offsets, self.shots = out["change_points"], out["shot_offsets"], out["shots"]
        self.costs, self.scores, self.totals = out["costs"], out["scores"], out["totals"]
        self._host = None

    def host(self):
        """One dict per video - ``shots`` [(start, end)], ``change_points`` int64 [m_best], ``costs`` float64
        [m_max + 1], ``flag`` - from ONE download (the fp64 costs travel as their bit patterns), kept."""
        if self._host is None:
            import torch
            plan, nv, cap = self.plan, self.plan.nvideos, self.shot_cap
            flat = torch.cat([self.shot_offsets, self.shots.reshape(-1), self.change_points, self.totals.reshape(-1),
                              self.costs.view(torch.int64)]).cpu().numpy()
            off, shots, cps, totals, costs = np.split(flat, np.cumsum([nv + 1, 2 * cap, cap, 4 * nv]))
            shots, totals, costs = shots.reshape(cap, 2), totals.reshape(nv, 4), costs.view(np.float64)
            if off[nv] > cap or (np.diff(off) != totals[:, 0] + 1).any():
                raise RuntimeError(f"kts_batch_device: shot offsets {off.tolist()} do not match the totals")
            c0 = plan.cost_offsets
            self._host = [{"shots": [(int(s), int(e)) for s, e in shots[off[v]:off[v + 1]]],
                           "change_points": cps[c0[v]:c0[v] + totals[v, 0]].copy(),
                           "costs": costs[c0[v]:c0[v + 1]].copy(), "flag": int(totals[v, 3])} for v in range(nv)]
        return self._host

    def shot_lists(self):
        """host()'s shot lists alone: one [(start, end)] list per video."""
        return [h["shots"] for h in self.host()]


def kts_batch_device(features, video_offsets, stride=15, ncp=None, vmax=1.0, lmin=1, select="auto"):
    """KTS of every video of a ragged batch on the device, nothing read back: ``features`` fp32 device [N, D] (the
    videos' per-frame embeddings concatenated, e.g. FrameScoringPipeline.embed's; unit column stride, any row pitch),
    ``video_offsets`` the host frame offsets [V + 1] or a prepared ops.KtsTables (then stride, ncp, vmax and lmin are
    the plan's).  One Gram launch on the fp64 matrix cores, three for the scatter tables, two for the dynamic programme
    and the shot table.  Returns a KtsResult."""
    import torch
    from .. import ops
    if not isinstance(features, torch.Tensor) or not features.is_cuda:
        raise ValueError("kts_batch_device: features must be a device tensor (there is no CPU fallback)")
    plan = video_offsets if isinstance(video_offsets, ops.KtsTables) else \
        ops.KtsTables(video_offsets, stride, ncp, vmax, lmin, features.device)
    gram = ops.kts_gram(plan, features)
    return KtsResult(plan, gram, ops.kts_segment(plan, gram, select))
