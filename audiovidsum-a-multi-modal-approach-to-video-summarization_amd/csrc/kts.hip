// Kernel temporal segmentation (Potapov et al., ECCV 2014: cpd_nonlin + cpd_auto, linear kernel) of a ragged batch of
// videos: the Gram matrix of the subsampled frame features on the fp64 matrix cores, the scatter tables, the dynamic
// programme with its model selection and backtrack, and the shot table the keyshot knapsack consumes where it lies.
// The definitions are those of features/kts.py, whose numpy oracle everything after the Gram matrix equals bit for bit:
// fixed fp64 recurrences, no atomics, nothing depends on the launch geometry.  No kernel here waits on another
// workgroup: a launch boundary is the only synchronisation between workgroups, and every loop bound comes from the
// host plan (ops.KtsTables), never from a value computed on the device.
//
// The plan's table `videos` int64 [V][KT_COLS] = (first feature row, frames N, samples n, m_max, and the first entry of
// the video's block in: the packed K / R buffers [n][n], K1 [n + 1], Jt [n + 1][n + 1], p [m_max + 1][n + 1], the
// cost / change-point / shot slots [m_max + 1]).  It is trusted, like every other plan's offsets.
// The workspace: K1 | R | Jt (fp64) | p (uint16), each part starting at a multiple of 256 bytes.
#include "avs_internal.h"

// the sizes ops.KtsTables shares (include/avsum_hip.h)
#define KT_COLS AVS_KTS_VIDEO_COLS
#define KT_MAX_SAMPLES AVS_KTS_MAX_SAMPLES
#define KT_TILE AVS_KTS_TILE                 // Gram tile: 4 waves x 16 rows, 4 column tiles of 16
#define KT_DP_THREADS 1024
#define KT_DP_WAVES (KT_DP_THREADS / AVS_WAVE)
#define KT_DP_ROWS 4                         // values of l a wave works on side by side
#define KT_JT_L 8                            // rows l of Jt per wave: the 64 bytes of R[t - 1][l - 1 ..] a lane reads
#define KT_MAX_VIDEOS AVS_KTS_MAX_VIDEOS

typedef double kt_f64x4 __attribute__((ext_vector_type(4)));

struct kt_video {
  long long row0, frames, n, m_max, k_off, k1_off, jt_off, p_off, c_off;
};
__device__ __forceinline__ kt_video kt_load(const long long* __restrict__ videos, int v) {
  const long long* t = videos + (long long)v * KT_COLS;
  kt_video r = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
  return r;
}

static inline size_t kt_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool kt_entries_ok(int64_t k1, int64_t k, int64_t jt, int64_t p) {
  const int64_t lim = (int64_t)1 << 31;
  return k1 >= 1 && k >= 1 && jt >= 1 && p >= 1 && k1 < lim && k < lim && jt < lim && p < lim;
}

extern "C" size_t avs_kts_workspace_bytes(int64_t k1_entries, int64_t k_entries, int64_t jt_entries, int64_t p_entries) {
  if (!kt_entries_ok(k1_entries, k_entries, jt_entries, p_entries)) return 0;
  return kt_align((size_t)k1_entries * 8) + kt_align((size_t)k_entries * 8) + kt_align((size_t)jt_entries * 8) +
         kt_align((size_t)p_entries * 2);
}

struct kt_ws {
  double *k1, *r, *jt;
  unsigned short* p;
};
static inline kt_ws kt_split(void* ws, int64_t k1_entries, int64_t k_entries, int64_t jt_entries) {
  char* b = (char*)ws;
  kt_ws w;
  w.k1 = (double*)b;
  b += kt_align((size_t)k1_entries * 8);
  w.r = (double*)b;
  b += kt_align((size_t)k_entries * 8);
  w.jt = (double*)b;
  b += kt_align((size_t)jt_entries * 8);
  w.p = (unsigned short*)b;
  return w;
}

// ---------------------------------------------------------------------------
// 1. K[i, j] = sum_d float64(x_i[d]) * float64(x_j[d]) on v_mfma_f64_16x16x4_f64.  A workgroup owns one 64 x 64 tile
// (video, ti <= tj) of the plan's tile table; wave w the rows 16 w .. of it against the four 16-column tiles.  The
// features are read where they lie (row row0 + i * stride, pitch ld, 4-byte alignment only) and widened, so every
// product is exact and a sum depends on the order of d alone: d in chunks of 16, inside a chunk lane quarter q feeds
// d = 16 c + 4 q + s at MFMA step s - the same for every tile, so a video's block does not depend on the batch.  Lane l
// feeds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]; result register j is row (l >> 4) + 4 j, column l & 15.
// Only the elements row <= col are stored, each to [row][col] and [col][row] from the one register.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kts_gram_kernel(const float* __restrict__ x, long long ld, int d, long long stride,
                                                       const long long* __restrict__ videos, const int* __restrict__ tiles,
                                                       double* __restrict__ gram) {
  const int* tile = tiles + 3ll * blockIdx.x;
  const int v = tile[0], ti = tile[1], tj = tile[2];
  const kt_video vd = kt_load(videos, v);
  const int n = (int)vd.n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  if (ti * KT_TILE + wave * 16 >= n) return;                           // (uniform over the wave)
  int ri = ti * KT_TILE + wave * 16 + lr;
  ri = ri < n ? ri : n - 1;                                            // (rows past the video: read a valid row, store nothing)
  const float* __restrict__ arow = x + (vd.row0 + (long long)ri * stride) * ld;
  const float* __restrict__ brow[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    int cj = tj * KT_TILE + nt * 16 + lr;
    cj = cj < n ? cj : n - 1;
    brow[nt] = x + (vd.row0 + (long long)cj * stride) * ld;
  }
  kt_f64x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (kt_f64x4){0.0, 0.0, 0.0, 0.0};
  int k0 = 0;
  for (; k0 + 16 <= d; k0 += 16) {
    const int k = k0 + 4 * lq;
    float a[4], b[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = arow[k + s];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int s = 0; s < 4; ++s) b[nt][s] = brow[nt][k + s];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[s], (double)b[nt][s], acc[nt], 0, 0, 0);
  }
  if (k0 < d) {                                                        // the last chunk: zeros past d
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * lq + s;
      const double a = k < d ? (double)arow[k] : 0.0;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const double b = k < d ? (double)brow[nt][k] : 0.0;
        acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nt], 0, 0, 0);
      }
    }
  }
  double* __restrict__ kv = gram + vd.k_off;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = tj * KT_TILE + nt * 16 + lr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = ti * KT_TILE + wave * 16 + lq + 4 * j;
      if (row < n && col < n && row <= col) {
        const double val = acc[nt][j];
        kv[(long long)row * n + col] = val;
        kv[(long long)col * n + row] = val;
      }
    }
  }
}

extern "C" int avs_kts_gram_f64(const float* d_x, int64_t rows, int d, int64_t ld, int64_t stride, const int64_t* d_videos,
                                int nvideos, const int* d_tiles, int64_t ntiles, double* d_gram, int64_t k_entries,
                                avs_stream_t stream) {
  AVS_REQUIRE(rows >= 1 && d >= 1 && ld >= d && stride >= 1 && nvideos >= 1 && nvideos <= KT_MAX_VIDEOS && ntiles >= 1 &&
                  ntiles < ((int64_t)1 << 31) && k_entries >= 1 && k_entries < ((int64_t)1 << 31), AVS_E_SHAPE,
              "avs_kts_gram_f64: rows=%lld d=%d ld=%lld stride=%lld nvideos=%d ntiles=%lld k_entries=%lld", (long long)rows,
              d, (long long)ld, (long long)stride, nvideos, (long long)ntiles, (long long)k_entries);
  AVS_REQUIRE(d_x && d_videos && d_tiles && d_gram, AVS_E_ARG, "avs_kts_gram_f64: null pointer");
  AVS_REQUIRE((((uintptr_t)d_x) & 3u) == 0 && (((uintptr_t)d_gram) & 7u) == 0, AVS_E_ARG,
              "avs_kts_gram_f64: the features need 4-byte and the Gram buffer 8-byte alignment");
  hipLaunchKernelGGL(kts_gram_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, d_x, (long long)ld, d,
                     (long long)stride, (const long long*)d_videos, d_tiles, d_gram);
  AVS_CHECK_LAUNCH("avs_kts_gram_f64");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 2. The scatter tables.  C = cumsum(K, axis 0): one lane walks one column, neighbouring lanes neighbouring columns
// (every step of a wave reads and writes one run of a row).  R = cumsum(C, axis 1) in place: one lane walks one row,
// neighbouring lanes neighbouring rows, eight columns (64 bytes) at a step.  Both sums are strictly sequential, the
// order of np.cumsum.  K2[a][b] = R[a - 1][b - 1], 0 on its first row and column.  K1 is the sequential sum of the
// diagonal (the lane of column 0 walks it).  Then Jt[l][t] = J(t, l) for t < l, contiguous in t: a wave takes 64 t and
// eight l, so that the 64 bytes R[t - 1][l - 1 .. l + 6] a lane needs for K2[t][l] are read once.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kts_colsum_kernel(const double* __restrict__ gram, const long long* __restrict__ videos,
                                                        double* __restrict__ rbuf, double* __restrict__ k1buf) {
  const kt_video vd = kt_load(videos, blockIdx.y);
  const int n = (int)vd.n;
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  const double* __restrict__ kv = gram + vd.k_off;
  double* __restrict__ rv = rbuf + vd.k_off;
  double acc = kv[c];                                                  // (np.cumsum starts from the element, not from 0)
  rv[c] = acc;
#pragma unroll 8
  for (int r = 1; r < n; ++r) {
    acc += kv[(long long)r * n + c];
    rv[(long long)r * n + c] = acc;
  }
  if (c == 0) {
    double* __restrict__ k1 = k1buf + vd.k1_off;
    double s = 0.0;
    k1[0] = 0.0;
#pragma unroll 8
    for (int r = 0; r < n; ++r) {
      s += kv[(long long)r * n + r];
      k1[r + 1] = s;
    }
  }
}

__global__ __launch_bounds__(64) void kts_rowsum_kernel(const long long* __restrict__ videos, double* __restrict__ rbuf,
                                                        long long* __restrict__ flags) {
  const kt_video vd = kt_load(videos, blockIdx.y);
  const int n = (int)vd.n;
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n) return;
  double* __restrict__ row = rbuf + vd.k_off + (long long)r * n;
  double acc = row[0];
  int c = 1;
  for (; c + 8 <= n; c += 8) {
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = row[c + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc += x[i];
      row[c + i] = acc;
    }
  }
  for (; c < n; ++c) {
    acc += row[c];
    row[c] = acc;
  }
  if (r == n - 1) flags[blockIdx.y] = isfinite(acc) ? 0 : 1;           // acc = K2[n][n]
}

__global__ __launch_bounds__(256) void kts_jt_kernel(const long long* __restrict__ videos, const double* __restrict__ rbuf,
                                                     const double* __restrict__ k1buf, double* __restrict__ jtbuf) {
  const kt_video vd = kt_load(videos, blockIdx.z);
  const int n = (int)vd.n;
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int l0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * KT_JT_L + 1;  // l = l0 .. l0 + 7, l >= 1
  if (t >= n || l0 > n || t >= l0 + KT_JT_L - 1) return;
  const double* __restrict__ rv = rbuf + vd.k_off;
  const double* __restrict__ k1 = k1buf + vd.k1_off;
  double* __restrict__ jt = jtbuf + vd.jt_off;
  const double k1t = k1[t];
  const double dt = t > 0 ? rv[(long long)(t - 1) * n + (t - 1)] : 0.0;         // K2[t][t]
#pragma unroll
  for (int i = 0; i < KT_JT_L; ++i) {
    const int l = l0 + i;
    if (l > n || t >= l) continue;
    const double dl = rv[(long long)(l - 1) * n + (l - 1)];                     // K2[l][l]
    const double klt = t > 0 ? rv[(long long)(l - 1) * n + (t - 1)] : 0.0;      // K2[l][t]
    const double ktl = t > 0 ? rv[(long long)(t - 1) * n + (l - 1)] : 0.0;      // K2[t][l]
    jt[(long long)l * (n + 1) + t] = (k1[l] - k1t) - (((dl + dt) - klt) - ktl) / (double)(l - t);
  }
}

extern "C" int avs_kts_scatters_f64(const double* d_gram, const int64_t* d_videos, int nvideos, int max_n, void* d_ws,
                                    size_t ws_bytes, int64_t k1_entries, int64_t k_entries, int64_t jt_entries,
                                    int64_t p_entries, int64_t* d_flags, avs_stream_t stream) {
  AVS_REQUIRE(nvideos >= 1 && nvideos <= KT_MAX_VIDEOS && max_n >= 1 && max_n <= KT_MAX_SAMPLES &&
                  kt_entries_ok(k1_entries, k_entries, jt_entries, p_entries), AVS_E_SHAPE,
              "avs_kts_scatters_f64: nvideos=%d max_n=%d entries=(%lld, %lld, %lld, %lld)", nvideos, max_n,
              (long long)k1_entries, (long long)k_entries, (long long)jt_entries, (long long)p_entries);
  AVS_REQUIRE(d_gram && d_videos && d_ws && d_flags, AVS_E_ARG, "avs_kts_scatters_f64: null pointer");
  AVS_REQUIRE((((uintptr_t)d_ws) & 7u) == 0 && (((uintptr_t)d_gram) & 7u) == 0, AVS_E_ARG,
              "avs_kts_scatters_f64: the Gram buffer and the workspace need 8-byte alignment");
  AVS_REQUIRE(ws_bytes >= avs_kts_workspace_bytes(k1_entries, k_entries, jt_entries, p_entries), AVS_E_WORKSPACE,
              "avs_kts_scatters_f64: workspace of %zu bytes, need %zu", ws_bytes,
              avs_kts_workspace_bytes(k1_entries, k_entries, jt_entries, p_entries));
  const kt_ws w = kt_split(d_ws, k1_entries, k_entries, jt_entries);
  const unsigned gx = (unsigned)avs_cdiv(max_n, 64);
  hipLaunchKernelGGL(kts_colsum_kernel, dim3(gx, (unsigned)nvideos), dim3(64), 0, (hipStream_t)stream, d_gram,
                     (const long long*)d_videos, w.r, w.k1);
  hipLaunchKernelGGL(kts_rowsum_kernel, dim3(gx, (unsigned)nvideos), dim3(64), 0, (hipStream_t)stream,
                     (const long long*)d_videos, w.r, (long long*)d_flags);
  hipLaunchKernelGGL(kts_jt_kernel, dim3(gx, (unsigned)avs_cdiv(max_n, 4 * KT_JT_L), (unsigned)nvideos), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)d_videos, w.r, w.k1, w.jt);
  AVS_CHECK_LAUNCH("avs_kts_scatters_f64");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 3. The dynamic programme of one video per workgroup of 1024 threads; the stages k are separated by workgroup
// barriers.  The two live rows I_{k-1}, I_k sit in LDS.  A wave takes one l (four side by side), its lanes stride over
// t = k lmin .. l - lmin (consecutive lanes read consecutive cells of the LDS row and of Jt[l]); a lane keeps the
// first minimum of its ascending t, and the lanes are reduced by (value, then smaller t): the smallest t attaining the
// minimum, np.argmin's.  p_k[l] goes to the uint16 workspace.  Thread 0 writes score[k] and cost[k] as the stages
// finish and keeps the smallest k attaining the least cost; it backtracks in m_best <= m_max steps with every index
// clamped into k lmin .. cur - lmin, so whatever the tables hold the change points ascend inside the video.
// A flagged video (K2[n][n] not finite) skips the stages: m_best = 0, costs NaN.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(KT_DP_THREADS) void kts_dp_kernel(const long long* __restrict__ videos, int lmin, int fixed,
                                                               const double* __restrict__ pen,
                                                               const double* __restrict__ jtbuf,
                                                               unsigned short* __restrict__ pbuf,
                                                               const long long* __restrict__ flags,
                                                               double* __restrict__ scores, double* __restrict__ costs,
                                                               long long* __restrict__ change_points,
                                                               long long* __restrict__ totals) {
  __shared__ double rows[2][KT_MAX_SAMPLES + 1];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const kt_video vd = kt_load(videos, v);
  const int n = (int)vd.n, m_max = (int)vd.m_max;
  const double* __restrict__ jt = jtbuf + vd.jt_off;
  unsigned short* __restrict__ p = pbuf + vd.p_off;
  const bool flagged = flags[v] != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  for (int j = tid; j <= m_max; j += KT_DP_THREADS) {
    change_points[vd.c_off + j] = -1;
    if (flagged) {
      scores[vd.c_off + j] = nan;
      costs[vd.c_off + j] = nan;
    }
  }
  int m_best = 0;
  if (!flagged) {                                                      // (uniform over the workgroup)
    for (int l = 1 + tid; l <= n; l += KT_DP_THREADS) rows[0][l] = jt[(long long)l * (n + 1)];
    __syncthreads();
    double best_cost = 0.0;
    if (tid == 0) {
      const double s = rows[0][n];
      best_cost = s / (double)n + pen[vd.c_off];
      scores[vd.c_off] = s;
      costs[vd.c_off] = best_cost;
    }
    int cur = 0;
    for (int k = 1; k <= m_max; ++k) {
      const double* prev = rows[cur];
      double* next = rows[cur ^ 1];
      const int lo = k * lmin;
      const double pen_k = tid == 0 ? pen[vd.c_off + k] : 0.0;         // (asked for ahead of the stage's end)
      // a wave takes KT_DP_ROWS values of l at a time (l, l + 16, ..): their Jt rows are loaded side by side, so the
      // latency of one global load is paid once for the group; a cell's arithmetic does not depend on the grouping
      for (int l0 = lo + lmin + wave; l0 <= n; l0 += KT_DP_WAVES * KT_DP_ROWS) {
        const double* jrow[KT_DP_ROWS];
        int hi[KT_DP_ROWS], bt[KT_DP_ROWS];
        double bv[KT_DP_ROWS];
        const double first = prev[lo];
        int hi_max = lo;
#pragma unroll
        for (int u = 0; u < KT_DP_ROWS; ++u) {
          int l = l0 + u * KT_DP_WAVES;
          const bool live = l <= n;
          l = live ? l : l0;                                           // (a row past n repeats the first: nothing is stored)
          jrow[u] = jt + (long long)l * (n + 1);
          hi[u] = live ? l - lmin : lo - 1;                            // lo <= hi for a live row
          hi_max = hi[u] > hi_max ? hi[u] : hi_max;
          bv[u] = first + jrow[u][lo];
          bt[u] = lo;
        }
        // the loads are unconditional, so that the four are asked for together: a cell past its row's range reads
        // column lo and is dropped
        for (int t = lo + lane; t <= hi_max; t += AVS_WAVE) {
          const double pv = prev[t];
          double x[KT_DP_ROWS];
#pragma unroll
          for (int u = 0; u < KT_DP_ROWS; ++u) x[u] = jrow[u][t <= hi[u] ? t : lo];
#pragma unroll
          for (int u = 0; u < KT_DP_ROWS; ++u) {
            const double c = pv + x[u];
            if (t <= hi[u] && c < bv[u]) {
              bv[u] = c;
              bt[u] = t;
            }
          }
        }
#pragma unroll
        for (int off = AVS_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
          for (int u = 0; u < KT_DP_ROWS; ++u) {
            const double ov = __shfl_xor(bv[u], off, AVS_WAVE);
            const int ot = __shfl_xor(bt[u], off, AVS_WAVE);
            if (ov < bv[u] || (ov == bv[u] && ot < bt[u])) {
              bv[u] = ov;
              bt[u] = ot;
            }
          }
        }
        if (lane == 0) {
#pragma unroll
          for (int u = 0; u < KT_DP_ROWS; ++u) {
            const int l = l0 + u * KT_DP_WAVES;
            if (l <= n) {
              next[l] = bv[u];
              p[(long long)k * (n + 1) + l] = (unsigned short)bt[u];
            }
          }
        }
      }
      __syncthreads();
      cur ^= 1;
      if (tid == 0) {
        const double s = rows[cur][n];
        const double c = s / (double)n + pen_k;
        scores[vd.c_off + k] = s;
        costs[vd.c_off + k] = c;
        if (c < best_cost) {
          best_cost = c;
          m_best = k;
        }
      }
    }
    if (fixed) m_best = m_max;
  }
  __syncthreads();                                                     // the p rows and the -1 fill before thread 0's tail
  if (tid == 0) {
    int cur = n;
    for (int k = m_max; k >= 1; --k) {                                 // (bound from the plan; the steps above m_best idle)
      if (k > m_best) continue;
      int t = p[(long long)k * (n + 1) + cur];
      const int lo = k * lmin, hi = cur - lmin;
      t = t < lo ? lo : (t > hi ? hi : t);
      change_points[vd.c_off + k - 1] = t;
      cur = t;
    }
    long long* t4 = totals + 4ll * v;
    t4[0] = m_best;
    t4[1] = n;
    t4[2] = m_max;
    t4[3] = flagged ? 1 : 0;
  }
}

// The shot table in the layout of avs_shot_tables_fill, one workgroup per video: shot_offsets = the exclusive prefix of
// m_best + 1 (every workgroup sums the totals of the previous launch itself: integers, any order), the shots
// (b_j, b_{j+1}) with b_0 = 0, b_j = cp[j - 1] * stride, b_last = N, and zeros in the rows past the last shot.
__global__ __launch_bounds__(256) void kts_shots_kernel(const long long* __restrict__ videos, int nvideos, long long stride,
                                                        const long long* __restrict__ totals,
                                                        const long long* __restrict__ change_points,
                                                        long long shot_cap, long long* __restrict__ shot_offsets,
                                                        long long* __restrict__ shots) {
  __shared__ long long red[2][256];
  const int v = blockIdx.x, tid = threadIdx.x;
  long long before = 0, all = 0;
  for (int u = tid; u < nvideos; u += 256) {
    const long long mm = videos[(long long)u * KT_COLS + 3];
    long long mb = totals[4ll * u];
    mb = mb < 0 ? 0 : (mb > mm ? mm : mb);
    all += mb + 1;
    if (u < v) before += mb + 1;
  }
  red[0][tid] = before;
  red[1][tid] = all;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  const long long base = red[0][0], total = red[1][0];
  const kt_video vd = kt_load(videos, v);
  long long mb = totals[4ll * v];
  mb = mb < 0 ? 0 : (mb > vd.m_max ? vd.m_max : mb);
  if (tid == 0) {
    shot_offsets[v] = base;
    if (v == nvideos - 1) shot_offsets[nvideos] = total;
  }
  const long long* cp = change_points + vd.c_off;
  const long long spare0 = total + (vd.c_off - base);                  // the video's share of the rows past the last shot
  for (long long j = tid; j <= vd.m_max; j += 256) {
    long long row, s = 0, e = 0;
    if (j <= mb) {
      row = base + j;
      s = j == 0 ? 0 : cp[j - 1] * stride;
      e = j == mb ? vd.frames : cp[j] * stride;
    } else {
      row = spare0 + (j - mb - 1);
    }
    if (row >= 0 && row < shot_cap) {
      shots[2 * row] = s;
      shots[2 * row + 1] = e;
    }
  }
}

extern "C" int avs_kts_dp_f64(const int64_t* d_videos, int nvideos, int max_n, int lmin, int64_t stride, int select_fixed,
                              const double* d_penalties, void* d_ws, size_t ws_bytes, int64_t k1_entries,
                              int64_t k_entries, int64_t jt_entries, int64_t p_entries, int64_t cost_cap,
                              const int64_t* d_flags, double* d_scores, double* d_costs, int64_t* d_change_points,
                              int64_t* d_shot_offsets, int64_t* d_shots, int64_t* d_totals, avs_stream_t stream) {
  AVS_REQUIRE(nvideos >= 1 && nvideos <= KT_MAX_VIDEOS && max_n >= 1 && max_n <= KT_MAX_SAMPLES && lmin >= 1 &&
                  stride >= 1 && cost_cap >= nvideos && cost_cap < ((int64_t)1 << 31) &&
                  kt_entries_ok(k1_entries, k_entries, jt_entries, p_entries), AVS_E_SHAPE,
              "avs_kts_dp_f64: nvideos=%d max_n=%d lmin=%d stride=%lld cost_cap=%lld entries=(%lld, %lld, %lld, %lld)",
              nvideos, max_n, lmin, (long long)stride, (long long)cost_cap, (long long)k1_entries, (long long)k_entries,
              (long long)jt_entries, (long long)p_entries);
  AVS_REQUIRE(d_videos && d_penalties && d_ws && d_flags && d_scores && d_costs && d_change_points && d_shot_offsets &&
                  d_shots && d_totals, AVS_E_ARG, "avs_kts_dp_f64: null pointer");
  AVS_REQUIRE((((uintptr_t)d_ws) & 7u) == 0, AVS_E_ARG, "avs_kts_dp_f64: the workspace needs 8-byte alignment");
  AVS_REQUIRE(ws_bytes >= avs_kts_workspace_bytes(k1_entries, k_entries, jt_entries, p_entries), AVS_E_WORKSPACE,
              "avs_kts_dp_f64: workspace of %zu bytes, need %zu", ws_bytes,
              avs_kts_workspace_bytes(k1_entries, k_entries, jt_entries, p_entries));
  const kt_ws w = kt_split(d_ws, k1_entries, k_entries, jt_entries);
  hipLaunchKernelGGL(kts_dp_kernel, dim3((unsigned)nvideos), dim3(KT_DP_THREADS), 0, (hipStream_t)stream,
                     (const long long*)d_videos, lmin, select_fixed ? 1 : 0, d_penalties, w.jt, w.p,
                     (const long long*)d_flags, d_scores, d_costs, (long long*)d_change_points, (long long*)d_totals);
  hipLaunchKernelGGL(kts_shots_kernel, dim3((unsigned)nvideos), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)d_videos, nvideos, (long long)stride, (const long long*)d_totals,
                     (const long long*)d_change_points, (long long)cost_cap, (long long*)d_shot_offsets,
                     (long long*)d_shots);
  AVS_CHECK_LAUNCH("avs_kts_dp_f64");
  return AVS_OK;
}
