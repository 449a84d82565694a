// Batched fusion: the three steps of fusion.hip (cost matrix, exact DTW, path-weighted gather) for P ragged
// (visual rows [n_p, D], audio rows [m_p, D]) pairs in a fixed number of launches, whatever P is.  The host builds the
// tables once per batch layout (ops.FusionTables); nothing here reads a result back or synchronises.
//
// Pair table: int64 [P, 8] = (v_row0, n, a_row0, m, cell_off, path_off, row_off, 0)
//   cell_off  first element of the pair's [n, m] row-major block in the cost buffer (doubles) and in the code workspace
//             (bytes): the pairs' blocks lie one after another, nothing padded
//   path_off  first row of the pair's path slot (capacity n + m - 1 rows of two int64)
//   row_off   first entry of the pair's n row counts
#include "avs_internal.h"
#include <math.h>

// the sizes ops.FusionTables shares (include/avsum_hip.h)
#define FB_COLS AVS_FUSION_PAIR_COLS  // int64 per pair-table row
#define FB_MAX_N AVS_FUSION_MAX_N     // as avs_dtw_path_f64: 3 * 6400 * 8 B = 150 KiB of the 160 KiB LDS
#define FB_SMALL_L AVS_FUSION_SMALL_L // class 0: min(n, m) <= 64, one wave per pair, four pairs per workgroup
#define FB_MID_L AVS_FUSION_MID_L     // class 1: min(n, m) <= 512, one 256-thread workgroup per pair; above: 1024 threads

// ---------------------------------------------------------------------------
// Cost matrices.  One 16x16-thread block per entry of the (pair, row tile, column tile) table; the arithmetic and its
// order are cdist_kernel's (float64 direct difference, k ascending in steps of 32, sqrt), so a pair's block is bit for
// bit what avs_cdist_f64 gives for that pair.
// ---------------------------------------------------------------------------
#define CB_T AVS_FUSION_TILE
#define CB_K 32
__global__ __launch_bounds__(256) void cdist_batch_kernel(const float* __restrict__ v, const float* __restrict__ a, int d,
                                                          const int64_t* __restrict__ pairs,
                                                          const int* __restrict__ tiles, double* __restrict__ out) {
  __shared__ float sv[CB_T][CB_K + 1];
  __shared__ float sa[CB_T][CB_K + 1];
  const int* tile = tiles + 3 * (long long)blockIdx.x;
  const int64_t* pr = pairs + FB_COLS * (long long)tile[0];
  const float* pv = v + pr[0] * d;
  const float* pa = a + pr[2] * d;
  const int tv = (int)pr[1], ta = (int)pr[3];
  double* po = out + pr[4];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = tile[1] * CB_T, j0 = tile[2] * CB_T;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int k0 = 0; k0 < d; k0 += CB_K) {
    for (int e = threadIdx.x; e < CB_T * CB_K; e += 256) {
      const int r = e / CB_K, k = e - r * CB_K;
      const int gi = i0 + r, gj = j0 + r, gk = k0 + k;
      sv[r][k] = (gi < tv && gk < d) ? pv[(long long)gi * d + gk] : 0.f;
      sa[r][k] = (gj < ta && gk < d) ? pa[(long long)gj * d + gk] : 0.f;
    }
    __syncthreads();
    const int kn = (d - k0) < CB_K ? (d - k0) : CB_K;
    for (int k = 0; k < kn; ++k) {
      const double v0 = (double)sv[ty][k], v1 = (double)sv[ty + 16][k];
      const double a0 = (double)sa[tx][k], a1 = (double)sa[tx + 16][k];
      double t;
      t = v0 - a0; acc[0][0] += t * t;
      t = v0 - a1; acc[0][1] += t * t;
      t = v1 - a0; acc[1][0] += t * t;
      t = v1 - a1; acc[1][1] += t * t;
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int gi = i0 + ty + 16 * p, gj = j0 + tx + 16 * q;
      if (gi < tv && gj < ta) po[(long long)gi * ta + gj] = sqrt(acc[p][q]);
    }
}

extern "C" int avs_cdist_batch_f64(const float* d_v, int64_t v_rows, const float* d_a, int64_t a_rows, int d,
                                   const int64_t* d_pairs, int npairs, const int32_t* d_tiles, int64_t ntiles,
                                   double* d_cost, int64_t cells, avs_stream_t stream) {
  AVS_REQUIRE(v_rows >= 0 && a_rows >= 0 && d > 0 && npairs >= 0 && ntiles >= 0 && cells >= 0, AVS_E_SHAPE,
              "avs_cdist_batch_f64: v_rows=%lld a_rows=%lld d=%d npairs=%d ntiles=%lld cells=%lld", (long long)v_rows,
              (long long)a_rows, d, npairs, (long long)ntiles, (long long)cells);
  // every pair has at least one row of each side, hence one cell and one tile
  AVS_REQUIRE(ntiles >= npairs && cells >= npairs && ntiles <= 0x7fffffffLL, AVS_E_SHAPE,
              "avs_cdist_batch_f64: ntiles=%lld cells=%lld for %d pairs", (long long)ntiles, (long long)cells, npairs);
  if (npairs == 0) return AVS_OK;
  AVS_REQUIRE(v_rows > 0 && a_rows > 0, AVS_E_SHAPE, "avs_cdist_batch_f64: %d pairs but no rows", npairs);
  AVS_REQUIRE(d_v && d_a && d_pairs && d_tiles && d_cost, AVS_E_ARG, "avs_cdist_batch_f64: null pointer");
  hipLaunchKernelGGL(cdist_batch_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, d_v, d_a, d,
                     d_pairs, d_tiles, d_cost);
  AVS_CHECK_LAUNCH("avs_cdist_batch_f64");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// DTW sweep + backtrack.  A workgroup of THREADS threads takes PPW pairs, THREADS / PPW threads each, and sweeps their
// anti-diagonals together (one barrier per diagonal, up to the longest of its pairs).  The recurrence and the tie
// order are dtw_sweep_kernel's: up (i-1,j), left (i,j-1), diagonal, under strict <.  The three live diagonals of a
// pair stay in LDS, indexed by the SHORTER side (row i when n <= m, column j otherwise), so a pair needs
// 3 * min(n, m) doubles whatever its longer side is; where a value is kept does not change it.  After the last
// barrier the first thread of each pair walks that pair's codes back from (n-1, m-1).
// ---------------------------------------------------------------------------
template <int THREADS, int PPW>
__global__ __launch_bounds__(THREADS) void dtw_batch_kernel(const double* __restrict__ cost,
                                                            const int64_t* __restrict__ pairs,
                                                            const int* __restrict__ order, int first, int count,
                                                            int lds_l, unsigned char* dir, int64_t* __restrict__ path,
                                                            int64_t* __restrict__ path_len, double* __restrict__ total,
                                                            int* __restrict__ rowcount) {
  extern __shared__ double diag[];  // [PPW][3][lds_l]
  constexpr int G = THREADS / PPW;
  const int sub = threadIdx.x / G, lane = threadIdx.x - sub * G;
  int dmax = 0;  // the same in every thread of the workgroup
#pragma unroll
  for (int s = 0; s < PPW; ++s) {
    const int q = blockIdx.x * PPW + s;
    if (q < count) {
      const int64_t* pr = pairs + FB_COLS * (long long)order[first + q];
      const int nd = (int)(pr[1] + pr[3] - 1);
      dmax = nd > dmax ? nd : dmax;
    }
  }
  const int q = blockIdx.x * PPW + sub;
  const bool have = q < count;
  int pid = 0, n = 0, m = 0;
  long long cell0 = 0, path0 = 0, row0 = 0;
  if (have) {
    pid = order[first + q];
    const int64_t* pr = pairs + FB_COLS * (long long)pid;
    n = (int)pr[1];
    m = (int)pr[3];
    cell0 = pr[4];
    path0 = pr[5];
    row0 = pr[6];
  }
  const double* c = cost + cell0;
  unsigned char* dr = dir + cell0;
  double* d0 = diag + 3 * (long long)lds_l * sub;
  double* d1 = d0 + lds_l;
  double* d2 = d1 + lds_l;
  const bool by_row = n <= m;
  const double INF = INFINITY;
  for (int d = 0; d < dmax; ++d) {
    if (d <= n + m - 2) {  // (never for an absent pair: n = m = 0)
      double* cur = d % 3 == 0 ? d0 : (d % 3 == 1 ? d1 : d2);
      const double* p1 = (d + 2) % 3 == 0 ? d0 : ((d + 2) % 3 == 1 ? d1 : d2);  // diagonal d-1
      const double* p2 = (d + 1) % 3 == 0 ? d0 : ((d + 1) % 3 == 1 ? d1 : d2);  // diagonal d-2
      const int ilo = d - (m - 1) > 0 ? d - (m - 1) : 0;
      const int ihi = d < n - 1 ? d : n - 1;
      for (int i = ilo + lane; i <= ihi; i += G) {
        const int j = d - i;
        const int t = by_row ? i : j;           // this cell's slot; (i-1,j-1) is slot t-1 either way
        const int tu = by_row ? t - 1 : t;      // slot of (i-1, j)
        const int tl = by_row ? t : t - 1;      // slot of (i, j-1)
        const double up = i > 0 ? p1[tu] : INF;
        const double left = j > 0 ? p1[tl] : INF;
        const double dg = (i > 0 && j > 0) ? p2[t - 1] : INF;
        double best = up;
        unsigned char code = 0;
        if (left < best) { best = left; code = 1; }
        if (dg < best) { best = dg; code = 2; }
        if (i == 0 && j == 0) { best = 0.0; code = 3; }
        const double val = c[(long long)i * m + j] + best;
        cur[t] = val;
        dr[(long long)i * m + j] = code;
        if (i == n - 1 && j == m - 1) total[pid] = val;
      }
    }
    __syncthreads();  // also orders this workgroup's code stores before the walk below
  }
  if (!have || lane != 0) return;
  // first pass: length and the number of path cells in every row; second pass: fill from the end so the path runs
  // start -> end
  int i = n - 1, j = m - 1, cnt = 1;
  long long len = 1;
  while (i > 0 || j > 0) {
    const unsigned char cd = dr[(long long)i * m + j];
    if (cd == 1) {
      --j;
      ++cnt;
    } else {
      rowcount[row0 + i] = cnt;
      cnt = 1;
      --i;
      if (cd != 0) --j;
    }
    ++len;
  }
  rowcount[row0] = cnt;
  path_len[pid] = len;
  int64_t* pp = path + 2 * path0;
  i = n - 1;
  j = m - 1;
  long long pos = len - 1;
  pp[2 * pos] = i;
  pp[2 * pos + 1] = j;
  while (i > 0 || j > 0) {
    const unsigned char cd = dr[(long long)i * m + j];
    if (cd == 0) --i; else if (cd == 1) --j; else { --i; --j; }
    --pos;
    pp[2 * pos] = i;
    pp[2 * pos + 1] = j;
  }
}

extern "C" int64_t avs_dtw_batch_workspace_bytes(int64_t cells) {
  if (cells <= 0) return 0;
  return (cells + 255) & ~(int64_t)255;
}

template <int THREADS, int PPW>
static int dtw_batch_launch(const double* d_cost, const int64_t* d_pairs, const int32_t* d_order, int first, int count,
                            int max_l, void* d_ws, int64_t* d_path, int64_t* d_path_len, double* d_total,
                            int32_t* d_rowcount, hipStream_t stream) {
  if (count == 0) return AVS_OK;
  const size_t shmem = (size_t)3 * max_l * PPW * sizeof(double);
  if (shmem > 64 * 1024) {
    static bool attr_set = false;  // (per instantiation)
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)dtw_batch_kernel<THREADS, PPW>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         3 * FB_MAX_N * PPW * (int)sizeof(double));
      if (e != hipSuccess) {
        avs_set_error("avs_dtw_batch_f64: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
        return AVS_E_HIP;
      }
      attr_set = true;
    }
  }
  hipLaunchKernelGGL((dtw_batch_kernel<THREADS, PPW>), dim3((unsigned)avs_cdiv(count, PPW)), dim3(THREADS), shmem, stream,
                     d_cost, d_pairs, d_order, first, count, max_l, (unsigned char*)d_ws, d_path, d_path_len, d_total,
                     d_rowcount);
  AVS_CHECK_LAUNCH("avs_dtw_batch_f64");
  return AVS_OK;
}

extern "C" int avs_dtw_batch_f64(const double* d_cost, int64_t cells, const int64_t* d_pairs, int npairs,
                                 const int32_t* d_order, int n_small, int n_mid, int n_large, int max_l_small,
                                 int max_l_mid, int max_l_large, int max_n, void* d_workspace, int64_t workspace_bytes,
                                 int64_t* d_path, int64_t* d_path_len, double* d_total, int32_t* d_rowcount,
                                 avs_stream_t stream) {
  AVS_REQUIRE(npairs >= 0 && n_small >= 0 && n_mid >= 0 && n_large >= 0 && cells >= npairs &&
                  (int64_t)n_small + n_mid + n_large == npairs,
              AVS_E_SHAPE, "avs_dtw_batch_f64: npairs=%d classes=%d+%d+%d cells=%lld", npairs, n_small, n_mid, n_large,
              (long long)cells);
  AVS_REQUIRE(max_n <= FB_MAX_N, AVS_E_SHAPE, "avs_dtw_batch_f64: n=%d exceeds the LDS-resident limit %d", max_n,
              FB_MAX_N);
  AVS_REQUIRE((n_small == 0 || (max_l_small >= 1 && max_l_small <= FB_SMALL_L)) &&
                  (n_mid == 0 || (max_l_mid > FB_SMALL_L && max_l_mid <= FB_MID_L)) &&
                  (n_large == 0 || (max_l_large > FB_MID_L && max_l_large <= FB_MAX_N)),
              AVS_E_SHAPE, "avs_dtw_batch_f64: class sizes %d/%d/%d outside (0,%d], (%d,%d], (%d,%d]", max_l_small,
              max_l_mid, max_l_large, FB_SMALL_L, FB_SMALL_L, FB_MID_L, FB_MID_L, FB_MAX_N);
  if (npairs == 0) return AVS_OK;
  AVS_REQUIRE(max_n >= 1, AVS_E_SHAPE, "avs_dtw_batch_f64: max_n=%d", max_n);
  AVS_REQUIRE(d_cost && d_pairs && d_order && d_workspace && d_path && d_path_len && d_total && d_rowcount, AVS_E_ARG,
              "avs_dtw_batch_f64: null pointer");
  AVS_REQUIRE(workspace_bytes >= avs_dtw_batch_workspace_bytes(cells), AVS_E_WORKSPACE,
              "avs_dtw_batch_f64: workspace %lld < %lld bytes", (long long)workspace_bytes,
              (long long)avs_dtw_batch_workspace_bytes(cells));
  hipStream_t s = (hipStream_t)stream;
  int rc = dtw_batch_launch<1024, 1>(d_cost, d_pairs, d_order, n_small + n_mid, n_large, max_l_large, d_workspace,
                                     d_path, d_path_len, d_total, d_rowcount, s);   // the longest first
  if (rc != AVS_OK) return rc;
  rc = dtw_batch_launch<256, 1>(d_cost, d_pairs, d_order, n_small, n_mid, max_l_mid, d_workspace, d_path, d_path_len,
                                d_total, d_rowcount, s);
  if (rc != AVS_OK) return rc;
  return dtw_batch_launch<256, 4>(d_cost, d_pairs, d_order, 0, n_small, max_l_small, d_workspace, d_path, d_path_len,
                                  d_total, d_rowcount, s);
}

// ---------------------------------------------------------------------------
// Path-weighted gather.  The path visits every row 0..n-1 of its pair, so unique(path[:,0]) is 0..n-1 and the weight
// of row i is rowcount[i] / path_len: out[out_off[p] + i, :] = x[v_row0 + i, :] * float(double(rowcount) /
// double(path_len)) for i < min(n, target_length) - gather_scale_kernel's multiply with interpolate_features' weights.
// row_pair[r] is the pair that entry r of the row counts belongs to.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fused_gather_batch_kernel(const float* __restrict__ x, long long ldx, int d,
                                                                 const int64_t* __restrict__ pairs,
                                                                 const int* __restrict__ row_pair, long long nrows,
                                                                 const int64_t* __restrict__ out_off,
                                                                 const int* __restrict__ rowcount,
                                                                 const int64_t* __restrict__ path_len,
                                                                 long long target_length, float* __restrict__ out) {
  const long long total = nrows * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / d;
    const int k = (int)(e - r * d);
    const int p = row_pair[r];
    const int64_t* pr = pairs + FB_COLS * (long long)p;
    const long long i = r - pr[6];
    if (i >= target_length) continue;
    const double w = (double)rowcount[r] / (double)path_len[p];
    out[(out_off[p] + i) * d + k] = x[(pr[0] + i) * ldx + k] * (float)w;
  }
}

extern "C" int avs_fused_gather_batch_f32(const float* d_x, int64_t ldx, int d, const int64_t* d_pairs, int npairs,
                                          const int32_t* d_row_pair, int64_t nrows, const int64_t* d_out_off,
                                          const int32_t* d_rowcount, const int64_t* d_path_len, int64_t target_length,
                                          float* d_out, avs_stream_t stream) {
  AVS_REQUIRE(d > 0 && ldx >= d && npairs >= 0 && nrows >= npairs && target_length >= 0, AVS_E_SHAPE,
              "avs_fused_gather_batch_f32: d=%d ldx=%lld npairs=%d nrows=%lld target_length=%lld", d, (long long)ldx,
              npairs, (long long)nrows, (long long)target_length);
  if (npairs == 0 || target_length == 0) return AVS_OK;
  AVS_REQUIRE(d_x && d_pairs && d_row_pair && d_out_off && d_rowcount && d_path_len && d_out, AVS_E_ARG,
              "avs_fused_gather_batch_f32: null pointer");
  long long gx = avs_cdiv(nrows * d, 256);
  if (gx > 16384) gx = 16384;
  hipLaunchKernelGGL(fused_gather_batch_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, d_x,
                     (long long)ldx, d, d_pairs, d_row_pair, (long long)nrows, d_out_off, d_rowcount, d_path_len,
                     (long long)target_length, d_out);
  AVS_CHECK_LAUNCH("avs_fused_gather_batch_f32");
  return AVS_OK;
}
