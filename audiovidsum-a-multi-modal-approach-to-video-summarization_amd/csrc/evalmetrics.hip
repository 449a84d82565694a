// Batched evaluation (scripts/evaluate.py:21-42 of the reference, for all videos at once): the mean-threshold masks with
// numpy's own reduction order, and the integer pair counts both rank correlations reduce to.  Every result is an
// integer or is computed in one fixed order: no float atomics, nothing depends on the launch geometry.
//
// The videos are segments [offsets[v], offsets[v + 1]) of concatenated vectors; the tables are trusted as in
// fusion_batch.hip (ops.EvalTables builds them).
#include "avs_internal.h"

#define EM_THREADS 256
#define EM_BUF 8192      // elements numpy's reduction hands to its pairwise sum at a time
#define EM_LEAF 128      // the pairwise sum's unrolled leaf (PW_BLOCKSIZE)
#define EM_MAX_LEAVES 128  // a leaf below a split holds at least 64 elements, so a buffer has at most 8192 / 64 leaves
// the sizes ops.EvalTables shares (include/avsum_hip.h): rows of a video per workgroup of the pair-count kernel, columns
// staged through LDS per step, the longest video, int64 per video of the fold
#define EM_TILE AVS_EVAL_TILE
#define EM_CHUNK AVS_EVAL_CHUNK
#define EM_MAX_T AVS_EVAL_MAX_T
#define EM_COLS AVS_EVAL_COLS

// ---------------------------------------------------------------------------
// Segment mean in numpy's order + mask.  One workgroup per segment.  np.mean of a contiguous vector sums buffers of
// 8192 elements left to right; a buffer of n elements is summed by pw(n):
//   n < 8     left to right from -0.0
//   n <= 128  r[k] = a[k]; r[k] += a[i + k] for i = 8, 16, .. < n - n % 8; ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)); then
//             the n % 8 last elements one by one
//   n > 128   n2 = n / 2, n2 -= n2 % 8; pw(first n2) + pw(rest)
// Thread 0 walks the recursion once and lists the leaves in order, each with the number of additions that complete
// right after it in the post-order evaluation; eight lanes take a leaf (lane k is accumulator r[k], the combine is three
// xor-shuffles: a + b and b + a are the same bits); thread 0 then replays the additions on a value stack in LDS.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(EM_THREADS) void segment_mean_mask_kernel(const T* __restrict__ x,
                                                                       const int64_t* __restrict__ offsets,
                                                                       T* __restrict__ mean,
                                                                       unsigned char* __restrict__ mask) {
  __shared__ int leaf_start[EM_MAX_LEAVES], leaf_len[EM_MAX_LEAVES], leaf_red[EM_MAX_LEAVES];
  __shared__ int st_start[32], st_len[32], st_red[32];
  __shared__ T leaf_sum[EM_MAX_LEAVES];
  __shared__ T vstack[32];
  __shared__ int nleaves;
  __shared__ T result;
  const long long a = offsets[blockIdx.x], b = offsets[blockIdx.x + 1];
  const long long n = b - a;
  const T* seg = x + a;
  const int tid = threadIdx.x;
  T total = (T)0;   // thread 0 only
  for (long long c0 = 0; c0 < n; c0 += EM_BUF) {
    const int cn = (int)((n - c0) < EM_BUF ? (n - c0) : EM_BUF);
    if (tid == 0) {
      int sp = 0, nl = 0;
      st_start[0] = 0;
      st_len[0] = cn;
      st_red[0] = 0;
      sp = 1;
      while (sp > 0) {
        --sp;
        int s = st_start[sp], len = st_len[sp], red = st_red[sp];
        while (len > EM_LEAF) {   // descend to the left, the right halves wait
          int n2 = len / 2;
          n2 -= n2 % 8;
          st_start[sp] = s + n2;
          st_len[sp] = len - n2;
          st_red[sp] = red + 1;
          ++sp;
          len = n2;
          red = 0;
        }
        leaf_start[nl] = s;
        leaf_len[nl] = len;
        leaf_red[nl] = red;
        ++nl;
      }
      nleaves = nl;
    }
    __syncthreads();
    const int nl = nleaves;
    const T* buf = seg + c0;
    const int k = tid & 7;
    for (int l = tid >> 3; l < nl; l += EM_THREADS / 8) {   // (uniform over each group of eight lanes)
      const int s = leaf_start[l], len = leaf_len[l];
      T res;
      if (len < 8) {   // only a whole buffer can be this short
        res = (T)-0.0;
        if (k == 0)
          for (int i = 0; i < len; ++i) res += buf[s + i];
      } else {
        const int body = len - len % 8;
        T r = buf[s + k];
        for (int i = 8; i < body; i += 8) r += buf[s + i + k];
        r += __shfl_xor(r, 1, 8);
        r += __shfl_xor(r, 2, 8);
        r += __shfl_xor(r, 4, 8);
        res = r;
        if (k == 0)
          for (int i = body; i < len; ++i) res += buf[s + i];
      }
      if (k == 0) leaf_sum[l] = res;
    }
    __syncthreads();
    if (tid == 0) {
      int vp = 0;
      for (int l = 0; l < nl; ++l) {
        T v = leaf_sum[l];
        for (int r = leaf_red[l]; r > 0; --r) v = vstack[--vp] + v;   // left operand first
        vstack[vp++] = v;
      }
      total = c0 == 0 ? vstack[0] : total + vstack[0];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const T m = total / (T)n;   // 0 / 0 = NaN for an empty segment, as np.mean
    mean[blockIdx.x] = m;
    result = m;
  }
  __syncthreads();
  const T m = result;
  for (long long i = tid; i < n; i += EM_THREADS) mask[a + i] = seg[i] > m ? 1 : 0;
}

extern "C" int avs_segment_mean_mask(const void* d_x, int elem_bytes, int64_t rows, const int64_t* d_offsets, int nseg,
                                     void* d_mean, uint8_t* d_mask, avs_stream_t stream) {
  AVS_REQUIRE(elem_bytes == 4 || elem_bytes == 8, AVS_E_ARG,
              "avs_segment_mean_mask: elem_bytes=%d (4 = float32, 8 = float64)", elem_bytes);
  AVS_REQUIRE(rows >= 0 && nseg >= 0, AVS_E_SHAPE, "avs_segment_mean_mask: rows=%lld nseg=%d", (long long)rows, nseg);
  if (nseg == 0) return AVS_OK;
  AVS_REQUIRE(d_offsets && d_mean && (rows == 0 || (d_x && d_mask)), AVS_E_ARG, "avs_segment_mean_mask: null pointer");
  if (elem_bytes == 4)
    hipLaunchKernelGGL(segment_mean_mask_kernel<float>, dim3((unsigned)nseg), dim3(EM_THREADS), 0, (hipStream_t)stream,
                       (const float*)d_x, d_offsets, (float*)d_mean, d_mask);
  else
    hipLaunchKernelGGL(segment_mean_mask_kernel<double>, dim3((unsigned)nseg), dim3(EM_THREADS), 0, (hipStream_t)stream,
                       (const double*)d_x, d_offsets, (double*)d_mean, d_mask);
  AVS_CHECK_LAUNCH("avs_segment_mean_mask");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// Pair counts per row.  One workgroup per entry of the (video, row tile) table; thread t owns row i = tile * 256 + t of
// its video and walks every j of that video, staged through LDS 1024 at a time (every lane reads the same j: a
// broadcast).  IEEE comparisons (-0.0 == 0.0; NaN is out of contract).  counts is int32 [5, rows], planes
// (less_x, eq_x, less_y, eq_y, s) with s = sum_j sign(x_i - x_j) sign(y_i - y_j); each is at most T <= 32768 in size.
// ---------------------------------------------------------------------------
template <typename TY>
__global__ __launch_bounds__(EM_TILE) void rank_pair_counts_kernel(const float* __restrict__ x, const TY* __restrict__ y,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const int* __restrict__ tiles, long long rows,
                                                                   int* __restrict__ counts) {
  __shared__ float sx[EM_CHUNK];
  __shared__ TY sy[EM_CHUNK];
  const int* tile = tiles + 2 * (long long)blockIdx.x;
  const long long a = offsets[tile[0]];
  const int t = (int)(offsets[tile[0] + 1] - a);
  const float* px = x + a;
  const TY* py = y + a;
  const int i = tile[1] * EM_TILE + threadIdx.x;
  const bool have = i < t;
  const float xi = have ? px[i] : 0.f;
  const TY yi = have ? py[i] : (TY)0;
  int lx = 0, ex = 0, ly = 0, ey = 0, s = 0;
  for (int j0 = 0; j0 < t; j0 += EM_CHUNK) {
    const int jn = (t - j0) < EM_CHUNK ? (t - j0) : EM_CHUNK;
    for (int e = threadIdx.x; e < jn; e += EM_TILE) {
      sx[e] = px[j0 + e];
      sy[e] = py[j0 + e];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
      const float xj = sx[j];
      const TY yj = sy[j];
      const int xl = xj < xi, xg = xj > xi, yl = yj < yi, yg = yj > yi;
      lx += xl;
      ex += xj == xi;
      ly += yl;
      ey += yj == yi;
      s += (xl - xg) * (yl - yg);
    }
    __syncthreads();
  }
  if (have) {
    const long long r = a + i;
    counts[r] = lx;
    counts[rows + r] = ex;
    counts[2 * rows + r] = ly;
    counts[3 * rows + r] = ey;
    counts[4 * rows + r] = s;
  }
}

extern "C" int avs_rank_pair_counts(const float* d_pred, const void* d_target, int target_bytes, int64_t rows,
                                    const int64_t* d_offsets, int nseg, const int32_t* d_tiles, int64_t ntiles,
                                    int max_t, int32_t* d_counts, avs_stream_t stream) {
  AVS_REQUIRE(target_bytes == 4 || target_bytes == 8, AVS_E_ARG,
              "avs_rank_pair_counts: target_bytes=%d (4 = float32, 8 = float64)", target_bytes);
  AVS_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL && nseg >= 0 && ntiles >= nseg && ntiles <= 0x7fffffffLL, AVS_E_SHAPE,
              "avs_rank_pair_counts: rows=%lld nseg=%d ntiles=%lld", (long long)rows, nseg, (long long)ntiles);
  AVS_REQUIRE(max_t <= EM_MAX_T, AVS_E_SHAPE, "avs_rank_pair_counts: a video of %d rows exceeds the limit %d", max_t,
              EM_MAX_T);
  if (nseg == 0) return AVS_OK;
  AVS_REQUIRE(max_t >= 1 && rows >= nseg, AVS_E_SHAPE, "avs_rank_pair_counts: max_t=%d rows=%lld for %d videos", max_t,
              (long long)rows, nseg);
  AVS_REQUIRE(d_pred && d_target && d_offsets && d_tiles && d_counts, AVS_E_ARG, "avs_rank_pair_counts: null pointer");
  if (target_bytes == 4)
    hipLaunchKernelGGL(rank_pair_counts_kernel<float>, dim3((unsigned)ntiles), dim3(EM_TILE), 0, (hipStream_t)stream,
                       d_pred, (const float*)d_target, d_offsets, d_tiles, (long long)rows, d_counts);
  else
    hipLaunchKernelGGL(rank_pair_counts_kernel<double>, dim3((unsigned)ntiles), dim3(EM_TILE), 0, (hipStream_t)stream,
                       d_pred, (const double*)d_target, d_offsets, d_tiles, (long long)rows, d_counts);
  AVS_CHECK_LAUNCH("avs_rank_pair_counts");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// Fold per video.  One workgroup per video sums its rows into int64 [10] =
//   (T, n_pred, n_tgt, tp, S2, E_x, E_y, S_xy, S_xx, S_yy), 2r = 2 less + eq + 1 the doubled average rank.
// Integer sums: any order gives the same value.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(EM_THREADS) void eval_fold_kernel(const int* __restrict__ counts,
                                                               const unsigned char* __restrict__ mask_x,
                                                               const unsigned char* __restrict__ mask_y,
                                                               const int64_t* __restrict__ offsets, long long rows,
                                                               int64_t* __restrict__ out) {
  __shared__ long long red[EM_COLS - 1][EM_THREADS];
  const long long a = offsets[blockIdx.x], b = offsets[blockIdx.x + 1];
  long long acc[EM_COLS - 1];
#pragma unroll
  for (int c = 0; c < EM_COLS - 1; ++c) acc[c] = 0;
  for (long long r = a + threadIdx.x; r < b; r += EM_THREADS) {
    const int mx = mask_x[r] != 0, my = mask_y[r] != 0;
    const long long lx = counts[r], ex = counts[rows + r], ly = counts[2 * rows + r], ey = counts[3 * rows + r];
    const long long rx = 2 * lx + ex + 1, ry = 2 * ly + ey + 1;
    acc[0] += mx;
    acc[1] += my;
    acc[2] += mx & my;
    acc[3] += counts[4 * rows + r];
    acc[4] += ex;
    acc[5] += ey;
    acc[6] += rx * ry;
    acc[7] += rx * rx;
    acc[8] += ry * ry;
  }
#pragma unroll
  for (int c = 0; c < EM_COLS - 1; ++c) red[c][threadIdx.x] = acc[c];
  __syncthreads();
  for (int w = EM_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int c = 0; c < EM_COLS - 1; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[EM_COLS * (long long)blockIdx.x] = b - a;
  if (threadIdx.x < EM_COLS - 1) out[EM_COLS * (long long)blockIdx.x + 1 + threadIdx.x] = red[threadIdx.x][0];
}

extern "C" int avs_eval_fold(const int32_t* d_counts, const uint8_t* d_mask_pred, const uint8_t* d_mask_target,
                             int64_t rows, const int64_t* d_offsets, int nseg, int max_t, int64_t* d_out,
                             avs_stream_t stream) {
  AVS_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL && nseg >= 0, AVS_E_SHAPE, "avs_eval_fold: rows=%lld nseg=%d",
              (long long)rows, nseg);
  AVS_REQUIRE(max_t <= EM_MAX_T, AVS_E_SHAPE, "avs_eval_fold: a video of %d rows exceeds the limit %d", max_t, EM_MAX_T);
  if (nseg == 0) return AVS_OK;
  AVS_REQUIRE(max_t >= 1 && rows >= nseg, AVS_E_SHAPE, "avs_eval_fold: max_t=%d rows=%lld for %d videos", max_t,
              (long long)rows, nseg);
  AVS_REQUIRE(d_counts && d_mask_pred && d_mask_target && d_offsets && d_out, AVS_E_ARG, "avs_eval_fold: null pointer");
  hipLaunchKernelGGL(eval_fold_kernel, dim3((unsigned)nseg), dim3(EM_THREADS), 0, (hipStream_t)stream, d_counts,
                     d_mask_pred, d_mask_target, d_offsets, (long long)rows, d_out);
  AVS_CHECK_LAUNCH("avs_eval_fold");
  return AVS_OK;
}
