// A ragged batch of videos per optimiser step (AVBiLSTMModel.train_rows, scripts/train_av_model.py: train_step_batch): the
// two pieces of the training step that know where one video ends and the next begins.  The videos are the segments
// [offsets[v], offsets[v + 1]) of concatenated rows; the table is trusted as in evalmetrics.hip (ops.SeqTable builds and
// validates it), and every row read is checked against `rows` all the same.  Nothing here uses atomics: every result is a
// copy or is summed in one fixed order.
#include "avs_internal.h"

#define TB_THREADS 256

// the segment that holds row r: the largest v with offsets[v] <= r (-1 when r lies before the first segment)
__device__ __forceinline__ int tb_segment_of(const int64_t* __restrict__ offsets, int nseq, long long r) {
  int lo = 0, hi = nseq + 1;   // offsets[0 .. lo) <= r < offsets[hi ..]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)offsets[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// ---------------------------------------------------------------------------
// h_{t-1} of a recurrence from its outputs: out[r, :] = src[r - dir, col0 : col0 + cols] where row r - dir belongs to the
// same segment as r, else 0 (dir = +1: the forward direction's previous step; dir = -1: the reverse direction's).  Exact
// copies.  W = 4: one float4 per thread (col0, cols and both row strides multiples of 4, 16-byte aligned bases); W = 1
// otherwise.  A thread finds its row's segment by binary search in the offsets (V + 1 entries: they stay in L1 / L2).
// ---------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(TB_THREADS) void seq_shift_rows_kernel(const float* __restrict__ src, long long ld_src,
                                                                    int col0, int cols, long long rows,
                                                                    const int64_t* __restrict__ offsets, int nseq,
                                                                    int dir, float* __restrict__ out, long long ld_out) {
  const int per_row = cols / W;
  const long long total = rows * per_row;
  for (long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TB_THREADS) {
    const long long r = i / per_row;
    const int c = (int)(i - r * per_row) * W;
    const int v = tb_segment_of(offsets, nseq, r);
    const long long from = r - dir;
    bool take = v >= 0 && v < nseq && from >= 0 && from < rows;
    if (take) take = from >= (long long)offsets[v] && from < (long long)offsets[v + 1];
    if (W == 4) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (take) x = *reinterpret_cast<const float4*>(src + from * ld_src + col0 + c);
      *reinterpret_cast<float4*>(out + r * ld_out + c) = x;
    } else {
      out[r * ld_out + c] = take ? src[from * ld_src + col0 + c] : 0.f;
    }
  }
}

extern "C" int avs_seq_shift_rows_f32(const float* d_src, int64_t ld_src, int col0, int cols, int64_t rows,
                                      const int64_t* d_offsets, int nseq, int direction, float* d_out, int64_t ld_out,
                                      avs_stream_t stream) {
  AVS_REQUIRE(rows >= 0 && rows < (1LL << 31) && nseq >= 0 && col0 >= 0 && cols > 0 && ld_src >= (int64_t)col0 + cols &&
                  ld_out >= cols,
              AVS_E_SHAPE, "avs_seq_shift_rows_f32: rows=%lld nseq=%d col0=%d cols=%d ld_src=%lld ld_out=%lld",
              (long long)rows, nseq, col0, cols, (long long)ld_src, (long long)ld_out);
  AVS_REQUIRE(direction == 1 || direction == -1, AVS_E_ARG, "avs_seq_shift_rows_f32: direction=%d (+1 or -1)", direction);
  if (rows == 0) return AVS_OK;
  AVS_REQUIRE(d_src && d_offsets && d_out, AVS_E_ARG, "avs_seq_shift_rows_f32: null pointer");
  const bool vec = cols % 4 == 0 && col0 % 4 == 0 && ld_src % 4 == 0 && ld_out % 4 == 0 && avs_aligned16(d_src) &&
                   avs_aligned16(d_out);
  const long long total = (long long)rows * (vec ? cols / 4 : cols);
  long long gx = avs_cdiv(total, TB_THREADS);
  if (gx > 4096) gx = 4096;
  if (vec)
    hipLaunchKernelGGL(seq_shift_rows_kernel<4>, dim3((unsigned)gx), dim3(TB_THREADS), 0, (hipStream_t)stream, d_src,
                       (long long)ld_src, col0, cols, (long long)rows, d_offsets, nseq, direction, d_out,
                       (long long)ld_out);
  else
    hipLaunchKernelGGL(seq_shift_rows_kernel<1>, dim3((unsigned)gx), dim3(TB_THREADS), 0, (hipStream_t)stream, d_src,
                       (long long)ld_src, col0, cols, (long long)rows, d_offsets, nseq, direction, d_out,
                       (long long)ld_out);
  AVS_CHECK_LAUNCH("avs_seq_shift_rows_f32");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// Per-video mean squared error (F.mse_loss of scripts/train_av_model.py:92, one per video).  One workgroup per video:
// thread t sums d * d, d = (double)p - (double)y, over rows t, t + 256, ... of its video in that order, the 256 partial
// sums are folded by a fixed binary tree in LDS, the total is divided by T_v and rounded ONCE to fp32.  The order depends
// on T_v alone, so a video's loss is the same bits wherever it sits in the batch.  target_stride 0: one target per video
// (targets [V]); 1: one per row (targets [R]).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void seq_mse_kernel(const float* __restrict__ scores,
                                                             const float* __restrict__ targets, int target_stride,
                                                             long long rows, const int64_t* __restrict__ offsets,
                                                             float* __restrict__ losses) {
  __shared__ double red[TB_THREADS];
  const int v = blockIdx.x, t = threadIdx.x;
  long long a = offsets[v], b = offsets[v + 1];
  const long long n = b - a;
  if (a < 0) a = 0;
  if (b > rows) b = rows;
  double s = 0.0;
  for (long long r = a + t; r < b; r += TB_THREADS) {
    const double d = (double)scores[r] - (double)targets[target_stride ? r : v];
    s += d * d;
  }
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = TB_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) losses[v] = (float)(red[0] / (double)n);   // 0 / 0 = NaN for an empty video, as F.mse_loss
}

extern "C" int avs_seq_mse_f32(const float* d_scores, const float* d_targets, int target_stride, int64_t rows,
                               const int64_t* d_offsets, int nseq, float* d_losses, avs_stream_t stream) {
  AVS_REQUIRE(rows >= 0 && nseq >= 0, AVS_E_SHAPE, "avs_seq_mse_f32: rows=%lld nseq=%d", (long long)rows, nseq);
  AVS_REQUIRE(target_stride == 0 || target_stride == 1, AVS_E_ARG,
              "avs_seq_mse_f32: target_stride=%d (0 = one target per video, 1 = one per row)", target_stride);
  if (nseq == 0) return AVS_OK;
  AVS_REQUIRE(d_offsets && d_losses && d_targets && (rows == 0 || d_scores), AVS_E_ARG, "avs_seq_mse_f32: null pointer");
  hipLaunchKernelGGL(seq_mse_kernel, dim3((unsigned)nseq), dim3(TB_THREADS), 0, (hipStream_t)stream, d_scores, d_targets,
                     target_stride, (long long)rows, d_offsets, d_losses);
  AVS_CHECK_LAUNCH("avs_seq_mse_f32");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// Its backward: dscores[r] = (dlosses[v] * (2 / T_v)) * (p_r - y) in fp32, for the rows of video v.  Workgroup (v, k)
// walks rows k * 256 + t, stepping by the grid's height.  Rows outside every video are not written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void seq_mse_bwd_kernel(const float* __restrict__ dlosses,
                                                                 const float* __restrict__ scores,
                                                                 const float* __restrict__ targets, int target_stride,
                                                                 long long rows, const int64_t* __restrict__ offsets,
                                                                 float* __restrict__ dscores) {
  const int v = blockIdx.x;
  long long a = offsets[v], b = offsets[v + 1];
  const float g = dlosses[v] * (2.f / (float)(b - a));
  if (a < 0) a = 0;
  if (b > rows) b = rows;
  for (long long r = a + (long long)blockIdx.y * TB_THREADS + threadIdx.x; r < b; r += (long long)gridDim.y * TB_THREADS)
    dscores[r] = g * (scores[r] - targets[target_stride ? r : v]);
}

extern "C" int avs_seq_mse_bwd_f32(const float* d_dlosses, const float* d_scores, const float* d_targets,
                                   int target_stride, int64_t rows, const int64_t* d_offsets, int nseq, int max_t,
                                   float* d_dscores, avs_stream_t stream) {
  AVS_REQUIRE(rows >= 0 && nseq >= 0 && max_t >= 0, AVS_E_SHAPE, "avs_seq_mse_bwd_f32: rows=%lld nseq=%d max_t=%d",
              (long long)rows, nseq, max_t);
  AVS_REQUIRE(target_stride == 0 || target_stride == 1, AVS_E_ARG,
              "avs_seq_mse_bwd_f32: target_stride=%d (0 = one target per video, 1 = one per row)", target_stride);
  if (nseq == 0 || rows == 0 || max_t == 0) return AVS_OK;
  AVS_REQUIRE(d_dlosses && d_scores && d_targets && d_offsets && d_dscores, AVS_E_ARG,
              "avs_seq_mse_bwd_f32: null pointer");
  AVS_REQUIRE(nseq <= 0x7fffffff / 2, AVS_E_SHAPE, "avs_seq_mse_bwd_f32: too many videos");
  long long gy = avs_cdiv(max_t, TB_THREADS);
  if (gy > 64) gy = 64;
  hipLaunchKernelGGL(seq_mse_bwd_kernel, dim3((unsigned)nseq, (unsigned)gy), dim3(TB_THREADS), 0, (hipStream_t)stream,
                     d_dlosses, d_scores, d_targets, target_stride, (long long)rows, d_offsets, d_dscores);
  AVS_CHECK_LAUNCH("avs_seq_mse_bwd_f32");
  return AVS_OK;
}
