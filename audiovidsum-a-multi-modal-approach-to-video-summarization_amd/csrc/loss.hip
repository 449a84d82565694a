// libavsum_loss.so: per-shot training targets and a pairwise ranking loss for a ragged batch of videos
// (include/avsum_loss.h; the comment there is the definition).  A sixth library: this file includes its own header only.
//
// The pair kernel has the shape of rank_pair_counts_kernel (evalmetrics.hip): a workgroup per (video, row tile), a
// thread per row, every j of the video through LDS so that the 64 lanes of a wave read one address (a broadcast).  What a
// thread does per j is a handful of fp64 transcendentals (logistic) or two compares and a subtraction (hinge), so the
// kernel is bound by the vector ALU, not by memory: the staged chunk is 8 KiB and the whole video is read once per tile.
// The fold kernel has the shape of seq_mse_kernel (train_batch.hip).  Nothing is accumulated across workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/avsum_loss.h"

static_assert(AVSL_TILE == 256 && AVSL_BLOCK == 256, "the launch bounds of the kernels");
static_assert(AVSL_CHUNK % AVSL_TILE == 0, "a chunk is staged in whole passes of the workgroup");
static_assert((long long)AVSL_MAX_T * AVSL_MAX_T <= (1LL << 30), "pairs of one video fit an int32 sum");

static thread_local char g_err[512] = "";

static void avsl_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSL_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsl_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSL_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsl_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSL_E_HIP;                                                         \
    }                                                                            \
  } while (0)

// ---------------------------------------------------------------------------------------------------- shot targets
// floor(((double)frame / fps) / bin) clipped to [-1, count]: NaN and everything negative give -1
__device__ __forceinline__ long long avsl_bin(long long frame, double fps, double bin, long long count) {
  const double x = floor(((double)frame / fps) / bin);
  if (!(x >= 0.0)) return -1;
  return x >= (double)count ? count : (long long)x;
}

__global__ __launch_bounds__(AVSL_BLOCK) void avsl_shot_targets_kernel(const float* __restrict__ ann, long long nann,
                                                                       const int64_t* __restrict__ ann_offsets,
                                                                       const int64_t* __restrict__ shots,
                                                                       long long nshots,
                                                                       const int64_t* __restrict__ shot_offsets,
                                                                       const double* __restrict__ fps_of, double bin,
                                                                       float* __restrict__ targets,
                                                                       unsigned char* __restrict__ flags) {
  const int v = blockIdx.x;
  long long a0 = ann_offsets[v], a1 = ann_offsets[v + 1];
  a0 = a0 < 0 ? 0 : (a0 > nann ? nann : a0);
  a1 = a1 < a0 ? a0 : (a1 > nann ? nann : a1);
  const long long count = a1 - a0;
  long long s0 = shot_offsets[v], s1 = shot_offsets[v + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > nshots ? nshots : s1;
  const double fps = fps_of[v];
  const float* seg = ann + a0;
  int empty = 0;
  for (long long s = s0 + threadIdx.x; s < s1; s += AVSL_BLOCK) {
    long long lo = avsl_bin(shots[2 * s], fps, bin, count);
    long long hi = avsl_bin(shots[2 * s + 1], fps, bin, count) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > count ? count : hi;
    if (hi <= lo) {
      targets[s] = __builtin_nanf("");
      empty = 1;
      continue;
    }
    double sum = 0.0;
    for (long long k = lo; k < hi; ++k) sum += (double)seg[k];
    targets[s] = (float)(sum / (double)(hi - lo));
  }
  const int any = __syncthreads_or(empty);
  if (threadIdx.x == 0) flags[v] = any ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------ pair terms
// Row partials in the workspace: loss fp64 [rows] | grad fp64 [rows] (logistic) or int32 [rows] in the same place
// (hinge) | count int32 [rows]
struct avsl_workspace {
  double* loss;
  double* grad;
  int* count;
};

__host__ __device__ inline size_t avsl_round256(size_t n) { return (n + 255) & ~(size_t)255; }

static avsl_workspace avsl_carve(void* base, long long rows) {
  char* p = (char*)base;
  avsl_workspace w;
  w.loss = (double*)p;
  w.grad = (double*)(p + avsl_round256(8 * (size_t)rows));
  w.count = (int*)(p + 2 * avsl_round256(8 * (size_t)rows));
  return w;
}

template <int KIND>
__global__ __launch_bounds__(AVSL_TILE) void avsl_rank_pairs_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ targets, long long rows,
                                                                    const int64_t* __restrict__ offsets, int nseq,
                                                                    const int* __restrict__ tiles, double scale,
                                                                    double margin, avsl_workspace w) {
  __shared__ float ss[AVSL_CHUNK];
  __shared__ float sy[AVSL_CHUNK];
  const int* tile = tiles + AVSL_TILE_COLS * (long long)blockIdx.x;
  const int v = tile[0];
  if (v < 0 || v >= nseq || tile[1] < 0) return;                       // (uniform over the workgroup)
  const long long a = offsets[v], b = offsets[v + 1];
  if (a < 0 || b > rows || b - a > AVSL_MAX_T || b <= a || (long long)tile[1] * AVSL_TILE >= b - a) return;
  const int t = (int)(b - a);
  const float* ps = scores + a;
  const float* py = targets + a;
  const int i = tile[1] * AVSL_TILE + threadIdx.x;
  const bool have = i < t;
  const double si = have ? (double)ps[i] : 0.0;
  const float yi = have ? py[i] : 0.f;
  double loss = 0.0, grad = 0.0;
  int c = 0, count = 0;
  for (int j0 = 0; j0 < t; j0 += AVSL_CHUNK) {
    const int jn = (t - j0) < AVSL_CHUNK ? (t - j0) : AVSL_CHUNK;
    for (int e = threadIdx.x; e < jn; e += AVSL_TILE) {
      ss[e] = ps[j0 + e];
      sy[e] = py[j0 + e];
    }
    __syncthreads();
    for (int j = 0; j < jn; ++j) {
      const float yj = sy[j];
      const double d = si - (double)ss[j];                             // d_ij, exact
      const int above = yi > yj, below = yj > yi;
      count += above;
      if (KIND == AVSL_LOGISTIC) {
        if (above | below) {
          // above: x = -scale * d_ij;  below: x = -scale * d_ji = scale * d_ij
          const double x = above ? -scale * d : scale * d;
          const double e = exp(-fabs(x));
          const double sig = (x >= 0.0 ? 1.0 : e) / (1.0 + e);
          if (above) {
            loss += fmax(x, 0.0) + log1p(e);
            grad -= sig;
          } else {
            grad += sig;
          }
        }
      } else {
        const double up = margin - d, down = margin + d;               // margin - d_ij, margin - d_ji
        if (above && up > 0.0) {
          loss += up;
          c -= 1;
        }
        if (below && down > 0.0) c += 1;
      }
    }
    __syncthreads();
  }
  if (have) {
    const long long r = a + i;
    w.loss[r] = loss;
    if (KIND == AVSL_LOGISTIC) w.grad[r] = grad;
    else ((int*)w.grad)[r] = c;
    w.count[r] = count;
  }
}

template <int KIND>
__global__ __launch_bounds__(AVSL_BLOCK) void avsl_rank_fold_kernel(long long rows, const int64_t* __restrict__ offsets,
                                                                    double scale, avsl_workspace w,
                                                                    float* __restrict__ losses, float* __restrict__ g,
                                                                    int64_t* __restrict__ pairs) {
  __shared__ double red[AVSL_BLOCK];
  __shared__ long long cred[AVSL_BLOCK];
  const int v = blockIdx.x, t = threadIdx.x;
  long long a = offsets[v], b = offsets[v + 1];
  if (a < 0) a = 0;
  if (b > rows) b = rows;
  double s = 0.0;
  long long n = 0;
  for (long long r = a + t; r < b; r += AVSL_BLOCK) {
    s += w.loss[r];
    n += w.count[r];
  }
  red[t] = s;
  cred[t] = n;
  __syncthreads();
#pragma unroll
  for (int k = AVSL_BLOCK / 2; k > 0; k >>= 1) {
    if (t < k) {
      red[t] += red[t + k];
      cred[t] += cred[t + k];
    }
    __syncthreads();
  }
  const long long p = cred[0];
  if (t == 0) {
    losses[v] = p > 0 ? (float)(red[0] / (double)p) : 0.f;
    pairs[v] = p;
  }
  for (long long r = a + t; r < b; r += AVSL_BLOCK) {
    const double rowgrad = KIND == AVSL_LOGISTIC ? scale * w.grad[r] : (double)((const int*)w.grad)[r];
    g[r] = p > 0 ? (float)(rowgrad / (double)p) : 0.f;
  }
}

// dscores[r] = dlosses[v] * g[r]; the video of a row: the last v in 0 .. nseq - 1 with offsets[v] <= r
__global__ __launch_bounds__(AVSL_BLOCK) void avsl_rank_bwd_kernel(const float* __restrict__ dlosses,
                                                                   const float* __restrict__ g, long long rows,
                                                                   const int64_t* __restrict__ offsets, int nseq,
                                                                   float* __restrict__ dscores) {
  for (long long r = (long long)blockIdx.x * AVSL_BLOCK + threadIdx.x; r < rows;
       r += (long long)gridDim.x * AVSL_BLOCK) {
    int lo = 0, hi = nseq - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offsets[mid] <= r) lo = mid;
      else hi = mid - 1;
    }
    dscores[r] = dlosses[lo] * g[r];
  }
}

// ----------------------------------------------------------------------------------------------------------- host
static bool avsl_aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

extern "C" int avsl_abi_version(void) { return AVSL_ABI_VERSION; }

extern "C" const char* avsl_last_error(void) { return g_err; }

extern "C" int avsl_shot_targets_f32(const float* d_annotations, int64_t nann, const int64_t* d_ann_offsets,
                                     const int64_t* d_shots, int64_t nshots, const int64_t* d_shot_offsets,
                                     const double* d_fps, int nvideos, double bin_seconds, float* d_targets,
                                     uint8_t* d_flags, avsl_stream_t stream) {
  const char* who = "avsl_shot_targets_f32";
  AVSL_REQUIRE(nvideos >= 1, AVSL_E_ARG, "%s: nvideos=%d, must be >= 1", who, nvideos);
  AVSL_REQUIRE(nann >= 0 && nann <= AVSL_MAX_ROWS && nshots >= 0 && nshots <= AVSL_MAX_ROWS, AVSL_E_SHAPE,
               "%s: nann=%lld nshots=%lld, each must lie in 0 .. %d", who, (long long)nann, (long long)nshots,
               AVSL_MAX_ROWS);
  AVSL_REQUIRE(isfinite(bin_seconds) && bin_seconds > 0.0, AVSL_E_ARG, "%s: bin_seconds=%g, must be finite and > 0", who,
               bin_seconds);
  AVSL_REQUIRE(d_ann_offsets && d_shot_offsets && d_fps && d_flags && (nann == 0 || d_annotations) &&
                   (nshots == 0 || (d_shots && d_targets)),
               AVSL_E_ARG, "%s: null pointer", who);
  AVSL_REQUIRE(avsl_aligned(d_ann_offsets, 8) && avsl_aligned(d_shot_offsets, 8) && avsl_aligned(d_shots, 8) &&
                   avsl_aligned(d_fps, 8) && avsl_aligned(d_annotations, 4) && avsl_aligned(d_targets, 4),
               AVSL_E_ALIGN, "%s: a table is not aligned to its element size", who);
  hipLaunchKernelGGL(avsl_shot_targets_kernel, dim3((unsigned)nvideos), dim3(AVSL_BLOCK), 0, (hipStream_t)stream,
                     d_annotations, (long long)nann, d_ann_offsets, d_shots, (long long)nshots, d_shot_offsets, d_fps,
                     bin_seconds, d_targets, d_flags);
  AVSL_CHECK_LAUNCH(who);
  return AVSL_OK;
}

extern "C" size_t avsl_rank_workspace_bytes(int64_t rows) {
  if (rows <= 0) return 0;
  return 2 * avsl_round256(8 * (size_t)rows) + avsl_round256(4 * (size_t)rows);
}

extern "C" int avsl_rank_loss_f32(const float* d_scores, const float* d_targets, int64_t rows, const int64_t* d_offsets,
                                  int nseq, const int32_t* d_tiles, int64_t ntiles, int max_t, int kind, double scale,
                                  double margin, void* d_workspace, size_t workspace_bytes, float* d_losses, float* d_g,
                                  int64_t* d_pairs, avsl_stream_t stream) {
  const char* who = "avsl_rank_loss_f32";
  AVSL_REQUIRE(rows >= 1 && rows <= AVSL_MAX_ROWS, AVSL_E_SHAPE, "%s: rows=%lld, must be 1 .. %d", who, (long long)rows,
               AVSL_MAX_ROWS);
  AVSL_REQUIRE(nseq >= 1 && nseq <= rows, AVSL_E_SHAPE, "%s: nseq=%d for %lld rows, must be 1 .. rows", who, nseq,
               (long long)rows);
  AVSL_REQUIRE(ntiles >= nseq && ntiles <= AVSL_MAX_ROWS, AVSL_E_SHAPE, "%s: ntiles=%lld for %d videos", who,
               (long long)ntiles, nseq);
  AVSL_REQUIRE(max_t >= 1 && max_t <= AVSL_MAX_T, AVSL_E_SHAPE, "%s: max_t=%d, a video has 1 .. %d rows", who, max_t,
               AVSL_MAX_T);
  AVSL_REQUIRE(kind == AVSL_LOGISTIC || kind == AVSL_HINGE, AVSL_E_ARG, "%s: kind=%d, must be 0 (logistic) or 1 (hinge)",
               who, kind);
  AVSL_REQUIRE(isfinite(scale) && scale > 0.0, AVSL_E_ARG, "%s: scale=%g, must be finite and > 0", who, scale);
  AVSL_REQUIRE(isfinite(margin), AVSL_E_ARG, "%s: margin=%g, must be finite", who, margin);
  AVSL_REQUIRE(d_scores && d_targets && d_offsets && d_tiles && d_workspace && d_losses && d_g && d_pairs, AVSL_E_ARG,
               "%s: null pointer", who);
  AVSL_REQUIRE(workspace_bytes >= avsl_rank_workspace_bytes(rows), AVSL_E_SHAPE,
               "%s: the workspace holds %zu bytes, %lld rows need %zu", who, workspace_bytes, (long long)rows,
               avsl_rank_workspace_bytes(rows));
  AVSL_REQUIRE(avsl_aligned(d_workspace, 8) && avsl_aligned(d_offsets, 8) && avsl_aligned(d_pairs, 8) &&
                   avsl_aligned(d_tiles, 4) && avsl_aligned(d_scores, 4) && avsl_aligned(d_targets, 4) &&
                   avsl_aligned(d_losses, 4) && avsl_aligned(d_g, 4),
               AVSL_E_ALIGN, "%s: the workspace, d_offsets and d_pairs must be 8-byte aligned, the rest 4-byte", who);
  const avsl_workspace w = avsl_carve(d_workspace, (long long)rows);
  if (kind == AVSL_LOGISTIC) {
    hipLaunchKernelGGL(avsl_rank_pairs_kernel<AVSL_LOGISTIC>, dim3((unsigned)ntiles), dim3(AVSL_TILE), 0,
                       (hipStream_t)stream, d_scores, d_targets, (long long)rows, d_offsets, nseq, d_tiles, scale, margin,
                       w);
    AVSL_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(avsl_rank_fold_kernel<AVSL_LOGISTIC>, dim3((unsigned)nseq), dim3(AVSL_BLOCK), 0,
                       (hipStream_t)stream, (long long)rows, d_offsets, scale, w, d_losses, d_g, d_pairs);
  } else {
    hipLaunchKernelGGL(avsl_rank_pairs_kernel<AVSL_HINGE>, dim3((unsigned)ntiles), dim3(AVSL_TILE), 0,
                       (hipStream_t)stream, d_scores, d_targets, (long long)rows, d_offsets, nseq, d_tiles, scale, margin,
                       w);
    AVSL_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(avsl_rank_fold_kernel<AVSL_HINGE>, dim3((unsigned)nseq), dim3(AVSL_BLOCK), 0, (hipStream_t)stream,
                       (long long)rows, d_offsets, scale, w, d_losses, d_g, d_pairs);
  }
  AVSL_CHECK_LAUNCH(who);
  return AVSL_OK;
}

extern "C" int avsl_rank_loss_bwd_f32(const float* d_dlosses, const float* d_g, int64_t rows, const int64_t* d_offsets,
                                      int nseq, float* d_dscores, avsl_stream_t stream) {
  const char* who = "avsl_rank_loss_bwd_f32";
  AVSL_REQUIRE(rows >= 1 && rows <= AVSL_MAX_ROWS, AVSL_E_SHAPE, "%s: rows=%lld, must be 1 .. %d", who, (long long)rows,
               AVSL_MAX_ROWS);
  AVSL_REQUIRE(nseq >= 1 && nseq <= rows, AVSL_E_SHAPE, "%s: nseq=%d for %lld rows, must be 1 .. rows", who, nseq,
               (long long)rows);
  AVSL_REQUIRE(d_dlosses && d_g && d_offsets && d_dscores, AVSL_E_ARG, "%s: null pointer", who);
  AVSL_REQUIRE(avsl_aligned(d_offsets, 8) && avsl_aligned(d_dlosses, 4) && avsl_aligned(d_g, 4) &&
                   avsl_aligned(d_dscores, 4),
               AVSL_E_ALIGN, "%s: d_offsets must be 8-byte aligned, the rest 4-byte", who);
  long long groups = ((long long)rows + AVSL_BLOCK - 1) / AVSL_BLOCK;
  if (groups > 2048) groups = 2048;
  hipLaunchKernelGGL(avsl_rank_bwd_kernel, dim3((unsigned)groups), dim3(AVSL_BLOCK), 0, (hipStream_t)stream, d_dlosses,
                     d_g, (long long)rows, d_offsets, nseq, d_dscores);
  AVSL_CHECK_LAUNCH(who);
  return AVSL_OK;
}
