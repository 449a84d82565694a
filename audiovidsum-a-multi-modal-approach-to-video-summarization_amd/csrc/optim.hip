// libavsum_optim.so: the fused multi-tensor AdamW step (include/avsum_optim.h).  Self-contained: this file is the
// whole library and includes nothing of libavsum_hip.so.
//
// Three kernels.  The pointer table of a launch (<= AVSO_MAX_TENSORS rows) and the exclusive scan of its chunk counts
// are a by-value kernel argument; a workgroup strides over the chunks, finds a chunk's row by binary search in the
// scan (all of it wave-uniform: scalar loads from the argument segment) and then works on <= AVSO_CHUNK elements.
// Every thread owns the same 16 elements of a chunk in every kernel and on both the 16-byte and the scalar path:
// elements 4 * (tid + 256 * k) + e, k = 0..3, e = 0..3.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/avsum_optim.h"

#define AVSO_THREADS 256
#define AVSO_GROUPS_PER_THREAD (AVSO_CHUNK / (4 * AVSO_THREADS))
static_assert(AVSO_CHUNK == 16 * AVSO_THREADS, "a thread owns four groups of four elements of a chunk");
static_assert(AVSO_COEF_OFFSET == 8 * AVSO_STATE_DOUBLES && AVSO_PARTIALS_OFFSET == AVSO_COEF_OFFSET + 4 * AVSO_COEF_FLOATS,
              "workspace layout");

static thread_local char g_err[512] = "";

static void avso_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSO_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avso_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSO_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avso_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSO_E_HIP;                                                         \
    }                                                                            \
  } while (0)

// the kernel argument: 1.4 KiB
struct avso_table {
  float* ptr[4][AVSO_MAX_TENSORS];    // param, grad, exp_avg, exp_avg_sq
  int64_t numel[AVSO_MAX_TENSORS];
  int start[AVSO_MAX_TENSORS + 1];    // exclusive scan of the rows' chunk counts; start[ntensors] = chunks of the launch
  int ntensors;
  unsigned vec_mask;                  // bit t: the four pointers of row t are 16-byte aligned
};

// the row of chunk c: the largest t with start[t] <= c (rows without elements share their start with the next row)
__device__ __forceinline__ int avso_row_of(const avso_table& tab, int c) {
  int lo = 0, hi = tab.ntensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.start[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

// a chunk of a row: its first element and its length
__device__ __forceinline__ int avso_chunk(const avso_table& tab, int c, int& t, int64_t& base, bool& vec) {
  t = avso_row_of(tab, c);
  base = (int64_t)(c - tab.start[t]) * AVSO_CHUNK;
  const int64_t left = tab.numel[t] - base;
  vec = (tab.vec_mask >> t) & 1u;
  return left < AVSO_CHUNK ? (int)left : AVSO_CHUNK;
}

__device__ __forceinline__ double avso_block_sum(double v, double* s_wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // every lane holds the wave's sum, one fixed tree
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                                  // (s_wave may still be read from the last chunk)
  if ((threadIdx.x & 63) == 0) s_wave[wave] = v;
  __syncthreads();
  return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ __launch_bounds__(AVSO_THREADS) void avso_grad_sumsq_kernel(const avso_table tab,
                                                                       double* __restrict__ d_partials) {
  __shared__ double s_wave[AVSO_THREADS / 64];
  const int nchunks = tab.start[tab.ntensors];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int t;
    int64_t base;
    bool vec;
    const int len = avso_chunk(tab, c, t, base, vec);
    const float* g = tab.ptr[1][t] + base;
    float x[AVSO_GROUPS_PER_THREAD][4];
    if (vec && len == AVSO_CHUNK) {
#pragma unroll
      for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k) {
        const float4 q = *reinterpret_cast<const float4*>(g + 4 * (threadIdx.x + AVSO_THREADS * k));
        x[k][0] = q.x, x[k][1] = q.y, x[k][2] = q.z, x[k][3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = 4 * (threadIdx.x + AVSO_THREADS * k) + e;
          x[k][e] = j < len ? g[j] : 0.f;      // (+0 leaves a sum of squares as it is)
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)x[k][e] * (double)x[k][e];
    const double sum = avso_block_sum(acc, s_wave);
    if (threadIdx.x == 0) d_partials[c] = sum;
  }
}

__global__ __launch_bounds__(AVSO_THREADS) void avso_adamw_prepare_kernel(const double* __restrict__ d_partials,
                                                                          int64_t npartials, double lr, double beta1,
                                                                          double beta2, double weight_decay,
                                                                          double max_norm, int skip_nonfinite,
                                                                          double* __restrict__ d_state,
                                                                          float* __restrict__ d_coef) {
  __shared__ double s_wave[AVSO_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < npartials; i += AVSO_THREADS) acc += d_partials[i];
  const double norm2 = avso_block_sum(acc, s_wave);
  if (threadIdx.x != 0) return;
  const bool have_norm = npartials > 0;
  const bool skip = have_norm && skip_nonfinite && !isfinite(norm2);
  float clip = 1.f;
  if (have_norm && max_norm > 0.0) {
    const double c = max_norm / (sqrt(norm2) + 1e-6);
    clip = c < 1.0 ? (float)c : 1.f;
  }
  d_state[AVSO_STATE_NORM2] = have_norm ? norm2 : -1.0;
  d_state[AVSO_STATE_CLIP] = (double)clip;
  d_coef[AVSO_COEF_CLIP] = clip;
  d_coef[AVSO_COEF_SKIP] = skip ? 1.f : 0.f;
  if (skip) {
    d_state[AVSO_STATE_SKIPPED] += 1.0;
    return;
  }
  const double t = d_state[AVSO_STATE_APPLIED] + 1.0;
  d_state[AVSO_STATE_APPLIED] = t;
  d_coef[AVSO_COEF_DECAY] = (float)(1.0 - lr * weight_decay);
  d_coef[AVSO_COEF_STEP_SIZE] = (float)(lr / (1.0 - pow(beta1, t)));
  d_coef[AVSO_COEF_BC2_SQRT] = (float)sqrt(1.0 - pow(beta2, t));
}

struct avso_hyper {
  float decay, step_size, bc2s, clip, omb1, beta2, omb2, eps;
};

__device__ __forceinline__ void avso_adamw_element(const avso_hyper& h, float& p, float g, float& m, float& v) {
  g = g * h.clip;
  p = p * h.decay;
  m = m + (g - m) * h.omb1;
  v = v * h.beta2 + g * g * h.omb2;
  p = p - h.step_size * m / (sqrtf(v) / h.bc2s + h.eps);
}

__global__ __launch_bounds__(AVSO_THREADS) void avso_adamw_apply_kernel(const avso_table tab,
                                                                        const float* __restrict__ d_coef, float omb1,
                                                                        float beta2, float omb2, float eps) {
  if (d_coef[AVSO_COEF_SKIP] != 0.f) return;
  const avso_hyper h = {d_coef[AVSO_COEF_DECAY], d_coef[AVSO_COEF_STEP_SIZE], d_coef[AVSO_COEF_BC2_SQRT],
                        d_coef[AVSO_COEF_CLIP], omb1, beta2, omb2, eps};
  const int nchunks = tab.start[tab.ntensors];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int t;
    int64_t base;
    bool vec;
    const int len = avso_chunk(tab, c, t, base, vec);
    float* p = tab.ptr[0][t] + base;
    const float* g = tab.ptr[1][t] + base;
    float* m = tab.ptr[2][t] + base;
    float* v = tab.ptr[3][t] + base;
    if (vec && len == AVSO_CHUNK) {
      float4 qp[AVSO_GROUPS_PER_THREAD], qg[AVSO_GROUPS_PER_THREAD], qm[AVSO_GROUPS_PER_THREAD],
          qv[AVSO_GROUPS_PER_THREAD];
#pragma unroll
      for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k) {     // all sixteen 16-byte loads in flight before the first use
        const int j = 4 * (threadIdx.x + AVSO_THREADS * k);
        qp[k] = *reinterpret_cast<const float4*>(p + j);
        qg[k] = *reinterpret_cast<const float4*>(g + j);
        qm[k] = *reinterpret_cast<const float4*>(m + j);
        qv[k] = *reinterpret_cast<const float4*>(v + j);
      }
#pragma unroll
      for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k) {
        const int j = 4 * (threadIdx.x + AVSO_THREADS * k);
        avso_adamw_element(h, qp[k].x, qg[k].x, qm[k].x, qv[k].x);
        avso_adamw_element(h, qp[k].y, qg[k].y, qm[k].y, qv[k].y);
        avso_adamw_element(h, qp[k].z, qg[k].z, qm[k].z, qv[k].z);
        avso_adamw_element(h, qp[k].w, qg[k].w, qm[k].w, qv[k].w);
        *reinterpret_cast<float4*>(p + j) = qp[k];
        *reinterpret_cast<float4*>(m + j) = qm[k];
        *reinterpret_cast<float4*>(v + j) = qv[k];
      }
    } else {
      // a row whose pointers are not all 16-byte aligned, and every tail chunk: the same elements per thread, one by one
      for (int k = 0; k < AVSO_GROUPS_PER_THREAD; ++k)
        for (int e = 0; e < 4; ++e) {
          const int j = 4 * (threadIdx.x + AVSO_THREADS * k) + e;
          if (j < len) {
            float ep = p[j], em = m[j], ev = v[j];
            avso_adamw_element(h, ep, g[j], em, ev);
            p[j] = ep, m[j] = em, v[j] = ev;
          }
        }
    }
  }
}

// h_table -> the kernel argument.  Validates every row; *nchunks = chunks of the launch.
static int avso_build_table(const char* who, const int64_t* h_table, int ntensors, bool need_all, avso_table* tab,
                            int* nchunks) {
  AVSO_REQUIRE(h_table != nullptr, AVSO_E_ARG, "%s: h_table is null", who);
  AVSO_REQUIRE(ntensors >= 1 && ntensors <= AVSO_MAX_TENSORS, AVSO_E_ARG, "%s: ntensors = %d, must be 1..%d", who,
               ntensors, AVSO_MAX_TENSORS);
  *tab = avso_table{};
  int64_t chunks = 0;
  for (int t = 0; t < ntensors; ++t) {
    const int64_t* row = h_table + (int64_t)t * AVSO_TABLE_COLS;
    const int64_t numel = row[4];
    AVSO_REQUIRE(numel >= 0, AVSO_E_ARG, "%s: row %d has numel = %lld", who, t, (long long)numel);
    bool vec = true;
    for (int a = 0; a < 4; ++a) {
      if (!need_all && a != 1) continue;          // the norm pass reads the gradient only
      AVSO_REQUIRE(numel == 0 || row[a] != 0, AVSO_E_ARG, "%s: row %d, pointer %d is null", who, t, a);
      AVSO_REQUIRE((row[a] & 3) == 0, AVSO_E_ALIGN, "%s: row %d, pointer %d is not 4-byte aligned", who, t, a);
      vec = vec && (row[a] & 15) == 0;
      tab->ptr[a][t] = reinterpret_cast<float*>(static_cast<uintptr_t>(row[a]));
    }
    tab->numel[t] = numel;
    tab->start[t] = (int)chunks;
    if (vec) tab->vec_mask |= 1u << t;
    chunks += (numel + AVSO_CHUNK - 1) / AVSO_CHUNK;
    AVSO_REQUIRE(chunks <= INT32_MAX, AVSO_E_SHAPE, "%s: more than 2^31 - 1 chunks in one launch", who);
  }
  tab->start[ntensors] = (int)chunks;
  tab->ntensors = ntensors;
  *nchunks = (int)chunks;
  return AVSO_OK;
}

static inline unsigned avso_grid(int nchunks) { return nchunks < AVSO_MAX_GROUPS ? nchunks : AVSO_MAX_GROUPS; }

extern "C" int avso_abi_version(void) { return AVSO_ABI_VERSION; }

extern "C" const char* avso_last_error(void) { return g_err; }

extern "C" size_t avso_workspace_bytes(int64_t total_chunks) {
  if (total_chunks < 0) return 0;
  return (size_t)AVSO_PARTIALS_OFFSET + sizeof(double) * (size_t)total_chunks;
}

extern "C" int avso_grad_sumsq_f32(const int64_t* h_table, int ntensors, double* d_partials, int64_t first_chunk,
                                   int64_t total_chunks, avso_stream_t stream) {
  avso_table tab;
  int nchunks = 0;
  const int st = avso_build_table("avso_grad_sumsq_f32", h_table, ntensors, false, &tab, &nchunks);
  if (st != AVSO_OK) return st;
  AVSO_REQUIRE(d_partials != nullptr, AVSO_E_ARG, "avso_grad_sumsq_f32: d_partials is null");
  AVSO_REQUIRE((((uintptr_t)d_partials) & 7u) == 0, AVSO_E_ALIGN, "avso_grad_sumsq_f32: d_partials is not 8-byte aligned");
  AVSO_REQUIRE(first_chunk >= 0 && total_chunks >= 0, AVSO_E_ARG,
               "avso_grad_sumsq_f32: first_chunk = %lld, total_chunks = %lld", (long long)first_chunk,
               (long long)total_chunks);
  AVSO_REQUIRE(first_chunk + nchunks <= total_chunks, AVSO_E_WORKSPACE,
               "avso_grad_sumsq_f32: chunks %lld .. %lld do not fit %lld partials", (long long)first_chunk,
               (long long)(first_chunk + nchunks), (long long)total_chunks);
  if (nchunks == 0) return AVSO_OK;
  hipLaunchKernelGGL(avso_grad_sumsq_kernel, dim3(avso_grid(nchunks)), dim3(AVSO_THREADS), 0, (hipStream_t)stream, tab,
                     d_partials + first_chunk);
  AVSO_CHECK_LAUNCH("avso_grad_sumsq_f32");
  return AVSO_OK;
}

extern "C" int avso_adamw_prepare(const double* d_partials, int64_t npartials, double lr, double beta1, double beta2,
                                  double weight_decay, double max_norm, int skip_nonfinite, double* d_state,
                                  float* d_coef, avso_stream_t stream) {
  AVSO_REQUIRE(npartials >= 0, AVSO_E_ARG, "avso_adamw_prepare: npartials = %lld", (long long)npartials);
  AVSO_REQUIRE(npartials == 0 || d_partials != nullptr, AVSO_E_ARG, "avso_adamw_prepare: d_partials is null");
  AVSO_REQUIRE(d_state != nullptr && d_coef != nullptr, AVSO_E_ARG, "avso_adamw_prepare: d_state or d_coef is null");
  AVSO_REQUIRE(((((uintptr_t)d_partials) | ((uintptr_t)d_state)) & 7u) == 0 && (((uintptr_t)d_coef) & 3u) == 0,
               AVSO_E_ALIGN, "avso_adamw_prepare: d_partials / d_state / d_coef not aligned to their elements");
  AVSO_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, AVSO_E_ARG, "avso_adamw_prepare: lr = %g, weight_decay = %g", lr,
               weight_decay);
  AVSO_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, AVSO_E_ARG,
               "avso_adamw_prepare: betas = (%g, %g), must lie in [0, 1)", beta1, beta2);
  AVSO_REQUIRE(max_norm == max_norm, AVSO_E_ARG, "avso_adamw_prepare: max_norm is NaN");
  hipLaunchKernelGGL(avso_adamw_prepare_kernel, dim3(1), dim3(AVSO_THREADS), 0, (hipStream_t)stream, d_partials,
                     npartials, lr, beta1, beta2, weight_decay, max_norm, skip_nonfinite, d_state, d_coef);
  AVSO_CHECK_LAUNCH("avso_adamw_prepare");
  return AVSO_OK;
}

extern "C" int avso_adamw_apply_f32(const int64_t* h_table, int ntensors, const float* d_coef, double beta1,
                                    double beta2, double eps, avso_stream_t stream) {
  avso_table tab;
  int nchunks = 0;
  const int st = avso_build_table("avso_adamw_apply_f32", h_table, ntensors, true, &tab, &nchunks);
  if (st != AVSO_OK) return st;
  AVSO_REQUIRE(d_coef != nullptr, AVSO_E_ARG, "avso_adamw_apply_f32: d_coef is null");
  AVSO_REQUIRE((((uintptr_t)d_coef) & 3u) == 0, AVSO_E_ALIGN, "avso_adamw_apply_f32: d_coef is not 4-byte aligned");
  AVSO_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, AVSO_E_ARG,
               "avso_adamw_apply_f32: betas = (%g, %g), must lie in [0, 1)", beta1, beta2);
  AVSO_REQUIRE(eps >= 0.0, AVSO_E_ARG, "avso_adamw_apply_f32: eps = %g", eps);
  if (nchunks == 0) return AVSO_OK;
  hipLaunchKernelGGL(avso_adamw_apply_kernel, dim3(avso_grid(nchunks)), dim3(AVSO_THREADS), 0, (hipStream_t)stream, tab,
                     d_coef, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
  AVSO_CHECK_LAUNCH("avso_adamw_apply_f32");
  return AVSO_OK;
}
