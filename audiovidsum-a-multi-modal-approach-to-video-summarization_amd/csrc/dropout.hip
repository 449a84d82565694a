// libavsum_dropout.so: counter-based Dropout masks for a ragged batch of videos (include/avsum_dropout.h; the
// comment there is the definition).  A fifth library: this file includes its own header only.
//
// One kernel body, three modes.  A thread owns AVSD_VEC = 4 consecutive columns of one row: one Philox4x32-10 call gives
// their four words, the inputs come in as one 16-byte load each, the result leaves as one 16-byte store.  Items
// (row, column quad) are numbered row-major, so the lanes of a wave read and write consecutive 16-byte pieces of a row;
// the launch is grid-stride, capped at AVSD_MAX_GROUPS workgroups.  The row's video is found by binary search over the
// device offsets: log2(nseq) loads that hit the cache, against 40 integer multiplies of the generator.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/avsum_dropout.h"

static_assert(AVSD_VEC == 4, "a Philox call yields four words: a thread owns four columns");
static_assert(AVSD_BLOCK == 256, "the launch bounds of the kernel");

static thread_local char g_err[512] = "";

static void avsd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSD_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsd_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSD_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsd_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSD_E_HIP;                                                         \
    }                                                                            \
  } while (0)

#define AVSD_TRY(call)                \
  do {                                \
    const int st__ = (call);          \
    if (st__ != AVSD_OK) return st__; \
  } while (0)

// ------------------------------------------------------------------------------------------------------ generator
struct avsd_words {
  uint32_t w[4];
};

__device__ __forceinline__ avsd_words avsd_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                         uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return {{c0, c1, c2, c3}};
}

// what every launch shares
struct avsd_batch {
  const int64_t* offsets;   // [nseq + 1], device
  const int64_t* samples;   // [nseq], device, or nullptr: sample_base + v
  long long sample_base;
  long long rows;
  int nseq;
  int quads;                // cols / 4
  uint32_t k0, k1, thr;
  uint32_t branch;
  float scale;
};

// the four multipliers of item (row, quad)
__device__ __forceinline__ float4 avsd_multipliers(const avsd_batch& b, long long row, int quad) {
  // the last v in 0 .. nseq - 1 with offsets[v] <= row
  int lo = 0, hi = b.nseq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (b.offsets[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t sample = (uint64_t)(b.samples ? b.samples[lo] : b.sample_base + lo);
  const uint32_t local = (uint32_t)(row - b.offsets[lo]);
  const avsd_words r = avsd_philox4x32_10((uint32_t)quad, local, (uint32_t)sample,
                                          (((uint32_t)(sample >> 32)) << 1) | b.branch, b.k0, b.k1);
  return make_float4(r.w[0] >= b.thr ? b.scale : 0.0f, r.w[1] >= b.thr ? b.scale : 0.0f,
                     r.w[2] >= b.thr ? b.scale : 0.0f, r.w[3] >= b.thr ? b.scale : 0.0f);
}

enum { AVSD_MODE_MASK = 0, AVSD_MODE_FWD = 1, AVSD_MODE_BWD = 2 };

// MASK: out = m.  FWD: out = a * m (a = x).  BWD: out = g > 0 ? a * m : 0 (a = dy, g = relu_out).
// a / out carry no __restrict__: the in-place forms read an item's 16 bytes before they write the same 16 bytes.
template <int MODE>
__global__ __launch_bounds__(AVSD_BLOCK) void avsd_kernel(const float* a, long long lda, const float* g, long long ldg,
                                                          float* out, long long ldo, const avsd_batch b) {
  const long long items = b.rows * b.quads;
  for (long long i = (long long)blockIdx.x * AVSD_BLOCK + threadIdx.x; i < items;
       i += (long long)gridDim.x * AVSD_BLOCK) {
    const long long row = i / b.quads;
    const int quad = (int)(i - row * b.quads);
    const float4 m = avsd_multipliers(b, row, quad);
    float4 r = m;
    if (MODE != AVSD_MODE_MASK) {
      const float4 x = *reinterpret_cast<const float4*>(a + row * lda + 4 * quad);
      r = make_float4(x.x * m.x, x.y * m.y, x.z * m.z, x.w * m.w);
    }
    if (MODE == AVSD_MODE_BWD) {
      const float4 y = *reinterpret_cast<const float4*>(g + row * ldg + 4 * quad);
      r = make_float4(y.x > 0.f ? r.x : 0.f, y.y > 0.f ? r.y : 0.f, y.z > 0.f ? r.z : 0.f, y.w > 0.f ? r.w : 0.f);
    }
    *reinterpret_cast<float4*>(out + row * ldo + 4 * quad) = r;
  }
}

// ----------------------------------------------------------------------------------------------------------- host
static bool avsd_aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

static int avsd_check_operand(const char* who, const char* name, const void* p, int64_t ld, int cols) {
  AVSD_REQUIRE(p, AVSD_E_ARG, "%s: %s is a null pointer", who, name);
  AVSD_REQUIRE(ld >= cols && ld % AVSD_VEC == 0, AVSD_E_SHAPE,
               "%s: the row stride of %s is %lld: it must be a multiple of %d and at least cols = %d", who, name,
               (long long)ld, AVSD_VEC, cols);
  AVSD_REQUIRE(avsd_aligned(p, 16), AVSD_E_ALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AVSD_OK;
}

static int avsd_check_batch(const char* who, const int64_t* d_offsets, int nseq, int64_t rows, int cols, int branch,
                            int64_t sample_base, const int64_t* d_samples) {
  AVSD_REQUIRE(rows >= 0 && cols >= 0, AVSD_E_SHAPE, "%s: negative size: rows=%lld cols=%d", who, (long long)rows, cols);
  AVSD_REQUIRE(nseq >= 1 && nseq <= AVSD_MAX_SEQ, AVSD_E_ARG, "%s: nseq=%d, must be 1 .. %d", who, nseq, AVSD_MAX_SEQ);
  AVSD_REQUIRE(rows <= AVSD_MAX_ROWS, AVSD_E_SHAPE, "%s: rows=%lld, at most %d", who, (long long)rows, AVSD_MAX_ROWS);
  AVSD_REQUIRE(cols % AVSD_VEC == 0, AVSD_E_SHAPE, "%s: cols=%d is not a multiple of %d", who, cols, AVSD_VEC);
  AVSD_REQUIRE(branch == 0 || branch == 1, AVSD_E_ARG, "%s: branch=%d, must be 0 (visual) or 1 (audio)", who, branch);
  AVSD_REQUIRE(d_offsets, AVSD_E_ARG, "%s: d_offsets is a null pointer", who);
  AVSD_REQUIRE(avsd_aligned(d_offsets, 8) && avsd_aligned(d_samples, 8), AVSD_E_ALIGN,
               "%s: d_offsets / d_samples must be 8-byte aligned", who);
  AVSD_REQUIRE(d_samples || (sample_base >= 0 && sample_base <= INT64_MAX - (nseq - 1)), AVSD_E_ARG,
               "%s: sample ids %lld .. +%d leave 0 .. 2^63 - 1", who, (long long)sample_base, nseq - 1);
  return AVSD_OK;
}

static avsd_batch avsd_make_batch(const int64_t* d_offsets, int nseq, int64_t rows, int cols, uint64_t seed,
                                  uint32_t thr, float scale, int branch, int64_t sample_base,
                                  const int64_t* d_samples) {
  avsd_batch b;
  b.offsets = d_offsets;
  b.samples = d_samples;
  b.sample_base = d_samples ? 0 : (long long)sample_base;
  b.rows = (long long)rows;
  b.nseq = nseq;
  b.quads = cols / AVSD_VEC;
  b.k0 = (uint32_t)(seed & 0xffffffffu);
  b.k1 = (uint32_t)(seed >> 32);
  b.thr = thr;
  b.branch = (uint32_t)branch;
  b.scale = scale;
  return b;
}

static unsigned avsd_groups(const avsd_batch& b) {
  const long long items = b.rows * b.quads;
  const long long groups = (items + AVSD_BLOCK - 1) / AVSD_BLOCK;
  return (unsigned)(groups > AVSD_MAX_GROUPS ? AVSD_MAX_GROUPS : groups);
}

extern "C" int avsd_abi_version(void) { return AVSD_ABI_VERSION; }

extern "C" const char* avsd_last_error(void) { return g_err; }

extern "C" int avsd_keep_mask_f32(float* d_out, int64_t ldo, const int64_t* d_offsets, int nseq, int64_t rows, int cols,
                                  uint64_t seed, uint32_t thr, float scale, int branch, int64_t sample_base,
                                  const int64_t* d_samples, avsd_stream_t stream) {
  const char* who = "avsd_keep_mask_f32";
  AVSD_TRY(avsd_check_batch(who, d_offsets, nseq, rows, cols, branch, sample_base, d_samples));
  AVSD_TRY(avsd_check_operand(who, "d_out", d_out, ldo, cols));
  if (rows == 0 || cols == 0) return AVSD_OK;
  const avsd_batch b = avsd_make_batch(d_offsets, nseq, rows, cols, seed, thr, scale, branch, sample_base, d_samples);
  hipLaunchKernelGGL((avsd_kernel<AVSD_MODE_MASK>), dim3(avsd_groups(b)), dim3(AVSD_BLOCK), 0, (hipStream_t)stream,
                     (const float*)nullptr, 0LL, (const float*)nullptr, 0LL, d_out, (long long)ldo, b);
  AVSD_CHECK_LAUNCH(who);
  return AVSD_OK;
}

extern "C" int avsd_dropout_fwd_f32(const float* d_x, int64_t ldx, float* d_out, int64_t ldo, const int64_t* d_offsets,
                                    int nseq, int64_t rows, int cols, uint64_t seed, uint32_t thr, float scale,
                                    int branch, int64_t sample_base, const int64_t* d_samples, avsd_stream_t stream) {
  const char* who = "avsd_dropout_fwd_f32";
  AVSD_TRY(avsd_check_batch(who, d_offsets, nseq, rows, cols, branch, sample_base, d_samples));
  AVSD_TRY(avsd_check_operand(who, "d_x", d_x, ldx, cols));
  AVSD_TRY(avsd_check_operand(who, "d_out", d_out, ldo, cols));
  if (rows == 0 || cols == 0) return AVSD_OK;
  const avsd_batch b = avsd_make_batch(d_offsets, nseq, rows, cols, seed, thr, scale, branch, sample_base, d_samples);
  hipLaunchKernelGGL((avsd_kernel<AVSD_MODE_FWD>), dim3(avsd_groups(b)), dim3(AVSD_BLOCK), 0, (hipStream_t)stream, d_x,
                     (long long)ldx, (const float*)nullptr, 0LL, d_out, (long long)ldo, b);
  AVSD_CHECK_LAUNCH(who);
  return AVSD_OK;
}

extern "C" int avsd_relu_dropout_bwd_f32(const float* d_dy, int64_t lddy, const float* d_relu_out, int64_t ldr,
                                         float* d_out, int64_t ldo, const int64_t* d_offsets, int nseq, int64_t rows,
                                         int cols, uint64_t seed, uint32_t thr, float scale, int branch,
                                         int64_t sample_base, const int64_t* d_samples, avsd_stream_t stream) {
  const char* who = "avsd_relu_dropout_bwd_f32";
  AVSD_TRY(avsd_check_batch(who, d_offsets, nseq, rows, cols, branch, sample_base, d_samples));
  AVSD_TRY(avsd_check_operand(who, "d_dy", d_dy, lddy, cols));
  AVSD_TRY(avsd_check_operand(who, "d_relu_out", d_relu_out, ldr, cols));
  AVSD_TRY(avsd_check_operand(who, "d_out", d_out, ldo, cols));
  if (rows == 0 || cols == 0) return AVSD_OK;
  const avsd_batch b = avsd_make_batch(d_offsets, nseq, rows, cols, seed, thr, scale, branch, sample_base, d_samples);
  hipLaunchKernelGGL((avsd_kernel<AVSD_MODE_BWD>), dim3(avsd_groups(b)), dim3(AVSD_BLOCK), 0, (hipStream_t)stream, d_dy,
                     (long long)lddy, d_relu_out, (long long)ldr, d_out, (long long)ldo, b);
  AVSD_CHECK_LAUNCH(who);
  return AVSD_OK;
}
