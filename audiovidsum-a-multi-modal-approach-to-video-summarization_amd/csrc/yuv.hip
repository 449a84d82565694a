// libavsum_yuv.so: planar, semi-planar and 10-bit YUV 4:2:0 frames read where they lie (include/avsum_yuv.h).  This file
// is the whole library.  It includes avs_internal.h and pixel_bodies.h for their inline helpers only (bgr2hsv_u8, the one
// definition of the HSV pixel arithmetic; the one text of the bilinear resize and of the shot scan) and references no
// symbol of another library: the error text, the argument checks and the launch check below are its own.
//
// Three kernels, one pixel definition (avsy_yuv2bgr), each compiled for (SB, PLANAR):
//   SB      bytes of a sample: 1 (depth 8, the int32 arithmetic of ingest.hip) or 2 (depth 10: the sample is
//           (word >> shift) & 1023 and the sums are 64-bit)
//   PLANAR  false: V lies one sample beside U (NV12, NV21, P010) - one pointer serves both, and the resize stages ONE row
//           of pairs per chroma line; true: U and V have planes of their own (I420, YV12, yuv420p10le) - a U row and a V row
// so no one-byte path carries a per-sample branch, a shift or a mask.
//   yuv_to_bgr_kernel          four pixels - two chroma samples - per thread, 12 output bytes; one load per plane
//                              where the frame's width and alignment allow it
//   yuv_resize_gather2_kernel  nv12_resize_gather2_kernel's structure (ingest.hip) over rows of either sample size: the
//                              band's luma and chroma rows staged into LDS at their global address modulo 16, converted
//                              per tap: pixel_bodies.h's 11-bit bilinear arithmetic
//   yuv_hsv_diff_batch_kernel  pixel_bodies.h's scan with a YUV pixel source
// Integers and fixed orders: two calls give the same bytes.
#include <stdarg.h>
#include "avs_internal.h"
#include "pixel_bodies.h"
#include "../../include/avsum_yuv.h"

#define NY_THREADS 256
#define NY_MAX_GRID_X (0xffffffffll / NY_THREADS)   // a launch holds at most 2^32 - 1 threads per grid dimension
#define NY_INFLIGHT 4                               // 16-byte loads a thread keeps in flight while staging rows
static_assert(NY_MAX_GRID_X + 1 == AVSY_MAX_DIFF_FRAMES, "the frame of the scan is on grid x");
static_assert(511ll * AVSY_MAX_COEF + (1 << (AVSY_SHIFT - 1)) < (1ll << 31), "the largest depth-8 accumulator fits int32");

static thread_local char g_err[512] = "";

static void avsy_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSY_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsy_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSY_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsy_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSY_E_HIP;                                                         \
    }                                                                            \
  } while (0)

extern "C" int avsy_abi_version(void) { return AVSY_ABI_VERSION; }
extern "C" const char* avsy_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// The frames of a call and the pixel definition.
// ---------------------------------------------------------------------------
struct avsy_mat {
  int y_off, cy, cub, cug, cvg, cvr;
};
struct avsy_frames {
  const uint8_t* src;
  long long n, frame_stride, u_offset, v_offset;
  int h, w, sample_bytes, shift, pitch_y, pitch_c, step;
  bool planar;   // U and V in planes of their own (false: V one sample before or after U, step of two samples)
  avsy_mat m;
};

__device__ __forceinline__ int avsy_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the sample at p: the byte, or ten bits of the 16-bit word (p is even: the checks saw to it)
template <int SB>
__device__ __forceinline__ int avsy_sample(const uint8_t* p, int shift) {
  if (SB == 1) return *p;
  return (*reinterpret_cast<const uint16_t*>(p) >> shift) & 1023;
}

template <int SB>
__device__ __forceinline__ void avsy_yuv2bgr(const avsy_mat& m, int Y, int U, int V, int& b, int& g, int& r) {
  if (SB == 1) {   // avsi_yuv2bgr of ingest.hip, integer for integer
    const int yy = max(Y - m.y_off, 0) * m.cy + (1 << (AVSY_SHIFT - 1));
    const int uu = U - 128, vv = V - 128;
    b = avsy_clamp8((yy + m.cub * uu) >> AVSY_SHIFT);
    g = avsy_clamp8((yy + m.cvg * vv + m.cug * uu) >> AVSY_SHIFT);
    r = avsy_clamp8((yy + m.cvr * vv) >> AVSY_SHIFT);
  } else {         // depth 10: k = 2; 1023 * 2^22 alone is past int32, so the sums are 64-bit (an int32 x int32 + int64
                   // multiply-add each); after >> 22 every one of them is within +-2^11 and the clamp is on ints again
    constexpr int K = 2;
    const long long yy = (long long)max(Y - (m.y_off << K), 0) * m.cy + (1ll << (AVSY_SHIFT - 1 + K));
    const int uu = U - (128 << K), vv = V - (128 << K);
    b = avsy_clamp8((int)((yy + (long long)m.cub * uu) >> (AVSY_SHIFT + K)));
    g = avsy_clamp8((int)((yy + (long long)m.cvg * vv + (long long)m.cug * uu) >> (AVSY_SHIFT + K)));
    r = avsy_clamp8((int)((yy + (long long)m.cvr * vv) >> (AVSY_SHIFT + K)));
  }
}

// the U and the V sample at chroma position (row, col) of frame `f`
template <int SB, bool PLANAR>
__device__ __forceinline__ void avsy_chroma(const avsy_frames& F, const uint8_t* f, int row, int col, int& U, int& V) {
  const long long o = (long long)row * F.pitch_c + (long long)col * F.step;
  const uint8_t* pu = f + F.u_offset + o;
  // interleaved: V through U's pointer, SB bytes before or after it (a wave-uniform difference)
  const uint8_t* pv = PLANAR ? f + F.v_offset + o : pu + (int)(F.v_offset - F.u_offset);
  U = avsy_sample<SB>(pu, F.shift), V = avsy_sample<SB>(pv, F.shift);
}

// pixel (y, x) of frame `f`, converted
template <int SB, bool PLANAR>
__device__ __forceinline__ void avsy_pixel(const avsy_frames& F, const uint8_t* f, int y, int x, int& b, int& g, int& r) {
  int U, V;
  avsy_chroma<SB, PLANAR>(F, f, y >> 1, x >> 1, U, V);
  avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(f + (long long)y * F.pitch_y + x * SB, F.shift), U, V, b, g, r);
}

// Do the samples of two chroma planes of the same pitch and step, `delta` bytes apart, share a byte?  Sample (r, c) of
// the one and (r + dr, c + dc) of the other do when |delta - dr * pitch - dc * step| < sb; a row of samples is shorter
// than the pitch, so only the two dr around delta / pitch can, and for each only the two dc around the rest / step.
static bool avsy_chroma_planes_meet(long long delta, long long pitch, long long step, long long sb, long long ch, long long cw) {
  if (delta < 0) delta = -delta;
  for (long long dr = delta / pitch; dr <= delta / pitch + 1; ++dr) {
    if (dr > ch - 1) continue;
    const long long rest = delta - dr * pitch;   // in (-pitch, pitch)
    const long long q = rest >= 0 ? rest / step : -((-rest + step - 1) / step);   // floor
    for (long long dc = q; dc <= q + 1; ++dc) {
      const long long d = rest - dc * step;
      if (dc >= -(cw - 1) && dc <= cw - 1 && d > -sb && d < sb) return true;
    }
  }
  return false;
}

// Does a sample of the chroma plane at `off` share a byte with a luma sample?  Luma row y is the bytes
// [y * pitch_y, y * pitch_y + w * sb); a chroma row meets few luma rows, and within one the first chroma sample that ends
// past the luma row's start decides.
static bool avsy_chroma_meets_luma(long long off, long long pitch_y, long long pitch_c, long long step, long long sb,
                                   long long h, long long w) {
  const long long ch = h / 2, cw = w / 2, luma_end = (h - 1) * pitch_y + w * sb;
  if (off >= luma_end) return false;   // the plane begins after the last luma sample: every layout in use
  for (long long r = 0; r < ch; ++r) {
    const long long a = off + r * pitch_c, b = a + (cw - 1) * step + sb;   // the chroma row's bytes [a, b)
    if (a >= luma_end) break;
    for (long long y = a / pitch_y; y < h && y * pitch_y < b; ++y) {
      const long long ya = y * pitch_y, yb = ya + w * sb;
      long long c = ya - sb - a < 0 ? 0 : (ya - sb - a) / step + 1;   // the first sample with a + c * step + sb > ya
      if (c < cw && a + c * step < yb) return true;
    }
  }
  return false;
}

// the checks every entry point shares; fills F
static int avsy_frames_arg(const char* what, avsy_frames& F, const uint8_t* d_src, const int64_t* h_surface,
                           const int* h_matrix) {
  AVSY_REQUIRE(h_surface, AVSY_E_ARG, "%s: h_surface is null", what);
  const long long n = h_surface[AVSY_S_N], h = h_surface[AVSY_S_H], w = h_surface[AVSY_S_W];
  const long long sb = h_surface[AVSY_S_SAMPLE_BYTES], shift = h_surface[AVSY_S_SHIFT];
  const long long pitch_y = h_surface[AVSY_S_PITCH_Y], pitch_c = h_surface[AVSY_S_PITCH_C];
  const long long step = h_surface[AVSY_S_CHROMA_STEP], u_off = h_surface[AVSY_S_U_OFFSET];
  const long long v_off = h_surface[AVSY_S_V_OFFSET], stride = h_surface[AVSY_S_FRAME_STRIDE];
  AVSY_REQUIRE(n >= 0, AVSY_E_SHAPE, "%s: n=%lld frames", what, n);
  AVSY_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, AVSY_E_SHAPE,
               "%s: 4:2:0 frames have even extents of at least 2, got %lldx%lld", what, h, w);
  AVSY_REQUIRE(h < (1ll << 31) && w < (1ll << 31) && h * w * 3 < (1ll << 31), AVSY_E_SHAPE,
               "%s: a frame of %lldx%lld is too large", what, h, w);
  AVSY_REQUIRE(sb == 1 || sb == 2, AVSY_E_SHAPE, "%s: sample_bytes %lld is neither 1 nor 2", what, sb);
  AVSY_REQUIRE((shift == 0 || shift == 6) && (sb == 2 || shift == 0), AVSY_E_SHAPE,
               "%s: shift %lld with samples of %lld bytes (0 or 6; 0 for one-byte samples)", what, shift, sb);
  const long long ch = h / 2, cw = w / 2;
  AVSY_REQUIRE(pitch_y >= w * sb && pitch_y < (1ll << 31), AVSY_E_SHAPE, "%s: pitch_y %lld below the %lld bytes of a luma row",
               what, pitch_y, w * sb);
  AVSY_REQUIRE(step >= sb && step < (1ll << 24), AVSY_E_SHAPE, "%s: chroma_step %lld below the %lld bytes of a sample", what,
               step, sb);
  const long long crow = (cw - 1) * step + sb;   // the bytes from a chroma row's first sample to the end of its last
  AVSY_REQUIRE(pitch_c >= crow && pitch_c < (1ll << 31), AVSY_E_SHAPE, "%s: pitch_c %lld below the %lld bytes of a chroma row",
               what, pitch_c, crow);
  AVSY_REQUIRE(u_off >= 0 && v_off >= 0, AVSY_E_SHAPE, "%s: negative plane offset (u_offset %lld, v_offset %lld)", what, u_off,
               v_off);
  const long long y_end = (h - 1) * pitch_y + w * sb;
  const long long u_end = u_off + (ch - 1) * pitch_c + crow, v_end = v_off + (ch - 1) * pitch_c + crow;
  AVSY_REQUIRE(stride >= y_end && stride >= u_end && stride >= v_end, AVSY_E_SHAPE,
               "%s: frame_stride %lld ends before a plane does (luma %lld, U %lld, V %lld)", what, stride, y_end, u_end, v_end);
  if (sb == 2)
    AVSY_REQUIRE(((uintptr_t)d_src | (unsigned long long)pitch_y | (unsigned long long)pitch_c | (unsigned long long)step |
                  (unsigned long long)u_off | (unsigned long long)v_off | (unsigned long long)stride) % 2 == 0,
                 AVSY_E_SHAPE, "%s: two-byte samples need an even base, pitch_y, pitch_c, chroma_step, u_offset, v_offset and "
                 "frame_stride", what);
  AVSY_REQUIRE(!avsy_chroma_planes_meet(v_off - u_off, pitch_c, step, sb, ch, cw), AVSY_E_SHAPE,
               "%s: the U and V planes overlap (u_offset %lld, v_offset %lld)", what, u_off, v_off);
  AVSY_REQUIRE(!avsy_chroma_meets_luma(u_off, pitch_y, pitch_c, step, sb, h, w) &&
               !avsy_chroma_meets_luma(v_off, pitch_y, pitch_c, step, sb, h, w), AVSY_E_SHAPE,
               "%s: a chroma plane overlaps the luma plane (u_offset %lld, v_offset %lld, luma ends at %lld)", what, u_off,
               v_off, y_end);
  AVSY_REQUIRE(h_matrix, AVSY_E_ARG, "%s: h_matrix is null", what);
  AVSY_REQUIRE(h_matrix[0] >= 0 && h_matrix[0] <= 255, AVSY_E_ARG, "%s: y_off %d outside 0 .. 255", what, h_matrix[0]);
  for (int k = 1; k < AVSY_MATRIX_INTS; ++k)
    AVSY_REQUIRE(h_matrix[k] >= -AVSY_MAX_COEF && h_matrix[k] <= AVSY_MAX_COEF, AVSY_E_ARG,
                 "%s: coefficient %d of the matrix is %d, above 2^22 in magnitude", what, k, h_matrix[k]);
  F.src = d_src;
  F.n = n, F.frame_stride = stride, F.u_offset = u_off, F.v_offset = v_off;
  F.h = (int)h, F.w = (int)w, F.sample_bytes = (int)sb, F.shift = (int)shift;
  F.pitch_y = (int)pitch_y, F.pitch_c = (int)pitch_c, F.step = (int)step;
  F.planar = !(step == 2 * sb && (v_off - u_off == sb || u_off - v_off == sb));
  F.m = avsy_mat{h_matrix[0], h_matrix[1], h_matrix[2], h_matrix[3], h_matrix[4], h_matrix[5]};
  return AVSY_OK;
}

// launches KERNEL<SB, PLANAR> of F
#define NY_LAUNCH(F, KERNEL, grid, lds, stream, ...)                                                              \
  do {                                                                                                            \
    if ((F).sample_bytes == 1 && !(F).planar)                                                                     \
      hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(NY_THREADS), lds, (hipStream_t)(stream), __VA_ARGS__);     \
    else if ((F).sample_bytes == 1)                                                                               \
      hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(NY_THREADS), lds, (hipStream_t)(stream), __VA_ARGS__);      \
    else if (!(F).planar)                                                                                         \
      hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(NY_THREADS), lds, (hipStream_t)(stream), __VA_ARGS__);     \
    else                                                                                                          \
      hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(NY_THREADS), lds, (hipStream_t)(stream), __VA_ARGS__);      \
  } while (0)

// ---------------------------------------------------------------------------
// 1. Dense BGR.  The h * w pixels of a frame in output order, four to a thread: w is even, so pixels 4g, 4g + 1 share
// a row and a chroma sample, and so do 4g + 2, 4g + 3.  A frame's output begins a multiple of 12 bytes after d_bgr, so
// the 12 bytes of a thread leave as three dwords where d_bgr is 4-byte aligned and singly where it is not.
// Where w is a multiple of 4 the four pixels share a row, and where the frame's base, the pitches and the plane offsets
// are multiples of four samples' bytes (what decoders allocate) the thread takes the WIDE form: its four luma samples
// in one load, its two chroma samples of each plane in one load per plane (planar, samples back to back) or the two
// pairs in one (interleaved) - three or two loads where the narrow form issues eight.  The same samples, the same bytes.
// ---------------------------------------------------------------------------
// four samples at p (4 * SB-aligned) into lo (and hi), two samples (2 * SB-aligned) into the result
template <int SB>
__device__ __forceinline__ void avsy_load4(const uint8_t* p, unsigned& lo, unsigned& hi) {
  if (SB == 1) {
    lo = *reinterpret_cast<const unsigned*>(p), hi = 0;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    lo = v.x, hi = v.y;
  }
}
template <int SB>
__device__ __forceinline__ unsigned avsy_load2(const uint8_t* p) {
  return SB == 1 ? (unsigned)*reinterpret_cast<const uint16_t*>(p) : *reinterpret_cast<const unsigned*>(p);
}
// sample k (0 .. 3) of the samples avsy_load4 (or, k < 2, avsy_load2 with hi = 0) brought
template <int SB>
__device__ __forceinline__ int avsy_lane(unsigned lo, unsigned hi, int k, int shift) {
  if (SB == 1) return (int)((lo >> (8 * k)) & 255u);
  const unsigned w = ((k < 2 ? lo : hi) >> (16 * (k & 1))) & 0xffffu;
  return (int)((w >> shift) & 1023u);
}

template <int SB, bool PLANAR>
__global__ __launch_bounds__(NY_THREADS) void yuv_to_bgr_kernel(avsy_frames F, const long long* __restrict__ index,
                                                                uint8_t* __restrict__ dst) {
  const long long i = blockIdx.x;
  const long long r = index ? index[i] : i;
  if (r < 0 || r >= F.n) return;
  const uint8_t* f = F.src + r * F.frame_stride;
  uint8_t* o = dst + i * ((long long)F.h * F.w * 3);
  const bool vec = ((unsigned)(uintptr_t)o & 3u) == 0;
  const int groups = (F.h * F.w) >> 2;
  // block-uniform: every address the wide form loads from is a multiple of 4 * SB (interleaved: the pairs begin at
  // the lower of the two offsets)
  const long long c_first = PLANAR ? F.u_offset : min(F.u_offset, F.v_offset);
  const unsigned long long low_bits = (unsigned long long)(uintptr_t)f | (unsigned)F.pitch_y | (unsigned)F.pitch_c |
                                      (unsigned long long)c_first | (PLANAR ? (unsigned long long)F.v_offset : 0ull);
  const bool wide = (F.w & 3) == 0 && (low_bits & (4 * SB - 1)) == 0 && (!PLANAR || F.step == SB);
  const int u_in_pair = F.u_offset > F.v_offset ? 1 : 0;   // (interleaved) which sample of a pair is U
  for (int g = blockIdx.y * NY_THREADS + threadIdx.x; g < groups; g += gridDim.y * NY_THREADS) {
    unsigned px[12];
    if (wide) {
      const int p = 4 * g;
      const int y = p / F.w, x = p - y * F.w;   // (x is a multiple of 4)
      unsigned ylo, yhi;
      avsy_load4<SB>(f + (long long)y * F.pitch_y + x * SB, ylo, yhi);
      const long long co = (long long)(y >> 1) * F.pitch_c + (long long)(x >> 1) * F.step;
      int U[2], V[2];
      if (PLANAR) {
        const unsigned uw = avsy_load2<SB>(f + F.u_offset + co), vw = avsy_load2<SB>(f + F.v_offset + co);
#pragma unroll
        for (int j = 0; j < 2; ++j) U[j] = avsy_lane<SB>(uw, 0, j, F.shift), V[j] = avsy_lane<SB>(vw, 0, j, F.shift);
      } else {
        unsigned clo, chi;
        avsy_load4<SB>(f + c_first + co, clo, chi);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          U[j] = avsy_lane<SB>(clo, chi, 2 * j + u_in_pair, F.shift);
          V[j] = avsy_lane<SB>(clo, chi, 2 * j + 1 - u_in_pair, F.shift);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int b, gg, rr;
        avsy_yuv2bgr<SB>(F.m, avsy_lane<SB>(ylo, yhi, j, F.shift), U[j >> 1], V[j >> 1], b, gg, rr);
        px[3 * j] = (unsigned)b, px[3 * j + 1] = (unsigned)gg, px[3 * j + 2] = (unsigned)rr;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int p = 4 * g + 2 * k;
        const int y = p / F.w, x = p - y * F.w;   // (x is even)
        const uint8_t* ly = f + (long long)y * F.pitch_y + x * SB;
        int U, V;
        avsy_chroma<SB, PLANAR>(F, f, y >> 1, x >> 1, U, V);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          int b, gg, rr;
          avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(ly + j * SB, F.shift), U, V, b, gg, rr);
          px[6 * k + 3 * j] = (unsigned)b, px[6 * k + 3 * j + 1] = (unsigned)gg, px[6 * k + 3 * j + 2] = (unsigned)rr;
        }
      }
    }
    uint8_t* q = o + 12ll * g;
    if (vec) {
      unsigned* q4 = reinterpret_cast<unsigned*>(q);
#pragma unroll
      for (int d = 0; d < 3; ++d)
        q4[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
    } else {
#pragma unroll
      for (int d = 0; d < 12; ++d) q[d] = (uint8_t)px[d];
    }
  }
}

extern "C" int avsy_to_bgr_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix, const int64_t* d_index,
                              int64_t count, uint8_t* d_bgr, avsy_stream_t stream) {
  avsy_frames F;
  const int st = avsy_frames_arg("avsy_to_bgr_u8", F, d_src, h_surface, h_matrix);
  if (st != AVSY_OK) return st;
  AVSY_REQUIRE(count >= 0 && count <= 0x7fffffffll, AVSY_E_SHAPE, "avsy_to_bgr_u8: count=%lld", (long long)count);
  AVSY_REQUIRE(d_index || count <= F.n, AVSY_E_SHAPE, "avsy_to_bgr_u8: count %lld above the %lld frames (no index)",
               (long long)count, F.n);
  if (count == 0) return AVSY_OK;
  AVSY_REQUIRE(d_src && d_bgr, AVSY_E_ARG, "avsy_to_bgr_u8: null pointer");
  const long long groups = ((long long)F.h * F.w) >> 2;
  long long by = avs_cdiv(groups, NY_THREADS);
  if (by > 65535) by = 65535;
  NY_LAUNCH(F, yuv_to_bgr_kernel, dim3((unsigned)count, (unsigned)by), 0, stream, F,
            reinterpret_cast<const long long*>(d_index), d_bgr);
  AVSY_CHECK_LAUNCH("avsy_to_bgr_u8");
  return AVSY_OK;
}

// ---------------------------------------------------------------------------
// 2. cv2.resize(..., INTER_LINEAR) of gathered, converted frames.  The coefficients, the band's source rows, the column
// table and the blend are pixel_bodies.h's, the one text resize_gather2_kernel (stage1_batch.hip) and
// nv12_resize_gather2_kernel (ingest.hip) run too (those files belong to other libraries: shared inline text, no symbol).
// ---------------------------------------------------------------------------
struct ny_dest {
  uint8_t* dst;        // [count, dh, dw, 3]
  int dh, dw, band;    // band: output rows per workgroup
  int luma_rows;       // most luma rows a band reads
  int chroma_rows;     // most chroma lines a band reads (each one staged row of pairs, or a U row and a V row)
  double scale_y, scale_x;
};
struct ny_args {
  ny_dest d[2];
};

// LDS bytes of one staged row of `bytes` bytes: the row sits at its global address modulo 16
__host__ __device__ __forceinline__ int ny_row_bytes(int bytes) { return ((bytes + 15) & ~15) + 16; }
// the bytes of a staged luma row, and of a staged chroma row: the pairs of a line, or the samples of one plane's line
// with whatever lies between them
__host__ __device__ __forceinline__ int ny_luma_bytes(const avsy_frames& F) { return F.w * F.sample_bytes; }
__host__ __device__ __forceinline__ int ny_chroma_bytes(const avsy_frames& F) {
  return (F.w / 2 - 1) * F.step + (F.planar ? 1 : 2) * F.sample_bytes;
}

// grid (row of the index, band of output rows, destination).  A workgroup: (a) the column coefficients of its
// destination into LDS; (b) the luma rows y_lo .. y_hi and the chroma lines y_lo >> 1 .. y_hi >> 1 its band reads, with
// 16-byte loads; (c) one wave per output row, a lane per pixel: four taps, each converted from its luma sample and its
// chroma samples, then the blend; (d) the band's output rows - one contiguous byte range - out with 16-byte stores.
// Every LDS row and the output image sit at their global address modulo 16, so a two-byte sample stays 2-aligned in LDS.
template <int SB, bool PLANAR>
__global__ __launch_bounds__(NY_THREADS) void yuv_resize_gather2_kernel(avsy_frames F, const long long* __restrict__ index,
                                                                        ny_args args) {
  extern __shared__ __align__(16) uint8_t ny_lds[];
  constexpr int CR = PLANAR ? 2 : 1;   // staged rows per chroma line
  const ny_dest& D = args.d[blockIdx.z];
  const int dy_lo = blockIdx.y * D.band;
  if (dy_lo >= D.dh) return;
  const long long i = blockIdx.x;
  const long long r = index[i];
  if (r < 0 || r >= F.n) return;
  const int dy_hi = min(dy_lo + D.band, D.dh);
  const int dw = D.dw, sw = F.w, sh = F.h, row_out = dw * 3;
  const int lbytes = ny_luma_bytes(F), cbytes = ny_chroma_bytes(F);
  const int lrow = ny_row_bytes(lbytes), crow = ny_row_bytes(cbytes);

  uint2* coef = reinterpret_cast<uint2*>(ny_lds);                 // per column (x0 | x1 << 16, a0 | a1 << 16)
  uint8_t* luma = ny_lds + ((dw * 8 + 15) & ~15);
  uint8_t* chroma = luma + D.luma_rows * lrow;                    // line c, plane p at row c * CR + p
  uint8_t* out_base = chroma + D.chroma_rows * CR * crow;

  cv_coef_fill<NY_THREADS>(coef, dw, D.scale_x, sw);
  int y_lo, y_hi;
  cv_band_rows(dy_lo, dy_hi, D.scale_y, sh, y_lo, y_hi);
  const int c_lo = y_lo >> 1, c_hi = y_hi >> 1;
  const int nl = y_hi - y_lo + 1, nc = (c_hi - c_lo + 1) * CR;
  const uint8_t* f_luma = F.src + r * F.frame_stride;
  // where staged chroma row 0 (and, planar, 1) of a line begins: the pairs at the lower of the two offsets
  const uint8_t* f_c0 = f_luma + (PLANAR ? F.u_offset : min(F.u_offset, F.v_offset));
  const uint8_t* f_c1 = f_luma + F.v_offset;
  // (b) row k < nl is luma row y_lo + k, the others are the chroma rows; a row is cut at its 16-byte boundaries into
  // `slots` pieces - its 16-byte units, then the bytes before the first boundary, then the bytes after the last - and
  // the workgroup walks all pieces of all rows, NY_INFLIGHT 16-byte loads ahead of the first store
  const int slots = (max(lbytes, cbytes) >> 4) + 2, pieces = (nl + nc) * slots;
  auto chroma_global = [&](int k) {   // staged chroma row k of the band
    return (PLANAR && (k & 1) ? f_c1 : f_c0) + (long long)(c_lo + k / CR) * F.pitch_c;
  };
  // piece j: a 16-byte unit is loaded into `unit` and its LDS address returned; the bytes of a head or a tail are
  // copied at once (nullptr)
  auto piece = [&](int j, uint4& unit) -> uint4* {
    if (j >= pieces) return nullptr;
    const int k = j / slots, s = j - k * slots;
    const bool is_luma = k < nl;
    const int len = is_luma ? lbytes : cbytes;
    const uint8_t* g = is_luma ? f_luma + (long long)(y_lo + k) * F.pitch_y : chroma_global(k - nl);
    uint8_t* l = (is_luma ? luma + k * lrow : chroma + (k - nl) * crow) + ((unsigned)(uintptr_t)g & 15u);
    const int head = min(len, (int)((16u - (unsigned)(uintptr_t)g) & 15u));
    const int nvec = (len - head) >> 4;
    if (s < nvec) {
      unit = reinterpret_cast<const uint4*>(g + head)[s];
      return reinterpret_cast<uint4*>(l + head) + s;
    }
    if (s == slots - 2)
      for (int o = 0; o < head; ++o) l[o] = g[o];
    if (s == slots - 1)
      for (int o = head + (nvec << 4); o < len; ++o) l[o] = g[o];
    return nullptr;
  };
  for (int j = threadIdx.x; j < pieces; j += NY_INFLIGHT * NY_THREADS) {
    uint4 u0, u1, u2, u3;
    uint4* const t0 = piece(j, u0);
    uint4* const t1 = piece(j + NY_THREADS, u1);
    uint4* const t2 = piece(j + 2 * NY_THREADS, u2);
    uint4* const t3 = piece(j + 3 * NY_THREADS, u3);
    if (t0) *t0 = u0;
    if (t1) *t1 = u1;
    if (t2) *t2 = u2;
    if (t3) *t3 = u3;
  }
  uint8_t* g_out = D.dst + (i * D.dh + dy_lo) * (long long)row_out;
  uint8_t* out = out_base + ((unsigned)(uintptr_t)g_out & 15u);
  __syncthreads();

  // the U and the V pointer into the staged row(s) of chroma line c, each where its global address put it
  const int u_in_pair = PLANAR ? 0 : (int)(F.u_offset - min(F.u_offset, F.v_offset));
  const int v_in_pair = PLANAR ? 0 : (int)(F.v_offset - min(F.u_offset, F.v_offset));
  auto staged_chroma = [&](int c, const uint8_t*& pu, const uint8_t*& pv) {
    const int k = (c - c_lo) * CR;
    const uint8_t* row0 = chroma + k * crow + ((unsigned)(uintptr_t)chroma_global(k) & 15u);
    if (PLANAR) {
      pu = row0;
      pv = chroma + (k + 1) * crow + ((unsigned)(uintptr_t)chroma_global(k + 1) & 15u);
    } else {
      pu = row0 + u_in_pair, pv = row0 + v_in_pair;
    }
  };
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int dy = dy_lo + wave; dy < dy_hi; dy += NY_THREADS / 64) {
    int y0, y1, b0, b1;
    cv_linear_coef(dy, D.scale_y, sh, y0, y1, b0, b1);
    // the staged rows of the two source rows
    const uint8_t* l0 = luma + (y0 - y_lo) * lrow + ((unsigned)(uintptr_t)(f_luma + (long long)y0 * F.pitch_y) & 15u);
    const uint8_t* l1 = luma + (y1 - y_lo) * lrow + ((unsigned)(uintptr_t)(f_luma + (long long)y1 * F.pitch_y) & 15u);
    const uint8_t *u0r, *v0r, *u1r, *v1r;
    staged_chroma(y0 >> 1, u0r, v0r);
    staged_chroma(y1 >> 1, u1r, v1r);
    uint8_t* o = out + (dy - dy_lo) * row_out;
    for (int dx = lane; dx < dw; dx += 64) {
      int x0, x1, a0, a1;
      cv_coef_at(coef, dx, x0, x1, a0, a1);
      const int q0 = (x0 >> 1) * F.step, q1 = (x1 >> 1) * F.step;
      int p00[3], p01[3], p10[3], p11[3];
      avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(l0 + x0 * SB, F.shift), avsy_sample<SB>(u0r + q0, F.shift),
                       avsy_sample<SB>(v0r + q0, F.shift), p00[0], p00[1], p00[2]);
      avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(l0 + x1 * SB, F.shift), avsy_sample<SB>(u0r + q1, F.shift),
                       avsy_sample<SB>(v0r + q1, F.shift), p01[0], p01[1], p01[2]);
      avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(l1 + x0 * SB, F.shift), avsy_sample<SB>(u1r + q0, F.shift),
                       avsy_sample<SB>(v1r + q0, F.shift), p10[0], p10[1], p10[2]);
      avsy_yuv2bgr<SB>(F.m, avsy_sample<SB>(l1 + x1 * SB, F.shift), avsy_sample<SB>(u1r + q1, F.shift),
                       avsy_sample<SB>(v1r + q1, F.shift), p11[0], p11[1], p11[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[dx * 3 + c] = cv_blend(p00[c], p01[c], p10[c], p11[c], a0, a1, b0, b1);
    }
  }
  __syncthreads();
  stage_out<NY_THREADS>(g_out, out, (dy_hi - dy_lo) * row_out);
}

// the band and the LDS rows of one destination: the most luma rows and the most chroma lines any band of `band` output
// rows reads, by the kernel's own arithmetic, each row at its real byte length (a two-byte row is twice as long, a
// planar chroma line is two rows of half the samples).  Returns the total LDS bytes (coefficients + staged rows +
// output rows), 0 when even a band of one output row does not fit.
static size_t ny_plan(ny_dest& D, const avsy_frames& F) {
  const int cr = F.planar ? 2 : 1;
  for (int band = AVSY_RESIZE_BAND; band >= 1; band >>= 1) {
    int nl = 1, nc = 1;
    for (int lo = 0; lo < D.dh; lo += band) {
      int y_lo, y_hi;
      cv_band_rows(lo, lo + band < D.dh ? lo + band : D.dh, D.scale_y, F.h, y_lo, y_hi);
      if (y_hi - y_lo + 1 > nl) nl = y_hi - y_lo + 1;
      if ((y_hi >> 1) - (y_lo >> 1) + 1 > nc) nc = (y_hi >> 1) - (y_lo >> 1) + 1;
    }
    const size_t in_bytes = (size_t)nl * ny_row_bytes(ny_luma_bytes(F)) + (size_t)nc * cr * ny_row_bytes(ny_chroma_bytes(F));
    const size_t out_bytes = ((size_t)band * D.dw * 3 + 16 + 15) & ~(size_t)15;
    const size_t total = (((size_t)D.dw * 8 + 15) & ~(size_t)15) + in_bytes + out_bytes;
    if (total <= AVSY_RESIZE_LDS_BYTES) {
      D.band = band;
      D.luma_rows = nl;
      D.chroma_rows = nc;
      return total;
    }
  }
  return 0;
}

static ny_dest ny_make_dest(uint8_t* dst, int sh, int sw, int dh, int dw) {
  // OpenCV: inv_scale = dsize/ssize (double); scale = 1/inv_scale.
  return ny_dest{dst, dh, dw, 1, 0, 0, 1.0 / ((double)dh / (double)sh), 1.0 / ((double)dw / (double)sw)};
}

// the resize's own limits on a description the shared checks passed: the column table holds source columns in 16 bits,
// and a staged chroma row's length is an int the plan multiplies
static bool ny_resize_takes(const avsy_frames& F) {
  return F.w <= 65535 && (long long)(F.w / 2 - 1) * F.step + 2 * F.sample_bytes <= AVSY_RESIZE_LDS_BYTES;
}

extern "C" int avsy_resize_band(const int64_t* h_surface, int dh, int dw) {
  const int no_matrix[AVSY_MATRIX_INTS] = {0, 0, 0, 0, 0, 0};   // (the plan does not depend on the conversion)
  avsy_frames F;
  const int st = avsy_frames_arg("avsy_resize_band", F, nullptr, h_surface, no_matrix);
  if (st != AVSY_OK) return st;
  AVSY_REQUIRE(dh > 0 && dw > 0, AVSY_E_SHAPE, "avsy_resize_band: size %dx%d", dh, dw);
  if (!ny_resize_takes(F) || dh > 65535) return 0;
  ny_dest D = ny_make_dest(nullptr, F.h, F.w, dh, dw);
  return ny_plan(D, F) > 0 ? D.band : 0;
}

extern "C" int avsy_resize_gather2_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix,
                                      const int64_t* d_index, int64_t count, uint8_t* d_dst0, int dh0, int dw0,
                                      uint8_t* d_dst1, int dh1, int dw1, avsy_stream_t stream) {
  avsy_frames F;
  const int st = avsy_frames_arg("avsy_resize_gather2_u8", F, d_src, h_surface, h_matrix);
  if (st != AVSY_OK) return st;
  AVSY_REQUIRE(dh0 > 0 && dw0 > 0 && count >= 0 && count <= 0x7fffffffll && (!d_dst1 || (dh1 > 0 && dw1 > 0)), AVSY_E_SHAPE,
               "avsy_resize_gather2_u8: count=%lld sizes %dx%d %dx%d", (long long)count, dh0, dw0, dh1, dw1);
  // the column table holds source columns in 16 bits; the bands are on grid y
  AVSY_REQUIRE(F.w <= 65535 && dh0 <= 65535 && (!d_dst1 || dh1 <= 65535), AVSY_E_UNSUPPORTED,
               "avsy_resize_gather2_u8: more than 65535 source columns or output rows");
  AVSY_REQUIRE(ny_resize_takes(F), AVSY_E_UNSUPPORTED,
               "avsy_resize_gather2_u8: a chroma row of %d samples %d bytes apart does not fit %d bytes of LDS", F.w / 2, F.step,
               AVSY_RESIZE_LDS_BYTES);
  if (count == 0) return AVSY_OK;
  AVSY_REQUIRE(d_src && d_index && d_dst0, AVSY_E_ARG, "avsy_resize_gather2_u8: null pointer");
  ny_args args;
  const int ndst = d_dst1 ? 2 : 1;
  const int dh[2] = {dh0, dh1}, dw[2] = {dw0, dw1};
  uint8_t* const dst[2] = {d_dst0, d_dst1};
  size_t lds = 0;
  int bands = 0;
  for (int k = 0; k < ndst; ++k) {
    ny_dest& D = args.d[k];
    D = ny_make_dest(dst[k], F.h, F.w, dh[k], dw[k]);
    const size_t need = ny_plan(D, F);
    AVSY_REQUIRE(need > 0, AVSY_E_UNSUPPORTED,
                 "avsy_resize_gather2_u8: the luma and chroma rows of one output row of %d pixels from rows of %d samples of "
                 "%d bytes do not fit %d bytes of LDS", D.dw, F.w, F.sample_bytes, AVSY_RESIZE_LDS_BYTES);
    if (need > lds) lds = need;
    const int nb = (int)avs_cdiv(D.dh, D.band);
    if (nb > bands) bands = nb;
  }
  if (ndst == 1) args.d[1] = args.d[0];   // (never read: grid z is 1)
  NY_LAUNCH(F, yuv_resize_gather2_kernel, dim3((unsigned)count, (unsigned)bands, (unsigned)ndst), lds, stream, F,
            reinterpret_cast<const long long*>(d_index), args);
  AVSY_CHECK_LAUNCH("avsy_resize_gather2_u8");
  return AVSY_OK;
}

// ---------------------------------------------------------------------------
// 3. |dH|, |dS|, |dV| sums of every frame against the previous frame of its video: hsv_diff_body (pixel_bodies.h), the
// one text hsv_frame_diff_batch_kernel (shots_batch.hip) runs too - the frame on grid x, a frame's strided pixels split
// over grid y, the first frame of every video left at the memset's zeros - with both pixels converted on the way in.
// ---------------------------------------------------------------------------
template <int SB, bool PLANAR>
struct ny_yuv_src {   // hsv_diff_body's pixel source: a luma sample and the nearest chroma samples, converted
  const avsy_frames& F;
  __device__ __forceinline__ void bgr(const uint8_t* frame, int y, int x, int& b, int& g, int& r) const {
    avsy_pixel<SB, PLANAR>(F, frame, y, x, b, g, r);
  }
};

template <int SB, bool PLANAR>
__global__ __launch_bounds__(NY_THREADS) void yuv_hsv_diff_batch_kernel(avsy_frames F, int step, int ph, int pw,
                                                                        const long long* __restrict__ offsets, int nvideos,
                                                                        unsigned* __restrict__ sums) {
  const long long f = (long long)blockIdx.x + 1;  // frame f against frame f-1
  // the video of f: the last v with offsets[v] <= f (block-uniform)
  int lo = 0, hi = nvideos;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= f)
      lo = mid;
    else
      hi = mid;
  }
  if (offsets[lo] == f) return;  // a video's first frame: no predecessor, the memset's zeros stay
  const uint8_t* cur = F.src + f * F.frame_stride;
  const uint8_t* prv = cur - F.frame_stride;
  hsv_diff_body<NY_THREADS>(ny_yuv_src<SB, PLANAR>{F}, cur, prv, step, ph, pw, blockIdx.y, gridDim.y, sums + f * 3);
}

extern "C" int avsy_hsv_diff_batch_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix, int step,
                                      const int64_t* d_offsets, int nvideos, uint32_t* d_sums, avsy_stream_t stream) {
  avsy_frames F;
  const int st = avsy_frames_arg("avsy_hsv_diff_batch_u8", F, d_src, h_surface, h_matrix);
  if (st != AVSY_OK) return st;
  const long long n = F.n;
  AVSY_REQUIRE(step > 0 && nvideos >= 0, AVSY_E_SHAPE, "avsy_hsv_diff_batch_u8: step=%d nvideos=%d", step, nvideos);
  AVSY_REQUIRE(n <= AVSY_MAX_DIFF_FRAMES, AVSY_E_SHAPE, "avsy_hsv_diff_batch_u8: at most %d frames per call, got %lld",
               AVSY_MAX_DIFF_FRAMES, n);
  if (n == 0) return AVSY_OK;
  AVSY_REQUIRE(nvideos > 0, AVSY_E_SHAPE, "avsy_hsv_diff_batch_u8: %lld frames in no video", n);
  AVSY_REQUIRE(d_src && d_offsets && d_sums, AVSY_E_ARG, "avsy_hsv_diff_batch_u8: null pointer");
  const int ph = (F.h + step - 1) / step, pw = (F.w + step - 1) / step;  // len(range(0, h, step))
  AVSY_REQUIRE((long long)ph * pw * 255 < (1ll << 32), AVSY_E_SHAPE, "avsy_hsv_diff_batch_u8: frame too large for u32 sums");
  hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * 3 * (size_t)n, (hipStream_t)stream);
  if (e != hipSuccess) {
    avsy_set_error("avsy_hsv_diff_batch_u8: memset failed: %s", hipGetErrorString(e));
    return AVSY_E_HIP;
  }
  if (n == 1) return AVSY_OK;
  int by = (int)avs_cdiv((long long)ph * pw, NY_THREADS * 8);  // the BGR scan's split of a frame
  if (by < 1) by = 1;
  if (by > 64) by = 64;
  NY_LAUNCH(F, yuv_hsv_diff_batch_kernel, dim3((unsigned)(n - 1), by), 0, stream, F, step, ph, pw,
            reinterpret_cast<const long long*>(d_offsets), nvideos, d_sums);
  AVSY_CHECK_LAUNCH("avsy_hsv_diff_batch_u8");
  return AVSY_OK;
}
