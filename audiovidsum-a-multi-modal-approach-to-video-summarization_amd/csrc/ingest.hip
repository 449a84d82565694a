// libavsum_ingest.so: NV12 frames read where they lie (include/avsum_ingest.h).  This file is the whole library.  It
// includes avs_internal.h and pixel_bodies.h for their inline helpers only (bgr2hsv_u8, the one definition of the HSV
// pixel arithmetic; the one text of the bilinear resize and of the shot scan) and references no symbol of
// libavsum_hip.so: the error text, the argument checks and the launch check below are its own.
//
// Three kernels, one pixel definition (avsi_yuv2bgr, 32-bit integers throughout):
//   nv12_to_bgr_kernel          four pixels - two chroma pairs - per thread, 12 output bytes
//   nv12_resize_gather2_kernel  resize_gather2_kernel (stage1_batch.hip) with the band's luma and chroma rows staged into
//                               LDS instead of its BGR rows, converted per tap: pixel_bodies.h's 11-bit bilinear arithmetic
//   nv12_hsv_diff_batch_kernel  hsv_frame_diff_batch_kernel (shots_batch.hip) with the two pixels converted on the way
//                               in: pixel_bodies.h's scan with an NV12 pixel source
// Integers and fixed orders: two calls give the same bytes.
#include <stdarg.h>
#include "avs_internal.h"
#include "pixel_bodies.h"
#include "../../include/avsum_ingest.h"

#define NI_THREADS 256
#define NI_MAX_GRID_X (0xffffffffll / NI_THREADS)   // a launch holds at most 2^32 - 1 threads per grid dimension
#define NI_INFLIGHT 4                               // 16-byte loads a thread keeps in flight while staging rows
static_assert(NI_MAX_GRID_X + 1 == AVSI_MAX_DIFF_FRAMES, "the frame of the scan is on grid x");
static_assert(511ll * AVSI_MAX_COEF + (1 << (AVSI_SHIFT - 1)) < (1ll << 31), "the largest accumulator fits int32");

static thread_local char g_err[512] = "";

static void avsi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSI_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsi_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSI_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsi_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSI_E_HIP;                                                         \
    }                                                                            \
  } while (0)

extern "C" int avsi_abi_version(void) { return AVSI_ABI_VERSION; }
extern "C" const char* avsi_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// The frames of a call and the pixel definition.
// ---------------------------------------------------------------------------
struct avsi_mat {
  int y_off, cy, cub, cug, cvg, cvr;
};
struct avsi_frames {
  const uint8_t* src;
  long long n, frame_stride, uv_offset;
  int h, w, pitch;
  avsi_mat m;
};

__device__ __forceinline__ int avsi_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void avsi_yuv2bgr(const avsi_mat& m, int Y, int U, int V, int& b, int& g, int& r) {
  const int yy = max(Y - m.y_off, 0) * m.cy + (1 << (AVSI_SHIFT - 1));
  const int uu = U - 128, vv = V - 128;
  b = avsi_clamp8((yy + m.cub * uu) >> AVSI_SHIFT);
  g = avsi_clamp8((yy + m.cvg * vv + m.cug * uu) >> AVSI_SHIFT);
  r = avsi_clamp8((yy + m.cvr * vv) >> AVSI_SHIFT);
}

// pixel (y, x) of frame `f`, converted
__device__ __forceinline__ void avsi_pixel(const avsi_frames& F, const uint8_t* f, int y, int x, int& b, int& g, int& r) {
  const uint8_t* c = f + F.uv_offset + (long long)(y >> 1) * F.pitch + (x & ~1);
  avsi_yuv2bgr(F.m, f[(long long)y * F.pitch + x], c[0], c[1], b, g, r);
}

// the checks every entry point shares; fills F
static int avsi_frames_arg(const char* what, avsi_frames& F, const uint8_t* d_src, int64_t n, int h, int w, int pitch,
                           int64_t frame_stride, int64_t uv_offset, const int* h_matrix) {
  AVSI_REQUIRE(n >= 0, AVSI_E_SHAPE, "%s: n=%lld frames", what, (long long)n);
  AVSI_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, AVSI_E_SHAPE,
               "%s: NV12 frames have even extents of at least 2, got %dx%d", what, h, w);
  AVSI_REQUIRE((long long)h * w * 3 < (1ll << 31), AVSI_E_SHAPE, "%s: a frame of %dx%d is too large", what, h, w);
  AVSI_REQUIRE(pitch >= w, AVSI_E_SHAPE, "%s: pitch %d below the width %d", what, pitch, w);
  AVSI_REQUIRE(uv_offset >= (long long)h * pitch, AVSI_E_SHAPE,
               "%s: uv_offset %lld lies inside the luma plane of %d rows of %d bytes", what, (long long)uv_offset, h, pitch);
  AVSI_REQUIRE(frame_stride >= uv_offset + (long long)(h / 2 - 1) * pitch + w, AVSI_E_SHAPE,
               "%s: frame_stride %lld ends before the chroma plane does (%lld)", what, (long long)frame_stride,
               (long long)(uv_offset + (long long)(h / 2 - 1) * pitch + w));
  AVSI_REQUIRE(h_matrix, AVSI_E_ARG, "%s: h_matrix is null", what);
  AVSI_REQUIRE(h_matrix[0] >= 0 && h_matrix[0] <= 255, AVSI_E_ARG, "%s: y_off %d outside 0 .. 255", what, h_matrix[0]);
  for (int k = 1; k < AVSI_MATRIX_INTS; ++k)
    AVSI_REQUIRE(h_matrix[k] >= -AVSI_MAX_COEF && h_matrix[k] <= AVSI_MAX_COEF, AVSI_E_ARG,
                 "%s: coefficient %d of the matrix is %d, above 2^22 in magnitude", what, k, h_matrix[k]);
  F.src = d_src;
  F.n = n, F.frame_stride = frame_stride, F.uv_offset = uv_offset;
  F.h = h, F.w = w, F.pitch = pitch;
  F.m = avsi_mat{h_matrix[0], h_matrix[1], h_matrix[2], h_matrix[3], h_matrix[4], h_matrix[5]};
  return AVSI_OK;
}

// ---------------------------------------------------------------------------
// 1. Dense BGR.  The h * w pixels of a frame in output order, four to a thread: w is even, so pixels 4g, 4g + 1 share
// a row and a chroma pair, and so do 4g + 2, 4g + 3.  A frame's output begins a multiple of 12 bytes after d_bgr, so
// the 12 bytes of a thread leave as three dwords where d_bgr is 4-byte aligned and singly where it is not.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NI_THREADS) void nv12_to_bgr_kernel(avsi_frames F, const long long* __restrict__ index,
                                                                 uint8_t* __restrict__ dst) {
  const long long i = blockIdx.x;
  const long long r = index ? index[i] : i;
  if (r < 0 || r >= F.n) return;
  const uint8_t* f = F.src + r * F.frame_stride;
  uint8_t* o = dst + i * ((long long)F.h * F.w * 3);
  const bool vec = ((unsigned)(uintptr_t)o & 3u) == 0;
  const int groups = (F.h * F.w) >> 2;
  for (int g = blockIdx.y * NI_THREADS + threadIdx.x; g < groups; g += gridDim.y * NI_THREADS) {
    unsigned px[12];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int p = 4 * g + 2 * k;
      const int y = p / F.w, x = p - y * F.w;
      const uint8_t* ly = f + (long long)y * F.pitch + x;
      const uint8_t* c = f + F.uv_offset + (long long)(y >> 1) * F.pitch + x;   // (x is even)
      const int U = c[0], V = c[1];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int b, gg, rr;
        avsi_yuv2bgr(F.m, ly[j], U, V, b, gg, rr);
        px[6 * k + 3 * j] = (unsigned)b, px[6 * k + 3 * j + 1] = (unsigned)gg, px[6 * k + 3 * j + 2] = (unsigned)rr;
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

extern "C" int avsi_nv12_to_bgr_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                                   int64_t uv_offset, const int* h_matrix, const int64_t* d_index, int64_t count,
                                   uint8_t* d_bgr, avsi_stream_t stream) {
  avsi_frames F;
  const int st = avsi_frames_arg("avsi_nv12_to_bgr_u8", F, d_src, n, h, w, pitch, frame_stride, uv_offset, h_matrix);
  if (st != AVSI_OK) return st;
  AVSI_REQUIRE(count >= 0 && count <= 0x7fffffffll, AVSI_E_SHAPE, "avsi_nv12_to_bgr_u8: count=%lld", (long long)count);
  AVSI_REQUIRE(d_index || count <= n, AVSI_E_SHAPE, "avsi_nv12_to_bgr_u8: count %lld above the %lld frames (no index)",
               (long long)count, (long long)n);
  if (count == 0) return AVSI_OK;
  AVSI_REQUIRE(d_src && d_bgr, AVSI_E_ARG, "avsi_nv12_to_bgr_u8: null pointer");
  const long long groups = ((long long)h * w) >> 2;
  long long by = avs_cdiv(groups, NI_THREADS);
  if (by > 65535) by = 65535;
  hipLaunchKernelGGL(nv12_to_bgr_kernel, dim3((unsigned)count, (unsigned)by), dim3(NI_THREADS), 0, (hipStream_t)stream, F,
                     reinterpret_cast<const long long*>(d_index), d_bgr);
  AVSI_CHECK_LAUNCH("avsi_nv12_to_bgr_u8");
  return AVSI_OK;
}

// ---------------------------------------------------------------------------
// 2. cv2.resize(..., INTER_LINEAR) of gathered, converted frames.  The coefficients, the band's source rows, the column
// table and the blend are pixel_bodies.h's, the one text resize_gather2_kernel (stage1_batch.hip) runs too (that file
// belongs to the other library: the two share inline text, no symbol).
// ---------------------------------------------------------------------------
struct ni_dest {
  uint8_t* dst;        // [count, dh, dw, 3]
  int dh, dw, band;    // band: output rows per workgroup
  int luma_rows;       // most luma rows a band reads (the chroma rows follow them in LDS)
  int rows;            // most luma rows + most chroma rows
  double scale_y, scale_x;
};
struct ni_args {
  ni_dest d[2];
};

// LDS bytes of one staged row of w bytes: the row sits at its global address modulo 16
__host__ __device__ __forceinline__ int ni_row_bytes(int w) { return ((w + 15) & ~15) + 16; }

// grid (row of the index, band of output rows, destination).  A workgroup: (a) the column coefficients of its
// destination into LDS; (b) the luma rows y_lo .. y_hi and the chroma rows y_lo >> 1 .. y_hi >> 1 its band reads, w
// bytes each, with 16-byte loads; (c) one wave per output row, a lane per pixel: four taps, each converted from its
// luma byte and its chroma pair, then the blend; (d) the band's output rows - one contiguous byte range - out with
// 16-byte stores.  Every LDS row and the output image sit at their global address modulo 16.
__global__ __launch_bounds__(NI_THREADS) void nv12_resize_gather2_kernel(avsi_frames F, const long long* __restrict__ index,
                                                                         ni_args args) {
  extern __shared__ __align__(16) uint8_t ni_lds[];
  const ni_dest& D = args.d[blockIdx.z];
  const int dy_lo = blockIdx.y * D.band;
  if (dy_lo >= D.dh) return;
  const long long i = blockIdx.x;
  const long long r = index[i];
  if (r < 0 || r >= F.n) return;
  const int dy_hi = min(dy_lo + D.band, D.dh);
  const int dw = D.dw, sw = F.w, sh = F.h, row_out = dw * 3, lrow = ni_row_bytes(sw);

  uint2* coef = reinterpret_cast<uint2*>(ni_lds);                 // per column (x0 | x1 << 16, a0 | a1 << 16)
  uint8_t* luma = ni_lds + ((dw * 8 + 15) & ~15);
  uint8_t* chroma = luma + D.luma_rows * lrow;
  uint8_t* out_base = luma + D.rows * lrow;

  cv_coef_fill<NI_THREADS>(coef, dw, D.scale_x, sw);
  int y_lo, y_hi;
  cv_band_rows(dy_lo, dy_hi, D.scale_y, sh, y_lo, y_hi);
  const int c_lo = y_lo >> 1, c_hi = y_hi >> 1;
  const int nl = y_hi - y_lo + 1, nc = c_hi - c_lo + 1;
  const uint8_t* f_luma = F.src + r * F.frame_stride;
  const uint8_t* f_chroma = f_luma + F.uv_offset;
  // (b) row k < nl is luma row y_lo + k, the others are the chroma rows; a row is cut at its 16-byte boundaries into
  // `slots` pieces - its 16-byte units (sw >> 4 at the most), then the bytes before the first boundary, then the bytes
  // after the last - and the workgroup walks all pieces of all rows, NI_INFLIGHT 16-byte loads ahead of the first store
  const int slots = (sw >> 4) + 2, pieces = (nl + nc) * slots;
  // piece j: a 16-byte unit is loaded into `unit` and its LDS address returned; the bytes of a head or a tail are
  // copied at once (nullptr)
  auto piece = [&](int j, uint4& unit) -> uint4* {
    if (j >= pieces) return nullptr;
    const int k = j / slots, s = j - k * slots;
    const bool is_luma = k < nl;
    const uint8_t* g = is_luma ? f_luma + (long long)(y_lo + k) * F.pitch : f_chroma + (long long)(c_lo + k - nl) * F.pitch;
    uint8_t* l = (is_luma ? luma + k * lrow : chroma + (k - nl) * lrow) + ((unsigned)(uintptr_t)g & 15u);
    const int head = min(sw, (int)((16u - (unsigned)(uintptr_t)g) & 15u));
    const int nvec = (sw - head) >> 4;
    if (s < nvec) {
      unit = reinterpret_cast<const uint4*>(g + head)[s];
      return reinterpret_cast<uint4*>(l + head) + s;
    }
    if (s == slots - 2)
      for (int o = 0; o < head; ++o) l[o] = g[o];
    if (s == slots - 1)
      for (int o = head + (nvec << 4); o < sw; ++o) l[o] = g[o];
    return nullptr;
  };
  for (int j = threadIdx.x; j < pieces; j += NI_INFLIGHT * NI_THREADS) {
    uint4 u0, u1, u2, u3;
    uint4* const t0 = piece(j, u0);
    uint4* const t1 = piece(j + NI_THREADS, u1);
    uint4* const t2 = piece(j + 2 * NI_THREADS, u2);
    uint4* const t3 = piece(j + 3 * NI_THREADS, u3);
    if (t0) *t0 = u0;
    if (t1) *t1 = u1;
    if (t2) *t2 = u2;
    if (t3) *t3 = u3;
  }
  uint8_t* g_out = D.dst + (i * D.dh + dy_lo) * (long long)row_out;
  uint8_t* out = out_base + ((unsigned)(uintptr_t)g_out & 15u);
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int dy = dy_lo + wave; dy < dy_hi; dy += NI_THREADS / 64) {
    int y0, y1, b0, b1;
    cv_linear_coef(dy, D.scale_y, sh, y0, y1, b0, b1);
    // the staged rows of the two source rows, each where its global address put it
    const uint8_t* l0 = luma + (y0 - y_lo) * lrow + ((unsigned)(uintptr_t)(f_luma + (long long)y0 * F.pitch) & 15u);
    const uint8_t* l1 = luma + (y1 - y_lo) * lrow + ((unsigned)(uintptr_t)(f_luma + (long long)y1 * F.pitch) & 15u);
    const uint8_t* c0 = chroma + ((y0 >> 1) - c_lo) * lrow + ((unsigned)(uintptr_t)(f_chroma + (long long)(y0 >> 1) * F.pitch) & 15u);
    const uint8_t* c1 = chroma + ((y1 >> 1) - c_lo) * lrow + ((unsigned)(uintptr_t)(f_chroma + (long long)(y1 >> 1) * F.pitch) & 15u);
    uint8_t* o = out + (dy - dy_lo) * row_out;
    for (int dx = lane; dx < dw; dx += 64) {
      int x0, x1, a0, a1;
      cv_coef_at(coef, dx, x0, x1, a0, a1);
      const int u0 = x0 & ~1, u1 = x1 & ~1;
      // a chroma pair through one pointer: its second byte is then the first one's address with an offset of 1,
      // whatever the compiler makes of an even index plus 1
      const uint8_t *q00 = c0 + u0, *q01 = c0 + u1, *q10 = c1 + u0, *q11 = c1 + u1;
      int p00[3], p01[3], p10[3], p11[3];
      avsi_yuv2bgr(F.m, l0[x0], q00[0], q00[1], p00[0], p00[1], p00[2]);
      avsi_yuv2bgr(F.m, l0[x1], q01[0], q01[1], p01[0], p01[1], p01[2]);
      avsi_yuv2bgr(F.m, l1[x0], q10[0], q10[1], p10[0], p10[1], p10[2]);
      avsi_yuv2bgr(F.m, l1[x1], q11[0], q11[1], p11[0], p11[1], p11[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[dx * 3 + c] = cv_blend(p00[c], p01[c], p10[c], p11[c], a0, a1, b0, b1);
    }
  }
  __syncthreads();
  stage_out<NI_THREADS>(g_out, out, (dy_hi - dy_lo) * row_out);
}

// the band and the LDS rows of one destination: the most luma rows and the most chroma rows any band of `band` output
// rows reads, by the kernel's own arithmetic.  Returns the total LDS bytes (coefficients + staged rows + output rows),
// 0 when even a band of one output row does not fit.
static size_t ni_plan(ni_dest& D, int sh, int sw) {
  for (int band = AVSI_RESIZE_BAND; band >= 1; band >>= 1) {
    int nl = 1, nc = 1;
    for (int lo = 0; lo < D.dh; lo += band) {
      int y_lo, y_hi;
      cv_band_rows(lo, lo + band < D.dh ? lo + band : D.dh, D.scale_y, sh, y_lo, y_hi);
      if (y_hi - y_lo + 1 > nl) nl = y_hi - y_lo + 1;
      if ((y_hi >> 1) - (y_lo >> 1) + 1 > nc) nc = (y_hi >> 1) - (y_lo >> 1) + 1;
    }
    const size_t in_bytes = (size_t)(nl + nc) * ni_row_bytes(sw);
    const size_t out_bytes = ((size_t)band * D.dw * 3 + 16 + 15) & ~(size_t)15;
    const size_t total = (((size_t)D.dw * 8 + 15) & ~(size_t)15) + in_bytes + out_bytes;
    if (total <= AVSI_RESIZE_LDS_BYTES) {
      D.band = band;
      D.luma_rows = nl;
      D.rows = nl + nc;
      return total;
    }
  }
  return 0;
}

static ni_dest ni_make_dest(uint8_t* dst, int sh, int sw, int dh, int dw) {
  // OpenCV: inv_scale = dsize/ssize (double); scale = 1/inv_scale.
  return ni_dest{dst, dh, dw, 1, 0, 0, 1.0 / ((double)dh / (double)sh), 1.0 / ((double)dw / (double)sw)};
}

extern "C" int avsi_nv12_resize_band(int h, int w, int dh, int dw) {
  AVSI_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && dh > 0 && dw > 0, AVSI_E_SHAPE,
               "avsi_nv12_resize_band: source %dx%d size %dx%d", h, w, dh, dw);
  if (w > 65535 || dh > 65535) return 0;
  ni_dest D = ni_make_dest(nullptr, h, w, dh, dw);
  return ni_plan(D, h, w) > 0 ? D.band : 0;
}

extern "C" int avsi_nv12_resize_gather2_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                                           int64_t uv_offset, const int* h_matrix, const int64_t* d_index, int64_t count,
                                           uint8_t* d_dst0, int dh0, int dw0, uint8_t* d_dst1, int dh1, int dw1,
                                           avsi_stream_t stream) {
  avsi_frames F;
  const int st = avsi_frames_arg("avsi_nv12_resize_gather2_u8", F, d_src, n, h, w, pitch, frame_stride, uv_offset, h_matrix);
  if (st != AVSI_OK) return st;
  AVSI_REQUIRE(dh0 > 0 && dw0 > 0 && count >= 0 && count <= 0x7fffffffll && (!d_dst1 || (dh1 > 0 && dw1 > 0)), AVSI_E_SHAPE,
               "avsi_nv12_resize_gather2_u8: count=%lld sizes %dx%d %dx%d", (long long)count, dh0, dw0, dh1, dw1);
  // the column table holds source columns in 16 bits; the bands are on grid y
  AVSI_REQUIRE(w <= 65535 && dh0 <= 65535 && (!d_dst1 || dh1 <= 65535), AVSI_E_UNSUPPORTED,
               "avsi_nv12_resize_gather2_u8: more than 65535 source columns or output rows");
  if (count == 0) return AVSI_OK;
  AVSI_REQUIRE(d_src && d_index && d_dst0, AVSI_E_ARG, "avsi_nv12_resize_gather2_u8: null pointer");
  ni_args args;
  const int ndst = d_dst1 ? 2 : 1;
  const int dh[2] = {dh0, dh1}, dw[2] = {dw0, dw1};
  uint8_t* const dst[2] = {d_dst0, d_dst1};
  size_t lds = 0;
  int bands = 0;
  for (int k = 0; k < ndst; ++k) {
    ni_dest& D = args.d[k];
    D = ni_make_dest(dst[k], h, w, dh[k], dw[k]);
    const size_t need = ni_plan(D, h, w);
    AVSI_REQUIRE(need > 0, AVSI_E_UNSUPPORTED,
                 "avsi_nv12_resize_gather2_u8: the luma and chroma rows of one output row of %d pixels from rows of %d do "
                 "not fit %d bytes of LDS", D.dw, w, AVSI_RESIZE_LDS_BYTES);
    if (need > lds) lds = need;
    const int nb = (int)avs_cdiv(D.dh, D.band);
    if (nb > bands) bands = nb;
  }
  if (ndst == 1) args.d[1] = args.d[0];   // (never read: grid z is 1)
  hipLaunchKernelGGL(nv12_resize_gather2_kernel, dim3((unsigned)count, (unsigned)bands, (unsigned)ndst), dim3(NI_THREADS),
                     lds, (hipStream_t)stream, F, reinterpret_cast<const long long*>(d_index), args);
  AVSI_CHECK_LAUNCH("avsi_nv12_resize_gather2_u8");
  return AVSI_OK;
}

// ---------------------------------------------------------------------------
// 3. |dH|, |dS|, |dV| sums of every frame against the previous frame of its video: hsv_diff_body (pixel_bodies.h), the
// one text hsv_frame_diff_batch_kernel (shots_batch.hip) runs too - the frame on grid x, a frame's strided pixels split
// over grid y, the first frame of every video left at the memset's zeros - with both pixels converted from NV12 on the
// way in.
// ---------------------------------------------------------------------------
struct ni_nv12_src {   // hsv_diff_body's pixel source: a luma byte and a chroma pair, converted
  const avsi_frames& F;
  __device__ __forceinline__ void bgr(const uint8_t* frame, int y, int x, int& b, int& g, int& r) const {
    avsi_pixel(F, frame, y, x, b, g, r);
  }
};

__global__ __launch_bounds__(NI_THREADS) void nv12_hsv_diff_batch_kernel(avsi_frames F, int step, int ph, int pw,
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
  hsv_diff_body<NI_THREADS>(ni_nv12_src{F}, cur, prv, step, ph, pw, blockIdx.y, gridDim.y, sums + f * 3);
}

extern "C" int avsi_nv12_hsv_diff_batch_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                                           int64_t uv_offset, const int* h_matrix, int step, const int64_t* d_offsets,
                                           int nvideos, uint32_t* d_sums, avsi_stream_t stream) {
  avsi_frames F;
  const int st = avsi_frames_arg("avsi_nv12_hsv_diff_batch_u8", F, d_src, n, h, w, pitch, frame_stride, uv_offset, h_matrix);
  if (st != AVSI_OK) return st;
  AVSI_REQUIRE(step > 0 && nvideos >= 0, AVSI_E_SHAPE, "avsi_nv12_hsv_diff_batch_u8: step=%d nvideos=%d", step, nvideos);
  AVSI_REQUIRE(n <= AVSI_MAX_DIFF_FRAMES, AVSI_E_SHAPE, "avsi_nv12_hsv_diff_batch_u8: at most %d frames per call, got %lld",
               AVSI_MAX_DIFF_FRAMES, (long long)n);
  if (n == 0) return AVSI_OK;
  AVSI_REQUIRE(nvideos > 0, AVSI_E_SHAPE, "avsi_nv12_hsv_diff_batch_u8: %lld frames in no video", (long long)n);
  AVSI_REQUIRE(d_src && d_offsets && d_sums, AVSI_E_ARG, "avsi_nv12_hsv_diff_batch_u8: null pointer");
  const int ph = (h + step - 1) / step, pw = (w + step - 1) / step;  // len(range(0, h, step))
  AVSI_REQUIRE((long long)ph * pw * 255 < (1ll << 32), AVSI_E_SHAPE,
               "avsi_nv12_hsv_diff_batch_u8: frame too large for u32 sums");
  hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * 3 * (size_t)n, (hipStream_t)stream);
  if (e != hipSuccess) {
    avsi_set_error("avsi_nv12_hsv_diff_batch_u8: memset failed: %s", hipGetErrorString(e));
    return AVSI_E_HIP;
  }
  if (n == 1) return AVSI_OK;
  int by = (int)avs_cdiv((long long)ph * pw, NI_THREADS * 8);  // the BGR scan's split of a frame
  if (by < 1) by = 1;
  if (by > 64) by = 64;
  hipLaunchKernelGGL(nv12_hsv_diff_batch_kernel, dim3((unsigned)(n - 1), by), dim3(NI_THREADS), 0, (hipStream_t)stream, F,
                     step, ph, pw, reinterpret_cast<const long long*>(d_offsets), nvideos, d_sums);
  AVSI_CHECK_LAUNCH("avsi_nv12_hsv_diff_batch_u8");
  return AVSI_OK;
}
