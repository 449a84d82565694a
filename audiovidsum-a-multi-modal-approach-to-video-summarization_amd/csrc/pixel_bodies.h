// The arithmetic of the uint8 pixel kernels, one text for every kernel that performs it.  Everything here is inline
// (__device__ or __host__ __device__ __forceinline__) and nothing has external linkage, so the two libraries that
// include this file - libavsum_hip.so (visual.hip, stage1_batch.hip, shots_batch.hip) and libavsum_ingest.so
// (ingest.hip) - share text, not symbols.
//
// 1. cv2.resize(..., INTER_LINEAR) for uint8: the source position and fraction of a destination index (cv_src_pos),
//    the two taps and their 11-bit coefficients (cv_linear_coef), the blend of four taps of one channel with the >> 4,
//    >> 16, + 2, >> 2 rounding of OpenCV's VResizeLinear (cv_blend); for the kernels that work in bands of output rows:
//    the source rows a band reads (cv_band_rows - the planners on the host size the LDS by it and the kernels stage by
//    it, so the two agree by construction), the per-column table in LDS (cv_coef_fill, cv_coef_at) and the 16-byte
//    stores of the finished band (stage_out).  Shared by resize_bilinear_kernel (visual.hip), resize_gather2_kernel
//    (stage1_batch.hip) and nv12_resize_gather2_kernel (ingest.hip).  What each kernel keeps is what tells them apart:
//    where a tap comes from - global memory, a staged BGR range, or staged luma and chroma rows converted per tap - and
//    how the source rows get into LDS.
//
// 2. The shot scan: |dH|, |dS|, |dV| of a frame against its predecessor, summed over the strided pixels (hsv_diff_body).
//    Shared by hsv_frame_diff_kernel (visual.hip), hsv_frame_diff_batch_kernel (shots_batch.hip) and
//    nv12_hsv_diff_batch_kernel (ingest.hip).  A kernel finds its frame, forms the two frame pointers and says which grid
//    axis splits a frame's pixels; where a pixel's B, G, R come from is the template parameter SRC:
//
//      void SRC::bgr(const uint8_t* frame, int y, int x, int& b, int& g, int& r) const
//
//    bgr_dense_src below reads three bytes of a dense [h, w, 3] frame; ingest.hip's source converts a luma byte and a
//    chroma pair.
//
// Integers throughout apart from cv_src_pos, whose operations and their order are fixed (the files are compiled with
// -ffp-contract=off): a pixel has the same bytes through every kernel.  The thread count of a workgroup enters as the
// template parameter THREADS; the kernels' own #defines stay in their files.
#pragma once
#include "avs_internal.h"   // bgr2hsv_u8

// ---------------------------------------------------------------------------
// 1. Resize
// ---------------------------------------------------------------------------
// the source index of destination index d, clamped to [0, smax - 1], and in f its fraction (0 where clamped)
__host__ __device__ __forceinline__ int cv_src_pos(int d, double scale, int smax, float& f) {
  f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= smax - 1) {
    f = 0.f;
    s = smax - 1;
  }
  return s;
}

__device__ __forceinline__ void cv_linear_coef(int d, double scale, int smax, int& s0, int& s1, int& c0, int& c1) {
  float f;
  s0 = cv_src_pos(d, scale, smax, f);
  s1 = min(s0 + 1, smax - 1);
  c0 = __float2int_rn((1.f - f) * 2048.f);
  c1 = __float2int_rn(f * 2048.f);
}

// one channel: taps p<row><column>, column coefficients a0, a1, row coefficients b0, b1
__device__ __forceinline__ uint8_t cv_blend(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  const int S0 = p00 * a0 + p01 * a1;
  const int S1 = p10 * a0 + p11 * a1;
  const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the source rows y_lo .. y_hi the output rows dy_lo .. dy_hi - 1 read
__host__ __device__ __forceinline__ void cv_band_rows(int dy_lo, int dy_hi, double scale_y, int sh, int& y_lo, int& y_hi) {
  float f;
  y_lo = cv_src_pos(dy_lo, scale_y, sh, f);
  y_hi = min(cv_src_pos(dy_hi - 1, scale_y, sh, f) + 1, sh - 1);
}

// the column table of one destination, (x0 | x1 << 16, a0 | a1 << 16) per output column: source columns in 16 bits,
// so sw <= 65535 (the launchers refuse more)
template <int THREADS>
__device__ __forceinline__ void cv_coef_fill(uint2* coef, int dw, double scale_x, int sw) {
  for (int dx = threadIdx.x; dx < dw; dx += THREADS) {
    int x0, x1, a0, a1;
    cv_linear_coef(dx, scale_x, sw, x0, x1, a0, a1);
    coef[dx] = make_uint2((unsigned)x0 | ((unsigned)x1 << 16), (unsigned)a0 | ((unsigned)a1 << 16));
  }
}

__device__ __forceinline__ void cv_coef_at(const uint2* coef, int dx, int& x0, int& x1, int& a0, int& a1) {
  const uint2 cf = coef[dx];
  x0 = (int)(cf.x & 0xffffu), x1 = (int)(cf.x >> 16);
  a0 = (int)(cf.y & 0xffffu), a1 = (int)(cf.y >> 16);
}

// bytes [0, n) of `l` to `g`, where l and g are congruent modulo 16: the bytes up to g's first 16-byte boundary and
// after its last one singly, everything between as 16-byte units
template <int THREADS>
__device__ __forceinline__ void stage_out(uint8_t* g, const uint8_t* l, int n) {
  const int head = min(n, (int)((16u - (unsigned)(uintptr_t)g) & 15u));
  const int nvec = (n - head) >> 4;
  uint4* gv = reinterpret_cast<uint4*>(g + head);
  const uint4* lv = reinterpret_cast<const uint4*>(l + head);
  for (int j = threadIdx.x; j < nvec; j += THREADS) gv[j] = lv[j];
  const int tail0 = head + (nvec << 4);
  for (int k = threadIdx.x; k < head + n - tail0; k += THREADS) {
    const int o = k < head ? k : tail0 + (k - head);
    g[o] = l[o];
  }
}

// ---------------------------------------------------------------------------
// 2. Shot scan
// ---------------------------------------------------------------------------
struct bgr_dense_src {   // a dense [h, w, 3] frame
  int w;
  __device__ __forceinline__ void bgr(const uint8_t* frame, int y, int x, int& b, int& g, int& r) const {
    const long long o = ((long long)y * w + x) * 3;
    b = frame[o], g = frame[o + 1], r = frame[o + 2];
  }
};

// Workgroup `part` of the `parts` that share frame `cur`: the strided pixels (y, x) = ((i / pw) * step, (i % pw) * step),
// i < ph * pw, dealt THREADS at a time; both frames' pixels to HSV, the three absolute differences summed per thread,
// per wave by shuffle, per workgroup through LDS, and one integer atomicAdd per channel into sums3[0 .. 2] - exact and
// independent of the order.  part and parts are unsigned, as the grid's own words are: the loop's counter then advances
// in wrapping arithmetic, the compiler cannot count its trips and leaves it a loop.  With int it unrolls the loop
// eightfold, and the NV12 form then takes 256 registers and one wave per SIMD.
template <int THREADS, class SRC>
__device__ __forceinline__ void hsv_diff_body(const SRC& src, const uint8_t* cur, const uint8_t* prv, int step, int ph,
                                              int pw, unsigned part, unsigned parts, unsigned* sums3) {
  __shared__ unsigned red[THREADS / 64][3];
  unsigned a0 = 0, a1 = 0, a2 = 0;
  const int npx = ph * pw;
  for (int i = part * THREADS + threadIdx.x; i < npx; i += parts * THREADS) {
    const int y = (i / pw) * step, x = (i % pw) * step;
    int b, g, r, h1, s1, v1, h0, s0, v0;
    src.bgr(cur, y, x, b, g, r);
    bgr2hsv_u8(b, g, r, h1, s1, v1);
    src.bgr(prv, y, x, b, g, r);
    bgr2hsv_u8(b, g, r, h0, s0, v0);
    a0 += (unsigned)abs(h1 - h0);
    a1 += (unsigned)abs(s1 - s0);
    a2 += (unsigned)abs(v1 - v0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, 64);
    a1 += __shfl_xor(a1, o, 64);
    a2 += __shfl_xor(a2, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a0;
    red[threadIdx.x >> 6][1] = a1;
    red[threadIdx.x >> 6][2] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned s = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < THREADS / 64; ++k) s += red[k][threadIdx.x];
    atomicAdd(sums3 + threadIdx.x, s);
  }
}
