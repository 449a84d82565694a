// Batched stage-1 extraction (features/extractors.py:344-362 for every shot of a ragged batch of videos): the glue between
// the sampling tables and the two CNN trunks, and between the trunks and the per-shot feature rows.
//   1. avs_resize_bilinear_gather2_u8: the sampled frames of one pass, read where they lie in the concatenated frames and
//      resized to the trunks' two input sizes in one launch - no dense full-resolution copy of the samples.
//   2. avs_segment_mean_perm_f32: the per-shot means of the feature rows, read through the permutation that undoes the
//      pass order.
// Integers or a fixed summation order throughout: two calls give the same bytes.
#include "avs_internal.h"
#include "pixel_bodies.h"

#define RG_THREADS 256
#define RG_BAND 8                     // output rows of one workgroup (halved until the source rows fit RG_LDS_BYTES)
#define RG_LDS_BYTES (64 * 1024)      // the dynamic LDS one workgroup may ask for without an opt-in
#define RG_INFLIGHT 4                 // 16-byte loads a lane keeps in flight while staging (as gather_rows_kernel)

// ---------------------------------------------------------------------------
// 1. cv2.resize(..., INTER_LINEAR) of gathered frames.  The arithmetic is pixel_bodies.h's, the one text
// resize_bilinear_kernel (visual.hip) runs too: coefficients, blend, column table, and cv_band_rows, by which the host
// sizes the LDS to the exact row span of a band and the kernel stages that span.
// ---------------------------------------------------------------------------
struct rg_dest {
  uint8_t* dst;       // [count, dh, dw, 3]
  int dh, dw, band;   // band: output rows per workgroup
  int in_bytes;       // LDS bytes of the staged source rows: (most source rows of a band) * sw * 3, + 16, to 16
  double scale_y, scale_x;
};
struct rg_args {
  rg_dest d[2];
};

// bytes [0, n) of `g` to `l`, where l and g are congruent modulo 16: the bytes up to g's first 16-byte boundary and
// after its last one singly, everything between as 16-byte units, RG_INFLIGHT loads ahead of the first store
__device__ __forceinline__ void rg_stage_in(uint8_t* l, const uint8_t* g, int n) {
  const int head = min(n, (int)((16u - (unsigned)(uintptr_t)g) & 15u));
  const int nvec = (n - head) >> 4;
  const uint4* gv = reinterpret_cast<const uint4*>(g + head);
  uint4* lv = reinterpret_cast<uint4*>(l + head);
  int j = threadIdx.x;
  for (; j + (RG_INFLIGHT - 1) * RG_THREADS < nvec; j += RG_INFLIGHT * RG_THREADS) {
    const uint4 a = gv[j], b = gv[j + RG_THREADS], c = gv[j + 2 * RG_THREADS], e = gv[j + 3 * RG_THREADS];
    lv[j] = a;
    lv[j + RG_THREADS] = b;
    lv[j + 2 * RG_THREADS] = c;
    lv[j + 3 * RG_THREADS] = e;
  }
  for (; j < nvec; j += RG_THREADS) lv[j] = gv[j];
  const int tail0 = head + (nvec << 4);
  for (int k = threadIdx.x; k < head + n - tail0; k += RG_THREADS) {
    const int o = k < head ? k : tail0 + (k - head);
    l[o] = g[o];
  }
}

// grid (row of the index, band of output rows, destination).  A workgroup: (a) the column coefficients of its
// destination, once, into LDS; (b) the source rows its band reads - one contiguous byte range of the frame - into LDS
// with 16-byte loads; (c) one wave per output row, a lane per pixel, LDS to LDS; (d) the band's output rows - one
// contiguous byte range again - out with 16-byte stores.  Both LDS images sit at their global address modulo 16.
__global__ __launch_bounds__(RG_THREADS) void resize_gather2_kernel(const uint8_t* __restrict__ src, long long src_rows,
                                                                    int sh, int sw, const long long* __restrict__ index,
                                                                    rg_args args) {
  extern __shared__ __align__(16) uint8_t rg_lds[];
  const rg_dest& D = args.d[blockIdx.z];
  const int dy_lo = blockIdx.y * D.band;
  if (dy_lo >= D.dh) return;
  const long long i = blockIdx.x;
  const long long r = index[i];
  if (r < 0 || r >= src_rows) return;
  const int dy_hi = min(dy_lo + D.band, D.dh);
  const int dw = D.dw, row_in = sw * 3, row_out = dw * 3;

  uint2* coef = reinterpret_cast<uint2*>(rg_lds);                 // per column (x0 | x1 << 16, a0 | a1 << 16)
  uint8_t* in_base = rg_lds + ((dw * 8 + 15) & ~15);
  uint8_t* out_base = in_base + D.in_bytes;

  cv_coef_fill<RG_THREADS>(coef, dw, D.scale_x, sw);
  int y_lo, y_hi;
  cv_band_rows(dy_lo, dy_hi, D.scale_y, sh, y_lo, y_hi);
  const uint8_t* g_in = src + (r * sh + y_lo) * (long long)row_in;
  uint8_t* in = in_base + ((unsigned)(uintptr_t)g_in & 15u);
  rg_stage_in(in, g_in, (y_hi - y_lo + 1) * row_in);
  uint8_t* g_out = D.dst + (i * D.dh + dy_lo) * (long long)row_out;
  uint8_t* out = out_base + ((unsigned)(uintptr_t)g_out & 15u);
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int dy = dy_lo + wave; dy < dy_hi; dy += RG_THREADS / 64) {
    int y0, y1, b0, b1;
    cv_linear_coef(dy, D.scale_y, sh, y0, y1, b0, b1);
    const uint8_t* r0 = in + (y0 - y_lo) * row_in;
    const uint8_t* r1 = in + (y1 - y_lo) * row_in;
    uint8_t* o = out + (dy - dy_lo) * row_out;
    for (int dx = lane; dx < dw; dx += 64) {
      int x0, x1, a0, a1;
      cv_coef_at(coef, dx, x0, x1, a0, a1);
      x0 *= 3, x1 *= 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[dx * 3 + c] = cv_blend(r0[x0 + c], r0[x1 + c], r1[x0 + c], r1[x1 + c], a0, a1, b0, b1);
    }
  }
  __syncthreads();
  stage_out<RG_THREADS>(g_out, out, (dy_hi - dy_lo) * row_out);
}

// the band and the LDS bytes of one destination: the most source rows any band of `band` output rows reads, by the
// kernel's own arithmetic.  Returns the total LDS bytes (coefficients + source rows + output rows), 0 when even a band
// of one output row does not fit.
static size_t rg_plan(rg_dest& D, int sh, int sw) {
  for (int band = RG_BAND; band >= 1; band >>= 1) {
    int span = 1;
    for (int lo = 0; lo < D.dh; lo += band) {
      int y_lo, y_hi;
      cv_band_rows(lo, lo + band < D.dh ? lo + band : D.dh, D.scale_y, sh, y_lo, y_hi);
      if (y_hi - y_lo + 1 > span) span = y_hi - y_lo + 1;
    }
    const size_t in_bytes = ((size_t)span * sw * 3 + 16 + 15) & ~(size_t)15;
    const size_t out_bytes = ((size_t)band * D.dw * 3 + 16 + 15) & ~(size_t)15;
    const size_t total = (((size_t)D.dw * 8 + 15) & ~(size_t)15) + in_bytes + out_bytes;
    if (total <= RG_LDS_BYTES) {
      D.band = band;
      D.in_bytes = (int)in_bytes;
      return total;
    }
  }
  return 0;
}

extern "C" int avs_resize_bilinear_gather2_u8(const uint8_t* d_src, int64_t src_rows, int sh, int sw,
                                              const int64_t* d_index, int64_t count, uint8_t* d_dst0, int dh0, int dw0,
                                              uint8_t* d_dst1, int dh1, int dw1, avs_stream_t stream) {
  AVS_REQUIRE(src_rows >= 0 && sh > 0 && sw > 0 && dh0 > 0 && dw0 > 0 && count >= 0 && count <= 0x7fffffffll &&
                  (!d_dst1 || (dh1 > 0 && dw1 > 0)),
              AVS_E_SHAPE, "avs_resize_bilinear_gather2_u8: src_rows=%lld source %dx%d count=%lld sizes %dx%d %dx%d",
              (long long)src_rows, sh, sw, (long long)count, dh0, dw0, dh1, dw1);
  // the column table holds source columns in 16 bits; the bands are on grid y
  AVS_REQUIRE(sw <= 65535 && dh0 <= 65535 && (!d_dst1 || dh1 <= 65535), AVS_E_UNSUPPORTED,
              "avs_resize_bilinear_gather2_u8: more than 65535 source columns or output rows");
  if (count == 0) return AVS_OK;
  AVS_REQUIRE(d_src && d_index && d_dst0, AVS_E_ARG, "avs_resize_bilinear_gather2_u8: null pointer");
  rg_args args;
  const int ndst = d_dst1 ? 2 : 1;
  const int dh[2] = {dh0, dh1}, dw[2] = {dw0, dw1};
  uint8_t* const dst[2] = {d_dst0, d_dst1};
  size_t lds = 0;
  int bands = 0;
  for (int k = 0; k < ndst; ++k) {
    rg_dest& D = args.d[k];
    // OpenCV: inv_scale = dsize/ssize (double); scale = 1/inv_scale.
    D = rg_dest{dst[k], dh[k], dw[k], 1, 0, 1.0 / ((double)dh[k] / (double)sh), 1.0 / ((double)dw[k] / (double)sw)};
    const size_t need = rg_plan(D, sh, sw);
    AVS_REQUIRE(need > 0, AVS_E_UNSUPPORTED,
                "avs_resize_bilinear_gather2_u8: two source rows of %d pixels and one output row of %d do not fit %d "
                "bytes of LDS", sw, D.dw, RG_LDS_BYTES);
    if (need > lds) lds = need;
    const int nb = (int)avs_cdiv(D.dh, D.band);
    if (nb > bands) bands = nb;
  }
  if (ndst == 1) args.d[1] = args.d[0];   // (never read: grid z is 1)
  hipLaunchKernelGGL(resize_gather2_kernel, dim3((unsigned)count, (unsigned)bands, (unsigned)ndst), dim3(RG_THREADS), lds,
                     (hipStream_t)stream, d_src, (long long)src_rows, sh, sw, reinterpret_cast<const long long*>(d_index),
                     args);
  AVS_CHECK_LAUNCH("avs_resize_bilinear_gather2_u8");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 2. out[s,:] = mean over k of x[perm[seg[s] + k], :], k ascending: segment_mean_kernel (visual.hip) reading its rows
// through a permutation - the same additions in the same order, so the bytes of segment_mean on the permuted rows.  An
// empty segment gives zeros.  An entry of seg outside perm, or of perm outside x, is passed over (never read).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segment_mean_perm_kernel(const float* __restrict__ x, long long ldx,
                                                                long long x_rows, int d,
                                                                const long long* __restrict__ perm, long long perm_len,
                                                                const long long* __restrict__ seg, int nseg,
                                                                float* __restrict__ out, long long ldo) {
  const long long total = (long long)nseg * d;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % d);
    const long long s = i / d;
    const long long r0 = seg[s], r1 = seg[s + 1];
    float a = 0.f;
    for (long long r = max(r0, 0ll); r < min(r1, perm_len); ++r) {
      const long long p = perm[r];
      if (p >= 0 && p < x_rows) a += x[p * ldx + ch];
    }
    out[s * ldo + ch] = r1 > r0 ? a / (float)(r1 - r0) : 0.f;
  }
}

extern "C" int avs_segment_mean_perm_f32(const float* d_x, int64_t ldx, int64_t x_rows, int d, const int64_t* d_perm,
                                         int64_t perm_len, const int64_t* d_seg, int nseg, float* d_out, int64_t ldo,
                                         avs_stream_t stream) {
  AVS_REQUIRE(d > 0 && ldx >= d && ldo >= d && nseg >= 0 && x_rows >= 0 && perm_len >= 0, AVS_E_SHAPE,
              "avs_segment_mean_perm_f32: bad extents");
  if (nseg == 0) return AVS_OK;
  AVS_REQUIRE(d_seg && d_out && (perm_len == 0 || (d_perm && (x_rows == 0 || d_x))), AVS_E_ARG,
              "avs_segment_mean_perm_f32: null pointer");
  long long gx = avs_cdiv((long long)nseg * d, 256);
  if (gx > 16384) gx = 16384;
  hipLaunchKernelGGL(segment_mean_perm_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, d_x, (long long)ldx,
                     (long long)x_rows, d, reinterpret_cast<const long long*>(d_perm), (long long)perm_len,
                     reinterpret_cast<const long long*>(d_seg), nseg, d_out, (long long)ldo);
  AVS_CHECK_LAUNCH("avs_segment_mean_perm_f32");
  return AVS_OK;
}
