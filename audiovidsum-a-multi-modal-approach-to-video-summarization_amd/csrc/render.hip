// libavsum_render.so: the summary rendered on the device (include/avsum_render.h, whose comment is the definition).  This
// file is the whole library: it includes the HIP runtime and its own header, and references no symbol of another
// library - the error text, the argument checks and the launch check below are its own.
//
//   index_count_kernel / index_scan_kernel / index_scatter_kernel   mask -> frame list and runs.  Order comes from the
//       three launch boundaries: per-tile counts, ONE workgroup's scan of them, per-tile scatter.  No atomics, no flags.
//   bgr_to_yuv_kernel<SB>    a thread owns four 2x2 blocks side by side: 2 x 24 BGR bytes in, 2 x 8 luma samples and
//                            4 U + 4 V samples out
//   repack_kernel<SB>        the same ownership, samples copied between two layouts of one depth
//   audio_bounds_kernel / audio_copy_kernel   the runs' sample bounds and their prefix in ONE workgroup, then the copy
// Memory access of the pixel kernels: every load and store is naturally aligned and as wide as the ADDRESS allows
// (nr_load / nr_store pick 16, 8, 4, 2 or 1 bytes per piece by the low bits of the address, wave-uniformly along a row
// since a thread's pieces are 8, 16 or 24 bytes apart); an odd address leaves through a scalar head byte, 2-byte pieces
// and a scalar tail byte, and the blocks of a row that do not fill a group of four (the row's tail) go sample by sample.
// Integers and fixed orders: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/avsum_render.h"

#define NR_THREADS 256
#define NR_PER (AVSR_TILE / NR_THREADS)   // frames of a tile per thread
static_assert(AVSR_TILE % NR_THREADS == 0, "a thread owns whole frames of a tile");
static_assert(AVSR_AUDIO_TILE % NR_THREADS == 0, "a thread owns whole samples of an audio tile");
static_assert((long long)AVSR_MAX_ROW_SUM * 1020 + (1 << 21) < (1ll << 31), "the largest chroma accumulator fits int32");

static thread_local char g_err[512] = "";

static void avsr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSR_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsr_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSR_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsr_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSR_E_HIP;                                                         \
    }                                                                            \
  } while (0)

extern "C" int avsr_abi_version(void) { return AVSR_ABI_VERSION; }
extern "C" const char* avsr_last_error(void) { return g_err; }

static long long nr_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// Exclusive prefix of one value per thread over the NR_THREADS threads of a workgroup, two values at once: a wave's
// inclusive scan by lane shuffles, the four wave totals through LDS.  a, b: in the thread's values, out their exclusive
// prefixes; ta, tb: the workgroup's totals.  Every thread of the workgroup calls it.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void nr_block_scan2(T& a, T& b, T& ta, T& tb) {
  __shared__ T wave_a[NR_THREADS / 64], wave_b[NR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T ia = a, ib = b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T xa = __shfl_up(ia, d), xb = __shfl_up(ib, d);
    if (lane >= d) ia += xa, ib += xb;
  }
  if (lane == 63) wave_a[wave] = ia, wave_b[wave] = ib;
  __syncthreads();
  T pa = 0, pb = 0;
  ta = 0, tb = 0;
#pragma unroll
  for (int w = 0; w < NR_THREADS / 64; ++w) {
    if (w < wave) pa += wave_a[w], pb += wave_b[w];
    ta += wave_a[w], tb += wave_b[w];
  }
  a = pa + ia - a, b = pb + ib - b;
  __syncthreads();   // the LDS words may be written again by the next call
}

// ---------------------------------------------------------------------------
// 1. The summary index.
// ---------------------------------------------------------------------------
struct nr_tile {
  long long lo, hi;      // the tile's video: frames lo .. hi
  long long first, end;  // the tile: frames first .. end
};

__device__ __forceinline__ nr_tile nr_tile_of(const long long* __restrict__ offsets, const int* __restrict__ tiles, long long t) {
  const int v = tiles[AVSR_TILE_COLS * t], k = tiles[AVSR_TILE_COLS * t + 1];
  nr_tile T;
  T.lo = offsets[v], T.hi = offsets[v + 1];
  T.first = T.lo + (long long)k * AVSR_TILE;
  T.end = T.first + AVSR_TILE < T.hi ? T.first + AVSR_TILE : T.hi;
  return T;
}

// the thread's NR_PER frames of tile T: sel[j] (frame i0 + j selected), begins[j] (it starts a run); returns i0
__device__ __forceinline__ long long nr_tile_frames(const uint8_t* __restrict__ mask, const nr_tile& T, bool (&sel)[NR_PER],
                                                    bool (&begins)[NR_PER]) {
  const long long i0 = T.first + (long long)threadIdx.x * NR_PER;
  bool prev = i0 > T.lo && i0 < T.end && mask[i0 - 1] != 0;   // (the frame before a video's first is not its own)
#pragma unroll
  for (int j = 0; j < NR_PER; ++j) {
    sel[j] = i0 + j < T.end && mask[i0 + j] != 0;
    begins[j] = sel[j] && !prev;
    prev = sel[j];
  }
  return i0;
}

__global__ __launch_bounds__(NR_THREADS) void index_count_kernel(const uint8_t* __restrict__ mask,
                                                                 const long long* __restrict__ offsets,
                                                                 const int* __restrict__ tiles, long long* __restrict__ work) {
  const long long t = blockIdx.x;
  const nr_tile T = nr_tile_of(offsets, tiles, t);
  bool sel[NR_PER], begins[NR_PER];
  nr_tile_frames(mask, T, sel, begins);
  int ones = 0, starts = 0, total_ones, total_starts;
#pragma unroll
  for (int j = 0; j < NR_PER; ++j) ones += sel[j], starts += begins[j];
  nr_block_scan2(ones, starts, total_ones, total_starts);
  if (threadIdx.x == 0) work[2 * t] = total_ones, work[2 * t + 1] = total_starts;
}

// ONE workgroup: the tile counts become exclusive prefixes in place (tiles are in video order, so the prefix at a
// video's first tile is the video's offset), then the per-video totals
__global__ __launch_bounds__(NR_THREADS) void index_scan_kernel(const int* __restrict__ tiles, long long ntiles, int nvideos,
                                                                long long* __restrict__ work, long long* __restrict__ frame_offsets,
                                                                long long* __restrict__ run_offsets,
                                                                long long* __restrict__ totals) {
  long long carry_f = 0, carry_r = 0;
  for (long long c = 0; c < ntiles; c += NR_THREADS) {
    const long long t = c + threadIdx.x;
    long long f = t < ntiles ? work[2 * t] : 0, r = t < ntiles ? work[2 * t + 1] : 0, tf, tr;
    nr_block_scan2(f, r, tf, tr);
    if (t < ntiles) {
      work[2 * t] = carry_f + f, work[2 * t + 1] = carry_r + r;
      if (tiles[AVSR_TILE_COLS * t + 1] == 0) {
        const int v = tiles[AVSR_TILE_COLS * t];
        frame_offsets[v] = carry_f + f, run_offsets[v] = carry_r + r;
      }
    }
    carry_f += tf, carry_r += tr;
  }
  if (threadIdx.x == 0) frame_offsets[nvideos] = carry_f, run_offsets[nvideos] = carry_r;
  __threadfence_block();
  __syncthreads();
  for (int v = threadIdx.x; v < nvideos; v += NR_THREADS) {
    totals[AVSR_TOTAL_COLS * (long long)v] = run_offsets[v + 1] - run_offsets[v];
    totals[AVSR_TOTAL_COLS * (long long)v + 1] = frame_offsets[v + 1] - frame_offsets[v];
    totals[AVSR_TOTAL_COLS * (long long)v + 2] = 0;
  }
}

// workgroups 0 .. ntiles - 1 scatter their tile; the others write the -1 tails (entries the scatter never touches)
__global__ __launch_bounds__(NR_THREADS) void index_scatter_kernel(const uint8_t* __restrict__ mask,
                                                                   const long long* __restrict__ offsets,
                                                                   const int* __restrict__ tiles, long long ntiles, int nvideos,
                                                                   const long long* __restrict__ work,
                                                                   const long long* __restrict__ frame_offsets,
                                                                   const long long* __restrict__ run_offsets,
                                                                   long long* __restrict__ frame_index, long long frame_cap,
                                                                   long long* __restrict__ runs, long long run_cap) {
  if (blockIdx.x >= ntiles) {
    const long long first = ((long long)blockIdx.x - ntiles) * AVSR_TILE;
    const long long nframes = frame_offsets[nvideos], nruns = run_offsets[nvideos];
    for (long long j = first + threadIdx.x; j < first + AVSR_TILE; j += NR_THREADS) {
      if (j >= nframes && j < frame_cap) frame_index[j] = -1;
      if (j >= nruns && j < run_cap) runs[2 * j] = -1, runs[2 * j + 1] = -1;
    }
    return;
  }
  const long long t = blockIdx.x;
  const nr_tile T = nr_tile_of(offsets, tiles, t);
  bool sel[NR_PER], begins[NR_PER];
  const long long i0 = nr_tile_frames(mask, T, sel, begins);
  int ones = 0, starts = 0, total_ones, total_starts;
#pragma unroll
  for (int j = 0; j < NR_PER; ++j) ones += sel[j], starts += begins[j];
  nr_block_scan2(ones, starts, total_ones, total_starts);
  long long at = work[2 * t] + ones;      // summary frames before frame i0 + j
  long long run = work[2 * t + 1] + starts;   // runs that start before frame i0 + j
#pragma unroll
  for (int j = 0; j < NR_PER; ++j) {
    if (!sel[j]) continue;
    const long long i = i0 + j;
    if (at < frame_cap) frame_index[at] = i;
    ++at;
    if (begins[j]) {
      if (run < run_cap) runs[2 * run] = i - T.lo;
      ++run;
    }
    // the run that holds frame i is the last one started: run - 1 (it may have started in an earlier tile)
    const bool ends = i + 1 == T.hi || mask[i + 1] == 0;
    if (ends && run - 1 < run_cap) runs[2 * (run - 1) + 1] = i + 1 - T.lo;
  }
}

extern "C" int avsr_summary_index(const uint8_t* d_mask, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets,
                                  int nvideos, const int32_t* d_tiles, int64_t ntiles, int64_t* d_work, int64_t* d_frame_index,
                                  int64_t frame_cap, int64_t* d_frame_offsets, int64_t* d_runs, int64_t run_cap,
                                  int64_t* d_run_offsets, int64_t* d_totals, avsr_stream_t stream) {
  AVSR_REQUIRE(frame_cap >= 1 && run_cap >= 1 && frame_cap < (1ll << 31) && run_cap < (1ll << 31), AVSR_E_ARG,
               "avsr_summary_index: capacities must lie in 1 .. 2^31 - 1, got frame_cap=%lld run_cap=%lld",
               (long long)frame_cap, (long long)run_cap);
  AVSR_REQUIRE(nvideos >= 1 && n >= 1 && n <= AVSR_MAX_FRAMES, AVSR_E_SHAPE,
               "avsr_summary_index: nvideos=%d n=%lld (at least one video, 1 .. %d frames)", nvideos, (long long)n,
               AVSR_MAX_FRAMES);
  AVSR_REQUIRE(h_offsets, AVSR_E_ARG, "avsr_summary_index: h_offsets is null");
  AVSR_REQUIRE(h_offsets[0] == 0 && h_offsets[nvideos] == n, AVSR_E_SHAPE,
               "avsr_summary_index: the offsets run from %lld to %lld, the mask has %lld frames", (long long)h_offsets[0],
               (long long)h_offsets[nvideos], (long long)n);
  long long want = 0;
  for (int v = 0; v < nvideos; ++v) {
    AVSR_REQUIRE(h_offsets[v + 1] > h_offsets[v], AVSR_E_SHAPE, "avsr_summary_index: video %d is empty (the offsets must increase)",
                 v);
    want += nr_cdiv(h_offsets[v + 1] - h_offsets[v], AVSR_TILE);
  }
  AVSR_REQUIRE(ntiles == want, AVSR_E_SHAPE, "avsr_summary_index: ntiles=%lld, the offsets give %lld tiles of %d frames",
               (long long)ntiles, want, AVSR_TILE);
  AVSR_REQUIRE(d_mask && d_offsets && d_tiles && d_work && d_frame_index && d_frame_offsets && d_runs && d_run_offsets &&
               d_totals, AVSR_E_ARG, "avsr_summary_index: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const long long* off = reinterpret_cast<const long long*>(d_offsets);
  long long* work = reinterpret_cast<long long*>(d_work);
  long long* fo = reinterpret_cast<long long*>(d_frame_offsets);
  long long* ro = reinterpret_cast<long long*>(d_run_offsets);
  hipLaunchKernelGGL(index_count_kernel, dim3((unsigned)ntiles), dim3(NR_THREADS), 0, s, d_mask, off, d_tiles, work);
  AVSR_CHECK_LAUNCH("avsr_summary_index (count)");
  hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(NR_THREADS), 0, s, d_tiles, (long long)ntiles, nvideos, work, fo, ro,
                     reinterpret_cast<long long*>(d_totals));
  AVSR_CHECK_LAUNCH("avsr_summary_index (scan)");
  const long long fill = nr_cdiv(frame_cap > run_cap ? frame_cap : run_cap, AVSR_TILE);
  hipLaunchKernelGGL(index_scatter_kernel, dim3((unsigned)(ntiles + fill)), dim3(NR_THREADS), 0, s, d_mask, off, d_tiles,
                     (long long)ntiles, nvideos, work, fo, ro, reinterpret_cast<long long*>(d_frame_index),
                     (long long)frame_cap, reinterpret_cast<long long*>(d_runs), (long long)run_cap);
  AVSR_CHECK_LAUNCH("avsr_summary_index (scatter)");
  return AVSR_OK;
}

// ---------------------------------------------------------------------------
// 2. Pixels.  The surface description and its checks (those of avsum_yuv.h, stated here for this library).
// ---------------------------------------------------------------------------
struct nr_surf {
  uint8_t* base;
  long long n, stride, u_off, v_off;
  int h, w, sb, shift, pitch_y, pitch_c, step;
  bool inter;   // V one sample beside U, a step of two samples: one run of (U, V) or (V, U) pairs per chroma row
};
struct nr_fwd {
  int y_off, yb, yg, yr, ub, ug, ur, vb, vg, vr;
};

// Do the samples of two chroma planes of the same pitch and step, `delta` bytes apart, share a byte?  Sample (r, c) of
// the one and (r + dr, c + dc) of the other do when |delta - dr * pitch - dc * step| < sb; only the two dr around
// delta / pitch can, and for each only the two dc around the rest / step.
static bool nr_chroma_planes_meet(long long delta, long long pitch, long long step, long long sb, long long ch, long long cw) {
  if (delta < 0) delta = -delta;
  for (long long dr = delta / pitch; dr <= delta / pitch + 1; ++dr) {
    if (dr > ch - 1) continue;
    const long long rest = delta - dr * pitch;
    const long long q = rest >= 0 ? rest / step : -((-rest + step - 1) / step);
    for (long long dc = q; dc <= q + 1; ++dc) {
      const long long d = rest - dc * step;
      if (dc >= -(cw - 1) && dc <= cw - 1 && d > -sb && d < sb) return true;
    }
  }
  return false;
}

// Does a sample of the chroma plane at `off` share a byte with a luma sample?
static bool nr_chroma_meets_luma(long long off, long long pitch_y, long long pitch_c, long long step, long long sb, long long h,
                                 long long w) {
  const long long ch = h / 2, cw = w / 2, luma_end = (h - 1) * pitch_y + w * sb;
  if (off >= luma_end) return false;
  for (long long r = 0; r < ch; ++r) {
    const long long a = off + r * pitch_c, b = a + (cw - 1) * step + sb;
    if (a >= luma_end) break;
    for (long long y = a / pitch_y; y < h && y * pitch_y < b; ++y) {
      const long long ya = y * pitch_y, yb = ya + w * sb;
      const long long c = ya - sb - a < 0 ? 0 : (ya - sb - a) / step + 1;
      if (c < cw && a + c * step < yb) return true;
    }
  }
  return false;
}

static int nr_surface_arg(const char* what, const char* which, nr_surf& S, const uint8_t* base, const int64_t* h_surface) {
  AVSR_REQUIRE(h_surface, AVSR_E_ARG, "%s: the %s description is null", what, which);
  const long long n = h_surface[AVSR_S_N], h = h_surface[AVSR_S_H], w = h_surface[AVSR_S_W];
  const long long sb = h_surface[AVSR_S_SAMPLE_BYTES], shift = h_surface[AVSR_S_SHIFT];
  const long long pitch_y = h_surface[AVSR_S_PITCH_Y], pitch_c = h_surface[AVSR_S_PITCH_C];
  const long long step = h_surface[AVSR_S_CHROMA_STEP], u_off = h_surface[AVSR_S_U_OFFSET];
  const long long v_off = h_surface[AVSR_S_V_OFFSET], stride = h_surface[AVSR_S_FRAME_STRIDE];
  AVSR_REQUIRE(n >= 0 && n < (1ll << 31), AVSR_E_SHAPE, "%s: %s n=%lld frames", what, which, n);
  AVSR_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, AVSR_E_SHAPE,
               "%s: %s: 4:2:0 frames have even extents of at least 2, got %lldx%lld", what, which, h, w);
  AVSR_REQUIRE(h < (1ll << 31) && w < (1ll << 31) && h * w * 3 < (1ll << 31), AVSR_E_SHAPE, "%s: %s: a frame of %lldx%lld is too large",
               what, which, h, w);
  AVSR_REQUIRE(sb == 1 || sb == 2, AVSR_E_SHAPE, "%s: %s sample_bytes %lld is neither 1 nor 2", what, which, sb);
  AVSR_REQUIRE((shift == 0 || shift == 6) && (sb == 2 || shift == 0), AVSR_E_SHAPE,
               "%s: %s shift %lld with samples of %lld bytes (0 or 6; 0 for one-byte samples)", what, which, shift, sb);
  const long long ch = h / 2, cw = w / 2;
  AVSR_REQUIRE(pitch_y >= w * sb && pitch_y < (1ll << 31), AVSR_E_SHAPE, "%s: %s pitch_y %lld below the %lld bytes of a luma row",
               what, which, pitch_y, w * sb);
  AVSR_REQUIRE(step >= sb && step < (1ll << 24), AVSR_E_SHAPE, "%s: %s chroma_step %lld below the %lld bytes of a sample", what,
               which, step, sb);
  const long long crow = (cw - 1) * step + sb;
  AVSR_REQUIRE(pitch_c >= crow && pitch_c < (1ll << 31), AVSR_E_SHAPE, "%s: %s pitch_c %lld below the %lld bytes of a chroma row",
               what, which, pitch_c, crow);
  AVSR_REQUIRE(u_off >= 0 && v_off >= 0, AVSR_E_SHAPE, "%s: %s: negative plane offset (u_offset %lld, v_offset %lld)", what, which,
               u_off, v_off);
  const long long y_end = (h - 1) * pitch_y + w * sb;
  const long long u_end = u_off + (ch - 1) * pitch_c + crow, v_end = v_off + (ch - 1) * pitch_c + crow;
  AVSR_REQUIRE(stride >= y_end && stride >= u_end && stride >= v_end, AVSR_E_SHAPE,
               "%s: %s frame_stride %lld ends before a plane does (luma %lld, U %lld, V %lld)", what, which, stride, y_end, u_end,
               v_end);
  if (sb == 2)
    AVSR_REQUIRE(((uintptr_t)base | (unsigned long long)pitch_y | (unsigned long long)pitch_c | (unsigned long long)step |
                  (unsigned long long)u_off | (unsigned long long)v_off | (unsigned long long)stride) % 2 == 0,
                 AVSR_E_SHAPE, "%s: %s: two-byte samples need an even base, pitch_y, pitch_c, chroma_step, u_offset, v_offset "
                 "and frame_stride", what, which);
  AVSR_REQUIRE(!nr_chroma_planes_meet(v_off - u_off, pitch_c, step, sb, ch, cw), AVSR_E_SHAPE,
               "%s: %s: the U and V planes overlap (u_offset %lld, v_offset %lld)", what, which, u_off, v_off);
  AVSR_REQUIRE(!nr_chroma_meets_luma(u_off, pitch_y, pitch_c, step, sb, h, w) &&
               !nr_chroma_meets_luma(v_off, pitch_y, pitch_c, step, sb, h, w), AVSR_E_SHAPE,
               "%s: %s: a chroma plane overlaps the luma plane (u_offset %lld, v_offset %lld, luma ends at %lld)", what, which,
               u_off, v_off, y_end);
  S.base = const_cast<uint8_t*>(base);
  S.n = n, S.stride = stride, S.u_off = u_off, S.v_off = v_off;
  S.h = (int)h, S.w = (int)w, S.sb = (int)sb, S.shift = (int)shift;
  S.pitch_y = (int)pitch_y, S.pitch_c = (int)pitch_c, S.step = (int)step;
  S.inter = step == 2 * sb && (v_off - u_off == sb || u_off - v_off == sb);
  return AVSR_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet?
static bool nr_ranges_meet(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na > 0 && nb > 0 && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// ---- naturally aligned pieces, as wide as the address allows.  w holds NB bytes, little-endian, in NB / 4 dwords
__device__ __forceinline__ unsigned nr_byte(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
__device__ __forceinline__ unsigned nr_half(const unsigned* w, int i) { return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu; }

template <int NB>
__device__ __forceinline__ void nr_store(uint8_t* p, const unsigned* w) {
  const unsigned a = (unsigned)(uintptr_t)p;
  if (NB % 16 == 0 && (a & 15u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 16; ++q) reinterpret_cast<uint4*>(p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else if (NB % 8 == 0 && (a & 7u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 8; ++q) reinterpret_cast<uint2*>(p)[q] = make_uint2(w[2 * q], w[2 * q + 1]);
  } else if ((a & 3u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) reinterpret_cast<unsigned*>(p)[q] = w[q];
  } else if ((a & 1u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) reinterpret_cast<uint16_t*>(p)[q] = (uint16_t)nr_half(w, q);
  } else {   // an odd address: a head byte, 2-byte pieces at the even addresses between, a tail byte
    p[0] = (uint8_t)nr_byte(w, 0);
#pragma unroll
    for (int q = 0; q < NB / 2 - 1; ++q)
      reinterpret_cast<uint16_t*>(p + 1)[q] = (uint16_t)(nr_byte(w, 2 * q + 1) | (nr_byte(w, 2 * q + 2) << 8));
    p[NB - 1] = (uint8_t)nr_byte(w, NB - 1);
  }
}

template <int NB>
__device__ __forceinline__ void nr_load(const uint8_t* p, unsigned* w) {
  const unsigned a = (unsigned)(uintptr_t)p;
  if (NB % 16 == 0 && (a & 15u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 16; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  } else if (NB % 8 == 0 && (a & 7u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 8; ++q) {
      const uint2 v = reinterpret_cast<const uint2*>(p)[q];
      w[2 * q] = v.x, w[2 * q + 1] = v.y;
    }
  } else if ((a & 3u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) w[q] = reinterpret_cast<const unsigned*>(p)[q];
  } else if ((a & 1u) == 0) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q)
      w[q] = (unsigned)reinterpret_cast<const uint16_t*>(p)[2 * q] | ((unsigned)reinterpret_cast<const uint16_t*>(p)[2 * q + 1] << 16);
  } else {
    unsigned prev = p[0];   // byte 0; then the 2-byte pieces hold bytes (2q + 1, 2q + 2)
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      const unsigned h0 = reinterpret_cast<const uint16_t*>(p + 1)[2 * q];                       // bytes 4q + 1, 4q + 2
      const unsigned h1 = 2 * q + 1 < NB / 2 - 1 ? (unsigned)reinterpret_cast<const uint16_t*>(p + 1)[2 * q + 1]
                                                 : (unsigned)p[NB - 1];                          // bytes 4q + 3 (, 4q + 4)
      w[q] = prev | (h0 << 8) | ((h1 & 255u) << 24);
      prev = h1 >> 8;
    }
  }
}

// N samples of SB bytes each, side by side at p
template <int SB, int N>
__device__ __forceinline__ void nr_put_samples(uint8_t* p, const int* s, int shift) {
  unsigned w[N * SB / 4];
  if (SB == 1) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      w[q] = (unsigned)s[4 * q] | ((unsigned)s[4 * q + 1] << 8) | ((unsigned)s[4 * q + 2] << 16) | ((unsigned)s[4 * q + 3] << 24);
  } else {
#pragma unroll
    for (int q = 0; q < N / 2; ++q) w[q] = ((unsigned)s[2 * q] << shift) | (((unsigned)s[2 * q + 1] << shift) << 16);
  }
  nr_store<N * SB>(p, w);
}
template <int SB, int N>
__device__ __forceinline__ void nr_get_samples(const uint8_t* p, int* s, int shift) {
  unsigned w[N * SB / 4];
  nr_load<N * SB>(p, w);
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = SB == 1 ? (int)nr_byte(w, q) : (int)((nr_half(w, q) >> shift) & 1023u);
}
template <int SB>
__device__ __forceinline__ void nr_put_one(uint8_t* p, int s, int shift) {
  if (SB == 1)
    *p = (uint8_t)s;
  else
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)(s << shift);
}
template <int SB>
__device__ __forceinline__ int nr_get_one(const uint8_t* p, int shift) {
  if (SB == 1) return *p;
  return (*reinterpret_cast<const uint16_t*>(p) >> shift) & 1023;
}

// The samples of `nb` (1 .. 4) 2x2 blocks side by side - chroma row cy, chroma columns cx0 .. cx0 + nb - 1 - of frame f:
// Y[r][x] the luma of row 2cy + r, column 2cx0 + x.  A full group of four goes in wide pieces; a shorter one (the tail
// of a row) and a chroma plane whose samples do not lie back to back go sample by sample.
template <int SB>
__device__ __forceinline__ void nr_put_group(const nr_surf& D, uint8_t* f, int cy, int cx0, int nb, const int (&Y)[2][8],
                                             const int (&U)[4], const int (&V)[4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    uint8_t* py = f + (long long)(2 * cy + r) * D.pitch_y + (long long)(2 * cx0) * SB;
    if (nb == 4) {
      nr_put_samples<SB, 8>(py, Y[r], D.shift);
    } else {
#pragma unroll
      for (int x = 0; x < 6; ++x)
        if (x < 2 * nb) nr_put_one<SB>(py + x * SB, Y[r][x], D.shift);
    }
  }
  const long long co = (long long)cy * D.pitch_c + (long long)cx0 * D.step;
  if (nb == 4 && D.inter) {
    const bool u_first = D.u_off < D.v_off;
    int uv[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) uv[2 * j] = u_first ? U[j] : V[j], uv[2 * j + 1] = u_first ? V[j] : U[j];
    nr_put_samples<SB, 8>(f + (u_first ? D.u_off : D.v_off) + co, uv, D.shift);
  } else if (nb == 4 && D.step == SB) {
    nr_put_samples<SB, 4>(f + D.u_off + co, U, D.shift);
    nr_put_samples<SB, 4>(f + D.v_off + co, V, D.shift);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nb) {
        nr_put_one<SB>(f + D.u_off + co + (long long)j * D.step, U[j], D.shift);
        nr_put_one<SB>(f + D.v_off + co + (long long)j * D.step, V[j], D.shift);
      }
  }
}

template <int SB>
__device__ __forceinline__ void nr_get_group(const nr_surf& S, const uint8_t* f, int cy, int cx0, int nb, int (&Y)[2][8],
                                             int (&U)[4], int (&V)[4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint8_t* py = f + (long long)(2 * cy + r) * S.pitch_y + (long long)(2 * cx0) * SB;
    if (nb == 4) {
      nr_get_samples<SB, 8>(py, Y[r], S.shift);
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) Y[r][x] = x < 2 * nb ? nr_get_one<SB>(py + x * SB, S.shift) : 0;
    }
  }
  const long long co = (long long)cy * S.pitch_c + (long long)cx0 * S.step;
  if (nb == 4 && S.inter) {
    const bool u_first = S.u_off < S.v_off;
    int uv[8];
    nr_get_samples<SB, 8>(f + (u_first ? S.u_off : S.v_off) + co, uv, S.shift);
#pragma unroll
    for (int j = 0; j < 4; ++j) U[j] = u_first ? uv[2 * j] : uv[2 * j + 1], V[j] = u_first ? uv[2 * j + 1] : uv[2 * j];
  } else if (nb == 4 && S.step == SB) {
    nr_get_samples<SB, 4>(f + S.u_off + co, U, S.shift);
    nr_get_samples<SB, 4>(f + S.v_off + co, V, S.shift);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      U[j] = j < nb ? nr_get_one<SB>(f + S.u_off + co + (long long)j * S.step, S.shift) : 0;
      V[j] = j < nb ? nr_get_one<SB>(f + S.v_off + co + (long long)j * S.step, S.shift) : 0;
    }
  }
}

__device__ __forceinline__ int nr_clamp(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }

// grid (destination frame, split of a frame's groups).  A group: chroma row cy, four chroma columns from cx0.
template <int SB>
__global__ __launch_bounds__(NR_THREADS) void bgr_to_yuv_kernel(const uint8_t* __restrict__ bgr, long long n, nr_surf D, nr_fwd M,
                                                                const long long* __restrict__ index) {
  constexpr int K = SB == 1 ? 0 : 2, TOP = (256 << K) - 1;
  const long long i = blockIdx.x;
  const long long r = index ? index[i] : i;
  if (r < 0 || r >= n) return;
  const uint8_t* s = bgr + r * ((long long)D.h * D.w * 3);
  uint8_t* f = D.base + i * D.stride;
  const int cw = D.w >> 1, ch = D.h >> 1, per_row = (cw + 3) >> 2, groups = ch * per_row;
  for (int g = blockIdx.y * NR_THREADS + threadIdx.x; g < groups; g += gridDim.y * NR_THREADS) {
    const int cy = g / per_row, cx0 = 4 * (g - cy * per_row);
    const int nb = cw - cx0 < 4 ? cw - cx0 : 4;
    int Y[2][8], U[4], V[4], sum_b[4] = {0, 0, 0, 0}, sum_g[4] = {0, 0, 0, 0}, sum_r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int row = 0; row < 2; ++row) {
      const uint8_t* p = s + ((long long)(2 * cy + row) * D.w + 2 * cx0) * 3;
      unsigned w[6] = {0, 0, 0, 0, 0, 0};
      if (nb == 4) {
        nr_load<24>(p, w);
      } else {
#pragma unroll
        for (int q = 0; q < 18; ++q)
          if (q < 6 * nb) w[q >> 2] |= (unsigned)p[q] << (8 * (q & 3));
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int B = (int)nr_byte(w, 3 * x), G = (int)nr_byte(w, 3 * x + 1), R = (int)nr_byte(w, 3 * x + 2);
        Y[row][x] = nr_clamp(((M.yb * B + M.yg * G + M.yr * R + (1 << (AVSR_SHIFT - 1 - K))) >> (AVSR_SHIFT - K)) + (M.y_off << K), TOP);
        sum_b[x >> 1] += B, sum_g[x >> 1] += G, sum_r[x >> 1] += R;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      U[j] = nr_clamp(((M.ub * sum_b[j] + M.ug * sum_g[j] + M.ur * sum_r[j] + (1 << (AVSR_SHIFT + 1 - K))) >> (AVSR_SHIFT + 2 - K)) +
                      (128 << K), TOP);
      V[j] = nr_clamp(((M.vb * sum_b[j] + M.vg * sum_g[j] + M.vr * sum_r[j] + (1 << (AVSR_SHIFT + 1 - K))) >> (AVSR_SHIFT + 2 - K)) +
                      (128 << K), TOP);
    }
    nr_put_group<SB>(D, f, cy, cx0, nb, Y, U, V);
  }
}

template <int SB>
__global__ __launch_bounds__(NR_THREADS) void repack_kernel(nr_surf S, nr_surf D, const long long* __restrict__ index) {
  const long long i = blockIdx.x;
  const long long r = index ? index[i] : i;
  if (r < 0 || r >= S.n) return;
  const uint8_t* s = S.base + r * S.stride;
  uint8_t* f = D.base + i * D.stride;
  const int cw = D.w >> 1, ch = D.h >> 1, per_row = (cw + 3) >> 2, groups = ch * per_row;
  for (int g = blockIdx.y * NR_THREADS + threadIdx.x; g < groups; g += gridDim.y * NR_THREADS) {
    const int cy = g / per_row, cx0 = 4 * (g - cy * per_row);
    const int nb = cw - cx0 < 4 ? cw - cx0 : 4;
    int Y[2][8], U[4], V[4];
    nr_get_group<SB>(S, s, cy, cx0, nb, Y, U, V);
    nr_put_group<SB>(D, f, cy, cx0, nb, Y, U, V);
  }
}

static dim3 nr_pixel_grid(const nr_surf& D, long long count) {
  const long long groups = (long long)(D.h / 2) * ((D.w / 2 + 3) / 4);
  long long by = nr_cdiv(groups, NR_THREADS);
  if (by > 65535) by = 65535;
  return dim3((unsigned)count, (unsigned)by);
}

extern "C" int avsr_bgr_to_yuv_u8(const uint8_t* d_bgr, int64_t n, uint8_t* d_dst, const int64_t* h_surface, const int* h_forward,
                                  const int64_t* d_index, int64_t count, avsr_stream_t stream) {
  nr_surf D;
  const int st = nr_surface_arg("avsr_bgr_to_yuv_u8", "destination", D, d_dst, h_surface);
  if (st != AVSR_OK) return st;
  AVSR_REQUIRE(h_forward, AVSR_E_ARG, "avsr_bgr_to_yuv_u8: h_forward is null");
  AVSR_REQUIRE(h_forward[0] >= 0 && h_forward[0] <= 255, AVSR_E_ARG, "avsr_bgr_to_yuv_u8: y_off %d outside 0 .. 255", h_forward[0]);
  for (int row = 0; row < 3; ++row) {
    long long sum = 0;
    for (int c = 0; c < 3; ++c) sum += h_forward[1 + 3 * row + c] < 0 ? -(long long)h_forward[1 + 3 * row + c] : h_forward[1 + 3 * row + c];
    AVSR_REQUIRE(sum <= AVSR_MAX_ROW_SUM, AVSR_E_ARG, "avsr_bgr_to_yuv_u8: row %d of the forward matrix sums to %lld in magnitude, "
                 "above 2^20", row, sum);
  }
  AVSR_REQUIRE(n >= 0 && n < (1ll << 31) && count >= 0 && count <= D.n, AVSR_E_SHAPE,
               "avsr_bgr_to_yuv_u8: n=%lld count=%lld, the destination holds %lld frames", (long long)n, (long long)count, D.n);
  AVSR_REQUIRE(d_index || count <= n, AVSR_E_SHAPE, "avsr_bgr_to_yuv_u8: count %lld above the %lld frames (no index)",
               (long long)count, (long long)n);
  if (count == 0) return AVSR_OK;
  AVSR_REQUIRE(d_bgr && d_dst, AVSR_E_ARG, "avsr_bgr_to_yuv_u8: null pointer");
  AVSR_REQUIRE(!nr_ranges_meet(d_bgr, n * (long long)D.h * D.w * 3, d_dst, D.n * D.stride), AVSR_E_SHAPE,
               "avsr_bgr_to_yuv_u8: the destination overlaps the source frames");
  const nr_fwd M{h_forward[0], h_forward[1], h_forward[2], h_forward[3], h_forward[4], h_forward[5], h_forward[6], h_forward[7],
                 h_forward[8], h_forward[9]};
  const long long* index = reinterpret_cast<const long long*>(d_index);
  if (D.sb == 1)
    hipLaunchKernelGGL((bgr_to_yuv_kernel<1>), nr_pixel_grid(D, count), dim3(NR_THREADS), 0, (hipStream_t)stream, d_bgr, (long long)n, D,
                       M, index);
  else
    hipLaunchKernelGGL((bgr_to_yuv_kernel<2>), nr_pixel_grid(D, count), dim3(NR_THREADS), 0, (hipStream_t)stream, d_bgr, (long long)n, D,
                       M, index);
  AVSR_CHECK_LAUNCH("avsr_bgr_to_yuv_u8");
  return AVSR_OK;
}

extern "C" int avsr_repack_u8(const uint8_t* d_src, const int64_t* h_src_surface, uint8_t* d_dst, const int64_t* h_dst_surface,
                              const int64_t* d_index, int64_t count, avsr_stream_t stream) {
  nr_surf S, D;
  int st = nr_surface_arg("avsr_repack_u8", "source", S, d_src, h_src_surface);
  if (st != AVSR_OK) return st;
  st = nr_surface_arg("avsr_repack_u8", "destination", D, d_dst, h_dst_surface);
  if (st != AVSR_OK) return st;
  AVSR_REQUIRE(S.h == D.h && S.w == D.w, AVSR_E_SHAPE, "avsr_repack_u8: source frames of %dx%d, destination frames of %dx%d", S.h,
               S.w, D.h, D.w);
  AVSR_REQUIRE(S.sb == D.sb, AVSR_E_UNSUPPORTED,
               "avsr_repack_u8: the depth differs (source samples of %d bytes, destination samples of %d): a repack copies samples",
               S.sb, D.sb);
  AVSR_REQUIRE(count >= 0 && count <= D.n, AVSR_E_SHAPE, "avsr_repack_u8: count=%lld, the destination holds %lld frames",
               (long long)count, D.n);
  AVSR_REQUIRE(d_index || count <= S.n, AVSR_E_SHAPE, "avsr_repack_u8: count %lld above the %lld frames (no index)",
               (long long)count, S.n);
  if (count == 0) return AVSR_OK;
  AVSR_REQUIRE(d_src && d_dst, AVSR_E_ARG, "avsr_repack_u8: null pointer");
  AVSR_REQUIRE(!nr_ranges_meet(d_src, S.n * S.stride, d_dst, D.n * D.stride), AVSR_E_SHAPE,
               "avsr_repack_u8: the destination overlaps the source frames");
  const long long* index = reinterpret_cast<const long long*>(d_index);
  if (D.sb == 1)
    hipLaunchKernelGGL((repack_kernel<1>), nr_pixel_grid(D, count), dim3(NR_THREADS), 0, (hipStream_t)stream, S, D, index);
  else
    hipLaunchKernelGGL((repack_kernel<2>), nr_pixel_grid(D, count), dim3(NR_THREADS), 0, (hipStream_t)stream, S, D, index);
  AVSR_CHECK_LAUNCH("avsr_repack_u8");
  return AVSR_OK;
}

// ---------------------------------------------------------------------------
// 3. Audio.
// ---------------------------------------------------------------------------
// the sample a frame boundary falls on: min((int64)floor((double)frame / fps * sr), len), never below 0
__device__ __forceinline__ long long nr_sample_of(long long frame, double fps, double sr, long long len) {
  const double x = floor((double)frame / fps * sr);
  long long a = x >= 9.2e18 ? len : (long long)x;   // (a conversion past int64 is not defined; such a bound is len anyway)
  if (!(x >= 0.0)) a = 0;                           // (NaN or negative: a bad fps must not become an address)
  return a < len ? a : len;
}

// ONE workgroup: per run (source start, destination start, length), run after run; then the per-video offsets
__global__ __launch_bounds__(NR_THREADS) void audio_bounds_kernel(const long long* __restrict__ wave_offsets, int nvideos,
                                                                  const double* __restrict__ fps, double sr,
                                                                  const long long* __restrict__ runs, long long run_cap,
                                                                  const long long* __restrict__ run_offsets,
                                                                  long long* __restrict__ work, long long* __restrict__ audio_offsets,
                                                                  long long* __restrict__ totals) {
  const long long nruns = run_offsets[nvideos] < run_cap ? run_offsets[nvideos] : run_cap;
  long long carry = 0;
  for (long long c = 0; c < nruns; c += NR_THREADS) {
    const long long r = c + threadIdx.x;
    long long len = 0, src = 0, unused = 0, total, total_unused;
    if (r < nruns) {
      int lo = 0, hi = nvideos;   // the video of run r: the last v with run_offsets[v] <= r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (run_offsets[mid] <= r)
          lo = mid;
        else
          hi = mid;
      }
      const long long track = wave_offsets[lo + 1] - wave_offsets[lo];
      const long long a = nr_sample_of(runs[2 * r], fps[lo], sr, track), b = nr_sample_of(runs[2 * r + 1], fps[lo], sr, track);
      len = b > a ? b - a : 0;
      src = wave_offsets[lo] + a;
    }
    const long long mine = len;
    nr_block_scan2(len, unused, total, total_unused);
    if (r < nruns)
      work[AVSR_AUDIO_COLS * r] = src, work[AVSR_AUDIO_COLS * r + 1] = carry + len, work[AVSR_AUDIO_COLS * r + 2] = mine;
    carry += total;
  }
  __threadfence_block();
  __syncthreads();
  for (int v = threadIdx.x; v <= nvideos; v += NR_THREADS) {
    const long long first = run_offsets[v];
    audio_offsets[v] = first < nruns ? work[AVSR_AUDIO_COLS * first + 1] : carry;
  }
  __threadfence_block();
  __syncthreads();
  for (int v = threadIdx.x; v < nvideos; v += NR_THREADS)
    totals[AVSR_TOTAL_COLS * (long long)v + 2] = audio_offsets[v + 1] - audio_offsets[v];
}

// workgroup g: output samples g * AVSR_AUDIO_TILE ..; a thread's samples are NR_THREADS apart (a wave's are adjacent)
__global__ __launch_bounds__(NR_THREADS) void audio_copy_kernel(const float* __restrict__ wave, int nvideos,
                                                                const long long* __restrict__ run_offsets, long long run_cap,
                                                                const long long* __restrict__ work,
                                                                const long long* __restrict__ audio_offsets, long long fade,
                                                                float* __restrict__ audio, long long sample_cap) {
  const long long total = audio_offsets[nvideos] < sample_cap ? audio_offsets[nvideos] : sample_cap;
  const long long first = (long long)blockIdx.x * AVSR_AUDIO_TILE;
  if (first >= total) return;
  const long long nruns = run_offsets[nvideos] < run_cap ? run_offsets[nvideos] : run_cap;
  long long run = -1, dst = 0, len = 0, src = 0;
  for (long long j = first + threadIdx.x; j < first + AVSR_AUDIO_TILE && j < total; j += NR_THREADS) {
    if (run < 0 || j >= dst + len) {   // the run of sample j: the last r with its destination start <= j
      long long lo = 0, hi = nruns;
      while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (work[AVSR_AUDIO_COLS * mid + 1] <= j)
          lo = mid;
        else
          hi = mid;
      }
      run = lo, src = work[AVSR_AUDIO_COLS * lo], dst = work[AVSR_AUDIO_COLS * lo + 1], len = work[AVSR_AUDIO_COLS * lo + 2];
    }
    const long long i = j - dst;
    if (i >= len) continue;   // (cannot happen for tables audio_bounds_kernel wrote; never read past a run)
    const long long f = fade < len / 2 ? fade : len / 2;
    float x = wave[src + i];
    if (i < f)
      x = x * ((float)(i + 1) / (float)(f + 1));
    else if (i >= len - f)
      x = x * ((float)(len - i) / (float)(f + 1));
    audio[j] = x;
  }
}

extern "C" int avsr_audio_cut(const float* d_wave, const int64_t* h_wave_offsets, const int64_t* d_wave_offsets, int nvideos,
                              const double* d_fps, double sr, int64_t fade, const int64_t* d_runs, int64_t run_cap,
                              const int64_t* d_run_offsets, int64_t* d_work, float* d_audio, int64_t sample_cap,
                              int64_t* d_audio_offsets, int64_t* d_totals, avsr_stream_t stream) {
  AVSR_REQUIRE(run_cap >= 1 && sample_cap >= 1 && run_cap < (1ll << 31), AVSR_E_ARG,
               "avsr_audio_cut: capacities must be at least 1 (run_cap below 2^31), got run_cap=%lld sample_cap=%lld",
               (long long)run_cap, (long long)sample_cap);
  AVSR_REQUIRE(fade >= 0, AVSR_E_ARG, "avsr_audio_cut: fade=%lld", (long long)fade);
  AVSR_REQUIRE(sr > 0.0 && sr < 1e12, AVSR_E_ARG, "avsr_audio_cut: sr=%g", sr);
  AVSR_REQUIRE(nvideos >= 1, AVSR_E_SHAPE, "avsr_audio_cut: nvideos=%d", nvideos);
  AVSR_REQUIRE(h_wave_offsets, AVSR_E_ARG, "avsr_audio_cut: h_wave_offsets is null");
  AVSR_REQUIRE(h_wave_offsets[0] == 0, AVSR_E_SHAPE, "avsr_audio_cut: the track offsets start at %lld", (long long)h_wave_offsets[0]);
  for (int v = 0; v < nvideos; ++v)
    AVSR_REQUIRE(h_wave_offsets[v + 1] >= h_wave_offsets[v], AVSR_E_SHAPE, "avsr_audio_cut: the track offsets decrease at video %d", v);
  const long long tiles = nr_cdiv(sample_cap, AVSR_AUDIO_TILE);
  AVSR_REQUIRE(tiles < (1ll << 31), AVSR_E_SHAPE, "avsr_audio_cut: sample_cap=%lld is too large", (long long)sample_cap);
  AVSR_REQUIRE(d_wave_offsets && d_fps && d_runs && d_run_offsets && d_work && d_audio && d_audio_offsets && d_totals &&
               (d_wave || h_wave_offsets[nvideos] == 0), AVSR_E_ARG, "avsr_audio_cut: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const long long* ro = reinterpret_cast<const long long*>(d_run_offsets);
  long long* work = reinterpret_cast<long long*>(d_work);
  long long* ao = reinterpret_cast<long long*>(d_audio_offsets);
  hipLaunchKernelGGL(audio_bounds_kernel, dim3(1), dim3(NR_THREADS), 0, s, reinterpret_cast<const long long*>(d_wave_offsets), nvideos,
                     d_fps, sr, reinterpret_cast<const long long*>(d_runs), (long long)run_cap, ro, work, ao,
                     reinterpret_cast<long long*>(d_totals));
  AVSR_CHECK_LAUNCH("avsr_audio_cut (bounds)");
  hipLaunchKernelGGL(audio_copy_kernel, dim3((unsigned)tiles), dim3(NR_THREADS), 0, s, d_wave, nvideos, ro, (long long)run_cap, work, ao,
                     (long long)fade, d_audio, (long long)sample_cap);
  AVSR_CHECK_LAUNCH("avsr_audio_cut (copy)");
  return AVSR_OK;
}
