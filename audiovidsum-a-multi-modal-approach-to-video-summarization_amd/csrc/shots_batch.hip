// Batched shot detection and frame sampling (SURVEY row F2 for a ragged batch of videos): the front half of stage 1 -
// features/shots.py and the sampling loop of features/extractors.py - for V videos in one set of launches, nothing read
// back before the tables are complete.  The videos are the segments [offsets[v], offsets[v + 1]) of the concatenated
// frames (the convention of FrameScoringPipeline); d_offsets is int64 [V + 1], starts at 0 and increases strictly
// (trusted: ops.ShotTables guarantees it).  Integers and fixed orders throughout: no atomics apart from the integer
// ones of the frame-difference sums, so two calls give the same bytes.
#include "avs_internal.h"
#include "pixel_bodies.h"

#define SB_THREADS 256
// most workgroups on grid x: a launch holds at most 2^32 - 1 threads per grid dimension (blocks x SB_THREADS)
#define SB_MAX_GRID_X (0xffffffffll / SB_THREADS)
#define SB_WORDS 64                   // mask words of one chunk: one per lane of the wave that walks them
#define SB_CHUNK (SB_WORDS * 64)      // frames of one chunk
#define SB_MAX_FRAMES AVS_SHOT_MAX_FRAMES   // features/extractors.py MAX_FRAMES (include/avsum_hip.h, as the next two)
#define SB_INTERVAL AVS_SHOT_INTERVAL       // FRAME_INTERVAL
#define SB_MICRO AVS_SHOT_MICRO_BATCH       // MICRO_BATCH

// ---------------------------------------------------------------------------
// 1. |dH|, |dS|, |dV| sums of every frame against the previous frame OF ITS VIDEO: hsv_diff_body (pixel_bodies.h), the
// one text hsv_frame_diff_kernel (visual.hip) runs too, with the frame on grid x (SB_MAX_GRID_X = 16 777 215 blocks)
// instead of y (65 535), and the first frame of every video left at zero.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SB_THREADS) void hsv_frame_diff_batch_kernel(const uint8_t* __restrict__ frames, int h, int w,
                                                                         int step, int ph, int pw,
                                                                         const long long* __restrict__ offsets, int nvideos,
                                                                         unsigned* __restrict__ sums) {
  const long long f = (long long)blockIdx.x + 1;  // frame f against frame f-1
  // the video of f: the last v with offsets[v] <= f (block-uniform; V + 1 offsets, all in cache after the first block)
  int lo = 0, hi = nvideos;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= f)
      lo = mid;
    else
      hi = mid;
  }
  if (offsets[lo] == f) return;  // a video's first frame: no predecessor, the memset's zeros stay
  const uint8_t* cur = frames + f * h * (long long)w * 3;
  const uint8_t* prv = cur - (long long)h * w * 3;
  hsv_diff_body<SB_THREADS>(bgr_dense_src{w}, cur, prv, step, ph, pw, blockIdx.y, gridDim.y, sums + f * 3);
}

extern "C" int avs_hsv_frame_diff_batch_u8(const uint8_t* d_frames, int64_t n, int h, int w, int step,
                                           const int64_t* d_offsets, int nvideos, uint32_t* d_sums, avs_stream_t stream) {
  AVS_REQUIRE(n >= 0 && h > 0 && w > 0 && step > 0 && nvideos >= 0, AVS_E_SHAPE, "avs_hsv_frame_diff_batch_u8: bad extents");
  if (n == 0) return AVS_OK;
  AVS_REQUIRE(nvideos > 0, AVS_E_SHAPE, "avs_hsv_frame_diff_batch_u8: %lld frames in no video", (long long)n);
  AVS_REQUIRE(d_frames && d_offsets && d_sums, AVS_E_ARG, "avs_hsv_frame_diff_batch_u8: null pointer");
  AVS_REQUIRE(n - 1 <= SB_MAX_GRID_X, AVS_E_SHAPE, "avs_hsv_frame_diff_batch_u8: at most %lld frames per call",
              SB_MAX_GRID_X + 1);
  const int ph = (h + step - 1) / step, pw = (w + step - 1) / step;  // len(range(0, h, step))
  AVS_REQUIRE((long long)ph * pw * 255 < (1ll << 32), AVS_E_SHAPE,
              "avs_hsv_frame_diff_batch_u8: frame too large for u32 sums");
  hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * 3 * (size_t)n, (hipStream_t)stream);
  if (e != hipSuccess) {
    avs_set_error("avs_hsv_frame_diff_batch_u8: memset failed: %s", hipGetErrorString(e));
    return AVS_E_HIP;
  }
  if (n == 1) return AVS_OK;
  int by = (int)avs_cdiv((long long)ph * pw, SB_THREADS * 8);  // the per-video entry point's split of a frame
  if (by < 1) by = 1;
  if (by > 64) by = 64;
  hipLaunchKernelGGL(hsv_frame_diff_batch_kernel, dim3((unsigned)(n - 1), by), dim3(SB_THREADS), 0, (hipStream_t)stream,
                     d_frames, h, w, step, ph, pw, reinterpret_cast<const long long*>(d_offsets), nvideos, d_sums);
  AVS_CHECK_LAUNCH("avs_hsv_frame_diff_batch_u8");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 2. content_scores + cuts_from_scores (features/shots.py) of every video, one workgroup per video.
// The score is the host's fp64 expression, operation for operation (this file is compiled with -ffp-contract=off and
// fp64 division is correctly rounded), so `score >= threshold` is the host's decision bit for bit.  The flags of a
// chunk of 4096 frames become 64 mask words in LDS (one ballot per 64 frames); wave 0 then applies the greedy rule -
// cut at the first flagged f with f - last >= min_scene_len, last = f - by jumping: lane l holds word l with the bits
// below `last + min_scene_len` cleared, a ballot finds the first non-empty word and a find-first-set its first bit.
// One step per CUT, not per frame; `last` is carried from chunk to chunk, so n is unbounded.
// ---------------------------------------------------------------------------
__device__ __forceinline__ long long sb_ceil3(long long x) { return (x + SB_INTERVAL - 1) / SB_INTERVAL; }
// frames sample_shot_indices(start, end) picks: the multiples of 3 in [start, end), at most 100
__device__ __forceinline__ int sb_shot_count(long long start, long long end) {
  const long long c = sb_ceil3(end) - sb_ceil3(start);
  return (int)(c < SB_MAX_FRAMES ? c : SB_MAX_FRAMES);
}

__global__ __launch_bounds__(SB_THREADS) void shot_cuts_batch_kernel(const unsigned* __restrict__ sums,
                                                                    const long long* __restrict__ offsets, double pixels,
                                                                    double threshold, int min_scene_len,
                                                                    const long long* __restrict__ cut_off,
                                                                    long long* __restrict__ cuts,
                                                                    long long* __restrict__ totals) {
  __shared__ unsigned long long mask[SB_WORDS];
  const int v = blockIdx.x;
  const long long base = offsets[v], n = offsets[v + 1] - base;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long* slot = cuts + cut_off[v];
  const long long cap = cut_off[v + 1] - cut_off[v];  // (n - 1) / min_scene_len: the greedy rule cannot place more
  // wave 0's state (wave-uniform): the last cut (0 before the first), the cuts so far, the closed shots' totals
  long long last = 0, ncuts = 0, nsample = 0, ngroup = 0;
  int maxc = 0;
  for (long long c0 = 0; c0 < n; c0 += SB_CHUNK) {
    for (int word = wave; word < SB_WORDS; word += SB_THREADS / 64) {
      const long long f = c0 + (long long)word * 64 + lane;
      bool flag = false;
      if (f >= 1 && f < n) {
        const unsigned* s = sums + (base + f) * 3;
        const double score = (((double)s[0] / pixels + (double)s[1] / pixels) + (double)s[2] / pixels) / 3.0;
        flag = score >= threshold;
      }
      const unsigned long long bits = __ballot(flag);
      if (lane == 0) mask[word] = bits;
    }
    __syncthreads();
    if (wave == 0) {
      const unsigned long long mine = mask[lane];
      for (;;) {
        const long long from = last + min_scene_len - c0;  // first chunk-relative frame that may be cut
        if (from >= SB_CHUNK) break;
        const long long lo = from > 0 ? from : 0;
        const int w0 = (int)(lo >> 6), b0 = (int)(lo & 63);
        const unsigned long long live =
            lane < w0 ? 0ull : (lane == w0 ? mine & (~0ull << b0) : mine);
        const unsigned long long any = __ballot(live != 0ull);
        if (any == 0ull || ncuts == cap) break;  // (the slot is full only if cut_off and min_scene_len disagree)
        const int w = __ffsll((long long)any) - 1;
        const unsigned long long word = __shfl(live, w, 64);
        const long long f = c0 + (long long)w * 64 + (__ffsll((long long)word) - 1);
        if (lane == 0) slot[ncuts] = f;
        const int c = sb_shot_count(last, f);  // the shot [last, f) is closed
        nsample += c;
        ngroup += (c + SB_MICRO - 1) / SB_MICRO;
        maxc = c > maxc ? c : maxc;
        ++ncuts;
        last = f;
      }
    }
    __syncthreads();  // the mask is rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    long long nshots = 0;
    if (ncuts > 0) {  // detect_shots: no cut, no shot; otherwise the tail [last, n) is the last shot
      const int c = sb_shot_count(last, n);
      nsample += c;
      ngroup += (c + SB_MICRO - 1) / SB_MICRO;
      maxc = c > maxc ? c : maxc;
      nshots = ncuts + 1;
    }
    totals[v * 4 + 0] = nshots;
    totals[v * 4 + 1] = nsample;
    totals[v * 4 + 2] = ngroup;
    totals[v * 4 + 3] = maxc;
  }
}

extern "C" int avs_shot_cuts_batch(const uint32_t* d_sums, int64_t n, const int64_t* d_offsets, int nvideos, double pixels,
                                   double threshold, int min_scene_len, const int64_t* d_cut_off, int64_t* d_cuts,
                                   int64_t* d_totals, avs_stream_t stream) {
  AVS_REQUIRE(n >= 0 && nvideos >= 0 && min_scene_len >= 1 && pixels > 0.0, AVS_E_SHAPE,
              "avs_shot_cuts_batch: n=%lld nvideos=%d min_scene_len=%d pixels=%g", (long long)n, nvideos, min_scene_len,
              pixels);
  if (nvideos == 0) return AVS_OK;
  AVS_REQUIRE(d_sums && d_offsets && d_cut_off && d_cuts && d_totals, AVS_E_ARG, "avs_shot_cuts_batch: null pointer");
  hipLaunchKernelGGL(shot_cuts_batch_kernel, dim3((unsigned)nvideos), dim3(SB_THREADS), 0, (hipStream_t)stream, d_sums,
                     reinterpret_cast<const long long*>(d_offsets), pixels, threshold, min_scene_len,
                     reinterpret_cast<const long long*>(d_cut_off), reinterpret_cast<long long*>(d_cuts),
                     reinterpret_cast<long long*>(d_totals));
  AVS_CHECK_LAUNCH("avs_shot_cuts_batch");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 3. The tables.  A one-workgroup exclusive scan of the V per-video totals (shots, sampled frames, micro-batch groups)
// gives every video its first row in each table and the batch totals; one workgroup per video then writes its rows.
// Both scans run in chunks of 256 with a carry: V and the shots of a video are unbounded.
// ---------------------------------------------------------------------------
// exclusive scan of one value per thread over the workgroup; `total` = the sum over all 256 threads
__device__ __forceinline__ long long sb_block_scan(long long x, long long* wave_sums, long long& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();  // wave_sums may still be read from the previous call
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  long long before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < SB_THREADS / 64; ++k) {
    const long long s = wave_sums[k];
    if (k < wave) before += s;
    total += s;
  }
  return before + inc - x;
}

// video_off: int64 [3, V + 1] = the exclusive scans of (shots, sampled frames, groups); plane 0 IS shot_offsets
__global__ __launch_bounds__(SB_THREADS) void shot_scan_kernel(const long long* __restrict__ totals, int nvideos,
                                                              long long* __restrict__ video_off,
                                                              long long* __restrict__ sample_offsets, long long shot_cap,
                                                              long long* __restrict__ group_offsets, long long group_cap,
                                                              long long* __restrict__ counts) {
  __shared__ long long wave_sums[SB_THREADS / 64];
  long long carry[3] = {0, 0, 0};
  int maxc = 0;
  for (int v0 = 0; v0 < nvideos; v0 += SB_THREADS) {
    const int v = v0 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long x = v < nvideos ? totals[v * 4 + k] : 0;
      long long total;
      const long long ex = sb_block_scan(x, wave_sums, total);
      if (v < nvideos) video_off[(long long)k * (nvideos + 1) + v] = carry[k] + ex;
      carry[k] += total;
    }
    if (v < nvideos) maxc = max(maxc, (int)totals[v * 4 + 3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxc = max(maxc, __shfl_xor(maxc, o, 64));
  __shared__ int wave_max[SB_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = maxc;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) video_off[(long long)k * (nvideos + 1) + nvideos] = carry[k];
    counts[0] = carry[0];
    counts[1] = carry[1];
    counts[2] = carry[2];
    counts[3] = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    // the closing entries of the two row-offset tables (their other entries come from the videos' workgroups)
    if (carry[0] <= shot_cap) sample_offsets[carry[0]] = carry[1];
    if (carry[2] <= group_cap) group_offsets[carry[2]] = carry[1];
  }
}

__global__ __launch_bounds__(SB_THREADS) void shot_tables_fill_kernel(
    const long long* __restrict__ offsets, int nvideos, const long long* __restrict__ cut_off,
    const long long* __restrict__ cuts, const long long* __restrict__ video_off, long long* __restrict__ shots,
    long long shot_cap, long long* __restrict__ sample_offsets, long long* __restrict__ sample_index, long long sample_cap,
    long long* __restrict__ group_offsets, long long group_cap) {
  __shared__ long long wave_sums[SB_THREADS / 64];
  __shared__ long long s_first[SB_THREADS];   // per shot of the chunk: its first sampled frame (row of the batch),
  __shared__ long long s_row[SB_THREADS];     // its first row of the sampled tensor,
  __shared__ long long s_group[SB_THREADS];   // its first group,
  __shared__ int s_count[SB_THREADS];         // and its sampled frames
  const int v = blockIdx.x;
  const long long base = offsets[v], n = offsets[v + 1] - base;
  const long long shot0 = video_off[v], nshots = video_off[v + 1] - shot0;
  long long row = video_off[(long long)(nvideos + 1) + v];          // carried: first sampled row of the chunk
  long long group = video_off[2ll * (nvideos + 1) + v];             // carried: first group of the chunk
  const long long* slot = cuts + cut_off[v];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long j0 = 0; j0 < nshots; j0 += SB_THREADS) {
    const long long j = j0 + threadIdx.x;
    const bool live = j < nshots;
    long long start = 0, end = 0;
    int c = 0;
    if (live) {
      start = j == 0 ? 0 : slot[j - 1];
      end = j == nshots - 1 ? n : slot[j];
      c = sb_shot_count(start, end);
    }
    long long total_c, total_g;
    const long long ex_c = sb_block_scan(c, wave_sums, total_c);
    const long long ex_g = sb_block_scan((c + SB_MICRO - 1) / SB_MICRO, wave_sums, total_g);
    s_first[threadIdx.x] = base + SB_INTERVAL * sb_ceil3(start);
    s_row[threadIdx.x] = row + ex_c;
    s_group[threadIdx.x] = group + ex_g;
    s_count[threadIdx.x] = c;
    if (live && shot0 + j < shot_cap) {
      shots[(shot0 + j) * 2] = start;
      shots[(shot0 + j) * 2 + 1] = end;
      sample_offsets[shot0 + j] = row + ex_c;
    }
    __syncthreads();
    // the rows of the chunk's shots, a wave per shot: at most 100 sampled frames and 25 groups each
    const int in_chunk = (int)(nshots - j0 < SB_THREADS ? nshots - j0 : SB_THREADS);
    for (int s = wave; s < in_chunk; s += SB_THREADS / 64) {
      const int cnt = s_count[s];
      const long long first = s_first[s], r0 = s_row[s], g0 = s_group[s];
      for (int k = lane; k < cnt; k += 64)
        if (r0 + k < sample_cap) sample_index[r0 + k] = first + (long long)SB_INTERVAL * k;
      const int ng = (cnt + SB_MICRO - 1) / SB_MICRO;
      if (lane < ng && g0 + lane < group_cap) group_offsets[g0 + lane] = r0 + (long long)SB_MICRO * lane;
    }
    row += total_c;
    group += total_g;
    __syncthreads();  // the chunk's LDS rows are rewritten by the next chunk
  }
}

extern "C" int avs_shot_tables_fill(const int64_t* d_offsets, int nvideos, const int64_t* d_cut_off, const int64_t* d_cuts,
                                    const int64_t* d_totals, int64_t* d_video_off, int64_t* d_shots, int64_t shot_cap,
                                    int64_t* d_sample_offsets, int64_t* d_sample_index, int64_t sample_cap,
                                    int64_t* d_group_offsets, int64_t group_cap, int64_t* d_counts, avs_stream_t stream) {
  AVS_REQUIRE(nvideos > 0 && shot_cap >= 0 && sample_cap >= 0 && group_cap >= 0, AVS_E_SHAPE,
              "avs_shot_tables_fill: nvideos=%d capacities %lld %lld %lld", nvideos, (long long)shot_cap,
              (long long)sample_cap, (long long)group_cap);
  AVS_REQUIRE(d_offsets && d_cut_off && d_cuts && d_totals && d_video_off && d_shots && d_sample_offsets && d_sample_index &&
                  d_group_offsets && d_counts,
              AVS_E_ARG, "avs_shot_tables_fill: null pointer");
  typedef long long* LP;
  typedef const long long* CLP;
  hipLaunchKernelGGL(shot_scan_kernel, dim3(1), dim3(SB_THREADS), 0, (hipStream_t)stream, (CLP)d_totals, nvideos,
                     (LP)d_video_off, (LP)d_sample_offsets, (long long)shot_cap, (LP)d_group_offsets, (long long)group_cap,
                     (LP)d_counts);
  AVS_CHECK_LAUNCH("avs_shot_tables_fill (scan)");
  hipLaunchKernelGGL(shot_tables_fill_kernel, dim3((unsigned)nvideos), dim3(SB_THREADS), 0, (hipStream_t)stream,
                     (CLP)d_offsets, nvideos, (CLP)d_cut_off, (CLP)d_cuts, (CLP)d_video_off, (LP)d_shots, (long long)shot_cap,
                     (LP)d_sample_offsets, (LP)d_sample_index, (long long)sample_cap, (LP)d_group_offsets,
                     (long long)group_cap);
  AVS_CHECK_LAUNCH("avs_shot_tables_fill");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 4. out[i] = src[index[i]] for rows of row_bytes, i < *d_count: the row count is read from DEVICE memory (the sampled
// frame total the scan wrote), the grid is sized by the host's capacity and the surplus blocks exit.  1 B read, 1 B
// written per byte: bound by HBM.  A row is cut into pieces of 256 lanes x 4 units, dealt to the row's workgroups; in a
// whole piece a lane keeps its four loads in flight before the first store, as pull_copy_kernel does.  The unit is 16
// bytes where the row size and both bases allow it, else 4 bytes, else 1.  A row whose index lies outside src is
// skipped (never read).
// ---------------------------------------------------------------------------
#define GR_INFLIGHT 4
template <typename T>
__global__ __launch_bounds__(SB_THREADS) void gather_rows_kernel(const T* __restrict__ src, long long src_rows,
                                                                const long long* __restrict__ index,
                                                                const long long* __restrict__ count, long long units,
                                                                T* __restrict__ out) {
  const long long i = blockIdx.x;
  if (i >= *count) return;
  const long long r = index[i];
  if (r < 0 || r >= src_rows) return;
  const T* s = src + r * units;
  T* d = out + i * units;
  const long long piece = SB_THREADS * GR_INFLIGHT;
  for (long long p0 = (long long)blockIdx.y * piece; p0 < units; p0 += (long long)gridDim.y * piece) {
    const long long u = p0 + threadIdx.x;
    if (p0 + piece <= units) {
      const T a = s[u], b = s[u + SB_THREADS], c = s[u + 2 * SB_THREADS], e = s[u + 3 * SB_THREADS];
      d[u] = a;
      d[u + SB_THREADS] = b;
      d[u + 2 * SB_THREADS] = c;
      d[u + 3 * SB_THREADS] = e;
    } else {
#pragma unroll
      for (int k = 0; k < GR_INFLIGHT; ++k)
        if (u + k * SB_THREADS < units) d[u + k * SB_THREADS] = s[u + k * SB_THREADS];
    }
  }
}

template <typename T>
static void gather_rows_launch(const void* src, int64_t src_rows, const int64_t* index, const int64_t* count, int64_t cap,
                               int64_t row_bytes, void* out, hipStream_t stream) {
  const long long units = row_bytes / (long long)sizeof(T);
  long long gy = avs_cdiv(units, SB_THREADS * GR_INFLIGHT);
  if (gy > 64) gy = 64;
  hipLaunchKernelGGL(gather_rows_kernel<T>, dim3((unsigned)cap, (unsigned)gy), dim3(SB_THREADS), 0, stream,
                     reinterpret_cast<const T*>(src), (long long)src_rows, reinterpret_cast<const long long*>(index),
                     reinterpret_cast<const long long*>(count), units, reinterpret_cast<T*>(out));
}

extern "C" int avs_gather_rows_u8(const uint8_t* d_src, int64_t src_rows, int64_t row_bytes, const int64_t* d_index,
                                  const int64_t* d_count, int64_t capacity, uint8_t* d_out, avs_stream_t stream) {
  AVS_REQUIRE(src_rows >= 0 && row_bytes > 0 && capacity >= 0 && capacity <= SB_MAX_GRID_X, AVS_E_SHAPE,
              "avs_gather_rows_u8: src_rows=%lld row_bytes=%lld capacity=%lld", (long long)src_rows, (long long)row_bytes,
              (long long)capacity);
  if (capacity == 0) return AVS_OK;
  AVS_REQUIRE(d_src && d_index && d_count && d_out, AVS_E_ARG, "avs_gather_rows_u8: null pointer");
  const uintptr_t both = (uintptr_t)d_src | (uintptr_t)d_out;
  if (row_bytes % 16 == 0 && (both & 15u) == 0)
    gather_rows_launch<uint4>(d_src, src_rows, d_index, d_count, capacity, row_bytes, d_out, (hipStream_t)stream);
  else if (row_bytes % 4 == 0 && (both & 3u) == 0)
    gather_rows_launch<uint32_t>(d_src, src_rows, d_index, d_count, capacity, row_bytes, d_out, (hipStream_t)stream);
  else
    gather_rows_launch<uint8_t>(d_src, src_rows, d_index, d_count, capacity, row_bytes, d_out, (hipStream_t)stream);
  AVS_CHECK_LAUNCH("avs_gather_rows_u8");
  return AVS_OK;
}
