// Keyshot summaries of a ragged batch of videos: per-shot value sums, one 0/1 knapsack per (score row, video) and the
// overlap counts the summary F1 reduces to.  There is no counterpart in the reference; the definitions are
// those of evaluation/keyshots.py, whose numpy oracle the kernels equal bit for bit.  Every result is an integer or an
// fp64 value that a fixed recurrence defines: no float atomics, nothing depends on the launch geometry.
//
// The videos are segments [offsets[v], offsets[v + 1]) of the concatenated frames; video v's shots are the entries
// shot_offsets[v] .. shot_offsets[v + 1] of the [shot_cap, 2] table of video-relative (start, end) pairs, the layout
// avs_shot_tables_fill writes.  The offsets and capacities are trusted (ops.SummaryTables builds them); the shot table
// may come from the device, so every shot is clipped to its video and every index is kept inside its buffer.
#include "avs_internal.h"

#define SM_SUM_THREADS 256                   // four waves, one (row, shot) each
#define SM_KNAP_THREADS 1024
#define SM_SHOT_CHUNK 1024                   // shots whose (weight, value) are staged in LDS at a time
#define SM_MAX_CAPACITY AVS_SUMMARY_MAX_CAPACITY   // what ops.SummaryTables refuses above (include/avsum_hip.h)
#define SM_CELLS (SM_MAX_CAPACITY + 1)       // the two fp64 rows of capacity + 1 cells are 128 KiB of the CU's 160 KiB
#define SM_OV_THREADS 256
#define SM_MAX_GRID_Y 65535

// q(x) = rint(clamp(x, 0, 1) * 2^32): the product is exact in fp64, rint rounds half to even; NaN fails x > 0 and maps to 0
__device__ __forceinline__ long long sm_quantise(float x) {
  double d = (double)x;
  d = d > 0.0 ? d : 0.0;
  d = d < 1.0 ? d : 1.0;
  return (long long)rint(d * 4294967296.0);
}

// the video of global shot g: the v with shot_offsets[v] <= g < shot_offsets[v + 1], or -1
__device__ __forceinline__ int sm_video_of_shot(const long long* __restrict__ shot_offsets, int nvideos, long long g) {
  if (g < shot_offsets[0] || g >= shot_offsets[nvideos]) return -1;
  int lo = 0, hi = nvideos;                  // shot_offsets[lo] <= g < shot_offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (shot_offsets[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// shot (s, e) clipped to a video of n frames: 0 <= s <= e <= n
__device__ __forceinline__ void sm_clip(long long& s, long long& e, long long n) {
  s = s < 0 ? 0 : (s > n ? n : s);
  e = e < s ? s : (e > n ? n : e);
}

// ---------------------------------------------------------------------------
// 1. sums[k, g] = sum of q(scores[k, base_v + r]) over the frames r of shot g.  One wave per (k, shot): the lanes up
// to the first 16-byte boundary take one score each, then every lane takes 16 bytes (a wave reads whole lines), then
// the up to three last scores.  int64 sums, so the lane order does not matter.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SM_SUM_THREADS) void shot_value_sums_kernel(const float* __restrict__ scores, long long ld,
                                                                         const long long* __restrict__ offsets, int nvideos,
                                                                         const long long* __restrict__ shot_offsets,
                                                                         const long long* __restrict__ shots,
                                                                         long long shot_cap, long long* __restrict__ sums) {
  const int lane = threadIdx.x & (AVS_WAVE - 1);
  const long long g = (long long)blockIdx.x * (SM_SUM_THREADS / AVS_WAVE) + (threadIdx.x >> 6);
  const long long k = blockIdx.y;
  if (g >= shot_cap) return;
  const int v = sm_video_of_shot(shot_offsets, nvideos, g);
  long long acc = 0;
  if (v >= 0) {
    const long long base = offsets[v], n = offsets[v + 1] - base;
    long long s = shots[2 * g], e = shots[2 * g + 1];
    sm_clip(s, e, n);
    const float* p = scores + k * ld + base + s;
    const long long w = e - s;
    long long head = (4 - (long long)((((uintptr_t)p) >> 2) & 3)) & 3;
    if (head > w) head = w;
    if (lane < head) acc += sm_quantise(p[lane]);
    const long long nvec = (w - head) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    for (long long i = lane; i < nvec; i += AVS_WAVE) {
      const float4 x = p4[i];
      acc += sm_quantise(x.x) + sm_quantise(x.y) + sm_quantise(x.z) + sm_quantise(x.w);
    }
    const long long done = head + 4 * nvec;
    if (lane < w - done) acc += sm_quantise(p[done + lane]);
#pragma unroll
    for (int off = AVS_WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, AVS_WAVE);
  }
  if (lane == 0) sums[k * shot_cap + g] = acc;   // (0 for the entries past the last shot)
}

extern "C" int avs_shot_value_sums(const float* d_scores, int64_t ld_scores, int nrows, int64_t n,
                                   const int64_t* d_offsets, int nvideos, const int64_t* d_shot_offsets,
                                   const int64_t* d_shots, int64_t shot_cap, int64_t* d_sums, avs_stream_t stream) {
  AVS_REQUIRE(nrows >= 0 && nrows <= SM_MAX_GRID_Y && n >= 0 && nvideos >= 1 && ld_scores >= n && shot_cap >= 1 &&
                  shot_cap <= 0x7fffffffLL, AVS_E_SHAPE,
              "avs_shot_value_sums: nrows=%d n=%lld ld=%lld nvideos=%d shot_cap=%lld", nrows, (long long)n,
              (long long)ld_scores, nvideos, (long long)shot_cap);
  if (nrows == 0) return AVS_OK;
  AVS_REQUIRE(d_scores && d_offsets && d_shot_offsets && d_shots && d_sums, AVS_E_ARG,
              "avs_shot_value_sums: null pointer");
  typedef const long long* CLP;
  const unsigned gx = (unsigned)avs_cdiv(shot_cap, SM_SUM_THREADS / AVS_WAVE);
  hipLaunchKernelGGL(shot_value_sums_kernel, dim3(gx, (unsigned)nrows), dim3(SM_SUM_THREADS), 0, (hipStream_t)stream,
                     d_scores, (long long)ld_scores, (CLP)d_offsets, nvideos, (CLP)d_shot_offsets, (CLP)d_shots,
                     (long long)shot_cap, (long long*)d_sums);
  AVS_CHECK_LAUNCH("avs_shot_value_sums");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 2. The knapsack of one (score row k, video v) per workgroup of 1024 threads.  Both fp64 rows live in LDS; thread t
// owns the cells t, t + 1024, ..: consecutive lanes read consecutive 8-byte cells at w and at w - w_i (an unaligned
// shift of the row, still one cell per lane and so without bank conflicts).  A cell reads two cells of the previous row
// only, so the result does not depend on the split.  One barrier per shot that fits; a shot heavier than the capacity
// changes nothing and costs none.  The (weight, value) of up to 1024 shots are staged in LDS ahead of the row loop, so
// a step waits for no global load.  The take bits of shot i are the wave ballots, one uint64 word per 64 cells, in row
// shot_offsets[v] + i of the workspace [K][shot_cap][words].  Thread 0 backtracks from w = capacity; all threads then
// paint the mask: every frame of the video is written, 0 first and 1 over the picked shots.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SM_KNAP_THREADS) void knapsack_batch_kernel(
    const long long* __restrict__ sums, long long n_total, const long long* __restrict__ offsets,
    const long long* __restrict__ capacity, int nvideos, const long long* __restrict__ shot_offsets,
    const long long* __restrict__ shots, long long shot_cap, unsigned long long* __restrict__ take, int words,
    unsigned char* __restrict__ picked, unsigned char* __restrict__ mask, double* __restrict__ optimum,
    long long* __restrict__ totals) {
  __shared__ double rows[2][SM_CELLS];
  __shared__ double shot_val[SM_SHOT_CHUNK];
  __shared__ int shot_w[SM_SHOT_CHUNK];
  const int tid = threadIdx.x;
  const int v = blockIdx.x;
  const long long k = blockIdx.y;
  const long long base = offsets[v], n = offsets[v + 1] - base;
  long long cap = capacity[v];
  const long long cell_limit = (long long)words * 64 < SM_CELLS ? (long long)words * 64 : SM_CELLS;
  if (cap > cell_limit - 1) cap = cell_limit - 1;   // (never: the plan sizes words by the largest capacity, at most 8191)
  if (cap < 0) cap = 0;
  const int C = (int)cap;
  const int nw = (C + 64) >> 6;                     // words that hold the cells 0 .. C
  long long g0 = shot_offsets[v], g1 = shot_offsets[v + 1];
  if (g0 < 0) g0 = 0;
  if (g1 > shot_cap) g1 = shot_cap;
  const long long S = g1 > g0 ? g1 - g0 : 0;
  const long long* ksums = sums + k * shot_cap;
  unsigned long long* ktake = take + k * shot_cap * (long long)words;
  unsigned char* kpicked = picked + k * shot_cap;
  unsigned char* kmask = mask + k * n_total + base;

  for (int w = tid; w <= C; w += SM_KNAP_THREADS) rows[0][w] = 0.0;
  int cur = 0;
  for (long long c0 = 0; c0 < S; c0 += SM_SHOT_CHUNK) {
    const int cn = (int)(S - c0 < SM_SHOT_CHUNK ? S - c0 : SM_SHOT_CHUNK);
    __syncthreads();                                // the row is zeroed / the last chunk's table is no longer read
    if (tid < cn) {
      const long long g = g0 + c0 + tid;
      long long s = shots[2 * g], e = shots[2 * g + 1];
      sm_clip(s, e, n);
      const long long wi = e - s;
      shot_w[tid] = (int)(wi > 0x7fffffffLL ? 0x7fffffffLL : wi);
      shot_val[tid] = wi >= 1 ? (double)ksums[g] / (double)wi : 0.0;
    }
    __syncthreads();
    for (int i = 0; i < cn; ++i) {
      const int wi = shot_w[i];
      unsigned long long* trow = ktake + (g0 + c0 + i) * (long long)words;
      if (wi < 1 || wi > C) {                       // never taken (uniform over the workgroup): the row stays
        for (int j = tid; j < nw; j += SM_KNAP_THREADS) trow[j] = 0ull;
        continue;
      }
      const double val = shot_val[i];
      const double* prev = rows[cur];
      double* next = rows[cur ^ 1];
      for (int w = tid; w < nw * 64; w += SM_KNAP_THREADS) {   // (whole waves: w >> 6 is uniform over a wave)
        bool t = false;
        if (w <= C) {
          const double keep = prev[w];
          double out = keep;
          if (w >= wi) {
            const double cand = prev[w - wi] + val;
            t = cand > keep;
            if (t) out = cand;
          }
          next[w] = out;
        }
        const unsigned long long bits = __ballot(t);
        if ((tid & (AVS_WAVE - 1)) == 0) trow[w >> 6] = bits;
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  __syncthreads();                                  // the last row, the zero row of S = 0 and the take bits are visible

  // backtrack: thread 0 carries w; the weights come through LDS a chunk at a time, the last chunk first
  int w = C;
  long long nsel = 0, nframes = 0;
  for (long long c0 = S > 0 ? ((S - 1) / SM_SHOT_CHUNK) * SM_SHOT_CHUNK : -1; c0 >= 0; c0 -= SM_SHOT_CHUNK) {
    const int cn = (int)(S - c0 < SM_SHOT_CHUNK ? S - c0 : SM_SHOT_CHUNK);
    __syncthreads();
    if (tid < cn) {
      const long long g = g0 + c0 + tid;
      long long s = shots[2 * g], e = shots[2 * g + 1];
      sm_clip(s, e, n);
      const long long wi = e - s;
      shot_w[tid] = (int)(wi > 0x7fffffffLL ? 0x7fffffffLL : wi);
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = cn - 1; i >= 0; --i) {
        const int wi = shot_w[i];
        const long long g = g0 + c0 + i;
        unsigned char pick = 0;
        if (wi >= 1 && wi <= w) pick = (unsigned char)((ktake[g * (long long)words + (w >> 6)] >> (w & 63)) & 1ull);
        if (pick) {
          w -= wi;
          ++nsel;
          nframes += wi;
        }
        kpicked[g] = pick;
      }
    }
  }
  if (tid == 0) {
    optimum[k * nvideos + v] = rows[cur][C];
    long long* t3 = totals + 3 * (k * nvideos + v);
    t3[0] = nsel;
    t3[1] = nframes;
    t3[2] = capacity[v];
  }
  for (long long f = tid; f < n; f += SM_KNAP_THREADS) kmask[f] = 0;
  __syncthreads();                                  // the zeros and thread 0's picked flags before the ones
  for (long long i = tid >> 6; i < S; i += SM_KNAP_THREADS / AVS_WAVE) {
    const long long g = g0 + i;
    if (!kpicked[g]) continue;
    long long s = shots[2 * g], e = shots[2 * g + 1];
    sm_clip(s, e, n);
    for (long long f = s + (tid & (AVS_WAVE - 1)); f < e; f += AVS_WAVE) kmask[f] = 1;
  }
}

extern "C" int avs_knapsack_batch_f64(const int64_t* d_sums, int nrows, int64_t n, const int64_t* d_offsets,
                                      const int64_t* d_capacity, int nvideos, int max_capacity,
                                      const int64_t* d_shot_offsets, const int64_t* d_shots, int64_t shot_cap,
                                      uint64_t* d_take, int words, uint8_t* d_picked, uint8_t* d_mask,
                                      double* d_optimum, int64_t* d_totals, avs_stream_t stream) {
  AVS_REQUIRE(nrows >= 0 && nrows <= SM_MAX_GRID_Y && n >= 0 && nvideos >= 1 && shot_cap >= 1 &&
                  shot_cap <= 0x7fffffffLL, AVS_E_SHAPE, "avs_knapsack_batch_f64: nrows=%d n=%lld nvideos=%d shot_cap=%lld",
              nrows, (long long)n, nvideos, (long long)shot_cap);
  AVS_REQUIRE(max_capacity >= 0 && max_capacity <= SM_MAX_CAPACITY, AVS_E_SHAPE,
              "avs_knapsack_batch_f64: a capacity of %d exceeds the LDS-resident limit %d", max_capacity, SM_MAX_CAPACITY);
  AVS_REQUIRE(words >= 1 && (int64_t)words * 64 >= (int64_t)max_capacity + 1, AVS_E_SHAPE,
              "avs_knapsack_batch_f64: %d take words per shot do not hold %d + 1 cells", words, max_capacity);
  if (nrows == 0) return AVS_OK;
  AVS_REQUIRE(d_sums && d_offsets && d_capacity && d_shot_offsets && d_shots && d_take && d_picked && d_optimum &&
                  d_totals && (n == 0 || d_mask), AVS_E_ARG, "avs_knapsack_batch_f64: null pointer");
  typedef const long long* CLP;
  const dim3 grid((unsigned)nvideos, (unsigned)nrows), block(SM_KNAP_THREADS);
  hipLaunchKernelGGL(knapsack_batch_kernel, grid, block, 0, (hipStream_t)stream, (CLP)d_sums, (long long)n, (CLP)d_offsets,
                     (CLP)d_capacity, nvideos, (CLP)d_shot_offsets, (CLP)d_shots, (long long)shot_cap,
                     (unsigned long long*)d_take, words, d_picked, d_mask, d_optimum, (long long*)d_totals);
  AVS_CHECK_LAUNCH("avs_knapsack_batch_f64");
  return AVS_OK;
}

// ---------------------------------------------------------------------------
// 3. counts[v, u] = (tp, n_pred, n_user) over the frames of video v: the sums of pred & user, pred and user, a mask
// byte counting as 1 when it is not 0.  One workgroup per (video, user); integer sums, any order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SM_OV_THREADS) void mask_overlap_counts_kernel(const unsigned char* __restrict__ pred,
                                                                            const unsigned char* __restrict__ users,
                                                                            long long ld_user,
                                                                            const long long* __restrict__ offsets,
                                                                            int nusers, long long* __restrict__ counts) {
  __shared__ long long red[3][SM_OV_THREADS];
  const int v = blockIdx.x, u = blockIdx.y;
  const long long a = offsets[v], b = offsets[v + 1];
  const unsigned char* um = users + (long long)u * ld_user;
  long long tp = 0, np = 0, nu = 0;
  for (long long r = a + threadIdx.x; r < b; r += SM_OV_THREADS) {
    const int p = pred[r] != 0, q = um[r] != 0;
    tp += p & q;
    np += p;
    nu += q;
  }
  red[0][threadIdx.x] = tp;
  red[1][threadIdx.x] = np;
  red[2][threadIdx.x] = nu;
  __syncthreads();
  for (int w = SM_OV_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) counts[3 * ((long long)v * nusers + u) + threadIdx.x] = red[threadIdx.x][0];
}

extern "C" int avs_mask_overlap_counts(const uint8_t* d_pred_mask, const uint8_t* d_user_masks, int64_t ld_user,
                                       int nusers, int64_t n, const int64_t* d_offsets, int nvideos, int64_t* d_counts,
                                       avs_stream_t stream) {
  AVS_REQUIRE(nusers >= 0 && nusers <= SM_MAX_GRID_Y && n >= 0 && nvideos >= 1 && ld_user >= n, AVS_E_SHAPE,
              "avs_mask_overlap_counts: nusers=%d n=%lld ld=%lld nvideos=%d", nusers, (long long)n, (long long)ld_user,
              nvideos);
  if (nusers == 0) return AVS_OK;
  AVS_REQUIRE(d_offsets && d_counts && (n == 0 || (d_pred_mask && d_user_masks)), AVS_E_ARG,
              "avs_mask_overlap_counts: null pointer");
  hipLaunchKernelGGL(mask_overlap_counts_kernel, dim3((unsigned)nvideos, (unsigned)nusers), dim3(SM_OV_THREADS), 0,
                     (hipStream_t)stream, d_pred_mask, d_user_masks, (long long)ld_user, (const long long*)d_offsets, nusers,
                     (long long*)d_counts);
  AVS_CHECK_LAUNCH("avs_mask_overlap_counts");
  return AVS_OK;
}
