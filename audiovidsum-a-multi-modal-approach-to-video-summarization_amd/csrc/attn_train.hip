// libavsum_attn.so: multi-head self-attention over a ragged batch of sequences, forward and fused backward
// (include/avsum_attn.h).  This file is the whole library; of libavsum_hip.so it shares one header, mhsa_flash_body.h,
// the body of the exact-fp32 fused forward, so that a sequence's ctx has the same bits through either library.
//
// The two gradient kernels.  At head dim 256 a wave that owned a 32-row tile outright would need 256 operand registers
// and 256 accumulators, the whole register file, so the workgroup's NW waves (2 at D = 64, else 4) each take a slice of
// DS = D / NW head-dim columns (32, 32, 64):
//
//   dK/dV kernel: the workgroup owns 32 keys of one (sequence, head) and sweeps the sequence's query tiles.
//     registers   the wave's slice of its 32 K and V rows as MFMA B fragments (2 * DS/2 per lane), its slice of
//                 dK^T and dV^T as accumulators (2 * DS/2)
//     LDS         the Q and dO tiles of the sweep (32 x D each, pitch D + 1), lse and delta of their 32 queries
//     per tile    partial S[q][key] = Q . K^T and dP[q][key] = dO . V^T over the wave's slice (A = the LDS tile, lane =
//                 query row; B = the register fragments); the NW partial 32 x 32 tiles go through LDS and EVERY wave
//                 adds them in the same order w = 0, 1, .., so every wave holds the same bits of S and dP;
//                 P = exp(S / sqrt(D) - lse), dS = P (dP - delta) / sqrt(D), zero for phantom queries and keys;
//                 dV^T[d][key] += dO^T . P and dK^T[d][key] += Q^T . dS with the tile in the accumulator registers as
//                 the MFMA B operand (it sums over the accumulator's ROW index, here the query) and A = the LDS tile
//                 read along d: no data moves between the products.
//   dQ kernel: the mirror image.  The workgroup owns 32 queries and sweeps the key tiles; Q and dO slices are the
//     register fragments, the K and V tiles are in LDS, S^T[key][q] and dP^T[key][q] have the query on the lane (one
//     lse and one delta per lane), dQ^T[d][q] += K^T . dS^T.
//
// Each output element is accumulated by one wave in one fixed order that depends on the sequence's length only, and
// stored once (transposed through LDS into 16-byte row stores): no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/avsum_attn.h"
#include "mhsa_flash_body.h"

static_assert(AVSA_FWD_TILE == 128 && AVSA_BWD_TILE == 32 && AVSA_TILE_COLS == 2, "tile sizes the kernels are written for");

static thread_local char g_err[512] = "";

static void avsa_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define AVSA_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      avsa_set_error(__VA_ARGS__);    \
      return (code);                  \
    }                                 \
  } while (0)

#define AVSA_CHECK_LAUNCH(name)                                                  \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      avsa_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e__)); \
      return AVSA_E_HIP;                                                         \
    }                                                                            \
  } while (0)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// register e of lane half lh of a 32x32 accumulator tile is the tile's row (e & 3) + 8 * (e >> 2) + 4 * lh
#define AVSA_ACC_ROW(e, lh) (((e) & 3) + 8 * ((e) >> 2) + 4 * (lh))

// ------------------------------------------------------------------------------------------------------- forward
// a workgroup's rows by the (sequence, tile) table
struct avsa_rows_range {
  const int64_t* offsets;
  const int32_t* tiles;
  int nseq;
  __device__ __forceinline__ bool resolve(long long& first_row, int& t, int& q_tile0) const {
    const int seq = tiles[AVSA_TILE_COLS * (long long)blockIdx.x];
    const int tile = tiles[AVSA_TILE_COLS * (long long)blockIdx.x + 1];
    if (seq < 0 || seq >= nseq || tile < 0) return false;
    first_row = offsets[seq];
    const long long len = offsets[seq + 1] - first_row;
    t = (int)len;
    q_tile0 = tile * AVSA_FWD_TILE;
    return (long long)tile * AVSA_FWD_TILE < len;
  }
};

template <int D>
__global__ __launch_bounds__(256, 1) void avsa_rows_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, long long ld,
                                                               const int64_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ tiles, int nseq, float sqrt_d,
                                                               float* __restrict__ ctx, long long ldo,
                                                               float* __restrict__ lse, int heads) {
  flash_mhsa_body<D, AVSA_FWD_TILE / 32, true, D / 2>(avsa_rows_range{offsets, tiles, nseq}, q, k, v, ld, sqrt_d, ctx, ldo, lse,
                                               heads);
}

// --------------------------------------------------------------------------------------------------------- delta
template <int D>
__global__ __launch_bounds__(256) void avsa_rows_delta_kernel(const float* __restrict__ dctx, long long lddo,
                                                              const float* __restrict__ ctx, long long ldo,
                                                              long long row_lo, long long npairs, int heads,
                                                              float* __restrict__ delta) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long p = (long long)blockIdx.x * 4 + wave; p < npairs; p += (long long)gridDim.x * 4) {
    const long long r = row_lo + p / heads;
    const int h = (int)(p % heads);
    const float* a = dctx + r * lddo + h * D;
    const float* b = ctx + r * ldo + h * D;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 64) acc += a[d + lane] * b[d + lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) delta[r * heads + h] = acc;
  }
}

// ------------------------------------------------------------------------------------------- the gradient kernels
template <int D>
struct avsa_bwd_shape {
  static constexpr int NW = D == 64 ? 2 : 4;     // waves of a workgroup
  static constexpr int DS = D / NW;              // head-dim columns of a wave's slice: 32, 32, 64
  static constexpr int NT = DS / 32;             // 32-wide d tiles of a wave's accumulators
  static constexpr int KP = D + 1;               // pitch of an operand tile in LDS
  static constexpr int PART = 2 * 16 * 64;       // floats of one wave's two partial tiles
};

// x / sqrt(D).  At D = 64 and 256 sqrt(D) is a power of two and the product with its reciprocal is the same bits as the
// correctly rounded division, which costs ten instructions; at D = 128 the division stays (the forward divides too).
template <int D>
__device__ __forceinline__ float avsa_unscale(float x, float sqrt_d, float inv_sqrt_d) {
  return D == 128 ? x / sqrt_d : x * inv_sqrt_d;
}

// rows r0 .. r0 + 31 of a sequence (zero past its end), columns h*D .. of two [rows, ld*] operands -> two LDS tiles
template <int D, int NTH>
__device__ __forceinline__ void avsa_stage_pair(const float* __restrict__ a, long long lda, const float* __restrict__ b,
                                                long long ldb, long long row0, int r0, int T, int h, float* as,
                                                float* bs) {
  constexpr int KP = D + 1;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < 32 * (D / 4); idx += NTH) {
    const int lrow = idx / (D / 4), c = 4 * (idx - lrow * (D / 4));
    const bool ok = r0 + lrow < T;
    const long long r = row0 + (ok ? r0 + lrow : 0);
    const float4 av = ok ? *reinterpret_cast<const float4*>(a + r * lda + h * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bv = ok ? *reinterpret_cast<const float4*>(b + r * ldb + h * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float* ad = as + lrow * KP + c;
    float* bd = bs + lrow * KP + c;
    ad[0] = av.x; ad[1] = av.y; ad[2] = av.z; ad[3] = av.w;
    bd[0] = bv.x; bd[1] = bv.y; bd[2] = bv.z; bd[3] = bv.w;
  }
}

// an LDS tile [32][D] (pitch D + 1) -> rows r0 .. of a sequence, 16-byte stores, rows past the end skipped
template <int D, int NTH>
__device__ __forceinline__ void avsa_store_tile(const float* ts, float* __restrict__ out, long long ldg, long long row0,
                                                int r0, int T, int h) {
  constexpr int KP = D + 1;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < 32 * (D / 4); idx += NTH) {
    const int lrow = idx / (D / 4), c = 4 * (idx - lrow * (D / 4));
    if (r0 + lrow < T) {
      const float* s = ts + lrow * KP + c;
      *reinterpret_cast<float4*>(out + (row0 + r0 + lrow) * ldg + h * D + c) = make_float4(s[0], s[1], s[2], s[3]);
    }
  }
}

// the wave's two partial tiles -> LDS; after the barrier every wave adds all NW partials in the order w = 0, 1, ..
template <int NW>
__device__ __forceinline__ void avsa_exchange(float* part, int wave, int lane, f32x16& s, f32x16& p) {
  constexpr int PART = 2 * 16 * 64;
  float* mine = part + wave * PART;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    mine[e * 64 + lane] = s[e];
    mine[1024 + e * 64 + lane] = p[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    float ss = part[e * 64 + lane], pp = part[1024 + e * 64 + lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      ss += part[w * PART + e * 64 + lane];
      pp += part[w * PART + 1024 + e * 64 + lane];
    }
    s[e] = ss;
    p[e] = pp;
  }
}

template <int D>
__global__ __launch_bounds__(64 * avsa_bwd_shape<D>::NW, 1) void avsa_rows_dkv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ld,
    const float* __restrict__ dctx, long long lddo, const float* __restrict__ lse, const float* __restrict__ delta,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ tiles, int nseq, int heads, float sqrt_d,
    float* __restrict__ dk, float* __restrict__ dv, long long ldg) {
  typedef avsa_bwd_shape<D> SH;
  constexpr int NW = SH::NW, DS = SH::DS, NT = SH::NT, KP = SH::KP, NTH = 64 * NW;
  __shared__ float qs[32 * KP];
  __shared__ float dos[32 * KP];
  __shared__ float part[NW * SH::PART];
  __shared__ float lss[32];
  __shared__ float dls[32];

  const int seq = tiles[AVSA_TILE_COLS * (long long)blockIdx.x];
  const int tile = tiles[AVSA_TILE_COLS * (long long)blockIdx.x + 1];
  if (seq < 0 || seq >= nseq || tile < 0) return;
  const long long row0 = offsets[seq];
  const long long len = offsets[seq + 1] - row0;
  if ((long long)tile * AVSA_BWD_TILE >= len) return;
  const int T = (int)len, k0 = tile * AVSA_BWD_TILE;

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lj = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y;
  const int d0 = wave * DS;
  const float inv_sqrt_d = 1.f / sqrt_d;
  const bool key_ok = k0 + lj < T;

  // the wave's slice of this lane's key row of K and V, as B fragments (reduction index 2s + lh)
  float kreg[DS / 2], vreg[DS / 2];
  {
    const long long roff = (row0 + (key_ok ? k0 + lj : 0)) * ld + h * D + d0 + lh;
#pragma unroll
    for (int s = 0; s < DS / 2; ++s) {
      kreg[s] = key_ok ? k[roff + 2 * s] : 0.f;
      vreg[s] = key_ok ? v[roff + 2 * s] : 0.f;
    }
  }
  f32x16 dkacc[NT], dvacc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) dkacc[i][e] = dvacc[i][e] = 0.f;

  for (int q0 = 0; q0 < T; q0 += 32) {
    __syncthreads();   // the previous tile, its partials and its lse / delta are no longer read
    avsa_stage_pair<D, NTH>(q, ld, dctx, lddo, row0, q0, T, h, qs, dos);
    if (t < 32) {
      const bool ok = q0 + t < T;
      const long long r = (row0 + (ok ? q0 + t : 0)) * heads + h;
      lss[t] = ok ? lse[r] : 0.f;
      dls[t] = ok ? delta[r] : 0.f;
    }
    __syncthreads();

    // partial S[query][key] and dP[query][key] over the wave's slice
    f32x16 sacc, pacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = pacc[e] = 0.f;
    const float* qrow_p = qs + lj * KP + d0 + lh;
    const float* dorow_p = dos + lj * KP + d0 + lh;
#pragma unroll
    for (int s = 0; s < DS / 2; ++s) {
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow_p[2 * s], kreg[s], sacc, 0, 0, 0);
      pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow_p[2 * s], vreg[s], pacc, 0, 0, 0);
    }
    avsa_exchange<NW>(part, wave, lane, sacc, pacc);

    // P and dS; a phantom query row or key column contributes nothing
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int qi = AVSA_ACC_ROW(e, lh);
      const bool ok = key_ok && q0 + qi < T;
      const float pe = ok ? expf(avsa_unscale<D>(sacc[e], sqrt_d, inv_sqrt_d) - lss[qi]) : 0.f;
      sacc[e] = pe;
      pacc[e] = avsa_unscale<D>(pe * (pacc[e] - dls[qi]), sqrt_d, inv_sqrt_d);
    }

    // dV^T[d][key] += sum_q dO[q][d] P[q][key];  dK^T[d][key] += sum_q Q[q][d] dS[q][key]
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int qi = AVSA_ACC_ROW(e, lh);
      const float* dorow = dos + qi * KP + d0 + lj;
      const float* qrow = qs + qi * KP + d0 + lj;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        dvacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow[32 * i], sacc[e], dvacc[i], 0, 0, 0);
        dkacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[32 * i], pacc[e], dkacc[i], 0, 0, 0);
      }
    }
  }

  // dK^T, dV^T (d rows in registers, key on the lane) -> LDS [key][d] -> rows of dK, dV
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int dd = d0 + 32 * i + AVSA_ACC_ROW(e, lh);
      qs[lj * KP + dd] = dkacc[i][e];
      dos[lj * KP + dd] = dvacc[i][e];
    }
  __syncthreads();
  avsa_store_tile<D, NTH>(qs, dk, ldg, row0, k0, T, h);
  avsa_store_tile<D, NTH>(dos, dv, ldg, row0, k0, T, h);
}

template <int D>
__global__ __launch_bounds__(64 * avsa_bwd_shape<D>::NW, 1) void avsa_rows_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long ld,
    const float* __restrict__ dctx, long long lddo, const float* __restrict__ lse, const float* __restrict__ delta,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ tiles, int nseq, int heads, float sqrt_d,
    float* __restrict__ dq, long long ldg) {
  typedef avsa_bwd_shape<D> SH;
  constexpr int NW = SH::NW, DS = SH::DS, NT = SH::NT, KP = SH::KP, NTH = 64 * NW;
  __shared__ float ks[32 * KP];
  __shared__ float vs[32 * KP];
  __shared__ float part[NW * SH::PART];

  const int seq = tiles[AVSA_TILE_COLS * (long long)blockIdx.x];
  const int tile = tiles[AVSA_TILE_COLS * (long long)blockIdx.x + 1];
  if (seq < 0 || seq >= nseq || tile < 0) return;
  const long long row0 = offsets[seq];
  const long long len = offsets[seq + 1] - row0;
  if ((long long)tile * AVSA_BWD_TILE >= len) return;
  const int T = (int)len, q0 = tile * AVSA_BWD_TILE;

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lj = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y;
  const int d0 = wave * DS;
  const float inv_sqrt_d = 1.f / sqrt_d;
  const bool q_ok = q0 + lj < T;

  // the wave's slice of this lane's query row of Q and dO, as B fragments; the row's lse and delta
  float qreg[DS / 2], doreg[DS / 2];
  const long long qr = row0 + (q_ok ? q0 + lj : 0);
  {
    const float* qp = q + qr * ld + h * D + d0 + lh;
    const float* dp = dctx + qr * lddo + h * D + d0 + lh;
#pragma unroll
    for (int s = 0; s < DS / 2; ++s) {
      qreg[s] = q_ok ? qp[2 * s] : 0.f;
      doreg[s] = q_ok ? dp[2 * s] : 0.f;
    }
  }
  const float lrow = q_ok ? lse[qr * heads + h] : 0.f;
  const float drow = q_ok ? delta[qr * heads + h] : 0.f;
  f32x16 dqacc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) dqacc[i][e] = 0.f;

  for (int k0 = 0; k0 < T; k0 += 32) {
    __syncthreads();   // the previous tile and its partials are no longer read
    avsa_stage_pair<D, NTH>(k, ld, v, ld, row0, k0, T, h, ks, vs);
    __syncthreads();

    // partial S^T[key][query] and dP^T[key][query] over the wave's slice
    f32x16 sacc, pacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = pacc[e] = 0.f;
    const float* krow_p = ks + lj * KP + d0 + lh;
    const float* vrow_p = vs + lj * KP + d0 + lh;
#pragma unroll
    for (int s = 0; s < DS / 2; ++s) {
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(krow_p[2 * s], qreg[s], sacc, 0, 0, 0);
      pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow_p[2 * s], doreg[s], pacc, 0, 0, 0);
    }
    avsa_exchange<NW>(part, wave, lane, sacc, pacc);

    // dS^T; a phantom key row or query column contributes nothing
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool ok = q_ok && k0 + AVSA_ACC_ROW(e, lh) < T;
      const float pe = ok ? expf(avsa_unscale<D>(sacc[e], sqrt_d, inv_sqrt_d) - lrow) : 0.f;
      pacc[e] = avsa_unscale<D>(pe * (pacc[e] - drow), sqrt_d, inv_sqrt_d);
    }

    // dQ^T[d][query] += sum_key K[key][d] dS^T[key][query]
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float* krow = ks + AVSA_ACC_ROW(e, lh) * KP + d0 + lj;
#pragma unroll
      for (int i = 0; i < NT; ++i)
        dqacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[32 * i], pacc[e], dqacc[i], 0, 0, 0);
    }
  }

  __syncthreads();
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) ks[lj * KP + d0 + 32 * i + AVSA_ACC_ROW(e, lh)] = dqacc[i][e];
  __syncthreads();
  avsa_store_tile<D, NTH>(ks, dq, ldg, row0, q0, T, h);
}

// ------------------------------------------------------------------------------------------------------ the host
static inline bool avsa_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline bool avsa_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// The batch description every entry point takes: the host offsets, the heads.  tile > 0: *ntiles_want = the rows the
// (sequence, tile) table of that tile size has.
static int avsa_check_batch(const char* who, const int64_t* h_offsets, int nseq, int heads, int head_dim, int tile,
                            int64_t* ntiles_want, int64_t* row_lo, int64_t* row_hi) {
  AVSA_REQUIRE(nseq >= 1, AVSA_E_ARG, "%s: nseq = %d, a batch holds at least one sequence", who, nseq);
  AVSA_REQUIRE(h_offsets != nullptr, AVSA_E_ARG, "%s: h_offsets is null", who);
  AVSA_REQUIRE(heads >= 1 && heads <= AVSA_MAX_HEADS, AVSA_E_SHAPE, "%s: heads = %d, must be 1..%d", who, heads,
               AVSA_MAX_HEADS);
  AVSA_REQUIRE(head_dim == 64 || head_dim == 128 || head_dim == 256, AVSA_E_SHAPE,
               "%s: head_dim = %d, must be 64, 128 or 256", who, head_dim);
  AVSA_REQUIRE(h_offsets[0] >= 0, AVSA_E_SHAPE, "%s: negative row offset %lld", who, (long long)h_offsets[0]);
  int64_t ntiles = 0;
  for (int s = 0; s < nseq; ++s) {
    // (the comparison first: offsets that lie far apart must not overflow the difference)
    AVSA_REQUIRE(h_offsets[s + 1] > h_offsets[s], AVSA_E_SHAPE,
                 "%s: sequence %d is empty (offsets %lld, %lld): every sequence needs at least one row", who, s,
                 (long long)h_offsets[s], (long long)h_offsets[s + 1]);
    AVSA_REQUIRE(h_offsets[s + 1] <= (int64_t)AVSA_MAX_ROWS, AVSA_E_SHAPE,
                 "%s: the offsets reach %lld, the kernels take fewer than 2^31 rows", who, (long long)h_offsets[s + 1]);
    if (tile > 0) ntiles += (h_offsets[s + 1] - h_offsets[s] + tile - 1) / tile;
  }
  if (ntiles_want) *ntiles_want = ntiles;
  *row_lo = h_offsets[0];
  *row_hi = h_offsets[nseq];
  return AVSA_OK;
}

static int avsa_check_stride(const char* who, const char* name, int64_t ld, int heads, int head_dim) {
  AVSA_REQUIRE(ld >= (int64_t)heads * head_dim && ld % 4 == 0, AVSA_E_SHAPE,
               "%s: row stride %s = %lld must be a multiple of 4 floats and at least heads * head_dim = %lld", who, name,
               (long long)ld, (long long)heads * head_dim);
  return AVSA_OK;
}

static int avsa_check_tiles(const char* who, const int32_t* d_tiles, int64_t ntiles, int64_t want) {
  AVSA_REQUIRE(ntiles == want, AVSA_E_SHAPE, "%s: ntiles = %lld, the offsets give %lld tiles", who, (long long)ntiles,
               (long long)want);
  AVSA_REQUIRE(want <= INT32_MAX, AVSA_E_SHAPE, "%s: %lld tiles, a launch takes at most 2^31 - 1", who, (long long)want);
  AVSA_REQUIRE(d_tiles != nullptr, AVSA_E_ARG, "%s: null pointer (d_tiles)", who);
  AVSA_REQUIRE(avsa_aligned4(d_tiles), AVSA_E_ALIGN, "%s: d_tiles is not 4-byte aligned", who);
  return AVSA_OK;
}

#define AVSA_TRY(call)            \
  do {                            \
    const int st__ = (call);      \
    if (st__ != AVSA_OK) return st__; \
  } while (0)

extern "C" int avsa_abi_version(void) { return AVSA_ABI_VERSION; }

extern "C" const char* avsa_last_error(void) { return g_err; }

extern "C" int avsa_mhsa_rows_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld,
                                      const int64_t* h_offsets, const int64_t* d_offsets, int nseq,
                                      const int32_t* d_tiles, int64_t ntiles, int heads, int head_dim, float* d_ctx,
                                      int64_t ldo, float* d_lse, avsa_stream_t stream) {
  const char* who = "avsa_mhsa_rows_fwd_f32";
  int64_t want = 0, lo = 0, hi = 0;
  AVSA_TRY(avsa_check_batch(who, h_offsets, nseq, heads, head_dim, AVSA_FWD_TILE, &want, &lo, &hi));
  AVSA_TRY(avsa_check_stride(who, "ld", ld, heads, head_dim));
  AVSA_TRY(avsa_check_stride(who, "ldo", ldo, heads, head_dim));
  AVSA_TRY(avsa_check_tiles(who, d_tiles, ntiles, want));
  AVSA_REQUIRE(d_q && d_k && d_v && d_ctx && d_lse && d_offsets, AVSA_E_ARG, "%s: null pointer", who);
  AVSA_REQUIRE(avsa_aligned16(d_q) && avsa_aligned16(d_k) && avsa_aligned16(d_v) && avsa_aligned16(d_ctx), AVSA_E_ALIGN,
               "%s: q, k, v and ctx must be 16-byte aligned", who);
  AVSA_REQUIRE(avsa_aligned4(d_lse) && (((uintptr_t)d_offsets) & 7u) == 0, AVSA_E_ALIGN,
               "%s: lse / d_offsets not aligned to their elements", who);
  const dim3 grid((unsigned)want, (unsigned)heads);
  const float sq = sqrtf((float)head_dim);
#define AVSA_FWD_LAUNCH(DD)                                                                                          \
  hipLaunchKernelGGL((avsa_rows_fwd_kernel<DD>), grid, dim3(256), 0, (hipStream_t)stream, d_q, d_k, d_v, (long long)ld, \
                     d_offsets, d_tiles, nseq, sq, d_ctx, (long long)ldo, d_lse, heads)
  if (head_dim == 64) AVSA_FWD_LAUNCH(64);
  else if (head_dim == 128) AVSA_FWD_LAUNCH(128);
  else AVSA_FWD_LAUNCH(256);
#undef AVSA_FWD_LAUNCH
  AVSA_CHECK_LAUNCH(who);
  return AVSA_OK;
}

extern "C" int avsa_mhsa_rows_delta_f32(const float* d_dctx, int64_t lddo, const float* d_ctx, int64_t ldo,
                                        const int64_t* h_offsets, int nseq, int heads, int head_dim, float* d_delta,
                                        avsa_stream_t stream) {
  const char* who = "avsa_mhsa_rows_delta_f32";
  int64_t lo = 0, hi = 0;
  AVSA_TRY(avsa_check_batch(who, h_offsets, nseq, heads, head_dim, 0, nullptr, &lo, &hi));
  AVSA_TRY(avsa_check_stride(who, "lddo", lddo, heads, head_dim));
  AVSA_TRY(avsa_check_stride(who, "ldo", ldo, heads, head_dim));
  AVSA_REQUIRE(d_dctx && d_ctx && d_delta, AVSA_E_ARG, "%s: null pointer", who);
  AVSA_REQUIRE(avsa_aligned16(d_dctx) && avsa_aligned16(d_ctx), AVSA_E_ALIGN, "%s: dctx and ctx must be 16-byte aligned",
               who);
  AVSA_REQUIRE(avsa_aligned4(d_delta), AVSA_E_ALIGN, "%s: delta is not 4-byte aligned", who);
  const long long npairs = (long long)(hi - lo) * heads;
  const long long groups = (npairs + 3) / 4;
  const dim3 grid((unsigned)(groups < AVSA_DELTA_GROUPS ? groups : AVSA_DELTA_GROUPS));
#define AVSA_DELTA_LAUNCH(DD)                                                                                      \
  hipLaunchKernelGGL((avsa_rows_delta_kernel<DD>), grid, dim3(256), 0, (hipStream_t)stream, d_dctx, (long long)lddo, \
                     d_ctx, (long long)ldo, (long long)lo, npairs, heads, d_delta)
  if (head_dim == 64) AVSA_DELTA_LAUNCH(64);
  else if (head_dim == 128) AVSA_DELTA_LAUNCH(128);
  else AVSA_DELTA_LAUNCH(256);
#undef AVSA_DELTA_LAUNCH
  AVSA_CHECK_LAUNCH(who);
  return AVSA_OK;
}

// what the two gradient entry points check alike
static int avsa_check_grad(const char* who, const float* d_q, const float* d_k, const float* d_v, int64_t ld,
                           const float* d_dctx, int64_t lddo, const float* d_lse, const float* d_delta,
                           const int64_t* h_offsets, const int64_t* d_offsets, int nseq, const int32_t* d_tiles,
                           int64_t ntiles, int heads, int head_dim, int64_t ldg, int64_t* want) {
  int64_t lo = 0, hi = 0;
  AVSA_TRY(avsa_check_batch(who, h_offsets, nseq, heads, head_dim, AVSA_BWD_TILE, want, &lo, &hi));
  AVSA_TRY(avsa_check_stride(who, "ld", ld, heads, head_dim));
  AVSA_TRY(avsa_check_stride(who, "lddo", lddo, heads, head_dim));
  AVSA_TRY(avsa_check_stride(who, "ldg", ldg, heads, head_dim));
  AVSA_TRY(avsa_check_tiles(who, d_tiles, ntiles, *want));
  AVSA_REQUIRE(d_q && d_k && d_v && d_dctx && d_lse && d_delta && d_offsets, AVSA_E_ARG, "%s: null pointer", who);
  AVSA_REQUIRE(avsa_aligned16(d_q) && avsa_aligned16(d_k) && avsa_aligned16(d_v) && avsa_aligned16(d_dctx), AVSA_E_ALIGN,
               "%s: q, k, v and dctx must be 16-byte aligned", who);
  AVSA_REQUIRE(avsa_aligned4(d_lse) && avsa_aligned4(d_delta) && (((uintptr_t)d_offsets) & 7u) == 0, AVSA_E_ALIGN,
               "%s: lse / delta / d_offsets not aligned to their elements", who);
  return AVSA_OK;
}

extern "C" int avsa_mhsa_rows_dkv_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld,
                                      const float* d_dctx, int64_t lddo, const float* d_lse, const float* d_delta,
                                      const int64_t* h_offsets, const int64_t* d_offsets, int nseq,
                                      const int32_t* d_tiles, int64_t ntiles, int heads, int head_dim, float* d_dk,
                                      float* d_dv, int64_t ldg, avsa_stream_t stream) {
  const char* who = "avsa_mhsa_rows_dkv_f32";
  int64_t want = 0;
  AVSA_TRY(avsa_check_grad(who, d_q, d_k, d_v, ld, d_dctx, lddo, d_lse, d_delta, h_offsets, d_offsets, nseq, d_tiles,
                           ntiles, heads, head_dim, ldg, &want));
  AVSA_REQUIRE(d_dk && d_dv, AVSA_E_ARG, "%s: null pointer (dk, dv)", who);
  AVSA_REQUIRE(avsa_aligned16(d_dk) && avsa_aligned16(d_dv), AVSA_E_ALIGN, "%s: dk and dv must be 16-byte aligned", who);
  const dim3 grid((unsigned)want, (unsigned)heads);
  const float sq = sqrtf((float)head_dim);
#define AVSA_DKV_LAUNCH(DD)                                                                                         \
  hipLaunchKernelGGL((avsa_rows_dkv_kernel<DD>), grid, dim3(64 * avsa_bwd_shape<DD>::NW), 0, (hipStream_t)stream, d_q, \
                     d_k, d_v, (long long)ld, d_dctx, (long long)lddo, d_lse, d_delta, d_offsets, d_tiles, nseq, heads, \
                     sq, d_dk, d_dv, (long long)ldg)
  if (head_dim == 64) AVSA_DKV_LAUNCH(64);
  else if (head_dim == 128) AVSA_DKV_LAUNCH(128);
  else AVSA_DKV_LAUNCH(256);
#undef AVSA_DKV_LAUNCH
  AVSA_CHECK_LAUNCH(who);
  return AVSA_OK;
}

extern "C" int avsa_mhsa_rows_dq_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld,
                                     const float* d_dctx, int64_t lddo, const float* d_lse, const float* d_delta,
                                     const int64_t* h_offsets, const int64_t* d_offsets, int nseq,
                                     const int32_t* d_tiles, int64_t ntiles, int heads, int head_dim, float* d_dq,
                                     int64_t ldg, avsa_stream_t stream) {
  const char* who = "avsa_mhsa_rows_dq_f32";
  int64_t want = 0;
  AVSA_TRY(avsa_check_grad(who, d_q, d_k, d_v, ld, d_dctx, lddo, d_lse, d_delta, h_offsets, d_offsets, nseq, d_tiles,
                           ntiles, heads, head_dim, ldg, &want));
  AVSA_REQUIRE(d_dq, AVSA_E_ARG, "%s: null pointer (dq)", who);
  AVSA_REQUIRE(avsa_aligned16(d_dq), AVSA_E_ALIGN, "%s: dq must be 16-byte aligned", who);
  const dim3 grid((unsigned)want, (unsigned)heads);
  const float sq = sqrtf((float)head_dim);
#define AVSA_DQ_LAUNCH(DD)                                                                                          \
  hipLaunchKernelGGL((avsa_rows_dq_kernel<DD>), grid, dim3(64 * avsa_bwd_shape<DD>::NW), 0, (hipStream_t)stream, d_q, \
                     d_k, d_v, (long long)ld, d_dctx, (long long)lddo, d_lse, d_delta, d_offsets, d_tiles, nseq, heads, \
                     sq, d_dq, (long long)ldg)
  if (head_dim == 64) AVSA_DQ_LAUNCH(64);
  else if (head_dim == 128) AVSA_DQ_LAUNCH(128);
  else AVSA_DQ_LAUNCH(256);
#undef AVSA_DQ_LAUNCH
  AVSA_CHECK_LAUNCH(who);
  return AVSA_OK;
}
