// The body of the exact-fp32 fused attention forward, shared by flash_mhsa_kernel (attention.hip: a dense (b, t) batch)
// and avsa_rows_fwd_kernel (attn_train.hip: a ragged batch of sequences).  The two differ only in WHERE a workgroup's
// rows lie, which is the template parameter RANGE:
//
//   bool RANGE::resolve(long long& first_row, int& T, int& q_tile0) const
//       the first row of the workgroup's sequence in the [rows, ld] operands, the sequence's length and the first
//       query (sequence-relative) of the workgroup's 32 * NW queries; false = the workgroup has nothing to do.
//
// and in one extra store: LSE = true writes L = m + log(l), the row's log-sum-exp of the scaled scores, to
// lse[row * heads + h] (what the backward kernels rebuild the probabilities from).  Everything a query's arithmetic
// consists of - the key tiles of 32 from the sequence's first key, the order of the products, the online rescaling -
// is this one text, so a sequence has the same ctx bits through either kernel, and the wave count NW (which only
// moves the staging loop's stride) does not enter it.
//
// SUNR is the unroll count of the S^T product's loop over D / 2 steps.  flash_mhsa_kernel keeps its 16: at D = 128 and
// 256 the loop then stays a loop, the Q fragments are indexed by its counter and the compiler keeps them in scratch
// (272 / 528 bytes per lane), which is how that kernel has been built and measured.  The ragged forward passes D / 2:
// the loop disappears, the fragments are registers and the kernel has no scratch.  The order of the products, and
// with it every result bit, is the same.
//
// The scheme (see attention.hip's head comment): everything TRANSPOSED so that a query lives on a lane;
// S^T = K . Q^T with A = K tile from LDS and B = the wave's Q rows in registers; online softmax per lane with one
// xor-32 shuffle; O^T += V^T . P with the S^T accumulator as the MFMA B operand.
#ifndef AVS_MHSA_FLASH_BODY_H
#define AVS_MHSA_FLASH_BODY_H

#include <hip/hip_runtime.h>
#include <math.h>

typedef float avs_flash_f32x16 __attribute__((ext_vector_type(16)));

template <int D, int NW, bool LSE, int SUNR, class RANGE>
__device__ __forceinline__ void flash_mhsa_body(const RANGE& range, const float* __restrict__ q,
                                                const float* __restrict__ k, const float* __restrict__ v, long long ld,
                                                float sqrt_d, float* __restrict__ ctx, long long ldo,
                                                float* __restrict__ lse, int heads) {
  typedef avs_flash_f32x16 f32x16;
  constexpr int KP = D + 1;          // K tile pitch (floats)
  constexpr int DT = D / 32;         // 32-wide d tiles of the output
  constexpr int OP = 33;             // output staging pitch
  __shared__ float ks[32 * KP];
  __shared__ float vs[32 * D];
  __shared__ float os[NW][32 * OP];

  long long boff;                    // first row of this sequence
  int T, q_tile0;
  if (!range.resolve(boff, T, q_tile0)) return;   // (workgroup-uniform)

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lj = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y;
  const int q0 = q_tile0 + wave * 32;
  const int qrow = q0 + lj;
  const bool q_ok = qrow < T;

  // this lane's query row, the half of its D entries that its lane half feeds to the MFMA (k = 2s + lh)
  float qreg[D / 2];
  {
    const float* qp = q + (boff + (q_ok ? qrow : 0)) * ld + h * D;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) qreg[s] = q_ok ? qp[2 * s + lh] : 0.f;
  }
  f32x16 oacc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[i][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < T; k0 += 32) {
    __syncthreads();  // the previous tile is no longer read
    // staging: float4 per thread, D/4 of them per key row, 32 rows
#pragma unroll 4
    for (int idx = t; idx < 32 * (D / 4); idx += 64 * NW) {
      const int lrow = idx / (D / 4), c = 4 * (idx - lrow * (D / 4));
      const int krow = k0 + lrow;
      const bool ok = krow < T;
      const long long roff = (boff + (ok ? krow : 0)) * ld + h * D + c;
      const float4 kv = ok ? *reinterpret_cast<const float4*>(k + roff) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 vv = ok ? *reinterpret_cast<const float4*>(v + roff) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* kd = ks + lrow * KP + c;
      kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
      *reinterpret_cast<float4*>(vs + lrow * D + c) = vv;
    }
    __syncthreads();

    // S^T[key][query] = sum_d K[key][d] * Q[query][d]
    f32x16 sacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
    const float* krow_p = ks + lj * KP + lh;
#pragma unroll SUNR
    for (int s = 0; s < D / 2; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(krow_p[2 * s], qreg[s], sacc, 0, 0, 0);

    // scale, mask the keys past T, online softmax per query (= per lane; the two lane halves hold different keys)
    float mt = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      const float sv = key < T ? sacc[e] / sqrt_d : -INFINITY;
      sacc[e] = sv;
      mt = fmaxf(mt, sv);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);           // finite: every tile holds at least one valid key
    const float corr = expf(m_run - m_new);         // exp(-inf) = 0 on the first tile
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pe = expf(sacc[e] - m_new);       // masked keys: exp(-inf) = 0
      sacc[e] = pe;
      ls += pe;
    }
    ls += __shfl_xor(ls, 32, 64);
    l_run = l_run * corr + ls;
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[i][e] *= corr;

    // O^T[d][query] += sum_key V[key][d] * P[key][query]; register e = key (e&3) + 8*(e>>2) + 4*lh
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float* vrow = vs + ((e & 3) + 8 * (e >> 2) + 4 * lh) * D + lj;
#pragma unroll
      for (int i = 0; i < DT; ++i)
        oacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * i], sacc[e], oacc[i], 0, 0, 0);
    }
  }

  // the row's log-sum-exp of the scaled scores: both lane halves hold the same m_run and l_run
  if (LSE) {
    if (q_ok && lh == 0) lse[(boff + qrow) * heads + h] = m_run + logf(l_run);
  }

  // normalise and store: O^T tile (d rows in registers, query on the lane) -> LDS [query][d] -> 128-byte rows
  const float inv_l = 1.f / l_run;
  float* osw = os[wave];
#pragma unroll
  for (int i = 0; i < DT; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int dd = (e & 3) + 8 * (e >> 2) + 4 * lh;
      osw[lj * OP + dd] = oacc[i][e] * inv_l;
    }
    // a wave only touches its own staging slice: wave-level ordering is enough
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = (lane >> 3) + 8 * it, c = (lane & 7) * 4;
      if (q0 + r < T) {
        float4 o4;
        o4.x = osw[r * OP + c];
        o4.y = osw[r * OP + c + 1];
        o4.z = osw[r * OP + c + 2];
        o4.w = osw[r * OP + c + 3];
        *reinterpret_cast<float4*>(ctx + (boff + q0 + r) * ldo + h * D + i * 32 + c) = o4;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

#endif  // AVS_MHSA_FLASH_BODY_H
