/*
 * avsum_attn.h — C-ABI of libavsum_attn.so: multi-head self-attention over a RAGGED batch of sequences on the MI355X
 * (gfx950), forward and a fused backward that never holds a [T, T] matrix in memory.  A fourth, self-contained
 * library beside libavsum_hip.so, libavsum_optim.so and libavsum_ingest.so: it shares no symbol and no state with them.
 *
 * The batch: V sequences lie one after another in the rows of the projections Q, K, V, fp32 [rows, ld]; sequence v is
 * rows offsets[v] .. offsets[v + 1] (T_v of them), head h its columns h * D .. (h + 1) * D.  Nothing is padded, keys
 * and queries never cross a sequence boundary, and what a workgroup computes depends on its own sequence's length
 * only: a sequence has the same result bits alone and in any batch.  Per sequence and head, alpha = 1 / sqrt(D):
 *
 *   S = alpha Q K^T     L = logsumexp_k S     P = exp(S - L)     O = P V
 *   delta = rowsum(dO o O)
 *   dV = P^T dO     dP = dO V^T     dS = alpha P o (dP - delta)     dQ = dS K     dK = dS^T Q
 *
 * Four launches, all exact fp32 on v_mfma_f32_32x32x2_f32:
 *
 *   avsa_mhsa_rows_fwd_f32     ctx (= O) and lse (= L); a workgroup = AVSA_FWD_TILE queries of one (sequence, head)
 *   avsa_mhsa_rows_delta_f32   delta, one pass over dctx and ctx in a fixed order
 *   avsa_mhsa_rows_dkv_f32     a workgroup owns AVSA_BWD_TILE keys of one (sequence, head), sweeps the sequence's query
 *                              tiles, recomputes S, P, dP, dS, keeps dK and dV on chip and stores them once
 *   avsa_mhsa_rows_dq_f32      a workgroup owns AVSA_BWD_TILE queries, sweeps the sequence's key tiles, stores dQ once
 *
 * Every output element has ONE owner: no float atomics, so every gradient is bit-identical from run to run and from
 * batch to batch.
 *
 * lse and delta are fp32 [rows, heads], dense (row r, head h at r * heads + h): row numbers are those of the
 * projections.  Rows outside offsets[0] .. offsets[V] are neither read nor written in any buffer.
 *
 * Tables.  h_offsets is HOST memory, int64 [nseq + 1]: it is validated here, before any launch.  d_offsets is the
 * same array in device memory.  d_tiles is int32 [ntiles, AVSA_TILE_COLS] in device memory, a row = (sequence, tile):
 * for every sequence in order, tile = 0 .. ceil(T_v / TILE) - 1, with TILE = AVSA_FWD_TILE for the forward and
 * AVSA_BWD_TILE for the two gradient kernels (which share one table: query tiles and key tiles have the same size).
 * ntiles must equal the count the host offsets give.
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSA_OK (0) or a negative AVSA_E_* code; never
 *     throws.  avsa_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller; nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside; no process-global mutable state.
 *
 * Limits, refused before any launch: nseq >= 1, every T_v >= 1, offsets[0] >= 0, offsets[nseq] < 2^31, heads in
 * 1 .. AVSA_MAX_HEADS, head_dim 64, 128 or 256, row strides multiples of 4 floats and >= heads * head_dim, 16-byte
 * aligned operand bases (lse, delta: 4-byte), no null pointer.
 */
#ifndef AVSUM_ATTN_H
#define AVSUM_ATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSA_ABI_VERSION 1

#define AVSA_FWD_TILE 128        /* queries of a forward workgroup: four waves of 32                                  */
#define AVSA_BWD_TILE 32         /* keys of a dK/dV workgroup, queries of a dQ workgroup, and the tile either sweeps   */
#define AVSA_TILE_COLS 2         /* int32 per row of d_tiles: (sequence, tile)                                         */
#define AVSA_MAX_HEADS 65535     /* the head is grid y                                                                 */
#define AVSA_MAX_ROWS 2147483647 /* offsets[nseq] at most: 2^31 - 1                                                    */
#define AVSA_DELTA_GROUPS 16384  /* workgroups of the delta launch at most; they stride over the (row, head) pairs     */

enum {
  AVSA_OK = 0,
  AVSA_E_ARG = -1,       /* null pointer / count out of range                  */
  AVSA_E_SHAPE = -2,     /* sizes inconsistent with what the kernels assume    */
  AVSA_E_ALIGN = -3,     /* pointer not aligned as required                    */
  AVSA_E_HIP = -4        /* the HIP runtime reported an error at launch        */
};

typedef void* avsa_stream_t;

int avsa_abi_version(void);
const char* avsa_last_error(void);

/* ctx[r, h*D + :] = O, lse[r, h] = L for every row of every sequence.  ctx is fp32 [rows, ldo].  The ctx bits of a
 * sequence are those avs_mhsa_flash_f32 gives for it as a batch of one: the two kernels share their body. */
int avsa_mhsa_rows_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const int64_t* h_offsets,
                           const int64_t* d_offsets, int nseq, const int32_t* d_tiles, int64_t ntiles, int heads,
                           int head_dim, float* d_ctx, int64_t ldo, float* d_lse, avsa_stream_t stream);

/* delta[r, h] = sum_d dctx[r, h*D + d] * ctx[r, h*D + d], rows offsets[0] .. offsets[nseq]: one wave per (row, head),
 * lane l adds d = l, l + 64, ... in ascending order, then the 64 lane sums meet in a fixed xor tree. */
int avsa_mhsa_rows_delta_f32(const float* d_dctx, int64_t lddo, const float* d_ctx, int64_t ldo,
                             const int64_t* h_offsets, int nseq, int heads, int head_dim, float* d_delta,
                             avsa_stream_t stream);

/* dK, dV fp32 [rows, ldg], written once for every row of every sequence.  d_tiles: the AVSA_BWD_TILE table. */
int avsa_mhsa_rows_dkv_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_dctx,
                           int64_t lddo, const float* d_lse, const float* d_delta, const int64_t* h_offsets,
                           const int64_t* d_offsets, int nseq, const int32_t* d_tiles, int64_t ntiles, int heads,
                           int head_dim, float* d_dk, float* d_dv, int64_t ldg, avsa_stream_t stream);

/* dQ fp32 [rows, ldg], written once for every row of every sequence.  d_tiles: the AVSA_BWD_TILE table. */
int avsa_mhsa_rows_dq_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_dctx,
                          int64_t lddo, const float* d_lse, const float* d_delta, const int64_t* h_offsets,
                          const int64_t* d_offsets, int nseq, const int32_t* d_tiles, int64_t ntiles, int heads,
                          int head_dim, float* d_dq, int64_t ldg, avsa_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_ATTN_H */
