/*
 * avsum_dropout.h — C-ABI of libavsum_dropout.so: counter-based Dropout over a RAGGED batch of videos on the MI355X
 * (gfx950).  A fifth, self-contained library beside libavsum_hip.so, libavsum_optim.so, libavsum_ingest.so and
 * libavsum_attn.so: it shares no symbol and no state with them.
 *
 * Nothing is drawn, stored or ordered: every element of a Dropout mask is a pure function of
 * (seed, sample id of its video, branch, row inside the video, column).  The forward computes it in registers while it
 * applies it, the backward computes it again, and a video has the same mask alone and in any batch.
 *
 * THE CONTRACT.  The generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2,
 * 3", SC'11): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments W0 = 0x9E3779B9, W1 = 0xBB67AE85, ten
 * rounds, the key advanced by (W0, W1) between rounds.  One round maps
 *
 *   (c0, c1, c2, c3)  ->  (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
 *
 * with hi / lo the upper / lower 32 bits of the 64-bit product.  For the element in row r of video v (r counted INSIDE
 * the video: global row - offsets[v]), column c, branch b (0 = visual, 1 = audio):
 *
 *   key     = (seed & 0xffffffff,  seed >> 32)                                    seed: unsigned 64-bit
 *   counter = (c >> 2,  r,  sample_v & 0xffffffff,  (((sample_v >> 32) << 1) | b) & 0xffffffff)
 *   word    = output word (c & 3) of Philox4x32-10(counter, key)
 *   kept    = word >= thr                                                         thr = floor(p * 2^32), in float64
 *   m       = kept ? scale : 0.0f                                                 scale = 1.0f / (1.0f - (float)p)
 *
 * sample_v is a 63-bit id of "this video in this step": sample_base + v when d_samples is NULL, d_samples[v]
 * otherwise.  thr and scale are computed once on the host and passed by value; p lies in [0, 1), and p = 0 (thr = 0,
 * scale = 1) keeps everything.  One Philox call yields the four words of four consecutive columns.
 *
 * The three entry points take the same batch arguments:
 *
 *   d_offsets    DEVICE int64 [nseq + 1]: the row offsets of the videos.  The caller has validated them on the host
 *                (they start at 0, increase strictly and end at `rows`); the kernels read entries 0 .. nseq only.  A
 *                row's video is the last v in 0 .. nseq - 1 with offsets[v] <= row, found by binary search.  Which
 *                memory is touched depends on rows, cols and the strides alone, never on what the offsets hold.
 *   rows, cols   the rows 0 .. rows - 1 and the columns 0 .. cols - 1 of every operand are read / written, nothing else
 *   ld*          row strides in ELEMENTS: a column slice of a wider buffer is fine
 *   seed, thr, scale, branch, sample_base, d_samples   as above; d_samples is DEVICE int64 [nseq] or NULL
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSD_OK (0) or a negative AVSD_E_* code; never
 *     throws.  avsd_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller; nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside; no process-global mutable state.
 *
 * Refused before any launch: a null pointer (d_samples excepted), rows or cols negative, nseq outside
 * 1 .. AVSD_MAX_SEQ, rows above AVSD_MAX_ROWS, cols not a multiple of AVSD_VEC, a row stride below cols or not a
 * multiple of AVSD_VEC, an operand base not 16-byte aligned, d_offsets / d_samples not 8-byte aligned, branch other
 * than 0 or 1, sample_base negative or sample_base + nseq - 1 above 2^63 - 1.  rows == 0 or cols == 0 is a no-op.
 *
 * Launch: a thread owns AVSD_VEC consecutive columns of one row (one Philox call, one 16-byte load per input, one
 * 16-byte store); AVSD_BLOCK threads per workgroup, at most AVSD_MAX_GROUPS workgroups, which stride over the
 * rows * cols / AVSD_VEC items.
 */
#ifndef AVSUM_DROPOUT_H
#define AVSUM_DROPOUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSD_ABI_VERSION 1

#define AVSD_VEC 4               /* columns of a thread: the four output words of one Philox call                      */
#define AVSD_BLOCK 256           /* threads of a workgroup                                                             */
#define AVSD_MAX_GROUPS 2048     /* workgroups of a launch at most: 8 per CU of the 256, every wave slot filled once   */
#define AVSD_MAX_SEQ 16777216    /* nseq at most: 2^24                                                                 */
#define AVSD_MAX_ROWS 2147483647 /* rows at most: 2^31 - 1 (the row inside a video is a 32-bit counter word)           */

enum {
  AVSD_OK = 0,
  AVSD_E_ARG = -1,       /* null pointer / count out of range                  */
  AVSD_E_SHAPE = -2,     /* sizes inconsistent with what the kernels assume    */
  AVSD_E_ALIGN = -3,     /* pointer not aligned as required                    */
  AVSD_E_HIP = -4        /* the HIP runtime reported an error at launch        */
};

typedef void* avsd_stream_t;

int avsd_abi_version(void);
const char* avsd_last_error(void);

/* out[r, c] = m: the multiplier itself, fp32 [rows, ldo]. */
int avsd_keep_mask_f32(float* d_out, int64_t ldo, const int64_t* d_offsets, int nseq, int64_t rows, int cols,
                       uint64_t seed, uint32_t thr, float scale, int branch, int64_t sample_base,
                       const int64_t* d_samples, avsd_stream_t stream);

/* out[r, c] = x[r, c] * m, a literal fp32 product (NaN, Inf and -0.0 behave as in x * mask).  d_out == d_x with
 * ldo == ldx is allowed; any other overlap is not. */
int avsd_dropout_fwd_f32(const float* d_x, int64_t ldx, float* d_out, int64_t ldo, const int64_t* d_offsets, int nseq,
                         int64_t rows, int cols, uint64_t seed, uint32_t thr, float scale, int branch,
                         int64_t sample_base, const int64_t* d_samples, avsd_stream_t stream);

/* out[r, c] = relu_out[r, c] > 0 ? dy[r, c] * m : 0: the gradient gate of Linear -> ReLU -> Dropout, the arithmetic of
 * avs_relu_dropout_bwd_f32 with the mask computed again.  d_out == d_dy with ldo == lddy is allowed. */
int avsd_relu_dropout_bwd_f32(const float* d_dy, int64_t lddy, const float* d_relu_out, int64_t ldr, float* d_out,
                              int64_t ldo, const int64_t* d_offsets, int nseq, int64_t rows, int cols, uint64_t seed,
                              uint32_t thr, float scale, int branch, int64_t sample_base, const int64_t* d_samples,
                              avsd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_DROPOUT_H */
