/*
 * avsum_loss.h — C-ABI of libavsum_loss.so: per-shot training targets and a pairwise ranking loss for a RAGGED batch of
 * videos on the MI355X (gfx950).  A sixth, self-contained library beside libavsum_hip.so, libavsum_optim.so,
 * libavsum_ingest.so, libavsum_attn.so and libavsum_dropout.so: it shares no symbol and no state with them.
 *
 * No atomics anywhere: every sum below has ONE order, which depends on the length of its video alone, so a video's
 * targets, loss and gradient are the same bits alone, in any batch and at any position in it.
 *
 * THE CONTRACT, part 1: avsl_shot_targets_f32 (the reference's utils/alignments.py, per shot).  Video v has the
 * annotation vector ann_v = d_annotations[ann_offsets[v] .. ann_offsets[v + 1]) of A_v entries, the frame rate fps_v
 * and the shots d_shots[s] = (start, end), s in shot_offsets[v] .. shot_offsets[v + 1]), video-relative frame bounds.
 * In fp64, with two IEEE divisions each and no contraction:
 *
 *   a = floor(((double)start / fps_v) / bin_seconds)          b = floor(((double)end / fps_v) / bin_seconds) + 1
 *
 * both clipped to [0, A_v] (what a numpy slice does to non-negative bounds; a negative or NaN bound clips to 0).  Then
 *
 *   targets[s] = (float)( (ann_v[a] + ann_v[a + 1] + ... + ann_v[b - 1]) / (double)(b - a) )
 *
 * the sum in fp64 in index order from 0.0, one division, ONE rounding to fp32.  b <= a (an empty slice) gives NaN and
 * sets flags[v] = 1; flags[v] is written 0 otherwise.  Rows of d_targets that no video owns (s outside
 * shot_offsets[0] .. shot_offsets[nvideos], which happens where a shot table lies at its capacity) are NOT written.
 * d_shot_offsets and d_shots may be the tables another kernel has just written; d_ann_offsets and d_fps are the
 * caller's, validated on the host.  Every read is clipped to the buffers' sizes (nann, nshots) whatever the tables hold.
 * One workgroup of AVSL_BLOCK threads per video, thread t takes the shots t, t + AVSL_BLOCK, ...
 *
 * THE CONTRACT, part 2: avsl_rank_loss_f32.  Video v is rows offsets[v] .. offsets[v + 1] of d_scores (s) and
 * d_targets (y), T_v <= AVSL_MAX_T of them.  A pair is (i, j) with y_i > y_j (an IEEE comparison: ties form no pair,
 * -0.0 == 0.0; NaN is out of contract), P_v their number, d_ij = (double)s_i - (double)s_j (exact).
 *
 *   AVSL_LOGISTIC   L_v = (1 / P_v) * sum_pairs softplus(-scale * d_ij),  softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *                   dL_v/ds_i = (scale / P_v) * ( sum_{j: y_j > y_i} sigma(-scale * d_ji)
 *                                               - sum_{j: y_i > y_j} sigma(-scale * d_ij) )
 *                   sigma(x) = 1 / (1 + e) for x >= 0, e / (1 + e) otherwise, e = exp(-|x|)
 *   AVSL_HINGE      L_v = (1 / P_v) * sum_pairs max(0, margin - d_ij); the pair is VIOLATED where margin - d_ij > 0
 *                   dL_v/ds_i = c_i / P_v,  c_i = #{j: y_j > y_i, (j, i) violated} - #{j: y_i > y_j, (i, j) violated}
 *
 * all in fp64 (exp, log1p and the divisions included).  P_v = 0 (one row, or every target tied): L_v = 0 and the
 * gradient is 0.
 *
 * Two launches.  (1) One workgroup of AVSL_TILE threads per entry (video, row tile) of d_tiles; thread t owns row
 * i = tile * AVSL_TILE + t of its video and walks EVERY j of that video in index order, staged through LDS
 * AVSL_CHUNK at a time (every lane reads the same j).  It writes for its row, into the workspace: the fp64 sum of the
 * terms of the pairs (i, j) it is the higher row of, the fp64 bracket of the gradient above (logistic) or the int32
 * c_i (hinge), and the int32 count of those pairs.  (2) One workgroup of AVSL_BLOCK threads per video: thread t sums the
 * row partials of rows t, t + AVSL_BLOCK, ... in that order, the AVSL_BLOCK partial sums are folded by a fixed binary
 * tree; P_v is an int64; losses[v] = (float)(sum / (double)P_v), rounded once; g[r] = (float)(rowgrad_r / (double)P_v)
 * with rowgrad_r = scale * bracket_r (logistic) or (double)c_r (hinge).  pairs[v] = P_v.
 *
 * avsl_rank_loss_bwd_f32: dscores[r] = dlosses[v] * g[r], a literal fp32 product, v the video of row r.
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSL_OK (0) or a negative AVSL_E_* code; never
 *     throws.  avsl_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller; nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside; no process-global mutable state.
 *   - d_offsets is DEVICE int64 [nseq + 1], validated by the caller on the host: it starts at 0, increases strictly and
 *     ends at `rows`.  d_tiles is DEVICE int32 [ntiles, 2] = (video, row tile): every video's tiles
 *     0 .. ceil(T_v / AVSL_TILE) - 1.  An entry that names no video, or rows outside 0 .. rows, is skipped.
 *
 * Refused before any launch: a null pointer, rows outside 1 .. AVSL_MAX_ROWS, nseq outside 1 .. rows, ntiles below
 * nseq or above AVSL_MAX_ROWS, max_t outside 1 .. AVSL_MAX_T, a kind other than the two, a scale that is not finite or
 * is <= 0, a margin that is not finite, a workspace smaller than avsl_rank_workspace_bytes(rows) or not 8-byte aligned;
 * for the targets: nvideos < 1, nshots or nann negative or above AVSL_MAX_ROWS, a bin_seconds that is not finite or
 * is <= 0.  nshots == 0 still writes the flags.
 */
#ifndef AVSUM_LOSS_H
#define AVSUM_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSL_ABI_VERSION 1

#define AVSL_TILE 256            /* rows of a video per workgroup of the pair kernel                                   */
#define AVSL_CHUNK 1024          /* rows it stages through LDS per step                                                */
#define AVSL_BLOCK 256           /* threads of a fold / shot-target workgroup                                          */
#define AVSL_MAX_T 32768         /* rows of one video: pair counts stay below 2^30 per row, below 2^31 per video      */
#define AVSL_MAX_ROWS 2147483647 /* the last offset at most: 2^31 - 1                                                  */
#define AVSL_TILE_COLS 2         /* int32 per row of the tile table                                                    */

enum {
  AVSL_OK = 0,
  AVSL_E_ARG = -1,       /* null pointer / value out of range                  */
  AVSL_E_SHAPE = -2,     /* sizes inconsistent with what the kernels assume    */
  AVSL_E_ALIGN = -3,     /* pointer not aligned as required                    */
  AVSL_E_HIP = -4        /* the HIP runtime reported an error at launch        */
};

enum {
  AVSL_LOGISTIC = 0,
  AVSL_HINGE = 1
};

typedef void* avsl_stream_t;

int avsl_abi_version(void);
const char* avsl_last_error(void);

/* targets fp32 [nshots], flags uint8 [nvideos]; d_fps fp64 [nvideos]; d_shots int64 [nshots, 2]. */
int avsl_shot_targets_f32(const float* d_annotations, int64_t nann, const int64_t* d_ann_offsets, const int64_t* d_shots,
                          int64_t nshots, const int64_t* d_shot_offsets, const double* d_fps, int nvideos,
                          double bin_seconds, float* d_targets, uint8_t* d_flags, avsl_stream_t stream);

/* bytes of the workspace of avsl_rank_loss_f32 for `rows` rows (0 for rows <= 0) */
size_t avsl_rank_workspace_bytes(int64_t rows);

/* losses fp32 [nseq], g fp32 [rows], pairs int64 [nseq] */
int avsl_rank_loss_f32(const float* d_scores, const float* d_targets, int64_t rows, const int64_t* d_offsets, int nseq,
                       const int32_t* d_tiles, int64_t ntiles, int max_t, int kind, double scale, double margin,
                       void* d_workspace, size_t workspace_bytes, float* d_losses, float* d_g, int64_t* d_pairs,
                       avsl_stream_t stream);

/* dscores fp32 [rows] */
int avsl_rank_loss_bwd_f32(const float* d_dlosses, const float* d_g, int64_t rows, const int64_t* d_offsets, int nseq,
                           float* d_dscores, avsl_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_LOSS_H */
