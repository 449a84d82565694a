/*
 * avsum_optim.h — C-ABI of libavsum_optim.so, the fused multi-tensor AdamW step of the scorer's training loop on
 * the MI355X (gfx950).  A second, self-contained library beside libavsum_hip.so: it shares no symbol, no state and
 * no header with it.
 *
 * One optimiser step is at most 1 + 2 * ceil(n / AVSO_MAX_TENSORS) launches on the caller's stream:
 *
 *   avso_grad_sumsq_f32   (optional)  one fp64 partial sum of squares per chunk of every gradient
 *   avso_adamw_prepare                partials -> norm2 -> clip coefficient and skip decision; the step count and the
 *                                     bias corrections; all of it on the device, the host sees none of it
 *   avso_adamw_apply_f32              p, m, v updated in one pass: 28 bytes per element
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSO_OK (0) or a negative AVSO_E_* code; never
 *     throws.  avso_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller; nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside.
 *
 * Pointer tables are HOST memory and travel in the kernel arguments: h_table is int64 [ntensors, AVSO_TABLE_COLS],
 * a row = (param, grad, exp_avg, exp_avg_sq, numel), the first four the device addresses of dense fp32 arrays of
 * numel elements (4-byte aligned; where all four of a row are 16-byte aligned the kernels use 16-byte accesses).
 * Gradients get new addresses every step (zero_grad sets them to None), so a device table would cost an upload per
 * step; the kernel argument costs none.  At most AVSO_MAX_TENSORS rows per launch: the caller slices longer lists.
 * A tensor is cut into chunks of AVSO_CHUNK elements, the last one shorter; a launch's chunks are numbered through
 * its rows in order, and a workgroup finds the row of a chunk by binary search in the exclusive scan of the rows'
 * chunk counts, which the entry point builds and passes beside the table.
 *
 * The workspace is one device buffer of avso_workspace_bytes(total_chunks) bytes, 16-byte aligned, zeroed ONCE by
 * the caller when the optimiser is created:
 *   bytes  0 .. 31   d_state:    AVSO_STATE_DOUBLES doubles (AVSO_STATE_*)
 *   bytes 32 .. 63   d_coef:     AVSO_COEF_FLOATS floats (AVSO_COEF_*), rewritten by every avso_adamw_prepare
 *   bytes 64 ..      d_partials: total_chunks doubles
 */
#ifndef AVSUM_OPTIM_H
#define AVSUM_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSO_ABI_VERSION 1

#define AVSO_MAX_TENSORS 32      /* rows of h_table per launch: the table and its scan are 1.4 KiB of kernel arguments */
#define AVSO_CHUNK 4096          /* elements of a chunk: one workgroup of 256 threads, 16 elements per thread          */
#define AVSO_TABLE_COLS 5        /* int64 per row of h_table                                                           */
#define AVSO_MAX_GROUPS 2048     /* workgroups of a launch at most; they stride over the chunks                        */
#define AVSO_STATE_DOUBLES 4
#define AVSO_COEF_FLOATS 8
#define AVSO_COEF_OFFSET 32      /* byte offsets into the workspace; d_state is at 0 */
#define AVSO_PARTIALS_OFFSET 64

enum {
  AVSO_OK = 0,
  AVSO_E_ARG = -1,       /* null pointer / count out of range / negative size  */
  AVSO_E_SHAPE = -2,     /* sizes inconsistent with what the kernel assumes    */
  AVSO_E_ALIGN = -3,     /* pointer not aligned to its element                 */
  AVSO_E_HIP = -4,       /* the HIP runtime reported an error at launch        */
  AVSO_E_WORKSPACE = -5  /* workspace too small                                */
};

/* d_state, doubles */
enum {
  AVSO_STATE_APPLIED = 0,  /* steps applied so far: the t of the next applied step is this + 1 */
  AVSO_STATE_SKIPPED = 1,  /* steps skipped so far                                             */
  AVSO_STATE_NORM2 = 2,    /* the last step's sum of squared gradients; -1 = not computed      */
  AVSO_STATE_CLIP = 3      /* the last step's clip coefficient (the fp32 value, as a double)   */
};
/* d_coef, floats: each rounded ONCE from its fp64 value */
enum {
  AVSO_COEF_DECAY = 0,      /* 1 - lr * weight_decay                                        */
  AVSO_COEF_STEP_SIZE = 1,  /* lr / (1 - beta1^t)                                           */
  AVSO_COEF_BC2_SQRT = 2,   /* sqrt(1 - beta2^t)                                            */
  AVSO_COEF_CLIP = 3,       /* max_norm > 0 ? min(1, max_norm / (sqrt(norm2) + 1e-6)) : 1   */
  AVSO_COEF_SKIP = 4        /* 1 = this step is skipped: the apply kernels store nothing    */
};

typedef void* avso_stream_t;

int avso_abi_version(void);
const char* avso_last_error(void);

/* Bytes of the workspace for total_chunks partials (0 when total_chunks < 0). */
size_t avso_workspace_bytes(int64_t total_chunks);

/* d_partials[first_chunk + c] = sum over chunk c of double(g) * double(g), c numbered through the rows of h_table.
 * Thread i of the chunk's workgroup adds elements 4*(i + 256*k) + e, k = 0..3, e = 0..3 in that order, then the 256
 * thread sums meet in a fixed tree: the order depends on the chunk's length only, not on its address, its alignment
 * or its place in the table.  No atomics.  first_chunk + (chunks of this table) <= total_chunks, or AVSO_E_WORKSPACE. */
int avso_grad_sumsq_f32(const int64_t* h_table, int ntensors, double* d_partials, int64_t first_chunk,
                        int64_t total_chunks, avso_stream_t stream);

/* One workgroup.  norm2 = d_partials[0 .. npartials) added in ascending index per thread (i, i + 256, ...) and then
 * in a fixed tree; npartials = 0: norm2 is not computed (stored as -1), clip = 1, the step is never skipped.
 * skip = skip_nonfinite && !isfinite(norm2).  Not skipped: t = applied + 1, the coefficients of AVSO_COEF_* are
 * written for t and `applied` becomes t; skipped: only AVSO_COEF_SKIP is set and `skipped` is bumped.
 * lr, weight_decay >= 0, beta1, beta2 in [0, 1), max_norm <= 0 = no clipping. */
int avso_adamw_prepare(const double* d_partials, int64_t npartials, double lr, double beta1, double beta2,
                       double weight_decay, double max_norm, int skip_nonfinite, double* d_state, float* d_coef,
                       avso_stream_t stream);

/* Per element, in fp32, no contraction (decoupled weight decay, torch's single-tensor AdamW):
 *   g' = g * clip;  p = p * decay;  m = m + (g' - m) * (1 - beta1);  v = v * beta2 + g' * g' * (1 - beta2);
 *   p = p - step_size * m / (sqrt(v) / bc2s + eps)
 * with (1 - beta1), beta2, (1 - beta2), eps each rounded once from fp64.  The gradient itself is NOT rescaled
 * (unlike clip_grad_norm_).  A skipped step stores nothing. */
int avso_adamw_apply_f32(const int64_t* h_table, int ntensors, const float* d_coef, double beta1, double beta2,
                         double eps, avso_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_OPTIM_H */
