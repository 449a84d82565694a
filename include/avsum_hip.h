/*
 * avsum_hip.h — C-ABI of libavsum_hip.so, the MI355X (gfx950) hot path of the
 * audio-visual frame-scoring pipeline.
 *
 * The reference (AudioVidSum) has no FFI layer: its boundary is the Python
 * class/function API of features/extractors.py, features/fusion.py,
 * models/attention.py and models/av_model.py.  This header is the thin C-ABI
 * the Python host mirror of those classes calls (ctypes).  Every entry point
 * names the reference lines it replaces.
 *
 * Conventions (all entry points):
 *   - `extern "C"`, plain pointers and sizes; no torch / C++ types.
 *   - returns int status: AVS_OK (0) or a negative AVS_E_* code; never throws.
 *     avs_last_error() returns a thread-local message for the last failure.
 *   - every pointer named d_* is DEVICE memory owned by the caller (the host
 *     side passes torch tensor data_ptr()s); nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*;
 *     NULL = the null stream); no host synchronisation inside.
 *   - tensors are dense row-major unless a stride is given; "NHWC" activations
 *     are [image][row][pixel][channel].
 *   - dtype: AVS_F32 = IEEE fp32 operands, fp32 accumulate on the f32 MFMA
 *     (exact fmaf chain; the parity mode).  AVS_BF16 = bf16 operands, fp32
 *     accumulate on the bf16 MFMA (the throughput mode).  AVS_F32_ACC64
 *     (avs_gemm_nt / avs_conv2d_nhwc only) = fp32 operands and fp32 MFMA over
 *     each reduction step (16 elements; 32 for long reductions), steps summed in fp64: used for
 *     the STFT, where a long fp32 running sum would lose the quiet bins.
 *     AVS_F32_SPLIT (avs_gemm_nt / avs_conv2d_nhwc[_bnstats] only) = fp32 operands
 *     in memory, products on the bf16 MFMA: every operand element is split into
 *     hi = bf16(x), lo = bf16(x - hi) in registers and a*b is taken as
 *     ah*bh + ah*bl + al*bh (fp32 accumulate): ~2^-15 relative per product instead
 *     of exact, 5.3x the matrix rate of the f32 MFMA.
 */
#ifndef AVSUM_HIP_H
#define AVSUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVS_ABI_VERSION 5

/* ---- sizes the host and the kernels share ---------------------------------
 * The host builds tables that the kernels index by these numbers, shapes buffers by them and refuses what exceeds
 * them.  Each is defined HERE and nowhere else: the kernel files use these names, and the Python host reads the
 * values from this header (_header.py), as it reads the prototypes, the enums and avs_conv_desc.               */
/* batched fusion (avs_cdist_batch_f64, avs_dtw_batch_f64; AVS_FUSION_MAX_N also avs_dtw_path_f64) */
#define AVS_FUSION_MAX_N 6400      /* visual rows n of a pair: 3 anti-diagonals of fp64 = 150 KiB of the 160 KiB LDS */
#define AVS_FUSION_SMALL_L 64      /* l = min(n, m) <= this: one wave per pair, four pairs per workgroup             */
#define AVS_FUSION_MID_L 512       /* l <= this: one 256-thread workgroup per pair; above: 1024 threads              */
#define AVS_FUSION_TILE 32         /* rows and columns of a cost tile of d_tiles                                     */
#define AVS_FUSION_PAIR_COLS 8     /* int64 per row of d_pairs                                                       */
/* batched evaluation (avs_rank_pair_counts, avs_eval_fold) */
#define AVS_EVAL_MAX_T 32768       /* rows of a video: 4 T^4 < 2^63, the fold's sums and the host's products fit int64 */
#define AVS_EVAL_TILE 256          /* rows of a video per entry of d_tiles                                           */
#define AVS_EVAL_CHUNK 1024        /* columns the pair-count kernel stages through LDS per step                      */
#define AVS_EVAL_COLS 10           /* int64 per video of avs_eval_fold's d_out                                       */
/* batched shot detection and frame sampling (avs_shot_cuts_batch, avs_shot_tables_fill; features/extractors.py) */
#define AVS_SHOT_INTERVAL 3        /* the sampled frames of a shot are the multiples of this                         */
#define AVS_SHOT_MAX_FRAMES 100    /* at most this many per shot                                                     */
#define AVS_SHOT_MICRO_BATCH 4     /* in BatchNorm groups of this many, with a shorter tail group                    */
/* keyshot summaries (avs_knapsack_batch_f64) */
#define AVS_SUMMARY_MAX_CAPACITY 8191  /* cells 0 .. capacity: two fp64 rows of 8192 cells = 128 KiB of the LDS      */
/* kernel temporal segmentation (avs_kts_*) */
#define AVS_KTS_MAX_SAMPLES 2048   /* samples n of a video: both live fp64 rows of the programme stay in LDS         */
#define AVS_KTS_TILE 64            /* rows and columns of a Gram tile of d_tiles                                     */
#define AVS_KTS_MAX_VIDEOS 65535   /* videos of a batch (a grid dimension)                                           */
#define AVS_KTS_VIDEO_COLS 10      /* int64 per row of d_videos                                                      */
/* the fused mel front end (avs_stft_mel_fused_f32 and the kernels built on it): the shapes of d_window, d_cos, d_sin */
#define AVS_FUSED_NFFT 400
#define AVS_FUSED_HOP 200
#define AVS_FUSED_COLS 208         /* the 201 bins padded to 13 tiles of 16                                          */
#define AVS_FUSED_RE_ROWS 204      /* n = 0 .. 200 padded to a multiple of 4                                         */
#define AVS_FUSED_IM_ROWS 200      /* n = 1 .. 199 padded to a multiple of 4                                         */
/* VGGish examples (avs_vggish_examples_f32) */
#define AVS_VGG_WINDOW 400         /* samples of a frame                                                             */
#define AVS_VGG_HOP 160
#define AVS_VGG_BINS 257           /* re | im columns of d_basis_t each, rows of d_fb                                */
#define AVS_VGG_FRAMES 96          /* frames of an example                                                           */

enum {
  AVS_OK = 0,
  AVS_E_ARG = -1,       /* null pointer / bad enum / negative size            */
  AVS_E_SHAPE = -2,     /* sizes inconsistent with what the kernel assumes    */
  AVS_E_ALIGN = -3,     /* pointer or stride not 16-byte aligned              */
  AVS_E_HIP = -4,       /* the HIP runtime reported an error at launch        */
  AVS_E_WORKSPACE = -5, /* workspace too small                                */
  AVS_E_UNSUPPORTED = -6 /* this entry point does not take the shape; use the documented alternative */
};

enum { AVS_F32 = 0, AVS_BF16 = 1, AVS_F32_ACC64 = 2, AVS_F32_SPLIT = 3, AVS_F16X2 = 4 };
/* AVS_F16X2 ("split-half" storage, the fast parity-grade arithmetic of the CNN trunk): a value is TWO fp16 numbers,
 * x ~ hi + lo with hi = fp16(x), lo = fp16(x - hi) - 22 significant bits, an absolute floor of 2^-25 (fp16
 * denormals, which the matrix cores keep), magnitudes saturating at 65504.  A tensor has the strides and the byte
 * size of the fp32 tensor of the same shape ("slots" of 4 bytes, all strides below in slots); every aligned run of
 * 8 slots (32 bytes) holds the 8 hi halves, then the 8 lo halves, of 8 consecutive elements of the innermost
 * (channel / reduction) axis - so channel counts, strides and offsets are multiples of 8 slots and pointers 32-byte
 * aligned.  The contraction kernel feeds the hi and lo runs to v_mfma_f32_32x32x16_f16 as they are: a product is
 * hi*hi + hi*lo + lo*hi (error ~2^-21 relative, fp32 accumulation) with NO arithmetic on the operands in the loop;
 * each output is split once, by the kernel that produces it.  Taken by avs_conv2d_nhwc, avs_conv2d_nhwc_bnstats,
 * avs_conv2d_nhwc_bnlocal (no bias / alpha), avs_bn_batch_stats, avs_bn_apply, avs_bn_maxpool_nhwc, avs_pool2d_nhwc,
 * avs_global_avgpool_nhwc (fp32 out), avs_frames_normalize_u8; avs_f16x2_pack_f32 / _unpack_f32 convert.         */
enum { AVS_ACT_NONE = 0, AVS_ACT_RELU = 1 };
enum { AVS_BIAS_NONE = 0, AVS_BIAS_COL = 1, AVS_BIAS_ROW = 2 };

typedef void* avs_stream_t;

/* ---- library ------------------------------------------------------------ */
int avs_abi_version(void);
const char* avs_last_error(void);
/* CU count, max clock (kHz), total HBM bytes and gcnArchName of device `dev`. */
int avs_device_info(int dev, int* cu_count, int* clock_khz, int64_t* hbm_bytes,
                    char* arch, int arch_len);

/* fp32 [n] <-> AVS_F16X2 [n] (n a multiple of 8; the fp32 side 16-byte, the f16x2 side 32-byte aligned).  Weights
 * are converted once per parameter version; the trunk's activations never leave the format.                      */
int avs_f16x2_pack_f32(const float* d_src, void* d_dst, int64_t n, avs_stream_t stream);
int avs_f16x2_unpack_f32(const void* d_src, float* d_dst, int64_t n, avs_stream_t stream);

/* AVS_F16P8: a value as fp16 hi + an 8-BIT remainder, 3 bytes: x ~ hi + (u - 128) * step(hi), hi = fp16(x),
 * step(hi) = ulp(max(|hi|, 2^-6)) / 256 (2^-24, the fp16 grid, below 2^-6), u = round((x - hi) / step) + 128 clamped to
 * 1..255 (128 when hi = 0): 19-20 significant bits, the absolute floor of AVS_F16X2; every remainder is itself an fp16
 * number - the lo half AVS_F16X2 holds for the same value.  Every run of 16 values is 48 bytes: the hi halves of
 * values 0-7, of values 8-15, the 16 remainder bytes.  The storage format of the inner block outputs of ResNet layers
 * 1-2 in the AVS_F16X2 trunk (features/extractors.py:29,65): written by avs_conv2d_nhwc_affine (AVS_Y_F16P8), read as
 * its residual (AVS_RES_F16P8) and as the input of avs_conv2d_nhwc_bnstats (AVS_X_F16P8), where the fp16 lo halves the
 * matrix cores take are rebuilt in registers: the same VALUES as the AVS_F16X2 input path on the same tensor, and the same
 * operand bits for |x| >= 2^-6 (below that the hi | lo split of a value is not unique - the 2^-24 floor - so outputs agree to
 * the format's resolution there, not bit for bit: tests/test_gpu_f16p8.py).
 * Both formats SATURATE at +-65504 and store a NaN as -65504 (the clamp is an fmin / fmax pair): the trunk's un-divided
 * inputs (up to 1131) with He-scale weights give raw stem outputs of O(10^3), far from the limit.
 * fp32 [n] <-> AVS_F16P8 [n], n a multiple of 16, both sides 16-byte aligned (tests, tools).                      */
int avs_f16p8_pack_f32(const float* d_src, void* d_dst, int64_t n, avs_stream_t stream);
int avs_f16p8_unpack_f32(const void* d_src, float* d_dst, int64_t n, avs_stream_t stream);

/* ---- dense contraction (K3, K6, K16-K20 of SURVEY §2.3) ------------------ */

/* Implicit-GEMM 2-D convolution on NHWC activations, weights [cout][kh][kw][cin]:
 *   y[n,ho,wo,co] = act( alpha * sum_{kh,kw,ci} x[n, ho*sh-ph+kh, wo*sw-pw+kw, ci]
 *                                              * w[co,kh,kw,ci] + bias[co] )
 * Replaces torch conv2d inside torchvision resnet50 / inception_v3 as called at
 * features/extractors.py:65,83.  Element strides allow padded / sliced views
 * (channel-concat outputs, pre-padded images).  cin must be a multiple of
 * 16 bytes / element size; out-of-image taps read as zero.                  */
typedef struct {
  int dtype;                /* AVS_F32 | AVS_BF16 (x, w, y); bias is fp32     */
  int n, h, w;              /* images, input rows, input pixels per row       */
  int cin, kh, kw;          /* reduction extent                               */
  int sh, sw, ph, pw;       /* stride, zero padding                           */
  int ho, wo, cout;         /* output extent                                  */
  int64_t x_img_stride;     /* elements between images                        */
  int64_t x_row_stride;     /* elements between input rows                    */
  int64_t x_px_stride;      /* elements between input pixels                  */
  int64_t w_row_stride;     /* elements between output channels in w (>= kh*kw*cin) */
  int64_t y_px_stride;      /* elements between output pixels (>= cout)       */
  int act;                  /* AVS_ACT_*                                      */
  float alpha;
  int w_layout;             /* AVS_W_ROWS: w[cout][w_row_stride], a row = (kh, kw, cin);
                             * AVS_W_KSTEP32 (kh*kw*cin a multiple of S = 32 bf16 / 16 fp32 elements, i.e. of a
                             * 64-byte step; not AVS_F32_ACC64): the same matrix stored
                             * reduction-step major, w[k / S][cout][S] - the 64 bytes of a filter that one
                             * reduction step reads sit next to the neighbouring filters', so the weight tile of
                             * a step is contiguous whole cache lines (+2..6 % on the ResNet layers);
                             * w_row_stride is ignored.  Weights are re-laid out once, offline.              */
  int variant;              /* 0 = the library's own choice.  Per-call overrides of the tile / staging variant (what the
                             * tests and the kernel-study tools force; there is NO process-global tuning state):
                             * AVS_TILE_128 / AVS_TILE_256 (bits 0-1): 128-row or, wherever the variant exists, 256-row
                             * output tiles; AVS_TILE_224 (avs_conv2d_nhwc_bnlocal, AVS_F16X2 only): the 224-row tile
                             * whose waves split the columns, for groups of 193..224 rows - what AVS_TILE_AUTO picks
                             * for such groups, AVS_TILE_256 keeps them on the 256-row tile (and keeps the AVS_F16X2
                             * stride-1 'same' layers - 3x3 under the BatchNorm epilogues, any KH x KW under bias + ReLU -
                             * on the tap-major walk instead of the shifted-row form);
                             * AVS_STAGING_GENERIC (bit 2): the general per-lane gather staging even where
                             * the scalar tap walk applies; AVS_CLUSTER_PACKED (bit 3): the packed form of
                             * avs_conv2d_nhwc_bncluster (see there; every other entry point ignores the bit).
                             * Results do not depend on it beyond fp32 summation order.                        */
  int formats;              /* 0, or AVS_F16P8 operands of the AVS_F16X2 1x1 forms (bits): AVS_X_F16P8 - the INPUT of
                             * avs_conv2d_nhwc_bnstats (1x1 / stride 1 on dense rows, cin a multiple of 32, >= 64);
                             * AVS_Y_F16P8 / AVS_RES_F16P8 - the OUTPUT / the RESIDUAL of avs_conv2d_nhwc_affine (cout and
                             * the row strides multiples of 16).  Strides stay in elements; a row of c elements is 3 c
                             * bytes.  Other combinations: AVS_E_UNSUPPORTED.                                           */
} avs_conv_desc;
enum { AVS_W_ROWS = 0, AVS_W_KSTEP32 = 1 };
enum { AVS_X_F16P8 = 1, AVS_Y_F16P8 = 2, AVS_RES_F16P8 = 4 };
enum { AVS_TILE_AUTO = 0, AVS_TILE_128 = 1, AVS_TILE_256 = 2, AVS_TILE_224 = 3, AVS_STAGING_GENERIC = 4,
       AVS_CLUSTER_PACKED = 8 };

int avs_conv2d_nhwc(const avs_conv_desc* desc, const void* d_x, const void* d_w,
                    const float* d_bias, void* d_y, avs_stream_t stream);
/* The same with TWO destinations, AVS_F16X2: output columns [0, n_split) go to d_y (row stride desc->y_px_stride), columns
 * [n_split, cout) to d_y2 (row stride y2_px_stride, column c at c - n_split).  Convolutions that read the same input - an
 * Inception block's 1x1 heads (features/extractors.py:26,73-90) - run as ONE contraction over their stacked filters: the
 * input is fetched once, and the head that belongs to the block's concatenated output still lands in its channel slice.
 * n_split, both strides in multiples of 8 slots; each row stride need only cover its OWN columns (y_px_stride >= n_split,
 * y2_px_stride >= cout - n_split).  relu_cols > 0 (a multiple of 8): with desc->act = ReLU only the columns
 * below it are rectified - a stacked head whose bias + ReLU follow a pooling of its output (Inception's branch_pool, run as
 * convolution -> average pooling -> bias -> ReLU) keeps its raw values.                                                  */
int avs_conv2d_nhwc_split(const avs_conv_desc* desc, const void* d_x, const void* d_w, const float* d_bias, void* d_y,
                          int n_split, void* d_y2, int64_t y2_px_stride, int relu_cols, avs_stream_t stream);

/* The same convolution (no bias, no activation) that also produces the BatchNorm batch statistics of its output
 * in its epilogue and folds them into the affine of avs_bn_batch_stats: for every group g = output_row /
 * rows_per_group (equal-sized micro-batch groups; a shorter last group is allowed) and channel c,
 *   d_scale[g,c] = gamma[c] / sqrt(var + eps),  d_shift[g,c] = beta[c] - mean * d_scale[g,c],
 * mean / biased variance of the group's rows (fp32 accumulators, before the output is rounded).  DETERMINISTIC:
 * every row tile stores its column sums into its own slots of the workspace (no atomics) and a second small
 * kernel adds a group's slots in tile order.  Saves the separate read pass of avs_bn_batch_stats
 * (features/extractors.py:29,65: the ResNet trunk's train-mode BatchNorm).
 * avs_conv2d_bnstats_workspace_bytes: bytes of d_ws (uninitialised, 16-byte aligned) for this shape, or
 * AVS_E_UNSUPPORTED when rows_per_group < 64 (use avs_bn_batch_stats then).                                   */
int64_t avs_conv2d_bnstats_workspace_bytes(const avs_conv_desc* desc, int64_t rows_per_group);
int avs_conv2d_nhwc_bnstats(const avs_conv_desc* desc, const void* d_x, const void* d_w, void* d_y,
                            int64_t rows_per_group, const float* d_gamma, const float* d_beta, float eps,
                            float* d_scale, float* d_shift, void* d_ws, int64_t ws_bytes, avs_stream_t stream);
/* The same with the input given RAW: x is the raw output of the convolution before, whose BatchNorm (+ ReLU) the kernel
 * applies as it stages its operand, x'[m,c] = act(x[m,c] * d_in_scale[g,c] + d_in_shift[g,c]), g = m / rows_per_group
 * (the same groups as the output's), act = ReLU when in_relu, the multiply and the add rounded separately as in
 * avs_bn_apply; the zero padding is that of x'.  Outputs, scale and shift are bit-identical to avs_bn_apply (in place)
 * followed by avs_conv2d_nhwc_bnstats, without the apply pass over x.  d_in_scale / d_in_shift: fp32 [groups, cin],
 * 16-byte aligned.  AVS_F16X2 3x3 / stride 1 / pad 1 convolutions on a dense input at most 63 pixels wide that take the
 * 256-row tiles (the nine-tap form) only: every other shape returns AVS_E_UNSUPPORTED before launching anything.
 * The workspace is avs_conv2d_bnstats_workspace_bytes'.                                                          */
int avs_conv2d_nhwc_bnstats_xin(const avs_conv_desc* desc, const void* d_x, const void* d_w, void* d_y,
                                int64_t rows_per_group, const float* d_gamma, const float* d_beta, float eps,
                                float* d_scale, float* d_shift, void* d_ws, int64_t ws_bytes, const float* d_in_scale,
                                const float* d_in_shift, int in_relu, avs_stream_t stream);

/* Convolution + the WHOLE batch-statistics BatchNorm (+ residual, + ReLU) in one launch, bf16, for equal-sized
 * groups that fit a 256-row output tile whole:
 *   y[m,:] = act( bn_g(conv(x)[m,:]) + residual[m,:] ),  g = m / rows_per_group,  act = desc->act.
 * A tile holds floor(256 / rows_per_group) whole groups, so a group's statistics are sums over that tile's own
 * accumulators: no traffic between workgroups, no atomics, deterministic; one read of x, one write of y, nothing
 * raw in HBM.  Replaces avs_conv2d_nhwc_bnstats + avs_bn_apply for the 14x14 / 7x7 layers of the train-mode
 * ResNet trunk (features/extractors.py:29,65).
 * avs_conv2d_bnlocal_tile_rows returns the rows of a tile that are used (> 0) when the shape takes this form, or
 * AVS_E_UNSUPPORTED: not bf16; cout not a multiple of the column tile; groups of fewer than 37 or more than 256
 * rows or filling less than 3/4 of a tile; a reduction of at most 128 bytes; unaligned output rows.          */
int avs_conv2d_bnlocal_tile_rows(const avs_conv_desc* desc, int64_t rows_per_group);
int avs_conv2d_nhwc_bnlocal(const avs_conv_desc* desc, const void* d_x, const void* d_w, void* d_y,
                            int64_t rows_per_group, const float* d_gamma, const float* d_beta, float eps,
                            const void* d_residual, int64_t ldr, avs_stream_t stream);

/* The same for groups LARGER than a tile, AVS_F16X2: a group = `cluster` consecutive tiles of rows_per_group / cluster
 * rows each (193..224: one 14x14 map per tile - the reference's micro-batches of 4 frames at ResNet-50's layer 3,
 * features/extractors.py:48).  Every tile computes its own centred statistics (mean, sum of squares about it) from its
 * accumulators, publishes them per column as 8-byte {value, epoch} granules (one agent-scope store each: the tag is the
 * flag), reads its partners' granules, and merges them by Chan's update in tile order - every tile of the group obtains
 * the same bits; then normalises its accumulators (+ residual, + desc->act) and writes y once.  Nothing raw in HBM, no
 * statistics / apply passes, deterministic.  The tiles of a group take consecutive block ids (they are dispatched together);
 * the wait for a partner is bounded: the first word of d_xchg counts the waves whose wait ran out (0 after a healthy
 * launch; check it where results are validated).
 * ASSUMES that this launch's workgroups reach the CUs in block order from ONE queue (what a process that owns its GPU gets):
 * complete groups then always finish and free the CUs the next groups need.  When several queues feed the chip at once with
 * kernels of this kind - two streams, or processes time-sharing one GPU - each can hold partial groups that keep the other's
 * partners out; the bounded waits then end the launch and the counter says so (observed with 4 processes on one GPU).
 * desc->variant & AVS_CLUSTER_PACKED: the packed form.  Tiles are 224 CONSECUTIVE rows of the launch whatever
 * rows_per_group is, so no tile runs a 32-row block for 4 live rows: groups of 784 rows (four 14x14 maps) take 7 full tiles
 * per 2 groups instead of 8 of 196 rows, groups of 3136 rows (four 28x28 maps) 14 instead of 16.  A tile meets at most two
 * groups, the boundary inside it at row 112 only: rows_per_group >= 224 and = 0 or 112 (mod 224), a group touching at most
 * 16 tiles; `cluster` and every other condition as without the bit (AVS_E_UNSUPPORTED otherwise: the caller keeps the
 * unpacked form).  Each tile publishes one granule per lane and segment (its rows inside one group) and merges the segments
 * of its group - or of both its groups - in tile order with their row counts: the same bits on every tile of a group,
 * deterministic.  The workspace holds two granules per lane and tile of 224 rows (ask with the same desc).  The tiles that
 * wait for each other - one group's, or two groups' around their shared tile: at most 31 - take consecutive block ids, under
 * the same single-queue assumption.  Sums run in another fixed order than the unpacked form's: equal to rounding.
 * d_xchg: avs_conv2d_bncluster_workspace_bytes(...) bytes, 64-byte aligned, ZEROED ONCE by the caller when allocated and
 * then left alone; epoch: a value that is new for this buffer on every call (1, 2, 3, ...; never 0) - granules of earlier
 * calls are then recognisably stale, nothing needs clearing between calls.
 * AVS_E_UNSUPPORTED: not AVS_F16X2, tiles of fewer than 193 or more than 224 rows, cout not a multiple of 128.          */
int64_t avs_conv2d_bncluster_workspace_bytes(const avs_conv_desc* desc, int64_t rows_per_group, int cluster);
int avs_conv2d_nhwc_bncluster(const avs_conv_desc* desc, const void* d_x, const void* d_w, void* d_y,
                              int64_t rows_per_group, int cluster, const float* d_gamma, const float* d_beta, float eps,
                              const void* d_residual, int64_t ldr, void* d_xchg, int64_t xchg_bytes, uint32_t epoch,
                              avs_stream_t stream);
/* AVS_F16X2, 1x1 convolutions whose BatchNorm groups are too large for a tile (the expanding 1x1 layers of ResNet
 * layers 1-2: conv3 and the downsample branch, features/extractors.py:29,65): the batch statistics of the OUTPUT are
 * taken from the second moments of the narrow INPUT (avs_bn_gram_affine_f16x2: mean_y = W mean(a),
 * var_y[n] = w_n^T C w_n, C = a^T a / R - mean mean^T per group), then the convolution is ONE streaming pass with the
 * folded affine in its epilogue (avs_conv2d_nhwc_affine) - the wide output is written once and never re-read.
 *
 * avs_bn_gram_affine_f16x2: x [groups * rows_per_group, k] (k = 64 | 128, row stride lin_stride slots), w [n, k]
 * (n a multiple of 32), both AVS_F16X2.  With d_in_scale / d_in_shift fp32 [groups, k] x is the RAW output of the
 * convolution before, a = relu(x * in_scale + in_shift) (that layer's BatchNorm + ReLU: this pass is its apply
 * pass) and, with d_a_out (may be d_x itself), the finished activation is stored.  Out: the folded affine of the
 * output BatchNorm, d_scale / d_shift fp32 [groups, n] = gamma / sqrt(var_y + eps), beta - mean_y * scale.
 * Deterministic; ~1e-6 relative on var_y for post-ReLU inputs (E[a a^T] - m m^T is formed in fp32).
 *
 * avs_conv2d_nhwc_affine: y = act((conv(x) * scale[g] + shift[g]) + residual * res_scale[g] + res_shift[g]),
 * g = output_row / rows_per_group (>= 32), desc->dtype AVS_F16X2, 1x1 kernel without padding, more than 32 input
 * channels; scale / shift (and the optional residual affine: the residual is then itself a raw convolution output)
 * fp32 [groups, cout]; residual AVS_F16X2 [rows, cout] with row stride ldr or NULL; act = desc->act.              */
int avs_bn_gram_affine_f16x2(const void* d_x, int64_t lin_stride, int k, const float* d_in_scale,
                             const float* d_in_shift, const void* d_w, int64_t ldb, int n, int64_t rows_per_group,
                             int groups, const float* d_gamma, const float* d_beta, float eps, float* d_scale,
                             float* d_shift, void* d_a_out, int64_t lda, avs_stream_t stream);
int avs_conv2d_nhwc_affine(const avs_conv_desc* desc, const void* d_x, const void* d_w, void* d_y,
                           int64_t rows_per_group, const float* d_scale, const float* d_shift,
                           const void* d_residual, int64_t ldr, const float* d_res_scale, const float* d_res_shift,
                           avs_stream_t stream);

/* The whole ResNet-50 stem of the bf16 throughput path: uint8 frames [n,224,224,3] -> (x / denom - mean) / std ->
 * conv1 7x7/2 (64 channels) -> bn1 in batch-statistics mode over groups of frames_per_group frames -> ReLU ->
 * maxpool 3x3/2 pad 1 -> d_y bf16 [n,56,56,64]  (features/extractors.py:126-140 + children()[0:4] of the trunk, :29,65).
 * Because y -> relu(scale * y + shift) is monotone, the 3x3/2 pooling is done on the RAW convolution output on chip
 * before the statistics exist - as a max for the channels with gamma >= 0 and a min for the others (sign(scale) =
 * sign(gamma)): bit-identical to avs_frames_normalize_u8 + avs_conv2d_nhwc_bnstats + avs_bn_maxpool_nhwc on the
 * same convolution values, with 1.35 instead of 4.6 MB of HBM traffic per frame (the normalised image and the
 * 112x112x64 map never reach HBM).
 * apply = 1: d_y receives the finished activations (relu applied when relu != 0).
 * apply = 0: d_y receives the pooled RAW map; the consumer applies relu(scale * y + shift) per group and channel
 *            while staging it (the d_in_scale / d_in_shift operands of avs_conv1x1_affine_bf16 and
 *            avs_bn_gram_affine_bf16): one pass over the map less.
 * d_w: bf16 [64, ldw >= 224], a row = 7 kernel rows x 8 pixels x 4 channels (zero where kx = 7 or channel = 3).
 * d_scale / d_shift [n / frames_per_group, 64] receive bn1's folded affine.  Deterministic (per-tile partial sums
 * added in a fixed order).  d_ws: avs_stem_workspace_bytes(n) bytes, uninitialised.
 * n must be a multiple of frames_per_group (AVS_E_UNSUPPORTED otherwise: use the unfused sequence).                */
int64_t avs_stem_workspace_bytes(int n);
int avs_stem_conv_bn_pool_bf16(const uint8_t* d_frames, int n, float denom, const float* mean3, const float* std3,
                               const void* d_w, int64_t ldw, int frames_per_group, const float* d_gamma,
                               const float* d_beta, float eps, int apply, int relu, void* d_y, float* d_scale,
                               float* d_shift, void* d_ws, int64_t ws_bytes, avs_stream_t stream);

/* The ResNet-50 stem of the AVS_F16X2 (parity-grade) path in one kernel + a fold: uint8 frames [n,224,224,3] ->
 * conv1 7x7/2 of (x / denom - mean) / std -> the batch statistics of bn1 over groups of frames_per_group frames, and the
 * 3x3/2 pad-1 pooling of the RAW convolution output -> d_y AVS_F16X2 [n,56,56,64]: per channel the window's maximum
 * (gamma >= 0) or minimum (gamma < 0), i.e. maxpool(relu(bn1(.))) = relu(scale * d_y + shift) exactly (monotone map,
 * sign(scale) = sign(gamma)); the consumer applies that affine + ReLU (avs_bn_gram_affine_f16x2's d_in_scale / d_in_shift).
 * Replaces avs_frames_normalize_u8 + avs_conv2d_nhwc_bnstats + avs_bn_maxpool_nhwc of features/extractors.py:126-140 +
 * children()[0:4] (:29,65); the normalised image and the 112x112x64 map never reach HBM.
 * The normalisation is folded into the operands (x is affine in the byte value v, and bytes are exact fp16 numbers):
 *   d_w    AVS_F16X2 [64, ldw >= 224 slots], a row = 7 kernel rows x 8 pixels x 4 channels (zero where kx = 7):
 *          channels 0-2 = w[o,c,ky,kx] / (denom * std_c); channel 3 = -sum_c w[o,c,ky,kx] * mean_c / std_c, which the
 *          kernel multiplies by 1 for a pixel inside the image and 0 outside (the convolution's zero padding is of
 *          the NORMALISED input: only the taps inside contribute their constant).
 * Two fp16 MFMAs per product (the image has no lo half).  Statistics: per frame sums about a pivot (the frame's own
 * output at an interior pixel), frames merged by Chan's update in frame order: centred, deterministic.
 * d_scale / d_shift [n / frames_per_group, 64]: bn1's folded affine.  d_ws: avs_stem_f16x2_workspace_bytes(n) bytes.
 * n must be a multiple of frames_per_group (AVS_E_UNSUPPORTED otherwise: use the unfused sequence).                  */
int64_t avs_stem_f16x2_workspace_bytes(int n);
int avs_stem_conv_pool_f16x2(const uint8_t* d_frames, int n, const void* d_w, int64_t ldw, int frames_per_group, const float* d_gamma, const float* d_beta, float eps, void* d_y,
                             float* d_scale, float* d_shift, void* d_ws, int64_t ws_bytes, avs_stream_t stream);

/* 1x1 convolution + batch-statistics BatchNorm (+ residual, + ReLU) in one kernel, bf16, for equal-sized
 * groups of rows_per_group consecutive rows (a micro-batch of frames at one resolution):
 *   y[m,:] = act( bn_g(x[m,:] . w^T) + residual[m,:] ),  statistics of group g = m / rows_per_group.
 * One workgroup owns a whole group for a slab of channels and walks it twice (statistics, then the
 * normalised output), so the raw convolution never goes to HBM: replaces avs_conv2d_nhwc_bnstats +
 * avs_bn_apply for the 1x1 layers of the train-mode ResNet trunk
 * (features/extractors.py:65).  x rows at stride lin_stride >= k; k, n and strides multiples of 8 elements. */
int avs_conv1x1_bn_bf16(const void* d_x, int64_t lin_stride, int k, const void* d_w, int64_t ldb, int n,
                        int64_t rows_per_group, int groups, const float* d_gamma, const float* d_beta,
                        float eps, const void* d_residual, int64_t ldr, int relu, void* d_y, int64_t ldc,
                        avs_stream_t stream);

/* The same kernel reading a RAW convolution output as its input: the previous layer's BatchNorm + ReLU is applied
 * on the way in,  a[m,k] = bf16( relu( x[m,k] * d_in_scale[g,k] + d_in_shift[g,k] ) )  (avs_bn_apply's arithmetic:
 * bit-identical to running avs_bn_apply on x first), so the previous layer needs no apply pass at all: the
 * conv2 -> bn2 -> relu -> conv3 -> bn3 -> +identity -> relu tail of a ResNet bottleneck in two launches.
 * d_in_scale / d_in_shift are [groups, k] fp32 (avs_conv2d_nhwc_bnstats output); k <= 512 (else AVS_E_UNSUPPORTED).                      */
int avs_conv1x1_bn_in_bf16(const void* d_x, int64_t lin_stride, int k, const float* d_in_scale,
                           const float* d_in_shift, const void* d_w, int64_t ldb, int n,
                           int64_t rows_per_group, int groups, const float* d_gamma, const float* d_beta,
                           float eps, const void* d_residual, int64_t ldr, int relu, void* d_y, int64_t ldc,
                           avs_stream_t stream);

/* The expanding 1x1 layers of ResNet layers 1-2 in ONE streaming pass: the BatchNorm statistics of y = a . w^T
 * follow from the Gram matrix of the (narrow) input,
 *   mean_y[n] = w_n . mean(a),  var_y[n] = w_n^T C w_n,  C = a^T a / R - mean(a) mean(a)^T  per group of R rows,
 * so avs_bn_gram_affine_bf16 reads only a (k = 64 or 128 channels; a^T a and W . C on the matrix cores, C carried as
 * bf16 hi + lo = 16 significant bits, everything else fp32; deterministic) and writes the folded affine
 * d_scale / d_shift [groups, n] of bn(conv(a)); avs_conv1x1_affine_bf16 is then the convolution with that affine
 * (+ residual, + ReLU) in its epilogue - no statistics pass over the wide output.  Same operands and meaning as
 * avs_conv1x1_bn_in_bf16 (d_in_scale / d_in_shift = NULL: a is x itself; else a = bf16(relu(x * in_scale + in_shift)),
 * the previous layer's BatchNorm applied on the way in).  Replaces avs_conv1x1_bn[_in]_bf16 for k in {64, 128},
 * n % 32 == 0 (features/extractors.py:29,65: conv3 / downsample of the train-mode ResNet bottlenecks); other
 * shapes: AVS_E_UNSUPPORTED.  Statistics agree with the two-pass kernel's to fp32 rounding, not bit for bit.
 * d_res_scale / d_res_shift (both or neither; fp32 [groups, n]): the residual is itself a RAW convolution output
 * (the downsample branch of a bottleneck, :29) whose BatchNorm is folded into the add,
 *   y = act( conv(a) * scale + shift + residual * res_scale + res_shift ),
 * so the downsample branch needs no apply pass of its own.
 * d_a_out (avs_bn_gram_affine_bf16; NULL = off; needs d_in_scale): the transformed input a is also stored, bf16
 * [rows, lda >= k] - d_a_out == d_x (lda == lin_stride) overwrites the raw input in place - so that the convolution
 * pass can read a finished input (d_in_scale = NULL) instead of transforming it once per 128-column slab.         */
int avs_bn_gram_affine_bf16(const void* d_x, int64_t lin_stride, int k, const float* d_in_scale,
                            const float* d_in_shift, const void* d_w, int64_t ldb, int n, int64_t rows_per_group,
                            int groups, const float* d_gamma, const float* d_beta, float eps, float* d_scale,
                            float* d_shift, void* d_a_out, int64_t lda, avs_stream_t stream);
int avs_conv1x1_affine_bf16(const void* d_x, int64_t lin_stride, int k, const float* d_in_scale,
                            const float* d_in_shift, const void* d_w, int64_t ldb, int n, int64_t rows_per_group,
                            int groups, const float* d_scale, const float* d_shift, const void* d_residual,
                            int64_t ldr, const float* d_res_scale, const float* d_res_shift, int relu, void* d_y,
                            int64_t ldc, avs_stream_t stream);

/* The library holds NO process-global mutable state: the tile / staging variant of a convolution is chosen per call
 * (avs_conv_desc.variant), everything else by fixed rules.  (The kernel-study build, `make study` ->
 * lib/libavsum_hip_study.so, additionally exports void avs_debug_flags(int) and the avs_tune_* setters of the rules'
 * thresholds for tools/; the shipped library has no such code paths and no such symbols.)                        */

/* Batched C[b] = act(alpha * A[b] . B[b]^T + bias):  A [M,K] (row stride lda),
 * B [N,K] (row stride ldb; the nn.Linear weight layout), C [M,N] (ldc).
 * Replaces nn.Linear (models/av_model.py:10-15,29-31; models/attention.py:8-11;
 * features/extractors.py:193), the LSTM input projections (av_model.py:18-23),
 * the in/out projections of nn.MultiheadAttention (av_model.py:26) and the two
 * einsums of models/attention.py:21,23.  K, lda, ldb, stride_a and stride_b
 * multiples of 16 bytes, A and B 16-byte aligned; ldb >= K; lda >= 0, and
 * lda = 0 is a broadcast row (every row of A is the one row).  C is free: any
 * ldc >= N, any stride_c (batch entries may interleave in the columns as long as
 * they do not overlap) and any element-aligned d_c are accepted, and nothing
 * outside [M, N] of a batch entry is written; the bf16 store is vectorised
 * (16 bytes) only for a 16-byte-aligned d_c with 16-byte row strides, and goes
 * element by element otherwise.  M = 0 is AVS_OK and launches nothing.
 * (tests/test_gpu_gemm_f64.py holds every kernel instance behind this entry
 * point to float64 on these layouts.)                                        */
int avs_gemm_nt(int dtype, int m, int n, int k,
                const void* d_a, int64_t lda, int64_t stride_a,
                const void* d_b, int64_t ldb, int64_t stride_b,
                void* d_c, int64_t ldc, int64_t stride_c,
                const float* d_bias, int bias_mode, int64_t stride_bias,
                float alpha, int act, int batch, avs_stream_t stream);

/* ---- visual front end (K1, K2, K4, K5, K7) ------------------------------ */

/* uint8 HWC frames -> normalised, zero-padded NHWC images with 4 channels
 * (4th = 0), in `dtype`:  out[n, pad_t+y, pad_l+x, c] = (src/denom - mean[c]) / std[c]
 * (then the per-channel affine a[c]*v + b[c] when affine6 = {a0,a1,a2,b0,b1,b2}
 * is given: torchvision inception_v3 transform_input).  Replaces _preprocess_frame
 * (features/extractors.py:126-140; denom 1, i.e. NO /255) and the arithmetic of
 * _preprocess_inception (:142-155; denom 255).  out is [n, out_h, out_w, 4].
 * mean3 / std3 / affine6 are HOST pointers (copied into the launch).         */
int avs_frames_normalize_u8(int dtype, const uint8_t* d_src, int n, int h, int w,
                            float denom, const float* mean3, const float* std3,
                            const float* affine6, void* d_out, int out_h, int out_w,
                            int pad_t, int pad_l, avs_stream_t stream);

/* Upload by a PULL kernel: `workgroups` 256-thread blocks read h_src_mapped - PINNED host memory by its device-visible
 * address (hipHostMalloc / torch pin_memory: the same pointer) - over PCIe and store to d_dst.  The upload's footprint on
 * the chip is the caller's choice, so the frames of the next pass can stream in beside the current pass's kernels
 * (the PCIe-inclusive path of the pipeline; the reference hands over host arrays, features/extractors.py:43).           */
int avs_pull_copy_u8(const uint8_t* h_src_mapped, uint8_t* d_dst, int64_t bytes, int workgroups, avs_stream_t stream);

/* OpenCV-style bilinear resize of uint8 HWC frames (cv2.resize INTER_LINEAR,
 * fixed-point 11-bit coefficients): features/extractors.py:132,147.          */
int avs_resize_bilinear_u8(const uint8_t* d_src, int n, int sh, int sw,
                           uint8_t* d_dst, int dh, int dw, avs_stream_t stream);

/* Batch-statistics BatchNorm2d, the mode the reference actually runs its
 * ResNet-50 trunk in (features/extractors.py:29 never calls .eval()):
 * statistics per (group, channel) over the rows of the group's frames, biased
 * variance, eps.  d_group_rows[g]..d_group_rows[g+1] are the row ranges of the
 * groups (a group = one micro-batch of <=4 frames, extractors.py:48-56).
 * Writes the folded affine  scale[g,c] = gamma*rstd,  shift[g,c] = beta - mean*scale.
 * A group with no rows gets scale[g,:] = shift[g,:] = 0 (avs_segment_mean_f32's convention: empty -> zeros).
 * Alignment: d_x 16 bytes (32 for AVS_F16X2); c and ldx multiples of 4 (8 for AVS_F16X2); else AVS_E_ALIGN / _SHAPE. */
int avs_bn_batch_stats(int dtype, const void* d_x, int64_t rows, int c, int64_t ldx,
                       const int64_t* d_group_rows, int groups,
                       const float* d_gamma, const float* d_beta, float eps,
                       float* d_scale, float* d_shift, avs_stream_t stream);

/* y = act( x*scale[g] + shift[g] (+ residual) ), rows of group g as above;
 * max_group_rows = the largest group's row count (sizes the launch).
 * groups==0 with d_group_rows NULL: one affine for all rows (folded eval BN).
 * y may be x (in place), with or without a residual.
 * Alignment (AVS_E_ALIGN otherwise): d_x, d_y and d_residual 16 bytes in fp32, 8 bytes in bf16 (16 bytes, with c and
 * every stride a multiple of 8, selects the 8-wide bf16 kernel), 32 bytes in AVS_F16X2; d_scale / d_shift 16 bytes.
 * c and the strides are multiples of 4 (8 for AVS_F16X2).                      */
int avs_bn_apply(int dtype, const void* d_x, int64_t rows, int c, int64_t ldx,
                 const int64_t* d_group_rows, int groups, int64_t max_group_rows,
                 const float* d_scale, const float* d_shift,
                 const void* d_residual, int64_t ldr, int act,
                 void* d_y, int64_t ldy, avs_stream_t stream);

/* 2-D pooling on NHWC.  mode 0 = max (padding = -inf), 1 = average with
 * count_include_pad (torch defaults).  ResNet maxpool 3x3/2 p1, Inception
 * max 3x3/2 p0 and avg 3x3/1 p1.  y may be a channel slice (y_px_stride).
 * d_bias (fp32 [c], may be NULL) and act (AVS_ACT_NONE / AVS_ACT_RELU) are applied after the pooling:
 * y = act(pool(x) + bias).  Inception's branch_pool (avg_pool2d 3x3/1 -> 1x1 conv -> folded BN -> ReLU,
 * torchvision inception.py as loaded at features/extractors.py:26) runs as 1x1 conv WITHOUT bias -> this call:
 * averaging and a 1x1 convolution commute (both linear; the zero padding of count_include_pad commutes too), and the
 * pooling then moves cout instead of cin channels (4-10x fewer).
 * Alignment (AVS_E_ALIGN otherwise): d_x and d_y 16 bytes in fp32, 8 bytes in bf16 (16 bytes, with c and both pixel
 * strides a multiple of 8, selects the 8-wide bf16 kernel), 32 bytes in AVS_F16X2; d_bias 4 bytes.  c and the pixel
 * strides are multiples of 4 (8 for AVS_F16X2).                                                                      */
int avs_pool2d_nhwc(int dtype, int mode, const void* d_x, int n, int h, int w, int c,
                    int64_t x_px_stride, int k, int s, int p, const float* d_bias, int act, void* d_y,
                    int ho, int wo, int64_t y_px_stride, avs_stream_t stream);

/* BatchNorm apply + ReLU + max pooling in one pass: y = maxpool_{k,s,p}( act( x*scale[g] + shift[g] ) ), g = the
 * group (d_group_rows ranges over INPUT rows, as in avs_bn_apply; groups == 0 / NULL: one affine) of the image.
 * The ResNet stem's bn1 -> relu -> maxpool (features/extractors.py:29) without writing the normalised
 * full-resolution map; bit-identical to avs_bn_apply followed by avs_pool2d_nhwc(max) (AVS_F16X2: the same stored
 * values - a value has more than one hi | lo image, and the two-kernel sequence splits twice).
 * An image belongs to the last group whose range starts at or before the image's first row: an empty group owns none.
 * Alignment (AVS_E_ALIGN otherwise): d_x and d_y as for avs_pool2d_nhwc; d_scale / d_shift 16 bytes.               */
int avs_bn_maxpool_nhwc(int dtype, const void* d_x, int n, int h, int w, int c, int64_t x_px_stride,
                        const int64_t* d_group_rows, int groups, const float* d_scale, const float* d_shift,
                        int relu, int k, int s, int p, void* d_y, int ho, int wo, int64_t y_px_stride,
                        avs_stream_t stream);

/* Global average pool: y[n,c] = mean over h*w (fp32 out).  (adaptive avgpool)
 * Alignment (AVS_E_ALIGN otherwise): d_x 16 bytes in fp32, 8 bytes in bf16, 32 bytes in AVS_F16X2; d_y 16 bytes;
 * c and ldy multiples of 4 (c of 8 for AVS_F16X2).                           */
int avs_global_avgpool_nhwc(int dtype, const void* d_x, int n, int hw, int c,
                            float* d_y, int64_t ldy, avs_stream_t stream);

/* Segment mean: out[s,:] = mean(x[seg[s]:seg[s+1], :]) summed in row order in
 * fp32 then divided (numpy .mean(axis=0), extractors.py:108-110); empty
 * segment -> zeros (extractors.py:44-45).                                   */
int avs_segment_mean_f32(const float* d_x, int64_t ldx, int d, const int64_t* d_seg,
                         int nseg, float* d_out, int64_t ldo, avs_stream_t stream);

/* Shot-boundary scan: d_sums[f, 0..2] = sum over the (strided) pixels of |H|,|S|,|V| differences
 * between frame f and f-1 in OpenCV's 8-bit HSV (d_sums[0,:] = 0): the per-frame content score of PySceneDetect's
 * ContentDetector is (sums / pixels).mean(), thresholded on the host (features/extractors.py:388-393).          */
int avs_hsv_frame_diff_u8(const uint8_t* d_frames, int n, int h, int w, int step, uint32_t* d_sums,
                          avs_stream_t stream);

/* ---- audio front end (K8-K12) ------------------------------------------- */

/* Reflect-pad a mono waveform by `pad` samples each side (torch.stft
 * center=True, pad_mode="reflect"); out has t + 2*pad samples (+ tail zeroed
 * up to out_len).                                                           */
int avs_reflect_pad_f32(const float* d_x, int64_t t, int pad, float* d_out,
                        int64_t out_len, avs_stream_t stream);

/* STFT of a (reflect-padded) waveform as a dense real DFT on the fp64 matrix cores:
 *   spec[f, c] = float( sum_n double(xpad[f*hop + n]) * basis_t[n, c] ),  f < frames, c < ncols
 * basis_t is [nfft, ncols_pad] float64 (window folded in; columns = re | im bins, zero padded to a
 * multiple of 64).  Replaces torch.stft inside torchaudio Spectrogram (features/extractors.py:237,242).
 * fp64 because log2(mel+1e-6) is ill-conditioned in quiet bins.            */
int avs_stft_f64(const float* d_xpad, int64_t xpad_len, int64_t frames, int hop, int nfft,
                 const double* d_basis_t, int ncols, int ncols_pad, float* d_spec,
                 avs_stream_t stream);

/* torchaudio MelSpectrogram / MFCC front end in ONE kernel (features/extractors.py:236-246: MelSpectrogram(sr,
 * n_mels) and MFCC(sr, n_mfcc) defaults: n_fft = win = 400, periodic Hann, hop 200, center + reflect padding, power
 * 2, onesided 201 bins): d_wave fp32 [t] (t > 200, 16-byte aligned) -> [1 + t / 200, nmel] each, any subset of
 *   d_log2mel = log2(mel + 1e-6)   (:245),   d_db = 10 log10(max(mel, 1e-10))   (AmplitudeToDB before its top_db
 *   clamp; d_max receives max(max(mel, 1e-10)) over the call for avs_clamp_topdb_f32; zero it first),   d_power = mel.
 * A workgroup stages the waveform span of its 32 frames in LDS (reflect padding by index, 16-byte loads), runs the
 * real DFT folded to half its length (d_window = the fp32 window values as float64 [AVS_FUSED_NFFT]; d_cos
 * [AVS_FUSED_RE_ROWS, AVS_FUSED_COLS] / d_sin [AVS_FUSED_IM_ROWS, AVS_FUSED_COLS] = cos / -sin(2 pi k n / 400), float64) on the fp64 matrix cores, then |X|^2, the sparse mel sum
 * (d_fb [201, nmel], filter m non-zero on bins d_fb_lo[m] .. d_fb_hi[m] - 1) and the log on chip: the spectrum
 * never reaches HBM.  Replaces avs_reflect_pad_f32 + avs_stft_f64 + avs_power_mel_f32 for this front end.          */
int avs_stft_mel_fused_f32(const float* d_wave, int64_t t, const double* d_window, const double* d_cos,
                           const double* d_sin, const float* d_fb, const int* d_fb_lo, const int* d_fb_hi, int nmel,
                           float* d_log2mel, float* d_db, float* d_power, float* d_max, avs_stream_t stream);
/* The same front end reduced to TIME MEANS per segment (a shot's slice of the track): d_blocks int32 [nblocks, 3] =
 * (first STFT frame, frames <= 32, segment) - every segment cut into runs of at most 32 frames, in order -,
 * d_seg_block int32 [nseg + 1] = first block of each segment, d_seg_frames int32 [nseg] = its frame count.  Out:
 * d_mean_log2 [nseg, ld_log2] = mean over the segment's frames of log2(mel + 1e-6), d_mean_db [nseg, ld_db] = mean of
 * max(10 log10(max(mel, 1e-10)), 10 log10(*d_max) - top_db) - by linearity the DCT / mfcc_proj of that mean IS the mean
 * of the MFCC rows (features/extractors.py:232-246 pool the per-frame matrices over time).  *d_max = the largest
 * clamped mel power the clamp is relative to:
 *   find_max = 0: given by the caller (an avs_stft_mel_fused_f32 call with only d_max requested: a second pass of the
 *                 DFT over the track) - nothing per frame reaches HBM;
 *   find_max = 1: found by THIS call over the frames of its blocks (a table that covers the whole track gives the track
 *                 maximum): ONE pass of the DFT that writes the blocks' unclamped dB rows to the workspace, then a
 *                 bandwidth-bound pass clamps and sums them - the same values in the same order, bit-identical to
 *                 find_max = 0 with that maximum.  *d_max is overwritten.
 * d_ws: avs_stft_mel_segmean_workspace_bytes(...) bytes; deterministic (block partial sums folded in order).          */
int64_t avs_stft_mel_segmean_workspace_bytes(int nblocks, int nmel, int want_log2, int want_db, int find_max);
int avs_stft_mel_segmean_f32(const float* d_wave, int64_t t, const double* d_window, const double* d_cos,
                             const double* d_sin, const float* d_fb, const int* d_fb_lo, const int* d_fb_hi, int nmel,
                             const int* d_blocks, int nblocks, const int* d_seg_block, const int* d_seg_frames, int nseg,
                             float* d_max, int find_max, float top_db, float* d_mean_log2, int64_t ld_log2,
                             float* d_mean_db, int64_t ld_db, void* d_ws, int64_t ws_bytes, avs_stream_t stream);
/* The same for a BATCH of tracks in one set of launches (find_max = 1 semantics per track): d_waves holds the tracks one
 * after another - track i at sample offset d_track_off[i] (a multiple of 4: 16-byte aligned), d_track_len[i] samples -,
 * d_blocks int32 [nblocks, 4] = (first STFT frame inside its track, frames <= 32, segment, track), segments numbered over
 * the whole batch (d_seg_block / d_seg_frames as above), d_max fp32 [ntracks] receives every track's maximum.  Four
 * launches for all tracks of a batch instead of five per track (configs[2]: 50 tracks).                                */
int avs_stft_mel_segmean_batch_f32(const float* d_waves, const int64_t* d_track_off, const int64_t* d_track_len, int ntracks,
                                   const double* d_window, const double* d_cos, const double* d_sin, const float* d_fb,
                                   const int* d_fb_lo, const int* d_fb_hi, int nmel, const int* d_blocks, int nblocks,
                                   const int* d_seg_block, const int* d_seg_frames, int nseg, float* d_max, float top_db,
                                   float* d_mean_log2, int64_t ld_log2, float* d_mean_db, int64_t ld_db, void* d_ws,
                                   int64_t ws_bytes, avs_stream_t stream);

/* PER-SHOT time means for the shots of a batch of tracks, each shot its own signal (features/extractors.py:351-356 slice
 * the waveform and :195-234 run the extractor on the slice): d_waves fp32 [waves_len] holds the tracks one after another
 * (16-byte aligned; track i at sample offset d_track_off[i], a multiple of 4, d_track_len[i] samples; waves_len a
 * multiple of 4), d_shots int64 [nshot, 3] = (track, first sample inside the track - any offset -, present length L after
 * clipping to the track).  Shot s is the signal x = clamp(pad(slice, Lp), -1, 1) with Lp = max(L, 960) (samples L .. Lp-1
 * zero), reflect padded by 200 at ITS first and last sample: 1 + Lp / 200 STFT frames, read in place (no per-shot copy).
 * d_blocks int32 [nblocks, 3] = (first STFT frame inside the shot, frames <= 32, shot) - every shot cut into runs of at
 * most 32 frames -, d_seg_block int32 [nshot + 1] = first block of each shot, d_seg_frames int32 [nshot] = its frames.
 * Out: d_mean_log2 [nshot, ld_log2] = time mean of log2(mel + 1e-6), d_mean_db [nshot, ld_db] = time mean of the dB mel
 * clamped at 10 log10(d_max[s]) - top_db, d_max fp32 [nshot] = each shot's OWN largest clamped mel power (find_max = 1
 * semantics per shot: one pass of the DFT writes the unclamped dB rows to the workspace, a bandwidth-bound pass clamps
 * and sums them).  Shots are independent: they may overlap, be unsorted or be empty; an empty shot (L = 0) has no blocks
 * and no launch work and its rows are zero.  Index fields are clamped on the device so that no load leaves the buffer.
 * d_ws: avs_stft_mel_shots_workspace_bytes(...) bytes; deterministic (block partial sums folded in order).              */
int64_t avs_stft_mel_shots_workspace_bytes(int nblocks, int nmel, int want_log2, int want_db);
int avs_stft_mel_shots_f32(const float* d_waves, int64_t waves_len, const int64_t* d_track_off, const int64_t* d_track_len,
                           int ntracks, const int64_t* d_shots, int nshot, const double* d_window, const double* d_cos,
                           const double* d_sin, const float* d_fb, const int* d_fb_lo, const int* d_fb_hi, int nmel,
                           const int* d_blocks, int nblocks, const int* d_seg_block, const int* d_seg_frames, float* d_max,
                           float top_db, float* d_mean_log2, int64_t ld_log2, float* d_mean_db, int64_t ld_db, void* d_ws,
                           int64_t ws_bytes, avs_stream_t stream);

/* VGGish log-mel examples of a ragged batch (vggish_input.waveform_to_examples per shot): example e = AVS_VGG_FRAMES (96)
 * frames of AVS_VGG_WINDOW (400) samples at hop AVS_VGG_HOP (160) (no padding) starting at sample d_ex_start[e] (int64 [nex]) of d_waves (waves_len samples; a start
 * is clamped on the device into [0, waves_len - 15600]), each sample clamped to [-1, 1] at load.  d_out fp32 [nex, 96,
 * nmel] = ln(|STFT| . mel + 0.01); d_basis_t as avs_stft_f64 ([AVS_VGG_WINDOW, ncols_pad] float64, AVS_VGG_BINS (257) re | as
 * many im columns), d_fb [AVS_VGG_BINS, nmel] as avs_power_mel_f32.  Two launches (the fp64 DFT into the workspace, then avs_power_mel_f32 mode 3's
 * kernel): the per-frame arithmetic of avs_stft_f64 + avs_power_mel_f32 mode 3, so the examples are bit-identical to those
 * of a clamped slice.  d_ws: avs_vggish_examples_workspace_bytes(nex) bytes.  nex = 0: no launch.                      */
int64_t avs_vggish_examples_workspace_bytes(int64_t nex);
int avs_vggish_examples_f32(const float* d_waves, int64_t waves_len, const int64_t* d_ex_start, int64_t nex,
                            const double* d_basis_t, int ncols_pad, const float* d_fb, const int* d_fb_lo, const int* d_fb_hi,
                            int nmel, float* d_out, void* d_ws, int64_t ws_bytes, avs_stream_t stream);

/* Power spectrum -> mel filterbank -> log.  d_spec is [frames, 2*nbins]
 * (re | im per frame, from avs_gemm_nt against the windowed DFT basis);
 * d_fb is [nbins, nmel] (torchaudio melscale_fbanks layout).
 *   mode 0: out = log2(mel + 1e-6)          (features/extractors.py:245)
 *   mode 1: out = 10*log10(max(mel,1e-10)), and atomically folds the maximum
 *           of max(mel,1e-10) into *d_max, which the caller zeroed
 *           (AmplitudeToDB, first half)
 *   mode 2: out = mel
 *   mode 3: the MAGNITUDE spectrum sqrt(re^2+im^2) through the filterbank, out = ln(mel + 0.01): the VGGish
 *           log-mel front end (torchvggish mel_features.log_mel_spectrogram; features/extractors.py:188,216) */
int avs_power_mel_f32(const float* d_spec, int64_t frames, int nbins,
                      const float* d_fb, const int* d_fb_lo, const int* d_fb_hi,
                      int nmel, int mode, float* d_out, float* d_max,
                      avs_stream_t stream);

/* x = max(x, 10*log10(*d_max) - top_db) in place (AmplitudeToDB top_db clamp). */
int avs_clamp_topdb_f32(float* d_x, int64_t count, const float* d_max, float top_db,
                        avs_stream_t stream);
int avs_fill_f32(float* d_x, int64_t count, float value, avs_stream_t stream);

/* y = rint((clamp(x, lo, hi) - lo) * scale), round-half-to-even, values kept as float: the 8-bit quantiser of the
 * VGGish post-processor (torchvggish Postprocessor.postprocess; features/extractors.py:188,216).              */
int avs_quantize_f32(const float* d_x, int64_t count, float lo, float hi, float scale, float* d_y,
                     avs_stream_t stream);

/* Channel mix-down + rational resampling by a polyphase FIR (the reference delegates to
 * pydub/ffmpeg set_channels(1).set_frame_rate(16000), features/extractors.py:364-378, and averages channels at
 * :326-328):  y[i*up + p] = sum_k mono[i*down + k - width] * d_taps[p*ntaps + k],  mono = mean over the
 * interleaved channels of d_x [t, channels], zero outside the clip.  The taps come from the host (audio.py).   */
int avs_resample_f32(const float* d_x, int64_t t, int channels, const float* d_taps, int up, int down,
                     int ntaps, int width, float* d_y, int64_t out_len, avs_stream_t stream);

/* ---- importance scorer (K17-K19) ---------------------------------------- */

/* Batched LSTM recurrences, PyTorch gate order i,f,g,o, h0=c0=0
 * (nn.LSTM at models/av_model.py:18-23,39-40).
 *   d_xproj [rows, ndir*4H]: x_t.W_ih^T + b_ih + b_hh for every direction
 *           (direction d occupies columns d*4H..), rows = sum of seq lengths;
 *   d_whh_t [ndir, H, 4H]: W_hh TRANSPOSED per direction;
 *   d_seq_rows[s]..d_seq_rows[s+1]: the rows of sequence s;
 *   reverse_mask bit d set = direction d runs t = T-1..0;
 *   d_out [rows, ldo]: h_t of direction d at columns out_col0 + d*H.
 *   variant: 0 = the library's choice.  hidden = 256 keeps part of W_hh^T on chip for the whole sequence
 *           (AVS_LSTM_RESIDENT_20_8: 20 of a thread's 64 row-vectors in registers + 8 in LDS, the default there;
 *           AVS_LSTM_RESIDENT_16_8: 16 + 8) instead of streaming all of it from L2 every step (AVS_LSTM_STREAM).
 *           Same arithmetic in the same order: bit-identical outputs.                                             */
enum { AVS_LSTM_AUTO = 0, AVS_LSTM_STREAM = 1, AVS_LSTM_RESIDENT_20_8 = 2, AVS_LSTM_RESIDENT_16_8 = 3 };
int avs_lstm_f32(const float* d_xproj, const float* d_whh_t, int hidden, int ndir,
                 unsigned reverse_mask, const int64_t* d_seq_rows, int nseq,
                 float* d_out, int64_t ldo, int out_col0, int variant, avs_stream_t stream);

/* Attention core of nn.MultiheadAttention fed [B,T,E] WITHOUT batch_first
 * (models/av_model.py:26,44): for every time-step t and head h,
 * softmax over the B axis.  d_qkv [B*T, 3E] (q|k|v, already projected),
 * d_ctx [B*T, E].  One wave per (t, head, b); wave-shuffle softmax.          */
int avs_mha_batchaxis_f32(const float* d_qkv, int b, int t, int e, int heads,
                          float* d_ctx, avs_stream_t stream);

/* scores[r] = sigmoid( dot(hid[r,:], w2) + b2 )  (scorer.2 + Sigmoid,
 * models/av_model.py:30).                                                    */
int avs_score_head_f32(const float* d_hid, int64_t rows, int d, int64_t ldh,
                       const float* d_w2, const float* d_b2, float* d_scores,
                       avs_stream_t stream);

/* Fused attention core of models/attention.py:21-24 (flash style: the [T,T] scores never reach memory):
 *   ctx[b,q,h*D+:] = softmax_k( Q[b,q,h,:] . K[b,k,h,:] / sqrt(D) ) . V[b,k,h,:]
 * d_q / d_k / d_v are the projected [b*t, heads*D] matrices (row stride ld), head_dim D in {64, 128, 256}.
 * fp32 MFMA for both products, per-query online softmax folded with one wave shuffle.                      */
int avs_mhsa_flash_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ld, int b, int t,
                       int heads, int head_dim, float* d_ctx, int64_t ldo, avs_stream_t stream);
/* The same fused core with AVS_F16X2 operands (d_q / d_k / d_v: the projections after avs_f16x2_pack_f32, row stride
 * ld slots; d_ctx fp32): every product hi*hi + lo*hi + hi*lo on v_mfma_f32_32x32x16_f16 (2^-21 relative, fp32
 * accumulation; the probabilities are split in registers), on 16-query tiles (v_mfma_f32_16x16x32_f16: 64
 * accumulator + 64 Q-fragment registers per lane at head dim 256, two waves per SIMD).  Whole forward at E = 1024,
 * H = 4, T = 5000: 1.40 ms against 2.69 ms for the fp32 form and 2.30 ms for the batched-GEMM path that materialises
 * the 400 MB of scores (models/attention.py:21-24).                                                               */
int avs_mhsa_flash_f16x2(const void* d_q, const void* d_k, const void* d_v, int64_t ld, int b, int t, int heads,
                         int head_dim, float* d_ctx, int64_t ldo, avs_stream_t stream);

/* Row softmax in place: x[r, 0:n] for `rows` rows of stride ldx
 * (torch.softmax(dim=-1) at models/attention.py:22).                         */
int avs_softmax_rows_f32(float* d_x, int64_t rows, int n, int64_t ldx,
                         avs_stream_t stream);
/* Backward of that softmax, in place on the upstream gradient: dp[r, j] <- alpha * p[r, j] * (dp[r, j] -
 * sum_k p[r, k] dp[r, k]), the gradient with respect to the unscaled scores of softmax(alpha * q.k^T)
 * (autograd through models/attention.py:21-22; the reference class is an ordinary autograd module).       */
int avs_softmax_bwd_rows_f32(const float* d_p, float* d_dp, int64_t rows, int n, int64_t ld, float alpha,
                             avs_stream_t stream);

/* ---- scorer backward (K22; scripts/train_av_model.py:86-96) ------------------ */
/* The dense parts of the backward reuse avs_gemm_nt on transposed copies (dX = dY.W uses W^T as the [N,K]
 * operand, dW = dY^T.X uses dY^T and X^T); the entry points below are the rest.                           */

/* dst[c, r] = src[r, c]; dst row stride ld_dst >= rows (pad columns are left untouched).                  */
int avs_transpose_f32(const float* d_src, int rows, int cols, int64_t ld_src, float* d_dst, int64_t ld_dst,
                      avs_stream_t stream);
/* out[c] = sum_r x[r,c] * (row_weight ? row_weight[r] : 1): bias gradients; deterministic order.          */
int avs_colsum_f32(const float* d_x, int64_t rows, int cols, int64_t ld, const float* d_row_weight,
                   float* d_out, avs_stream_t stream);
/* out = dy * (keep ? keep : 1) * (relu_out > 0): gradient through Dropout(keep = mask/(1-p)) and ReLU
 * (models/av_model.py:10-15).                                                                             */
int avs_relu_dropout_bwd_f32(const float* d_dy, const float* d_relu_out, const float* d_keep, int64_t n,
                             float* d_out, avs_stream_t stream);
int avs_mul_f32(const float* d_a, const float* d_b, int64_t n, float* d_out, avs_stream_t stream);
/* dz[r] = ds[r]*s[r]*(1-s[r]);  dhid_pre[r,k] = dz[r]*w2[k]*(hid[r,k] > 0)   (scorer.2 + Sigmoid and the
 * ReLU of scorer.0 backwards, models/av_model.py:29-31).                                                  */
int avs_score_head_bwd_f32(const float* d_dscores, const float* d_scores, const float* d_hid, int64_t rows,
                           int d, int64_t ldh, const float* d_w2, float* d_dz, float* d_dhid_pre,
                           avs_stream_t stream);
/* avs_lstm_f32 that also saves the post-activation gates [rows, ndir*4H] (i,f,g,o) and the cell state
 * [rows, ndir*H] for the backward (the forward of scripts/train_av_model.py:88).  variant: AVS_LSTM_AUTO (hidden = 256:
 * W_hh^T partly resident in registers / LDS, as avs_lstm_f32 does) or AVS_LSTM_STREAM; bit-identical outputs.          */
int avs_lstm_train_fwd_f32(const float* d_xproj, const float* d_whh_t, int hidden, int ndir,
                           unsigned reverse_mask, const int64_t* d_seq_rows, int nseq, float* d_out,
                           int64_t ldo, int out_col0, float* d_gates, float* d_cell, int variant, avs_stream_t stream);
/* Backward through time (loss.backward() of scripts/train_av_model.py:93): from dL/dh_t (d_dout, same layout as the
 * forward's d_out) to the gradient of the pre-activations d_dxproj [rows, ndir*4H].  d_whh is W_hh in its ORIGINAL
 * layout [ndir, 4H, H].  variant: AVS_LSTM_AUTO (hidden = 256: W_hh partly resident on chip, the step's saved inputs
 * fetched one step ahead; sums in another fixed order than the streaming kernel's - equal to rounding, deterministic)
 * or AVS_LSTM_STREAM.                                                                                               */
int avs_lstm_bwd_f32(const float* d_dout, int64_t ldo, int out_col0, const float* d_gates,
                     const float* d_cell, const float* d_whh, int hidden, int ndir, unsigned reverse_mask,
                     const int64_t* d_seq_rows, int nseq, float* d_dxproj, int variant, avs_stream_t stream);

/* The hidden = 256 recurrence with ONE recurrence split over FOUR CUs (models/av_model.py:39-40 forward,
 * scripts/train_av_model.py:94-95 backward): each of the four workgroups of a recurrence owns 64 hidden units and keeps its
 * quarter of W_hh in registers for the whole sequence; per time step the four exchange the step's vector (h_t forward, the
 * gate gradients backward) through tagged 8-byte granules in the workspace.  Same arguments and bit-identical outputs as
 * avs_lstm_f32 / avs_lstm_train_fwd_f32 (d_gates and d_cell given: both or neither) / avs_lstm_bwd_f32 with AVS_LSTM_AUTO;
 * a time step costs ~1.6 us (forward) / 1.85 us (backward) instead of 5.2 / 5.3: for FEW recurrences (one video per
 * training step, a few dozen videos at inference).  A launch runs 4 * ndir * nseq workgroups of 512 threads, one per CU: up
 * to 64 recurrences are all resident at once; more run in rounds (partners are dispatched together: complete groups always
 * finish) and past ~250 recurrences avs_lstm_f32's one recurrence per CU is the faster use of the chip.
 * d_ws: avs_lstm_split_workspace_bytes(ndir, nseq) bytes, 8-byte aligned, ZEROED ONCE by the caller before its first use
 * and then left alone; epoch: tags of a launch are epoch + 1 ... epoch + longest sequence - the caller passes values whose
 * ranges do not overlap from launch to launch on the same workspace (e.g. a running sum of rows + 1) and stay below 2^32
 * (tag 0 is the zeroed workspace's: before the sum would wrap, zero the workspace again and start over).
 * The FIRST 64 bytes of the workspace hold an error word (uint32, first of them): the number of workgroups whose bounded
 * wait (2^20 polls: of the order of a second) for a partner ran out - 0 after a healthy launch; such a launch ends, its
 * outputs are incomplete.  The same single-queue assumption as avs_conv2d_nhwc_bncluster: not for GPUs time-shared between
 * processes, nor for two streams running such kernels at once.                                                       */
size_t avs_lstm_split_workspace_bytes(int ndir, int nseq);
int avs_lstm_split_f32(const float* d_xproj, const float* d_whh_t, int hidden, int ndir, unsigned reverse_mask,
                       const int64_t* d_seq_rows, int nseq, float* d_out, int64_t ldo, int out_col0, float* d_gates,
                       float* d_cell, void* d_ws, size_t ws_bytes, unsigned epoch, avs_stream_t stream);
int avs_lstm_bwd_split_f32(const float* d_dout, int64_t ldo, int out_col0, const float* d_gates, const float* d_cell,
                           const float* d_whh, int hidden, int ndir, unsigned reverse_mask, const int64_t* d_seq_rows,
                           int nseq, float* d_dxproj, void* d_ws, size_t ws_bytes, unsigned epoch, avs_stream_t stream);

/* ---- fusion (K13-K15) --------------------------------------------------- */

/* out[i,j] = sqrt(sum_d (double(v[i,d]) - double(a[j,d]))^2), float64 out
 * (scipy cdist "euclidean" at features/fusion.py:11).                        */
int avs_cdist_f64(const float* d_v, int tv, const float* d_a, int ta, int d,
                  double* d_out, avs_stream_t stream);

/* Exact DTW on a cost matrix [n,m] (features/fusion.py:15-18 intent; SURVEY
 * A.9): D = C + min(up, left, diag) with tie order up, left, diag; path from
 * (0,0) to (n-1,m-1) written as int64 pairs to d_path (capacity n+m-1 pairs),
 * its length to *d_path_len, total cost to *d_cost.  The three live
 * anti-diagonals stay in LDS (n <= AVS_FUSION_MAX_N); the workspace holds one predecessor
 * byte per cell.                                                            */
int64_t avs_dtw_workspace_bytes(int n, int m);
int avs_dtw_path_f64(const double* d_cost_matrix, int n, int m, void* d_workspace,
                     int64_t workspace_bytes, int64_t* d_path, int64_t* d_path_len,
                     double* d_cost, avs_stream_t stream);

/* out[u,:] = x[idx[u],:] * float(w[u])  (features/fusion.py:28-32).          */
int avs_gather_scale_f32(const float* d_x, int64_t ldx, int d, const int64_t* d_idx,
                         const double* d_w, int count, float* d_out,
                         avs_stream_t stream);

/* ---- batched fusion: P ragged (visual [n_p,D], audio [m_p,D]) pairs per call, a fixed number of launches ----------
 * The pairs are row ranges of two row-major fp32 matrices; nothing is padded.  d_pairs is int64 [npairs, AVS_FUSION_PAIR_COLS] =
 * (v_row0, n, a_row0, m, cell_off, path_off, row_off, 0): cell_off = first element of the pair's row-major [n, m]
 * block in the cost buffer (doubles) and in the code workspace (bytes), path_off = first row of its path slot
 * (capacity n + m - 1 rows), row_off = first of its n row counts.  The tables are trusted: the caller (ops.FusionTables)
 * guarantees that every range lies inside its buffer; the entry points check the host-side sizes only.  No entry
 * point synchronises or reads a result back.                                                                        */

/* Every pair's cost matrix, bit for bit avs_cdist_f64 of that pair.  d_tiles is int32 [ntiles, 3] = (pair, row tile,
 * column tile) over tiles of AVS_FUSION_TILE rows and columns; cells = the sum of n*m.                              */
int avs_cdist_batch_f64(const float* d_v, int64_t v_rows, const float* d_a, int64_t a_rows, int d,
                        const int64_t* d_pairs, int npairs, const int32_t* d_tiles, int64_t ntiles, double* d_cost,
                        int64_t cells, avs_stream_t stream);

/* Exact DTW of every pair (recurrence and tie order of avs_dtw_path_f64) + backtrack.  d_order is int32 [npairs]: the
 * pairs sorted into three size classes by l = min(n, m): the first n_small have l <= AVS_FUSION_SMALL_L (one wave per
 * pair, four pairs per workgroup), the next n_mid AVS_FUSION_SMALL_L < l <= AVS_FUSION_MID_L (256 threads per pair), the
 * last n_large l > AVS_FUSION_MID_L (1024 threads); max_l_* is the largest l of each class (it sizes that launch's LDS)
 * and max_n the largest n (<= AVS_FUSION_MAX_N).  One launch
 * per non-empty class.  Per pair: the path (int64 pairs, start to end) into its slot of d_path, d_path_len[p],
 * d_total[p], and d_rowcount[row_off + i] = the number of path cells in row i.  The workspace holds one predecessor
 * byte per cell.                                                                                                     */
int64_t avs_dtw_batch_workspace_bytes(int64_t cells);
int avs_dtw_batch_f64(const double* d_cost, int64_t cells, const int64_t* d_pairs, int npairs, const int32_t* d_order,
                      int n_small, int n_mid, int n_large, int max_l_small, int max_l_mid, int max_l_large, int max_n,
                      void* d_workspace, int64_t workspace_bytes, int64_t* d_path, int64_t* d_path_len,
                      double* d_total, int32_t* d_rowcount, avs_stream_t stream);

/* out[out_off[p] + i, :] = x[v_row0 + i, :] * float(double(rowcount[row_off + i]) / double(path_len[p])) for
 * i < min(n_p, target_length): interpolate_features (features/fusion.py:21-32) of every pair, the unique path rows
 * being 0..n-1.  d_row_pair is int32 [nrows] (nrows = the sum of n): the pair of each row count; d_out_off int64
 * [npairs] the first output row of each pair.                                                                        */
int avs_fused_gather_batch_f32(const float* d_x, int64_t ldx, int d, const int64_t* d_pairs, int npairs,
                               const int32_t* d_row_pair, int64_t nrows, const int64_t* d_out_off,
                               const int32_t* d_rowcount, const int64_t* d_path_len, int64_t target_length,
                               float* d_out, avs_stream_t stream);

/* ---- batched evaluation: the mean-threshold F1 and both rank correlations of V videos per call ---------------------
 * (scripts/evaluate.py:21-42, evaluation/metrics.py:1-9.)  The videos are the segments [offsets[v], offsets[v + 1]) of
 * concatenated vectors; d_offsets is int64 [nseg + 1], non-decreasing and inside the vectors (trusted, as the pair
 * tables above: ops.EvalTables guarantees it).  Every result is an integer or is computed in one fixed order, so two
 * calls on the same input give the same bytes.  No entry point synchronises or reads a result back.                  */

/* mean[v] = np.mean(x[a:b]) bit for bit - numpy's own order: buffers of 8192 elements summed left to right, each
 * buffer by numpy's pairwise rule (eight strided accumulators below 128 elements, halves cut at a multiple of 8
 * above), sum / n in the element type - and mask[r] = x[r] > mean[v] for the rows of segment v (rows outside every
 * segment are not written).  elem_bytes: 4 = float32, 8 = float64 (d_x and d_mean of that type).  One workgroup per
 * segment.                                                                                                           */
int avs_segment_mean_mask(const void* d_x, int elem_bytes, int64_t rows, const int64_t* d_offsets, int nseg,
                          void* d_mean, uint8_t* d_mask, avs_stream_t stream);

/* Per row i of every video, over all j of the same video: d_counts int32 [5, rows] = planes (#{x_j < x_i},
 * #{x_j == x_i} self included, the same two on y, sum_j sign(x_i - x_j) sign(y_i - y_j)), x = d_pred (float32),
 * y = d_target (target_bytes 4 = float32, 8 = float64).  IEEE comparisons (-0.0 == 0.0); the inputs must be finite.
 * d_tiles is int32 [ntiles, 2] = (video, row tile) over tiles of AVS_EVAL_TILE rows; max_t = the longest video
 * (<= AVS_EVAL_MAX_T).                                                                                               */
int avs_rank_pair_counts(const float* d_pred, const void* d_target, int target_bytes, int64_t rows,
                         const int64_t* d_offsets, int nseg, const int32_t* d_tiles, int64_t ntiles, int max_t,
                         int32_t* d_counts, avs_stream_t stream);

/* d_out int64 [nseg, AVS_EVAL_COLS] = (T, n_pred, n_tgt, tp, S2, E_x, E_y, S_xy, S_xx, S_yy) per video: the mask sums and their
 * overlap, S2 = sum s = 2 (concordant - discordant), E = sum eq (tied pairs = (E - T) / 2), and the sums of products
 * of the doubled average ranks 2r = 2 less + eq + 1.  With T <= AVS_EVAL_MAX_T every sum, and T * S_xy on the host, fits int64. */
int avs_eval_fold(const int32_t* d_counts, const uint8_t* d_mask_pred, const uint8_t* d_mask_target, int64_t rows,
                  const int64_t* d_offsets, int nseg, int max_t, int64_t* d_out, avs_stream_t stream);

/* ---- batched training: a ragged batch of V videos per optimiser step -------------------------------------------------
 * (scripts/train_av_model.py:86-96 for several videos at once.)  The videos are the segments [offsets[v], offsets[v + 1])
 * of concatenated rows; d_offsets is int64 [nseq + 1], starts at 0, increases and ends at `rows` (trusted: ops.SeqTable
 * guarantees it; rows outside every segment are still never read out of bounds).  The recurrences themselves already
 * take such a table (avs_lstm_*_f32's d_seq_rows); these are the two other places that must know where a video ends.
 * No float atomics; no entry point synchronises or reads a result back.                                               */

/* d_out[r, 0:cols] = d_src[r - direction, col0 : col0 + cols] when row r - direction lies in the same segment as r, else
 * 0.  direction +1: the previous row (h_{t-1} of a forward recurrence from its outputs h_t), -1: the next row (of a
 * reverse recurrence).  Exact copies.                                                                                 */
int avs_seq_shift_rows_f32(const float* d_src, int64_t ld_src, int col0, int cols, int64_t rows,
                           const int64_t* d_offsets, int nseq, int direction, float* d_out, int64_t ld_out,
                           avs_stream_t stream);

/* d_losses[v] = float(sum_r (double(p_r) - double(y_r))^2 / T_v) over the rows of video v: the sum in fp64 in an order
 * that depends on T_v alone (a video's loss is the same bits wherever it sits in the batch), one rounding to fp32.
 * target_stride 0: d_targets is [nseq], one target per video (the broadcast target of scripts/train_av_model.py:77-92);
 * 1: d_targets is [rows], one per row.  One workgroup per video.                                                      */
int avs_seq_mse_f32(const float* d_scores, const float* d_targets, int target_stride, int64_t rows,
                    const int64_t* d_offsets, int nseq, float* d_losses, avs_stream_t stream);
/* d_dscores[r] = (d_dlosses[v] * (2 / T_v)) * (p_r - y_r) in fp32 for the rows of video v; max_t = the longest video
 * (it sizes the grid).                                                                                                */
int avs_seq_mse_bwd_f32(const float* d_dlosses, const float* d_scores, const float* d_targets, int target_stride,
                        int64_t rows, const int64_t* d_offsets, int nseq, int max_t, float* d_dscores,
                        avs_stream_t stream);

/* ---- batched shot detection and frame sampling: the front half of stage 1 for V videos per call ----------------------
 * (features/shots.py and the sampling loop of features/extractors.py.)  The videos are the segments [offsets[v],
 * offsets[v + 1]) of the concatenated frames; d_offsets is int64 [nvideos + 1], starts at 0, increases strictly and ends
 * at n (trusted: ops.ShotTables guarantees it).  Integers and fixed orders only, so two calls on the same input give
 * the same bytes.  No entry point synchronises or reads a result back.                                                */

/* d_sums uint32 [n, 3]: per frame the sums of |dH|, |dS|, |dV| against the previous frame of the SAME video - the
 * integers of one avs_hsv_frame_diff_u8 call per video; the first frame of every video gets zeros.  The frame is on
 * grid x: n is bounded by 2^24 = 16 777 216 (a launch holds at most 2^32 - 1 threads per grid dimension, in workgroups
 * of 256), not by 65 536.                                                                                             */
int avs_hsv_frame_diff_batch_u8(const uint8_t* d_frames, int64_t n, int h, int w, int step, const int64_t* d_offsets,
                                int nvideos, uint32_t* d_sums, avs_stream_t stream);

/* Every video's cut list, one workgroup per video: frame f >= 1 is flagged when ((s0/p + s1/p) + s2/p) / 3.0 >=
 * threshold in fp64 (p = pixels, the strided pixel count; the host's expression and so the host's decision bit for
 * bit), and is a cut when it is the first flagged frame with f - last >= min_scene_len (last = the previous cut, 0
 * before the first).  Video v's cuts (video-relative frames, ascending) go to d_cuts[d_cut_off[v] ...]; d_cut_off is
 * int64 [nvideos + 1], the exclusive scan of the slot sizes (n_v - 1) / min_scene_len - the most the rule can place.
 * The rest of a slot is not written; a slot that is full ends the video's cuts (no store leaves the slot).
 * d_totals int64 [nvideos, 4] = (shots: 0 without a cut, else cuts + 1; sampled frames; micro-batch groups of
 * AVS_SHOT_MICRO_BATCH; the most sampled frames of one shot), a shot (s, e) holding min(AVS_SHOT_MAX_FRAMES, ceil(e/i) -
 * ceil(s/i)) sampled frames, i = AVS_SHOT_INTERVAL.                                                                  */
int avs_shot_cuts_batch(const uint32_t* d_sums, int64_t n, const int64_t* d_offsets, int nvideos, double pixels,
                        double threshold, int min_scene_len, const int64_t* d_cut_off, int64_t* d_cuts,
                        int64_t* d_totals, avs_stream_t stream);

/* The tables, from the cuts and totals above: a one-workgroup scan of the totals, then one workgroup per video.
 * d_video_off int64 [3, nvideos + 1]: the exclusive scans of (shots, sampled frames, groups) per video; plane 0 is the
 * shot_offsets table.  d_shots int64 [S, 2]: video-relative (start, end).  d_sample_offsets int64 [S + 1]: first row
 * of each shot in the sampled tensor.  d_sample_index int64 [F]: rows of the concatenated frames, frame k of shot
 * (s, e) of video v being offsets[v] + i (ceil(s/i) + k), i = AVS_SHOT_INTERVAL.  d_group_offsets int64 [G + 1]: rows of
 * the sampled tensor, each shot cut into groups of AVS_SHOT_MICRO_BATCH with a shorter tail group.  d_counts int64 [4] = (S, F, G, most frames of a shot).
 * The capacities are those of the buffers (S + 1 <= shot_cap + 1 entries of d_sample_offsets, ...); nothing is written
 * past them.                                                                                                          */
int avs_shot_tables_fill(const int64_t* d_offsets, int nvideos, const int64_t* d_cut_off, const int64_t* d_cuts,
                         const int64_t* d_totals, int64_t* d_video_off, int64_t* d_shots, int64_t shot_cap,
                         int64_t* d_sample_offsets, int64_t* d_sample_index, int64_t sample_cap,
                         int64_t* d_group_offsets, int64_t group_cap, int64_t* d_counts, avs_stream_t stream);

/* d_out[i] = d_src[d_index[i]] for rows of row_bytes bytes, i < min(*d_count, capacity): the row count is read from
 * device memory, the grid is sized by `capacity` and rows past the count are left as they were.  16-byte units when
 * row_bytes % 16 == 0 and both bases are 16-byte aligned, else 4-byte, else single bytes.  An index outside
 * [0, src_rows) is skipped.  capacity < 2^24 (one workgroup of 256 per row on grid x).                                */
int avs_gather_rows_u8(const uint8_t* d_src, int64_t src_rows, int64_t row_bytes, const int64_t* d_index,
                       const int64_t* d_count, int64_t capacity, uint8_t* d_out, avs_stream_t stream);

/* ---- keyshot summaries: shot values, one 0/1 knapsack per (score row, video), summary overlap ------------------------
 * (No counterpart in the reference: SURVEY Q17.  evaluation/keyshots.py holds the definitions and their numpy oracle.)
 * The videos are the segments [offsets[v], offsets[v + 1]) of the concatenated frames, d_offsets int64 [nvideos + 1]
 * (trusted: ops.SummaryTables guarantees it).  Video v's shots are the entries d_shot_offsets[v] .. d_shot_offsets[v + 1]
 * of d_shots int64 [shot_cap, 2] = video-relative (start, end), the layout avs_shot_tables_fill writes; a shot is
 * clipped to its video.  Integers, or fp64 values a fixed recurrence defines: two calls on the same input give the same
 * bytes.  No float atomics; no entry point allocates, synchronises or reads a result back.                           */

/* d_sums int64 [nrows, shot_cap]: d_sums[k, g] = sum over the frames r of shot g of q(d_scores[k * ld_scores + base_v +
 * r]), q(x) = rint(clamp(x, 0, 1) * 2^32) in fp64 (round half to even; NaN -> 0).  The entries from
 * d_shot_offsets[nvideos] on get 0.  One wave per (k, shot), 16-byte loads from the first aligned score on.           */
int avs_shot_value_sums(const float* d_scores, int64_t ld_scores, int nrows, int64_t n, const int64_t* d_offsets,
                        int nvideos, const int64_t* d_shot_offsets, const int64_t* d_shots, int64_t shot_cap,
                        int64_t* d_sums, avs_stream_t stream);

/* One 0/1 knapsack per (k, v), one workgroup of 1024 threads each: shot i of video v has weight w_i = end - start and
 * value double(sum_i) / double(w_i); the capacity is d_capacity[v] (int64 [nvideos], at most max_capacity <=
 * AVS_SUMMARY_MAX_CAPACITY).
 * row[w] = max over "skip" and, where w >= w_i, row'[w - w_i] + value, the shot TAKEN only where that is strictly
 * greater; both fp64 rows live in LDS (128 KiB of a CU's 160 KiB).  The take bits of shot g =
 * d_shot_offsets[v] + i are written as uint64 words (bit w & 63 of word w >> 6) to d_take [nrows][shot_cap][words],
 * words >= ceil((max_capacity + 1) / 64); the backtrack starts at w = capacity with the last shot.
 * d_picked uint8 [nrows, shot_cap] (1 = in the summary; written for the shots below d_shot_offsets[nvideos]),
 * d_mask uint8 [nrows, n] (EVERY frame of every video is written, 0 or 1), d_optimum fp64 [nrows, nvideos],
 * d_totals int64 [nrows, nvideos, 3] = (shots picked, frames picked, capacity).  A video without shots gets an
 * all-zero mask, optimum 0 and totals (0, 0, capacity).                                                              */
int avs_knapsack_batch_f64(const int64_t* d_sums, int nrows, int64_t n, const int64_t* d_offsets,
                           const int64_t* d_capacity, int nvideos, int max_capacity, const int64_t* d_shot_offsets,
                           const int64_t* d_shots, int64_t shot_cap, uint64_t* d_take, int words, uint8_t* d_picked,
                           uint8_t* d_mask, double* d_optimum, int64_t* d_totals, avs_stream_t stream);

/* d_counts int64 [nvideos, nusers, 3] = (tp, n_pred, n_user) over the frames of video v: the sums of pred & user, pred
 * and user with d_pred_mask uint8 [n] and d_user_masks uint8 [nusers, n] (row stride ld_user), a byte counting as 1
 * when it is not 0.  One workgroup per (video, user).                                                                */
int avs_mask_overlap_counts(const uint8_t* d_pred_mask, const uint8_t* d_user_masks, int64_t ld_user, int nusers,
                            int64_t n, const int64_t* d_offsets, int nvideos, int64_t* d_counts, avs_stream_t stream);

/* ---- batched stage-1 extraction: the glue around the two CNN trunks (features/extractors.py:344-362 for every shot of
 * a ragged batch; csrc/stage1_batch.hip) ------------------------------------------------------------------------------
 * d_dst0[i] = cv2.resize(d_src[d_index[i]], (dw0, dh0), INTER_LINEAR) for i < count and, where d_dst1 is not null, the
 * same for d_dst1 at (dw1, dh1), in ONE launch: d_src uint8 [src_rows, sh, sw, 3] is read where it lies (no dense copy
 * of the gathered frames), d_index int64 [>= count] on the device, count a host integer, d_dst* uint8 [count, dh, dw, 3].
 * The bytes are those of avs_resize_bilinear_u8 on the gathered frames.  An index outside [0, src_rows) is skipped: its
 * destination rows are left as they were.  Any alignment of the three bases is taken.  One workgroup resizes a band of
 * 8 output rows (fewer while the source rows of a band exceed 64 KiB of LDS); AVS_E_UNSUPPORTED when two source rows and
 * one output row do not fit, or for more than 65535 source columns or output rows.  count < 2^31.                      */
int avs_resize_bilinear_gather2_u8(const uint8_t* d_src, int64_t src_rows, int sh, int sw, const int64_t* d_index,
                                   int64_t count, uint8_t* d_dst0, int dh0, int dw0, uint8_t* d_dst1, int dh1, int dw1,
                                   avs_stream_t stream);

/* d_out[s, 0:d] = mean over k of d_x[d_perm[d_seg[s] + k], 0:d], k ascending, for s < nseg: avs_segment_mean_f32 reading
 * its rows through a permutation, with the same additions in the same order (the bytes of avs_segment_mean_f32 on the
 * permuted rows).  d_x fp32 [x_rows, >= d] with row stride ldx, d_perm int64 [perm_len], d_seg int64 [nseg + 1] positions
 * in d_perm, d_out fp32 with row stride ldo (a column slice of a wider matrix is fine).  An empty segment gives a row of
 * zeros.  A position outside d_perm, or a row outside d_x, is passed over.                                              */
int avs_segment_mean_perm_f32(const float* d_x, int64_t ldx, int64_t x_rows, int d, const int64_t* d_perm,
                              int64_t perm_len, const int64_t* d_seg, int nseg, float* d_out, int64_t ldo,
                              avs_stream_t stream);

/* ---- kernel temporal segmentation of a ragged batch (csrc/kts.hip; the definitions: features/kts.py) ----------------
 * The host plan (ops.KtsTables) gives d_videos int64 [nvideos][AVS_KTS_VIDEO_COLS] = per video (first feature row, frames
 * N, samples n = ceil(N / stride) <= AVS_KTS_MAX_SAMPLES, m_max, first entry of its block in the packed K / R buffers [n][n], in K1 [n + 1], in
 * Jt [n + 1][n + 1], in p [m_max + 1][n + 1], in the cost / change-point / shot slots [m_max + 1], 0) and the packed
 * sizes: k1_entries, k_entries, jt_entries, p_entries, cost_cap, each below 2^31.  The table is trusted.  The workspace
 * holds K1 | R | Jt (fp64) | p (uint16), each part at a multiple of 256 bytes: avs_kts_workspace_bytes (0 for sizes out
 * of range).  nvideos <= AVS_KTS_MAX_VIDEOS.  No atomics; no kernel waits on another workgroup; nothing allocates or synchronises. */
size_t avs_kts_workspace_bytes(int64_t k1_entries, int64_t k_entries, int64_t jt_entries, int64_t p_entries);

/* d_gram[k_off_v + i * n + j] = sum over c < d of double(x_i[c]) * double(x_j[c]) on v_mfma_f64_16x16x4_f64, x_i = row
 * first_row_v + i * stride of d_x fp32 [rows, d] with row pitch ld >= d (4-byte alignment suffices; read in place).
 * d_tiles int32 [ntiles][3] = (video, ti, tj) with ti <= tj: the AVS_KTS_TILE x AVS_KTS_TILE tiles of the upper triangles.  The elements
 * i <= j are stored to [i][j] and [j][i] from one register: K is symmetric to the bit, and a video's block does not
 * depend on the batch around it.                                                                                      */
int avs_kts_gram_f64(const float* d_x, int64_t rows, int d, int64_t ld, int64_t stride, const int64_t* d_videos,
                     int nvideos, const int* d_tiles, int64_t ntiles, double* d_gram, int64_t k_entries,
                     avs_stream_t stream);

/* K1 (the sequential sums of the diagonal), R = cumsum(cumsum(K, 0), 1) (both strictly sequential; K2[a][b] =
 * R[a - 1][b - 1], 0 on the first row and column) and Jt[l][t] = (K1[l] - K1[t]) - (((K2[l][l] + K2[t][t]) - K2[l][t])
 * - K2[t][l]) / double(l - t) for 0 <= t < l <= n into the workspace; d_flags int64 [nvideos]: 1 where K2[n][n] is not
 * finite.  Three launches; max_n: the largest n of the plan.                                                          */
int avs_kts_scatters_f64(const double* d_gram, const int64_t* d_videos, int nvideos, int max_n, void* d_ws,
                         size_t ws_bytes, int64_t k1_entries, int64_t k_entries, int64_t jt_entries, int64_t p_entries,
                         int64_t* d_flags, avs_stream_t stream);

/* The dynamic programme on the Jt of avs_kts_scatters_f64, one workgroup of 1024 threads per video (both live rows in
 * LDS): I_0[l] = Jt[l][0]; I_k[l] = min over t = k lmin .. l - lmin of I_{k-1}[t] + Jt[l][t], p_k[l] the smallest t
 * attaining it; d_scores[c_off_v + k] = I_k[n], d_costs[..] = score / double(n) + d_penalties[c_off_v + k] (fp64
 * [cost_cap], from the host).  m_best = the smallest k of least cost (select_fixed = 0) or m_max; a flagged video gets
 * m_best = 0 and NaN costs.  d_change_points int64 [cost_cap]: m_best ascending sample indices per video slot, -1
 * after them.  d_totals int64 [nvideos][4] = (m_best, n, m_max, flag).  A second launch writes d_shot_offsets int64
 * [nvideos + 1] (exclusive prefix of m_best + 1) and d_shots int64 [cost_cap][2], the layout of avs_shot_tables_fill:
 * (b_j, b_{j+1}) with b_0 = 0, b_j = change point j - 1 times stride, the last end N; zeros past the last shot.       */
int avs_kts_dp_f64(const int64_t* d_videos, int nvideos, int max_n, int lmin, int64_t stride, int select_fixed,
                   const double* d_penalties, void* d_ws, size_t ws_bytes, int64_t k1_entries, int64_t k_entries,
                   int64_t jt_entries, int64_t p_entries, int64_t cost_cap, const int64_t* d_flags, double* d_scores,
                   double* d_costs, int64_t* d_change_points, int64_t* d_shot_offsets, int64_t* d_shots,
                   int64_t* d_totals, avs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AVSUM_HIP_H */
