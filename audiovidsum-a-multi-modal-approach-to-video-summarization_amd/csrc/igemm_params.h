// Shared by the contraction kernels of libavsum_hip.so (igemm.hip, local224.hip; convbn.hip takes the block remap, the LDS
// slot map and AVS_GLDS16): the launch parameters, the epilogue forms, the inline-asm helpers of the hand-counted pipelines
// and the pieces of staging and epilogue text these kernels have in common.
#pragma once
#include "avs_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct IgemmParams {
  const char* x;
  const char* w;
  char* y;
  const float* bias;
  int M, N, K;
  int HoWo, Wo, H, W, cin, KW;
  int sh, sw, ph, pw;
  long long x_img_stride, x_row_stride, x_px_stride;
  long long ldb, ldc;
  long long sA, sB, sC, sBias;
  float alpha;
  int act, bias_mode;
  int tiles_n;
  // EPI_STATS (fused BatchNorm batch statistics): every row tile writes, for each group it overlaps, its column sums
  // and sums of squares of the fp32 accumulators to its OWN slot stat_part[tile][slot][sum | sumsq][N] (plain stores,
  // no atomics); bn_fold_kernel adds a group's slots in tile order, so the statistics are reproducible bit for bit
  float* stat_part;
  int stat_slots;    // slots per row tile = groups a tile can overlap
  int rows_per_group;
  long long lin_stride;  // >= 0: output row m reads input row m at x + m*lin_stride (no (n,ho,wo) decode needed)
  // EPI_BNLOCAL (whole BatchNorm in the epilogue): BatchNorm parameters, optional residual
  const float* gamma;
  const float* beta;
  float eps;
  const char* residual;
  long long ldr;
  int split;         // fp32 operands only: 1 = products on the bf16 matrix cores as hi*hi + hi*lo + lo*hi (AVS_F32_SPLIT)
  int tall;          // 1: the 256-row tile variants (WR = 4)
  int w_kstep;       // 1: w is stored reduction-step major (AVS_W_KSTEP32), [K / S][N][S], S = 32 bf16 / 16 fp32: the 64 bytes a B row needs
                     //    in one step sit next to the neighbouring rows' (whole cache lines per DMA instruction)
  int tile_rows;     // EPI_BNLOCAL: rows of the tile that are used (whole groups), also the pitch between tiles
  // EPI_AFFINE (AVS_F16X2): y = act((conv * scale[g] + shift[g]) + residual (* res_scale[g] + res_shift[g])), the folded
  // affines given per group of rows_per_group rows: gamma / beta point at scale / shift [groups, N]
  int affine;
  const float* res_scale;
  const float* res_shift;
  int variant;       // avs_conv_desc.variant: AVS_TILE_128 / AVS_TILE_256 (bits 0-1), AVS_STAGING_GENERIC (bit 2)
  // AVS_F16P8 operands of the AVS_F16X2 1x1 forms (avs_conv_desc.formats): the input of the convolution + statistics
  // form (fetched into registers, the lo halves rebuilt there), the output / the residual of the given-affine form
  int x_p8, y_p8, res_p8;
  // two destinations (AVS_F16X2, avs_conv2d_nhwc_split): output columns >= nsplit go to y2 (row stride ldc2, column c at
  // c - nsplit) - several 1x1 convolutions that read the same input run as ONE contraction with their filters stacked
  char* y2;
  long long ldc2;
  int nsplit;
  int relu_cols;     // > 0: only the columns below it take the ReLU of a bias + ReLU epilogue
  // clustered tile-local BatchNorm (local224.hip): a group = `cluster` consecutive tiles of tile_rows rows; every wave
  // publishes its tile's (mean, centred sum of squares) per column as 8-byte {value, epoch} granules in xchg
  // [tiles_m][tiles_n][4 waves][64] and reads its partners' - one exchange, merged by Chan's update in tile order
  int cluster;
  unsigned epoch;
  unsigned long long* xchg;
  unsigned* xerr;    // a counter of waves whose bounded wait ran out (0 = every exchange completed)
  // packed form of the clustered BatchNorm (AVS_CLUSTER_PACKED): tiles are 224 consecutive rows of the launch whatever
  // rows_per_group is (a multiple of 112); a tile meets at most two groups, the boundary inside it at row 112; xchg holds
  // two granules per lane, [tiles_m][tiles_n][4 waves][2 segments][64].  packed = row tiles per dispatch unit (the tiles
  // that can wait for each other: those of one group, or of two groups that share a tile), 0 = the unpacked form
  int packed;
  // input affine of the nine-tap convolution + statistics form (AVS_F16X2, avs_conv2d_nhwc_bnstats_xin): the input is a
  // RAW activation whose BatchNorm (+ ReLU) is applied as each 16-channel block lands in LDS - x = act(x * in_scale[g] +
  // in_shift[g]), g = row / rows_per_group, in_scale / in_shift [groups, cin]
  const float* in_scale;
  const float* in_shift;
  int in_relu;
  // 1 (set by igemm_run from rows_per_group and cin): groups of at least XIN_TABLE_MIN_GROUP_ROWS rows - a tile's 384 buffer
  // rows touch at most two of them, whose affines the kernel keeps in an LDS table; 0: the group is looked up per row
  int xin_table;
#ifdef AVS_STUDY
  int debug;  // ablation switches of the kernel-study build (tools/): 1 = skip output stores, 2 = skip A/B loads, ...
#endif
};

enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_ANY = 2, EPI_BRELU = 3, EPI_BNLOCAL = 5, EPI_AFFINE = 6 };
constexpr int BNLOCAL_MAX_GROUPS = 6;  // groups per 256-row tile (rows_per_group >= 37: six groups of 37 .. 42 rows)
constexpr int STATS_MIN_GROUP_ROWS = 64;  // EPI_STATS: a wave's 64 rows then overlap at most two groups
constexpr int XIN_TABLE_MIN_GROUP_ROWS = 384;  // XIN: the nine-tap form's 384 buffer rows then touch at most two groups
constexpr int XIN_TABLE_MAX_CIN = 128;         // ... and the two groups' affines fit the LDS table (2 x cin x 2 floats)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// Passes a fragment THROUGH an empty asm: every later use of it depends on this statement, so it cannot be scheduled
// ahead of the (volatile) wait that precedes the statement.
__device__ __forceinline__ void avs_pin(uint4& v) {
  u32x4 r = __builtin_bit_cast(u32x4, v);
  asm volatile("" : "+v"(r));
  v = __builtin_bit_cast(uint4, r);
}

__device__ __forceinline__ void avs_pin2(uint2& v) {
  u32x2 r = __builtin_bit_cast(u32x2, v);
  asm volatile("" : "+v"(r));
  v = __builtin_bit_cast(uint2, r);
}
__device__ __forceinline__ uint2 avs_lds_read_b64(unsigned byte_addr) {
  uint2 v;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}
__device__ __forceinline__ uint4 avs_lds_read_b128(unsigned byte_addr) {
  uint4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}

// ---- pieces the contraction kernels share (igemm.hip, local224.hip, convbn.hip): each stated once, here ----
// 16 bytes from a per-lane global address straight into LDS (wave-linear destination)
#define AVS_GLDS16(src, dst)                                                                        \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),            \
                                   (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

// XCD-aware, bijective block remap: blocks that share an XCD (orig % 8) take consecutive tiles, so neighbouring column
// tiles reuse A rows in L2.  nwg = gridDim.x, orig = blockIdx.x
__device__ __forceinline__ unsigned avs_xcd_remap(unsigned nwg, unsigned orig) {
  const unsigned q = nwg >> 3, rr = nwg & 7, xcd = orig & 7;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (orig >> 3);
}

// The LDS image of an operand tile: a row is CPRR 16-byte slots, chunk q of row r lives in slot q ^ (r >> SH) mod CPRR (1 << SH
// rows share a 256-byte bank row).  Its own inverse: the chunk a thread FETCHES into slot c of row r is AVS_LDS_CHUNK(r, c).
// (Macros: as functions the expressions reach the optimiser in another order, which added instructions to the hot kernels.)
#define AVS_LDS_CHUNK(CPRR, SH, row, chunk) ((chunk) ^ (((row) >> SH) & (CPRR - 1)))
#define AVS_LDS_SLOT(CPRR, SH, row, chunk) ((row) * CPRR + AVS_LDS_CHUNK(CPRR, SH, row, chunk))

// Register e of a 32x32 accumulator tile is row (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), column lane & 31.  The row
// counted from `base` (a block's first row); the sum stays in this order, which is the order the kernels were written in
__device__ __forceinline__ constexpr int avs_acc_row(int base, int e) { return base + (e & 3) + 8 * (e >> 2); }

// eight consecutive floats as two 16-byte loads
__device__ __forceinline__ void avs_load8(const float* src, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
// ---- the buffer-load staging of the scalar tap walk (igemm_kernel's FASTK branch, igemm_h2_local224_kernel) ----
// Operands are fetched with buffer_load_dwordx4 ... lds: address = resource base (SGPRs) + per-lane offset (one
// VGPR, fixed for the whole reduction) + scalar offset (the tap walk / the k step).  A lane whose tap falls into
// the padding (or whose row does not exist) presents an offset beyond num_records and the hardware returns
// zeros, so staging costs no vector arithmetic per step beyond that select.  The A base is moved back by the
// padding so that every row's own offset is non-negative; the launcher guarantees a tile's rows and the tap walk
// stay inside the 2 GiB window.
constexpr unsigned AVS_BUF_OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t avs_buffer_window(const char* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, (int)AVS_BUF_OOB, 0x00020000);
}
// uniform tile origin, in elements: the first image the tile touches (n_first), or its first row (lin_row elements apart)
__device__ __forceinline__ long long avs_tap_origin(const IgemmParams& p, int m0, long long lin_row, int& n_first) {
  n_first = 0;
  if (p.lin_stride >= 0) return (long long)m0 * lin_row;
  n_first = m0 / p.HoWo;
  return (long long)n_first * p.x_img_stride - (long long)p.ph * p.x_row_stride - (long long)p.pw * p.x_px_stride;
}
// a row's 32-bit offset: its first tap relative to the tile origin, n_rel = the row's image minus the tile's first
template <int ES>
__device__ __forceinline__ unsigned avs_tap_first(const IgemmParams& p, int n_rel, int hi0, int wi0) {
  return (unsigned)(((long long)n_rel * p.x_img_stride + (long long)(hi0 + p.ph) * p.x_row_stride +
                     (long long)(wi0 + p.pw) * p.x_px_stride) * ES);
}
// The tap walk (kh, kw, ci) is the same for every thread: kept in scalar registers and advanced by additions.  Next step: the
// same tap's next channel block (step_elems channels = a_step bytes further), or the next tap; b_step = bytes between a weight
// row's steps.  f_koff: bytes, the current tap + channel block relative to a row's first tap; f_kb: bytes, the current k step
// inside a B row.  (Five ints by reference: as a struct the walk moved instructions in 236 of igemm_kernel's instantiations.)
template <int ES>
__device__ __forceinline__ void avs_tap_advance(const IgemmParams& p, int& f_tap, int& f_ci0, int& f_kw, int& f_koff,
                                                int& f_kb, int step_elems, int a_step, int b_step) {
  f_kb += b_step;
  f_ci0 += step_elems;
  f_koff += a_step;
  if (f_ci0 == p.cin) {
    f_ci0 = 0;
    ++f_tap;
    f_koff += (int)((p.x_px_stride - p.cin) * ES);
    if (++f_kw == p.KW) {
      f_kw = 0;
      f_koff += (int)((p.x_row_stride - (long long)p.KW * p.x_px_stride) * ES);
    }
  }
}
// XIN, a run of 8 channels of the raw activation: join hi + lo, v * scale + shift (a multiply and an add, as avs_bn_apply), ReLU, split
__device__ __forceinline__ void avs_xin_affine8(const uint4& hi, const uint4& lo, const float (&sc)[8], const float (&sf)[8],
                                                int relu, uint4& h, uint4& l) {
  float v[8];
  avs_f16x2_join8(hi, lo, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = v[j] * sc[j] + sf[j];
  if (relu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
  }
  avs_f16x2_split8(v, h, l);
}
// rows roff, roff + 1 of a column of the packed-bf16 staging tile (pitch PITCH bytes; cbase: the lane's row 0, tile 0): two 2-byte stores
template <int PITCH>
__device__ __forceinline__ void avs_ct_store2(char* cbase, int roff, int nt, unsigned pk) {
  *reinterpret_cast<unsigned short*>(cbase + roff * PITCH + nt * 64) = (unsigned short)pk;
  *reinterpret_cast<unsigned short*>(cbase + (roff + 1) * PITCH + nt * 64) = (unsigned short)(pk >> 16);
}

// What igemm_plan() chooses for one call - which kernel (the template arguments of igemm_kernel, or the 224-row tile of
// local224.hip) on which grid - from the dtype, the geometry and the options alone: it reads no operand.
struct IgemmPlan {
  int status;          // AVS_OK, or the status of the first of the plan's checks that failed
  int operand_checks;  // how many of igemm_run's operand checks come before the point the plan reached (0..3)
  int dtype, batch;
  int es;              // bytes per element
  int split;           // SPLIT: 0 operands as stored, 1 AVS_F32_SPLIT, 2 AVS_F16X2
  int bn;              // columns of a tile: 64 / 96 / 128
  bool acc64;
  bool tall;           // the rules ask for the 256-row tiles
  bool spatial;        // a tap can leave the image: the per-tap bounds tests are needed
  long long lin_stride;  // IgemmParams::lin_stride
  int rowb;            // bytes of a reduction step: 64 / 128
  int epi;             // EPI_*
  bool pipe;           // the 3-buffer hand-counted pipeline
  int wr;              // rows of waves: 2 (128-row tiles) / 4 (256-row tiles)
  bool fastk;          // the scalar tap walk
  bool tap9, ap8, xin; // the shifted-row staging, the AVS_F16P8 input, the input affine
  bool in_affine;      // the caller gives an input affine: only the XIN kernel may run
  bool groupw;         // EPI_AFFINE: rows_per_group is a multiple of 64, so every wave's 64 rows lie in ONE group (GROUPW)
  bool local224;       // the 224-row tile takes it
  int tile_rows;       // rows of a tile that are used = the pitch between tiles
  long long tiles_m;
  int tiles_n;
  long long grid;      // workgroups per batch entry = tiles_m * tiles_n; 0: nothing to launch
};

// The buffer window of the scalar tap walk (buffer_load ... lds): a tile's rows (at most 256, spread over whole images)
// plus the tap walk, and bn rows of the weights, must each lie below 2 GiB; es = bytes per element
inline bool igemm_buffer_window_ok(const IgemmParams& p, long long lin_stride, int es, int bn) {
  const long long rows = 256;
  long long extent;
  if (lin_stride >= 0)
    extent = rows * lin_stride + p.K;
  else
    extent = (rows / p.HoWo + 2) * p.x_img_stride + (long long)(p.K / (p.cin * p.KW) + p.ph) * p.x_row_stride +
             (long long)(p.KW + p.pw) * p.x_px_stride + p.cin;
  return extent * es < (1ll << 31) && (long long)bn * p.ldb * es + (long long)p.K * es < (1ll << 31) &&
         p.x_img_stride >= 0 && p.x_row_stride >= 0 && p.x_px_stride >= 0;
}

// local224.hip: the AVS_F16X2 tile-local BatchNorm form on 224-row tiles (one group of 193..224 rows per tile)
bool igemm_h2_local224_ok(const IgemmParams& p, int dtype, long long lin_stride);
void igemm_h2_local224_launch(const IgemmParams& p, bool spatial, dim3 grid, hipStream_t stream);
