// AVS_F16X2 convolution + whole BatchNorm (+ residual, + ReLU) for groups of 193..224 rows - the per-frame 14x14 maps of
// ResNet-50's layer 3 - on a tile that FITS the group (features/extractors.py:65: self.resnet(resnet_batch), train-mode
// BatchNorm per micro-batch group).
//
// The general kernel (igemm.hip, EPI_BNLOCAL) puts such a group into a 256-row tile whose four waves own 64 rows each: a
// quarter of the matrix work and of the operand DMA is spent on rows that do not exist, and four waves cannot share seven
// 32-row blocks evenly by ROWS.  Here the tile is 224 rows x 128 columns and the waves split the COLUMNS: every wave owns
// all seven 32-row blocks of its 32 columns (7 accumulator blocks = 112 registers).
//   * 7/8 of the matrix instructions and 352 instead of 384 staged rows per reduction step;
//   * a column's statistics are sums over ONE wave's registers: two shuffle-free rounds (sum -> mean -> centred squares)
//     plus one cross-half exchange each - no LDS tables, no barriers between the rounds;
//   * fragment reads per step and wave: 14 (A, shared by the four waves) + 2 (B) ds_read_b128 for 21 MFMAs - 0.76 per
//     MFMA, inside what the LDS sustains next to the DMA writes (2 per MFMA gap are free).
// Operand staging, the scalar tap walk, the LDS image (64-byte rows, chunk q of row r in slot q ^ ((r >> 2) & 3)), the
// three-buffer pipeline with hand-counted waits and the order of the three fp16 MFMAs per product are those of
// igemm_kernel<..., PIPE, FASTK, SPLIT = 2>: the convolution itself is bit-identical to the 256-row form, the statistics
// are summed in a different (fixed) order.  Waves 0 and 1 issue six DMA instructions per step, waves 2 and 3 five (352 rows
// = 5.5 passes of the 256 threads); each wave waits on its own count.
//
// Groups larger than a tile run clustered (p.cluster > 1: one tile per 193..224-row member of the group, the tiles exchange
// their statistics), or PACKED (p.packed: tiles of 224 consecutive rows whatever the group size - a multiple of 112 rows - so
// no tile runs a 32-row block for 4 live rows; a tile then holds rows of one or of two groups, the boundary at its row 112).
//
// The main loop exists in two matrix-instruction shapes (template parameter SHAPE, chosen per instance at compile time from
// the measurements in profiles/r07_*): 32 = the loop described above; 16 = v_mfma_f32_16x16x32_f16 on the same tile per
// wave, two reduction steps paired - see the comment in front of the kernel.
#include "avs_internal.h"
#include "igemm_params.h"
#include <type_traits>
#include <utility>

namespace {
constexpr int L_ROWS = 224;                 // A rows of a tile
constexpr int L_MT = L_ROWS / 32;           // 32-row blocks per wave
constexpr int L_BN = 128;                   // columns of a tile (32 per wave)
constexpr int L_CPRR = 4;                   // 16-byte slots per 64-byte LDS row
constexpr int L_STEP = 16;                  // reduction elements (slots) per step
constexpr int L_BUF = (L_ROWS + L_BN) * L_CPRR;   // uint4 slots per operand buffer
constexpr int L_P = 32 + 8;                 // words per staged output row

template <int OFF>
__device__ __forceinline__ uint4 lds_read_b128_at(unsigned byte_addr) {
  uint4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(byte_addr), "n"(OFF));
  return v;
}
template <int... I>
__device__ __forceinline__ void read_blocks(uint4 (&f)[L_MT], unsigned addr, std::integer_sequence<int, I...>) {
  ((f[I] = lds_read_b128_at<I * 32 * 64>(addr)), ...);
}

// ---- SHAPE 16 (v_mfma_f32_16x16x32_f16): fourteen 16-row blocks, two 16-column blocks per wave ----
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int L_MT16 = L_ROWS / 16;         // 16-row blocks per wave
template <int... I>
__device__ __forceinline__ void read_blocks16(uint4 (&f)[L_MT16], unsigned addr, std::integer_sequence<int, I...>) {
  ((f[I] = lds_read_b128_at<I * 16 * 64>(addr)), ...);
}
// Seven blocks' ds_read_b128 on ONE half of the wave (UPPER: lanes 32 .. 63, else lanes 0 .. 31); the other half of every
// register keeps what it holds.  All 64 lanes are active around the main loop, so EXEC is restored to all ones.
template <int B0, bool UPPER>
__device__ __forceinline__ void read_half7(uint4 (&f)[L_MT16], unsigned addr) {
  u32x4 r0 = __builtin_bit_cast(u32x4, f[B0 + 0]), r1 = __builtin_bit_cast(u32x4, f[B0 + 1]),
        r2 = __builtin_bit_cast(u32x4, f[B0 + 2]), r3 = __builtin_bit_cast(u32x4, f[B0 + 3]),
        r4 = __builtin_bit_cast(u32x4, f[B0 + 4]), r5 = __builtin_bit_cast(u32x4, f[B0 + 5]),
        r6 = __builtin_bit_cast(u32x4, f[B0 + 6]);
  if constexpr (UPPER)
    asm volatile(
        "s_mov_b32 exec_lo, 0\n\t"
        "ds_read_b128 %0, %7 offset:%8\n\tds_read_b128 %1, %7 offset:%9\n\tds_read_b128 %2, %7 offset:%10\n\t"
        "ds_read_b128 %3, %7 offset:%11\n\tds_read_b128 %4, %7 offset:%12\n\tds_read_b128 %5, %7 offset:%13\n\t"
        "ds_read_b128 %6, %7 offset:%14\n\t"
        "s_mov_b32 exec_lo, -1"
        : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6)
        : "v"(addr), "n"((B0 + 0) * 1024), "n"((B0 + 1) * 1024), "n"((B0 + 2) * 1024), "n"((B0 + 3) * 1024),
          "n"((B0 + 4) * 1024), "n"((B0 + 5) * 1024), "n"((B0 + 6) * 1024));
  else
    asm volatile(
        "s_mov_b32 exec_hi, 0\n\t"
        "ds_read_b128 %0, %7 offset:%8\n\tds_read_b128 %1, %7 offset:%9\n\tds_read_b128 %2, %7 offset:%10\n\t"
        "ds_read_b128 %3, %7 offset:%11\n\tds_read_b128 %4, %7 offset:%12\n\tds_read_b128 %5, %7 offset:%13\n\t"
        "ds_read_b128 %6, %7 offset:%14\n\t"
        "s_mov_b32 exec_hi, -1"
        : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6)
        : "v"(addr), "n"((B0 + 0) * 1024), "n"((B0 + 1) * 1024), "n"((B0 + 2) * 1024), "n"((B0 + 3) * 1024),
          "n"((B0 + 4) * 1024), "n"((B0 + 5) * 1024), "n"((B0 + 6) * 1024));
  f[B0 + 0] = __builtin_bit_cast(uint4, r0); f[B0 + 1] = __builtin_bit_cast(uint4, r1);
  f[B0 + 2] = __builtin_bit_cast(uint4, r2); f[B0 + 3] = __builtin_bit_cast(uint4, r3);
  f[B0 + 4] = __builtin_bit_cast(uint4, r4); f[B0 + 5] = __builtin_bit_cast(uint4, r5);
  f[B0 + 6] = __builtin_bit_cast(uint4, r6);
}
// the wave's two B blocks (16 columns = 1024 bytes apart), lanes 32 .. 63 only
__device__ __forceinline__ void read_upper2(uint4 (&f)[2], unsigned addr) {
  u32x4 r0 = __builtin_bit_cast(u32x4, f[0]), r1 = __builtin_bit_cast(u32x4, f[1]);
  asm volatile(
      "s_mov_b32 exec_lo, 0\n\t"
      "ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\t"
      "s_mov_b32 exec_lo, -1"
      : "+v"(r0), "+v"(r1)
      : "v"(addr));
  f[0] = __builtin_bit_cast(uint4, r0);
  f[1] = __builtin_bit_cast(uint4, r1);
}
// zeroes lanes 32 .. 63 of a fragment (the partner half of a pair that has no second step)
__device__ __forceinline__ void zero_upper(uint4& f) {
  asm volatile(
      "s_mov_b32 exec_lo, 0\n\t"
      "v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0\n\t"
      "s_mov_b32 exec_lo, -1"
      : "+v"(f.x), "+v"(f.y), "+v"(f.z), "+v"(f.w));
}
}  // namespace

// SHAPE: the matrix instruction of the main loop.  32 = v_mfma_f32_32x32x16_f16, 21 per step.  16 = v_mfma_f32_16x16x32_f16
// on the same tile per wave (14 x 2 blocks of 16 x 16): an instruction reduces over 32 slots and a step carries 16
// channels x three terms = 48, so steps are PAIRED.  Every step issues P = (hi + lo) . hi per block (A lane groups: hi 0-7,
// hi 8-15, lo 0-7, lo 8-15 of the step; B: hi 0-7, hi 8-15 twice); every second step issues Q = hi . lo of BOTH steps (lanes
// 0 .. 31: the even step's chunks, lanes 32 .. 63: the odd step's).  Q's operands are formed in place: lanes 0 .. 31 of the
// even step's P fragment are its hi chunks already, at the odd step a half-wave read puts the odd step's hi chunks into lanes
// 32 .. 63 of the same registers, and when Q has been issued a second half-wave read puts the odd step's lo chunks into lanes
// 0 .. 31 - the registers then are the odd step's P fragment (lo | hi).  Nothing is read from a buffer after its own step.
// A lane (i = lane & 15) reads row i ^ ((i >> 1) & 4) of a block (rows 8 .. 11 and 12 .. 15 trade places): with the image's
// swizzle the chunk pairs (0, 2) and (1, 3) of one instruction then fall on sixteen different 16-byte slots per lane group.
template <bool SPATIAL, int SHAPE>
__global__ __launch_bounds__(256, 2) void igemm_h2_local224_kernel(IgemmParams p) {
  static_assert(SHAPE == 32 || SHAPE == 16, "SHAPE: 32 (v_mfma_f32_32x32x16_f16) or 16 (v_mfma_f32_16x16x32_f16)");
  __shared__ uint4 lds[3 * L_BUF];

  const unsigned nwg = gridDim.x, orig = blockIdx.x;
  const unsigned wg = avs_xcd_remap(nwg, orig);   // (as igemm_kernel)
  int tn = wg % p.tiles_n;
  int tm = wg / p.tiles_n;
  if (p.packed) {
    // packed clustered form: the tiles that wait for each other are the p.packed row tiles of a unit (one group, or two groups
    // around a shared tile) - CONSECUTIVE block ids, as below.  Super-unit = 56 row tiles (7- and 14-tile units divide it) x
    // all column tiles, block = column tile * 56 + row tile: a row tile's column tiles sit on XCD (row tile % 8)
    const unsigned u_t = (unsigned)p.packed, tnn = (unsigned)p.tiles_n;
    const unsigned tiles_m = nwg / tnn;
    const unsigned full = (56u % u_t == 0u) ? (tiles_m / 56u) * 56u : 0u;
    if (orig < full * tnn) {
      const unsigned su = orig / (56u * tnn), l = orig - su * (56u * tnn);
      tn = (int)(l / 56u);
      tm = (int)(su * 56u + l % 56u);
    } else {
      // (units that do not divide 56, and the last row tiles of a launch: the last unit may be short) unit x column tiles
      const unsigned o2 = orig - full * tnn, unit = u_t * tnn;
      const unsigned u = o2 / unit, l = o2 - u * unit;
      const unsigned left = tiles_m - full - u * u_t, ul = left < u_t ? left : u_t;
      tn = (int)(l / ul);
      tm = (int)(full + u * u_t + l % ul);
    }
  } else if (p.cluster > 1) {
    // clustered form: the tiles of a group wait for each other, so they take CONSECUTIVE block ids (dispatched together);
    // XCD placement (round-robin over block ids: speed only, never correctness) keeps a row tile's column tiles together
    const unsigned c = (unsigned)p.cluster, tnn = (unsigned)p.tiles_n;
    const unsigned tiles_m = nwg / tnn;
    const unsigned full = (8u % c == 0u) ? (tiles_m / 8u) * 8u : 0u;   // row tiles covered by whole super-units of 8
    if (orig < full * tnn) {
      // super-unit = 8 row tiles x all column tiles, block = column tile * 8 + row tile: a row tile's column tiles all sit on
      // XCD (row tile % 8) and share its L2 copy of the A rows; the tiles of a cluster (c | 8) are c consecutive blocks
      const unsigned su = orig / (8u * tnn), l = orig - su * (8u * tnn);
      tn = (int)(l >> 3);
      tm = (int)(su * 8u + (l & 7u));
    } else {
      // (cluster sizes that do not divide 8, and the last row tiles of a launch) unit = cluster x column tiles
      const unsigned o2 = orig - full * tnn, unit = c * tnn;
      const unsigned u = o2 / unit, l = o2 - u * unit;
      tn = (int)(l / c);
      tm = (int)(full + u * c + l % c);
    }
  }
  const int m0 = tm * p.tile_rows;
  const int n0 = tn * L_BN;
  // rows of this tile that exist: one group, or one member of a cluster; the packed form: rows of one or two groups (the
  // staging below decodes every row's own frame, so a tile may start and end anywhere in a frame)
  const int used = m0 + p.tile_rows <= p.M ? p.tile_rows : p.M - m0;

  const char* __restrict__ x = p.x;
  const char* __restrict__ w = p.w;
  char* __restrict__ y = p.y;

  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const bool extra = wave < 2;                      // this wave stages rows 192 .. 223 too
  const int c = t & (L_CPRR - 1);
  const int rb = t >> 2;                            // 0 .. 63
  const int cq = AVS_LDS_CHUNK(L_CPRR, 2, rb, c);   // the k-chunk this thread fetches into slot c

  // ---- staging state: per-row tap masks and 32-bit buffer offsets (vector), the tap walk (scalar): igemm_params.h ----
  unsigned amask[4], aoff[4], boff[2];
  int f_tap = 0, f_ci0 = 0, f_kw = 0, f_koff = 0, f_kb = 0;
  __amdgpu_buffer_rsrc_t a_rsrc, b_rsrc;
  {
    const int taps = p.K / p.cin;
    int n_first;
    const long long a_origin = avs_tap_origin(p, m0, p.lin_stride, n_first);
    a_rsrc = avs_buffer_window(x + a_origin * 4);
    b_rsrc = avs_buffer_window(w + (p.w_kstep ? (long long)n0 * 64 : (long long)n0 * p.ldb * 4));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned mk = 0, off = AVS_BUF_OOB;
      const int r = rb + 64 * i;
      if (r < used) {
        const int m = m0 + r;
        if (p.lin_stride >= 0) {
          mk = ~0u;
          off = (unsigned)((long long)r * p.lin_stride * 4) + cq * 16;
        } else {
          const int n = m / p.HoWo;
          const int rem = m - n * p.HoWo;
          const int ho = rem / p.Wo;
          const int wo = rem - ho * p.Wo;
          const int hi0 = ho * p.sh - p.ph, wi0 = wo * p.sw - p.pw;
          if constexpr (SPATIAL) {
            for (int tp = 0; tp < taps; ++tp) {
              const int th = tp / p.KW, tw = tp - th * p.KW;
              if ((unsigned)(hi0 + th) < (unsigned)p.H && (unsigned)(wi0 + tw) < (unsigned)p.W) mk |= 1u << tp;
            }
          } else {
            mk = ~0u;
          }
          off = avs_tap_first<4>(p, n - n_first, hi0, wi0) + cq * 16;
        }
      }
      amask[i] = mk;
      aoff[i] = off;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      boff[i] = p.w_kstep ? (unsigned)((rb + 64 * i) * 64) + (unsigned)(cq >> 2) * (unsigned)p.N * 64u + (cq & 3) * 16
                          : (unsigned)((long long)(rb + 64 * i) * p.ldb * 4) + cq * 16;
  }

  auto stage = [&](int buf) {
    uint4* abuf = lds + buf * L_BUF + wave * 64;        // wave-uniform; lane l lands at +l
    uint4* bbuf = abuf + L_ROWS * L_CPRR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      unsigned off = aoff[i];
      if constexpr (SPATIAL) off = ((amask[i] >> f_tap) & 1u) ? off : AVS_BUF_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(abuf + 256 * i), 16,
                                               (int)off, f_koff, 0, 0);
    }
    if (extra) {
      unsigned off = aoff[3];
      if constexpr (SPATIAL) off = ((amask[3] >> f_tap) & 1u) ? off : AVS_BUF_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(abuf + 256 * 3), 16,
                                               (int)off, f_koff, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(b_rsrc, (__attribute__((address_space(3))) void*)(bbuf + 256 * i), 16,
                                               (int)boff[i], f_kb, 0, 0);
    avs_tap_advance<4>(p, f_tap, f_ci0, f_kw, f_koff, f_kb, L_STEP, L_STEP * 4, p.w_kstep ? p.N * 64 : L_STEP * 4);
  };

  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[L_MT];             // SHAPE 32
  f32x4 acc16[L_MT16][2];       // SHAPE 16: [16-row block][16-column block]
  if constexpr (SHAPE == 32) {
#pragma unroll
    for (int i = 0; i < L_MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < L_MT16; ++i)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc16[i][cb][e] = 0.f;
  }
  // SHAPE 16: lane (li, lg) feeds slots 8 * lg .. + 7 of A row rho(li) / B column li of a block and holds, of the result,
  // column li, rows 4 * rgp + 0 .. 3 (the row groups 2 and 3 trade places as the A rows do)
  const int li = lane & 15, lg = lane >> 4;
  const int rho = li ^ ((li >> 1) & 4);
  const int rgp = lg ^ (lg >> 1);
  // byte offsets inside a buffer (block b of A: + b * 1024, the second B block: + 1024; the swizzle term depends on the
  // row's low four bits only).  Even step: A chunks [0, 2, 1, 3][lg].  Odd step: [1, 3, 0, 2][lg] - the upper half read
  // first, the lower half when Q is issued.  B: P reads [0, 2, 0, 2][lg], Q reads [1, 3][lg & 1] (lanes 0 .. 31 from the even
  // step's buffer, lanes 32 .. 63 from the odd step's).
  unsigned fa16_even, fa16_odd, fb16_p, fb16_q;
  {
    const int hk = 2 * (lg & 1);
    fa16_even = (unsigned)AVS_LDS_SLOT(L_CPRR, 2, rho, hk + (lg >> 1)) * 16u;
    fa16_odd = (unsigned)AVS_LDS_SLOT(L_CPRR, 2, rho, hk + 1 - (lg >> 1)) * 16u;
    const int brow = wave * 32 + li;
    fb16_p = (unsigned)((L_ROWS + brow) * L_CPRR + AVS_LDS_CHUNK(L_CPRR, 2, brow, hk)) * 16u;
    fb16_q = (unsigned)((L_ROWS + brow) * L_CPRR + AVS_LDS_CHUNK(L_CPRR, 2, brow, hk + 1)) * 16u;
  }

  // per-lane fragment byte offsets inside a buffer: a row's chunks alternate hi8 | lo8; this lane half feeds elements
  // 8 * lh .. + 7 of the step: hi = chunk 2 * lh, lo = chunk 2 * lh + 1.  Block mt of A is mt * 32 rows further: an
  // immediate offset of the read (the swizzle term only depends on the row's low bits).
  const unsigned lds_base = (unsigned)(unsigned long long)((__attribute__((address_space(3))) char*)lds);
  unsigned fa_off[2], fb_off[2];
#pragma unroll
  for (int hl = 0; hl < 2; ++hl) {
    const int chunk = 2 * lh + hl;
    fa_off[hl] = (unsigned)AVS_LDS_SLOT(L_CPRR, 2, lr, chunk) * 16u;
    const int brow = wave * 32 + lr;
    fb_off[hl] = (unsigned)((L_ROWS + brow) * L_CPRR + AVS_LDS_CHUNK(L_CPRR, 2, brow, chunk)) * 16u;
  }

  // The residual rows of the first three blocks are fetched BEFORE the reduction (48 registers through the main loop),
  // the next three when it ends: no memory latency is left in front of the first stores, and the rest land under them.
  const int col = n0 + wave * 32 + lr;
  const float inv_n = 1.f / (float)p.tile_rows;   // (a tile holds exactly one group, or one member of a cluster; packed: unused)
  const int lim = used - 4 * lh;   // block-local row offsets below this one exist
  // the residual runs of a block: staged row rl0 (+ 16) of the block, columns 8 * grp .. + 7 of the wave's 32
  const int rl0 = lane >> 2, grp = lane & 3;
  const int col8 = n0 + wave * 32 + grp * 8;
  constexpr int DEPTH = 6;   // blocks of residual rows in flight
  uint4 rhi[DEPTH][2], rlo[DEPTH][2];
  auto res_fetch = [&](auto blk) {
    constexpr int mt = decltype(blk)::value;
    const long long row0 = (long long)m0 + mt * 32 + rl0;
    const char* base = p.residual + (row0 * p.ldr + col8) * 4;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      // rows that do not exist read the residual's first run (never used): no divergent branch around the loads
      const bool ok = mt * 32 + rl0 + 16 * it < used;
      const uint4* rp = reinterpret_cast<const uint4*>(ok ? base + (long long)it * 16 * p.ldr * 4 : p.residual);
      rhi[mt % DEPTH][it] = rp[0];
      rlo[mt % DEPTH][it] = rp[1];
    }
  };
  // (SHAPE 16 holds eight more fragment registers through the loop and keeps two blocks' rows in flight there, not three)
  if (p.residual) {
    res_fetch(std::integral_constant<int, 0>{});
    res_fetch(std::integral_constant<int, 1>{});
    if constexpr (SHAPE == 32) res_fetch(std::integral_constant<int, 2>{});
  }

  const int steps = p.K / L_STEP;
  stage(0);
  if (steps > 1) stage(1);
  int cur = 0;  // buffer holding step s
  if constexpr (SHAPE == 32) {
    for (int s = 0; s < steps; ++s) {
      if (s + 1 < steps) {
        if (extra)
          asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      const unsigned bbase = lds_base + (unsigned)cur * (L_BUF * 16u);
      uint4 fah[L_MT], fal[L_MT], fbh, fbl;
      fbh = avs_lds_read_b128(bbase + fb_off[0]);
      read_blocks(fah, bbase + fa_off[0], std::make_integer_sequence<int, L_MT>{});
      fbl = avs_lds_read_b128(bbase + fb_off[1]);
      read_blocks(fal, bbase + fa_off[1], std::make_integer_sequence<int, L_MT>{});
      // the DMA of step s+2 is issued while the fragment reads are in flight
      if (s + 2 < steps) stage(cur == 0 ? 2 : cur - 1);  // (s+2) % 3 == (cur + 2) % 3
      // hi*hi starts as soon as the hi fragments have landed (LDS reads return in order); every fragment passes through an
      // empty asm after the wait that covers it, so no use of it can be scheduled ahead of that wait
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(1 + L_MT) : "memory");
      avs_pin(fbh);
  #pragma unroll
      for (int mt = 0; mt < L_MT; ++mt) avs_pin(fah[mt]);
      __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
      for (int mt = 0; mt < L_MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(avs_f16x8, fah[mt]),
                                                         __builtin_bit_cast(avs_f16x8, fbh), acc[mt], 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      avs_pin(fbl);
  #pragma unroll
      for (int mt = 0; mt < L_MT; ++mt) avs_pin(fal[mt]);
      __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
      for (int mt = 0; mt < L_MT; ++mt) {
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(avs_f16x8, fal[mt]),
                                                         __builtin_bit_cast(avs_f16x8, fbh), acc[mt], 0, 0, 0);
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(avs_f16x8, fah[mt]),
                                                         __builtin_bit_cast(avs_f16x8, fbl), acc[mt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      cur = cur == 2 ? 0 : cur + 1;
    }
  } else {
    // the same ring, barriers, DMA position and vmcnt waits; two steps per trip.  LDS reads return in order: every wait
    // below names how many of the reads issued so far may still be in flight.
    auto step_wait = [&](int s) {
      if (s + 1 < steps) {
        if (extra)
          asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    };
    auto mfma_blocks = [&](auto first, const uint4 (&a)[L_MT16], const uint4 (&b)[2]) {
      constexpr int b0 = decltype(first)::value;
#pragma unroll
      for (int mt = b0; mt < b0 + 7; ++mt)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          acc16[mt][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(avs_f16x8, a[mt]),
                                                                 __builtin_bit_cast(avs_f16x8, b[cb]), acc16[mt][cb], 0, 0, 0);
    };
    auto pin7 = [&](auto first, uint4 (&a)[L_MT16]) {
      constexpr int b0 = decltype(first)::value;
#pragma unroll
      for (int mt = b0; mt < b0 + 7; ++mt) avs_pin(a[mt]);
    };
    constexpr std::integral_constant<int, 0> B0{};
    constexpr std::integral_constant<int, 7> B7{};
    uint4 fa[L_MT16], fbp[2], fbq[2];
    auto even_step = [&](int s) {
      // ---- even step: P from full-wave reads; fa's lanes 0 .. 31 and fbq's (the step's lo chunks) stay for Q ----
      step_wait(s);
      const unsigned bbase = lds_base + (unsigned)cur * (L_BUF * 16u);
      fbp[0] = lds_read_b128_at<0>(bbase + fb16_p);
      fbp[1] = lds_read_b128_at<1024>(bbase + fb16_p);
      read_blocks16(fa, bbase + fa16_even, std::make_integer_sequence<int, L_MT16>{});
      if (s + 2 < steps) stage(cur == 0 ? 2 : cur - 1);
      asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");     // fbp, fa[0 .. 6]
      avs_pin(fbp[0]);
      avs_pin(fbp[1]);
      pin7(B0, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B0, fa, fbp);
      __builtin_amdgcn_sched_barrier(0);
      fbq[0] = lds_read_b128_at<0>(bbase + fb16_q);          // (never more than 16 reads in flight, as in the SHAPE 32 loop)
      fbq[1] = lds_read_b128_at<1024>(bbase + fb16_q);
      asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");     // fa[7 .. 13]
      pin7(B7, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B7, fa, fbp);
      __builtin_amdgcn_sched_barrier(0);
      cur = cur == 2 ? 0 : cur + 1;
    };
    auto odd_step = [&](int s) {
      // ---- odd step: Q of the pair from upper-half reads, then P from lower-half reads into the same registers ----
      step_wait(s);
      const unsigned bbase = lds_base + (unsigned)cur * (L_BUF * 16u);
      read_upper2(fbq, bbase + fb16_q);
      read_half7<0, true>(fa, bbase + fa16_odd);
      read_half7<7, true>(fa, bbase + fa16_odd);
      if (s + 2 < steps) stage(cur == 0 ? 2 : cur - 1);
      asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");     // fbq, fa[0 .. 6] (upper)
      avs_pin(fbq[0]);
      avs_pin(fbq[1]);
      pin7(B0, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B0, fa, fbq);
      __builtin_amdgcn_sched_barrier(0);
      read_half7<0, false>(fa, bbase + fa16_odd);
      fbp[0] = lds_read_b128_at<0>(bbase + fb16_p);
      fbp[1] = lds_read_b128_at<1024>(bbase + fb16_p);
      asm volatile("s_waitcnt lgkmcnt(9)" ::: "memory");     // fa[7 .. 13] (upper)
      pin7(B7, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B7, fa, fbq);
      __builtin_amdgcn_sched_barrier(0);
      read_half7<7, false>(fa, bbase + fa16_odd);
      asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");     // fbp, fa[0 .. 6] (lower)
      avs_pin(fbp[0]);
      avs_pin(fbp[1]);
      pin7(B0, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B0, fa, fbp);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      pin7(B7, fa);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B7, fa, fbp);
      __builtin_amdgcn_sched_barrier(0);
      cur = cur == 2 ? 0 : cur + 1;
    };
    int s = 0;
    for (; s + 1 < steps; s += 2) {
      even_step(s);
      odd_step(s + 1);
    }
    if (s < steps) {
      even_step(s);
      // an odd step count: the last Q carries one step, its partner half zeroed on both operands
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      zero_upper(fbq[0]);
      zero_upper(fbq[1]);
#pragma unroll
      for (int mt = 0; mt < L_MT16; ++mt) zero_upper(fa[mt]);
      __builtin_amdgcn_sched_barrier(0);
      mfma_blocks(B0, fa, fbq);
      mfma_blocks(B7, fa, fbq);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: the group's BatchNorm from this wave's own registers, then 32 rows at a time through LDS ----
  // A lane holds column lr of its wave's 32, rows avs_acc_row(0, e) + 4 * lh of every block; rows >= used are
  // exact zeros (their operand rows were never fetched).
  if (p.residual) {
    if constexpr (SHAPE == 16) res_fetch(std::integral_constant<int, 2>{});
    res_fetch(std::integral_constant<int, 3>{});
    res_fetch(std::integral_constant<int, 4>{});
    res_fetch(std::integral_constant<int, 5>{});
  }
  // The packed form's tile may hold rows of two groups, the boundary at row 112: blocks 0 .. 2 and elements e < 8 of block 3
  // (rows 96 .. 111) are the first segment - static per accumulator element, no selects.  A tile without a boundary adds
  // its two halves' sums up (one segment); the unpacked form keeps its one sequential sum (the bits it always gave).
  const int seg0 = p.packed ? (int)min((long long)used, (m0 / p.rows_per_group + 1ll) * p.rows_per_group - m0) : used;
  const bool shared = seg0 < used;   // (block-uniform) two segments, 112 rows each
  float mean, mean_b, s2, s2b = 0.f;
  if constexpr (SHAPE == 16) {
    // A lane holds columns li and 16 + li of its wave's 32, rows 16 * mt + 4 * rgp + e of both: a column's sums are this
    // lane's plus the three other row groups' (shuffles across 16 and 32 lanes), two centred rounds as above.  The packed
    // boundary at row 112 lies between blocks 6 and 7.  The lane then keeps, as a SHAPE 32 lane does, the statistics of
    // column lr = lane & 31 - those of its column block (lane >> 4) & 1 - so the exchanges below are the same bytes.
    const int lim16 = used - 4 * rgp;   // block-local row offsets below this one exist
    const float inv0 = p.packed ? 1.f / (float)seg0 : inv_n, inv1 = 1.f / (float)(shared ? used - seg0 : seg0);   // (uniform)
    float mc[2], mbc[2], qc[2], qbc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float s1 = 0.f, s1b = 0.f;
#pragma unroll
      for (int mt = 0; mt < L_MT16; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (mt < L_MT16 / 2)
            s1 += acc16[mt][cb][e];
          else
            s1b += acc16[mt][cb][e];
        }
      s1 += __shfl_xor(s1, 16, 64);
      s1b += __shfl_xor(s1b, 16, 64);
      s1 += __shfl_xor(s1, 32, 64);
      s1b += __shfl_xor(s1b, 32, 64);
      mc[cb] = (shared ? s1 : s1 + s1b) * inv0;
      mbc[cb] = shared ? s1b * inv1 : mc[cb];
      float q = 0.f, qb = 0.f;
#pragma unroll
      for (int mt = 0; mt < L_MT16; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int roff = mt * 16 + e;
          if (mt < L_MT16 / 2) {
            const float d = acc16[mt][cb][e] - mc[cb];
            q = roff < lim16 ? fmaf(d, d, q) : q;
          } else {
            const float d = acc16[mt][cb][e] - mbc[cb];
            qb = roff < lim16 ? fmaf(d, d, qb) : qb;
          }
        }
      q += __shfl_xor(q, 16, 64);
      qb += __shfl_xor(qb, 16, 64);
      q += __shfl_xor(q, 32, 64);
      qb += __shfl_xor(qb, 32, 64);
      qc[cb] = shared ? q : q + qb;
      qbc[cb] = qb;
    }
    const bool c1 = (lg & 1) != 0;
    mean = c1 ? mc[1] : mc[0];
    mean_b = c1 ? mbc[1] : mbc[0];
    s2 = c1 ? qc[1] : qc[0];
    s2b = c1 ? qbc[1] : qbc[0];
  } else if (p.packed) {
    float s1 = 0.f, s1b = 0.f;
#pragma unroll
    for (int mt = 0; mt < L_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (mt < 3 || (mt == 3 && e < 8))
          s1 += acc[mt][e];
        else
          s1b += acc[mt][e];
      }
    s1 += __shfl_xor(s1, 32, 64);
    s1b += __shfl_xor(s1b, 32, 64);
    const float inv0 = 1.f / (float)seg0, inv1 = 1.f / (float)(shared ? used - seg0 : seg0);   // (uniform)
    mean = (shared ? s1 : s1 + s1b) * inv0;
    mean_b = shared ? s1b * inv1 : mean;
    s2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < L_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int roff = avs_acc_row(mt * 32, e);
        if (mt < 3 || (mt == 3 && e < 8)) {
          const float d = acc[mt][e] - mean;
          s2 = roff < lim ? fmaf(d, d, s2) : s2;
        } else {
          const float d = acc[mt][e] - mean_b;
          s2b = roff < lim ? fmaf(d, d, s2b) : s2b;
        }
      }
    s2 += __shfl_xor(s2, 32, 64);
    s2b += __shfl_xor(s2b, 32, 64);
    if (!shared) s2 += s2b;
  } else {
    float s1 = 0.f;
#pragma unroll
    for (int mt = 0; mt < L_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) s1 += acc[mt][e];
    s1 += __shfl_xor(s1, 32, 64);
    mean = mean_b = s1 * inv_n;
    s2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < L_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int roff = avs_acc_row(mt * 32, e);
        const float d = acc[mt][e] - mean;
        s2 = roff < lim ? fmaf(d, d, s2) : s2;
      }
    s2 += __shfl_xor(s2, 32, 64);
  }
  float g_mean = mean, g_var = s2 * inv_n;
  float g_mean_b = 0.f, g_var_b = 0.f;   // the shared tile's second group
  if (p.packed) {
    // ---- the packed form's exchange: the protocol of the unpacked one below (value | epoch in one agent-scope store, every
    // wave publishes - both segments - before it polls, a bounded poll, p.xerr), one granule per lane and SEGMENT: slot
    // [tile][column tile][wave][segment][lane].  A tile gathers, for each of its one or two groups, the group's segment of
    // every tile the group touches and merges them by Chan's update in tile order, the row counts (112 or 224) taken from
    // the geometry.  ONE copy of the merge code runs for both groups of a shared tile (a loop that is not unrolled): every
    // tile of a group applies the same instructions to the same operands in the same order -> the same bits.
    const long long gstride = (long long)p.tiles_n * 4 * 2 * 64;   // granules between consecutive row tiles
    // (a uniform base + the lane: the loads and stores take the base from scalar registers)
    unsigned long long* const cbase = p.xchg + ((long long)tn * 4 + wave) * 2 * 64;
    unsigned long long* slot = cbase + tm * gstride + lane;
    __hip_atomic_store(slot, ((unsigned long long)p.epoch << 32) | (unsigned long long)__float_as_uint(lh ? s2 : mean),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (shared)
      __hip_atomic_store(slot + 64, ((unsigned long long)p.epoch << 32) | (unsigned long long)__float_as_uint(lh ? s2b : mean_b),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long rpg = p.rows_per_group;
    const long long g0 = m0 / rpg;
#pragma unroll 1
    for (int sg = 0; sg <= (shared ? 1 : 0); ++sg) {
      const long long f0 = (g0 + sg) * rpg;                        // the group's rows f0 .. f0 + rpg - 1
      const int tf = (int)(f0 / L_ROWS), tl = (int)((f0 + rpg - 1) / L_ROWS);
      float n = 0.f, mu = 0.f, m2 = 0.f;
      for (int j0 = tf; j0 <= tl; j0 += 4) {
        // four granules in flight at once (one latency for the usual four tiles of a group), then each is verified and - only
        // if its tag is not this launch's yet - polled on.  The tile's own granule is read back like a partner's (the same
        // bits): its statistics need not stay in registers through the merge.
        unsigned long long g[4];
        // tile j's granule of this group (a scalar offset): segment 1 where the group starts inside the tile
        auto granule = [&](int j) { return cbase + (j * gstride + ((long long)j * L_ROWS < f0 ? 64 : 0)) + lane; };
#pragma unroll
        for (int u = 0; u < 4; ++u)   // (past the group: a valid address, unused)
          g[u] = __hip_atomic_load(granule(j0 + u <= tl ? j0 + u : tm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u;
          if (j > tl) break;
          const long long lo = max(f0, (long long)j * L_ROWS), hi = min(f0 + rpg, (long long)(j + 1) * L_ROWS);
          const float nt = (float)(hi - lo);
          bool ok = (unsigned)(g[u] >> 32) == p.epoch;
#pragma unroll 1
          for (int spin = 0; spin < (1 << 20) && __builtin_amdgcn_read_exec() != __builtin_amdgcn_ballot_w64(ok); ++spin) {
            __builtin_amdgcn_s_sleep(8);
            g[u] = __hip_atomic_load(granule(j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = (unsigned)(g[u] >> 32) == p.epoch;
          }
          if (__builtin_amdgcn_read_exec() != __builtin_amdgcn_ballot_w64(ok) && lane == 0) atomicAdd(p.xerr, 1u);
          const float v = __uint_as_float((unsigned)g[u]);
          const float o = __shfl_xor(v, 32, 64);
          const float mj = lh ? o : v, qj = lh ? v : o;
          // Chan's update in tile order: the same operands in the same order on every tile of the group -> the same bits
          const float tot = n + nt, delta = mj - mu;
          mu += delta * (nt / tot);
          m2 += qj + delta * delta * (n * nt / tot);
          n = tot;
        }
      }
      const float gv = m2 / n;
      if (sg) {
        g_mean_b = mu;
        g_var_b = gv;
      } else {
        g_mean = mu;
        g_var = gv;
      }
    }
  } else if (p.cluster > 1) {
    // ---- one exchange with the other tiles of the group (same columns): lane (lr, lh) publishes the tile's mean (lh = 0) or
    // centred sum of squares (lh = 1) of column lr as an 8-byte {value, epoch} granule - ONE agent-scope store, untorn, so
    // the tag IS the flag: no fence, no separate flag word - then reads the same granule of every partner until its tag is
    // this launch's epoch.  Every wave publishes before it polls (no circular wait); partners are neighbours in dispatch
    // order; the wait is bounded (p.xerr counts the waves that gave up: 0 after a healthy launch).
    const int cj = tm % p.cluster, t0 = tm - cj;
    unsigned long long* slot = p.xchg + (((long long)tm * p.tiles_n + tn) * 4 + wave) * 64 + lane;
    const float mine = lh ? s2 : mean;
    __hip_atomic_store(slot, ((unsigned long long)p.epoch << 32) | (unsigned long long)__float_as_uint(mine), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    const float nt = (float)p.tile_rows;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    const unsigned long long* const gbase = p.xchg + (((long long)t0 * p.tiles_n + tn) * 4 + wave) * 64 + lane;
    const long long gstride = (long long)p.tiles_n * 4 * 64;      // granules between consecutive row tiles
    for (int j0 = 0; j0 < p.cluster; j0 += 4) {
      // four partners' granules in flight at once (one latency for the usual cluster of four), then each is verified and -
      // only if its tag is not this launch's yet - polled on
      unsigned long long g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u < p.cluster ? j0 + u : cj;           // (past the cluster / own tile: a valid address, unused)
        g[u] = __hip_atomic_load(gbase + j * gstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j >= p.cluster) break;
        float mj = mean, qj = s2;
        if (j != cj) {
          bool ok = (unsigned)(g[u] >> 32) == p.epoch;
          for (int spin = 0; spin < (1 << 20) && __builtin_amdgcn_read_exec() != __builtin_amdgcn_ballot_w64(ok); ++spin) {
            __builtin_amdgcn_s_sleep(8);
            g[u] = __hip_atomic_load(gbase + j * gstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = (unsigned)(g[u] >> 32) == p.epoch;
          }
          if (__builtin_amdgcn_read_exec() != __builtin_amdgcn_ballot_w64(ok) && lane == 0) atomicAdd(p.xerr, 1u);
          const float v = __uint_as_float((unsigned)g[u]);
          const float o = __shfl_xor(v, 32, 64);
          mj = lh ? o : v;
          qj = lh ? v : o;
        }
        // Chan's update in tile order: the same operands in the same order on every tile of the group -> the same bits
        const float tot = n + nt, delta = mj - mu;
        mu += delta * (nt / tot);
        m2 += qj + delta * delta * (n * nt / tot);
        n = tot;
      }
    }
    g_mean = mu;
    g_var = m2 / n;
  }
  const float sc = p.gamma[col] / sqrtf(g_var + p.eps);
  const float sf = p.beta[col] - g_mean * sc;
  float sc_b = sc, sf_b = sf;   // rows 112 .. 223: the shared tile's second (scale, shift) pair, else the same
  if (shared) {
    sc_b = p.gamma[col] / sqrtf(g_var_b + p.eps);
    sf_b = p.beta[col] - g_mean_b * sc_b;
  }
  if constexpr (SHAPE == 32) {
#pragma unroll
    for (int mt = 0; mt < L_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const bool first = mt < 3 || (mt == 3 && e < 8);   // (static per element)
        acc[mt][e] = fmaf(acc[mt][e], first ? sc : sc_b, first ? sf : sf_b);
      }
  } else {
    // the pairs above are column lr's: one shuffle each gives the lane those of the other column block
    const bool c1 = (lg & 1) != 0;
    const float sc_o = __shfl_xor(sc, 16, 64), sf_o = __shfl_xor(sf, 16, 64);
    const float scb_o = __shfl_xor(sc_b, 16, 64), sfb_o = __shfl_xor(sf_b, 16, 64);
    const float sc2[2] = {c1 ? sc_o : sc, c1 ? sc : sc_o}, sf2[2] = {c1 ? sf_o : sf, c1 ? sf : sf_o};
    const float scb2[2] = {c1 ? scb_o : sc_b, c1 ? sc_b : scb_o}, sfb2[2] = {c1 ? sfb_o : sf_b, c1 ? sf_b : sfb_o};
#pragma unroll
    for (int mt = 0; mt < L_MT16; ++mt)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool first = mt < L_MT16 / 2;   // (static per block)
          acc16[mt][cb][e] = fmaf(acc16[mt][cb][e], first ? sc2[cb] : scb2[cb], first ? sf2[cb] : sfb2[cb]);
        }
  }
  const bool relu = p.act == AVS_ACT_RELU;

  __syncthreads();   // every wave has read its last fragments: the staging regions alias the operand buffers
  float* const wreg = reinterpret_cast<float*>(lds) + wave * (32 * L_P);
  auto emit = [&](auto blk) {
    constexpr int mt = decltype(blk)::value;
    if constexpr (SHAPE == 32) {
#pragma unroll
      for (int e = 0; e < 16; ++e) wreg[(avs_acc_row(0, e) + 4 * lh) * L_P + lr] = acc[mt][e];
    } else {
      // two 16-row blocks make the 32 staged rows; lanes li and 16 + li of a store share a bank (two-way: free for stores)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e) wreg[(h * 16 + 4 * rgp + e) * L_P + cb * 16 + li] = acc16[2 * mt + h][cb][e];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const long long row0 = (long long)m0 + mt * 32 + rl0;
    char* const ybase = y + (row0 * p.ldc + col8) * 4;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const float* src = wreg + (rl0 + 16 * it) * L_P + grp * 8;
      const float4 f0 = *reinterpret_cast<const float4*>(src);
      const float4 f1 = *reinterpret_cast<const float4*>(src + 4);
      if (!(mt * 32 + rl0 + 16 * it < used)) continue;
      float v[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
      if (p.residual) {
        float rv[8];
        avs_pin(rhi[mt % DEPTH][it]);
        avs_pin(rlo[mt % DEPTH][it]);
        avs_f16x2_join8(rhi[mt % DEPTH][it], rlo[mt % DEPTH][it], rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += rv[j];
      }
      if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      uint4 hi, lo;
      avs_f16x2_split8(v, hi, lo);
      uint4* dst = reinterpret_cast<uint4*>(ybase + (long long)it * 16 * p.ldc * 4);
      dst[0] = hi;
      dst[1] = lo;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if constexpr (mt + DEPTH < L_MT) {
      if (p.residual) res_fetch(std::integral_constant<int, mt + DEPTH>{});
    }
  };
  emit(std::integral_constant<int, 0>{});
  emit(std::integral_constant<int, 1>{});
  emit(std::integral_constant<int, 2>{});
  emit(std::integral_constant<int, 3>{});
  emit(std::integral_constant<int, 4>{});
  emit(std::integral_constant<int, 5>{});
  emit(std::integral_constant<int, 6>{});
}

// The shapes the 224-row form takes: AVS_F16X2, one group of 193 .. 224 rows per tile, cout in multiples of 128, a
// reduction walked by the scalar tap walk in 64-byte steps inside the 2 GiB buffer window, the caller not asking for
// another tile (avs_conv_desc.variant: AVS_TILE_AUTO or AVS_TILE_224).  The packed clustered form (AVS_CLUSTER_PACKED): tiles
// of 224 consecutive rows, groups of a multiple of 112 rows.
bool igemm_h2_local224_ok(const IgemmParams& p, int dtype, long long lin_stride) {
  const int tile_mode = p.variant & 3;
  if (dtype != AVS_F16X2 || !(tile_mode == AVS_TILE_AUTO || tile_mode == AVS_TILE_224)) return false;
  if (p.variant & AVS_STAGING_GENERIC) return false;
  const int cl = p.cluster > 1 ? p.cluster : 1;
  if (p.packed) {
    // (bncluster_plan: 224 consecutive rows per tile, groups of a multiple of 112 rows)
    if (p.tile_rows != L_ROWS || p.cluster <= 1 || p.rows_per_group < L_ROWS || p.rows_per_group % (L_ROWS / 2) != 0) return false;
  } else if (p.tile_rows * cl != p.rows_per_group || p.tile_rows <= 192 || p.tile_rows > L_ROWS) {
    return false;
  }
  if (p.N % L_BN != 0 || p.M % p.rows_per_group != 0) return false;
  if (p.cin % L_STEP != 0 || p.K % L_STEP != 0 || p.K % p.cin != 0 || p.K / p.cin > 32) return false;
  return igemm_buffer_window_ok(p, lin_stride, 4, L_BN);
}

// The matrix instruction each instance ships with (profiles/r07_*: kept per instance as measured).  The study build can
// force either shape for both instances: AVS_LOCAL224_MFMA = 16 or 32.
constexpr int L_SHAPE_SPATIAL = 32;
constexpr int L_SHAPE_POINT = 16;

void igemm_h2_local224_launch(const IgemmParams& p, bool spatial, dim3 grid, hipStream_t stream) {
#ifdef AVS_STUDY
  const int forced = getenv("AVS_LOCAL224_MFMA") ? atoi(getenv("AVS_LOCAL224_MFMA")) : 0;
  if (forced == 16 || forced == 32) {
    if (spatial && forced == 16)
      hipLaunchKernelGGL((igemm_h2_local224_kernel<true, 16>), grid, dim3(256), 0, stream, p);
    else if (spatial)
      hipLaunchKernelGGL((igemm_h2_local224_kernel<true, 32>), grid, dim3(256), 0, stream, p);
    else if (forced == 16)
      hipLaunchKernelGGL((igemm_h2_local224_kernel<false, 16>), grid, dim3(256), 0, stream, p);
    else
      hipLaunchKernelGGL((igemm_h2_local224_kernel<false, 32>), grid, dim3(256), 0, stream, p);
    return;
  }
#endif
  if (spatial)
    hipLaunchKernelGGL((igemm_h2_local224_kernel<true, L_SHAPE_SPATIAL>), grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((igemm_h2_local224_kernel<false, L_SHAPE_POINT>), grid, dim3(256), 0, stream, p);
}
