/*
 * avsum_render.h — C-ABI of libavsum_render.so: the summary itself, rendered on the MI355X (gfx950) - a selection mask
 * in; the list of picked frames, the frames in the layout an encoder takes, and the matching audio out; nothing read
 * back.  An eighth, self-contained library: it shares no symbol and no state with the other seven.
 *
 *   avsr_summary_index     mask -> frame list, runs and per-video offsets (three launches, no atomics, no waiting)
 *   avsr_bgr_to_yuv_u8     (gathered) uint8 BGR frames -> YUV 4:2:0 of any layout the surface description covers
 *   avsr_repack_u8         (gathered) YUV 4:2:0 frames -> another layout of the SAME depth, samples copied
 *   avsr_audio_cut         the runs' samples of every track, concatenated, with an optional linear fade
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSR_OK (0) or a negative AVSR_E_* code; never
 *     throws.  avsr_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller, h_* is HOST memory read before the call returns;
 *     nothing is allocated or freed: workspaces are the caller's.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside.
 *
 * 1. THE SUMMARY INDEX.  d_mask uint8 [n]: frame i is in the summary where d_mask[i] != 0.  h_offsets / d_offsets
 * int64 [nvideos + 1] (the same numbers on the host, where they are checked, and on the device, where they are read):
 * video v is frames offsets[v] .. offsets[v + 1]; they start at 0, increase strictly and end at n <= AVSR_MAX_FRAMES.
 * d_tiles int32 [ntiles, AVSR_TILE_COLS] = (video, k): every video's tiles k = 0 .. ceil(n_v / AVSR_TILE) - 1 of
 * AVSR_TILE frames, video after video; ntiles must be the number the offsets give.  A RUN is a maximal stretch of
 * selected frames inside ONE video: frame i starts one where it is selected and is its video's first frame or follows an
 * unselected one, so a run never crosses a video boundary.  Results, all int64:
 *   d_frame_index [frame_cap]     the global source frame of summary frame j, videos in order; every entry from the true
 *                                 count on is -1 (the gathered entry points skip an index outside their frames)
 *   d_frame_offsets [nvideos + 1] summary frames before video v (the TRUE numbers, even past frame_cap)
 *   d_runs [run_cap, 2]           (start, end) of every run, video-relative, end exclusive; rows from the true count on
 *                                 are (-1, -1)
 *   d_run_offsets [nvideos + 1]   runs before video v (TRUE numbers)
 *   d_totals [nvideos, AVSR_TOTAL_COLS] = (runs, frames, 0) of video v, TRUE counts; the third column is
 *                                 avsr_audio_cut's
 * Every store is guarded by its capacity: what does not fit is not written, and nothing is written past a buffer.
 * d_work int64 [ntiles, 2] is the caller's workspace (per-tile counts, scanned in place).  Three launches: (1) one
 * workgroup per tile counts its selected frames and its run starts; (2) ONE workgroup scans the tile counts in order
 * and writes the per-video tables; (3) one workgroup per tile scatters, and further workgroups write the -1 tails.  No
 * atomic operation, and no workgroup waits for another: the order comes from the launch boundaries alone.
 *
 * 2. PIXELS.  ONE surface description for every 4:2:0 layout, that of avsum_yuv.h: h_surface, a host
 * int64_t[AVSR_SURFACE_INTS] holding, in this order (the AVSR_S_* indices), n, h, w, sample_bytes (1: depth 8; 2: depth
 * 10 in a little-endian 16-bit word), shift (0 or 6; 0 for one-byte samples), pitch_y, pitch_c, chroma_step, u_offset,
 * v_offset, frame_stride, offsets in bytes from a frame's first byte.  Sample addresses as in avsum_yuv.h:
 *   Y(y, x)   at f + y * pitch_y + x * sample_bytes
 *   U(cy, cx) at f + u_offset + cy * pitch_c + cx * chroma_step,   V likewise from v_offset
 * Refused (AVSR_E_SHAPE) before any HIP call: extents that are odd or below 2; a sample_bytes, shift or step outside the
 * above; a pitch shorter than its row of samples; a plane whose last sample ends past frame_stride; Y, U and V sample
 * sets of a frame that share a byte (an OVERLAPPING destination would be written twice); for two-byte samples an odd
 * base, offset, pitch, chroma_step or frame_stride; and a destination whose bytes overlap the source's.  A one-byte
 * surface may start at ANY byte.
 * Storage: a one-byte sample is stored as the byte; a two-byte sample as the little-endian word sample << shift, its
 * other bits zero.  Destination bytes that belong to no sample (pitch padding, gaps, spare rows) are left as they were.
 *
 * The FORWARD definition.  h_forward is AVSR_FORWARD_INTS = ten ints (y_off, yb, yg, yr, ub, ug, ur, vb, vg, vr) in
 * AVSR_SHIFT = 20 fractional bits.  Refused (AVSR_E_ARG) before any HIP call: y_off outside 0 .. 255; a row (yb, yg,
 * yr), (ub, ug, ur) or (vb, vg, vr) whose sum of |c| exceeds AVSR_MAX_ROW_SUM = 2^20 - with that limit no sum below
 * leaves int32 (2^20 * 1020 + 2^21 < 2^31).  With k = depth - 8, top = 2^depth - 1 and >> the arithmetic shift:
 *   Y(y, x)   = clamp(((yb * B + yg * G + yr * R + 2^(19 - k)) >> (20 - k)) + (y_off << k), 0, top)
 *   SB, SG, SR = the sums of B, G, R over the block's four pixels (2cy .. 2cy + 1, 2cx .. 2cx + 1)
 *   U(cy, cx) = clamp(((ub * SB + ug * SG + ur * SR + 2^(21 - k)) >> (22 - k)) + (128 << k), 0, top)
 *   V(cy, cx) likewise with vb, vg, vr
 * The chroma sample is the ONE rounding of the block's mean, not the mean of four rounded values.
 *
 * avsr_repack_u8 copies samples: destination sample = source sample, Y for Y, U for U, V for V, for source and
 * destination descriptions of the same h, w and sample_bytes.  Whatever the other six bits of a 16-bit source word hold
 * is dropped: the destination word is ((w16 >> shift_src) & 1023) << shift_dst.  A differing sample_bytes is refused
 * (AVSR_E_UNSUPPORTED): changing the depth would need tone mapping to mean anything.
 *
 * 3. AUDIO.  d_wave fp32 [wave_offsets[nvideos]]: the tracks concatenated, track v at wave_offsets[v] ..
 * wave_offsets[v + 1] (h_ / d_wave_offsets int64 [nvideos + 1], start at 0, do not decrease).  d_fps double [nvideos].
 * For run (s, e) of video v, with len_v the samples of its track,
 *   a = min((int64)floor((double)s / fps_v * (double)sr), len_v),   b likewise from e,   L = b - a
 * in IEEE double arithmetic, no contraction (the arithmetic of ShotBatchResult.audio_bounds).  The L samples a .. b of
 * the track are copied in order, run after run, video after video.  With F' = min(fade, L / 2) (integer division),
 * sample i of the run is multiplied, in fp32, by (float)(i + 1) / (float)(F' + 1) for i < F', by
 * (float)(L - i) / (float)(F' + 1) for i >= L - F', and is copied otherwise: one fp32 division and one fp32
 * multiplication.  fade = 0 is a pure copy.  Results: d_audio fp32 [sample_cap] (samples from the true count on are
 * left as they were), d_audio_offsets int64 [nvideos + 1] (TRUE numbers), column 2 of d_totals.  Runs are read from
 * d_runs / d_run_offsets as avsr_summary_index left them; rows past run_cap do not exist and are not read.  d_work
 * int64 [run_cap, AVSR_AUDIO_COLS] = (first source sample in d_wave, first destination sample, L) per run.  Two
 * launches: ONE workgroup computes the bounds and their prefix (no atomics), then the copy, whose grid covers sample_cap
 * in pieces of AVSR_AUDIO_TILE samples; workgroups past the true count exit.
 */
#ifndef AVSUM_RENDER_H
#define AVSUM_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSR_ABI_VERSION 1

#define AVSR_TILE 1024             /* frames of one tile of the summary index                                    */
#define AVSR_TILE_COLS 2           /* int32 per row of the tile table: (video, k)                                */
#define AVSR_MAX_FRAMES 16777216   /* 2^24: frames of one avsr_summary_index call at most                        */
#define AVSR_TOTAL_COLS 3          /* int64 per video of d_totals: (runs, frames, samples)                       */
#define AVSR_SHIFT 20              /* fractional bits of the forward matrix                                      */
#define AVSR_MAX_ROW_SUM 1048576   /* 2^20: the largest sum of |c| over a row of the forward matrix              */
#define AVSR_FORWARD_INTS 10       /* ints of h_forward                                                          */
#define AVSR_SURFACE_INTS 11       /* int64s of h_surface                                                        */
#define AVSR_AUDIO_TILE 2048       /* output samples of one workgroup of the audio copy                          */
#define AVSR_AUDIO_COLS 3          /* int64 per run of avsr_audio_cut's workspace                                */

enum {                             /* the order of h_surface: avsum_yuv.h's */
  AVSR_S_N = 0,
  AVSR_S_H = 1,
  AVSR_S_W = 2,
  AVSR_S_SAMPLE_BYTES = 3,
  AVSR_S_SHIFT = 4,
  AVSR_S_PITCH_Y = 5,
  AVSR_S_PITCH_C = 6,
  AVSR_S_CHROMA_STEP = 7,
  AVSR_S_U_OFFSET = 8,
  AVSR_S_V_OFFSET = 9,
  AVSR_S_FRAME_STRIDE = 10
};

enum {
  AVSR_OK = 0,
  AVSR_E_ARG = -1,         /* null pointer / coefficient, count or capacity out of range */
  AVSR_E_SHAPE = -2,       /* sizes inconsistent with what the kernel assumes            */
  AVSR_E_HIP = -4,         /* the HIP runtime reported an error at launch                */
  AVSR_E_UNSUPPORTED = -6  /* this entry point does not take the request                 */
};

typedef void* avsr_stream_t;

int avsr_abi_version(void);
const char* avsr_last_error(void);

/* Section 1.  frame_cap >= 1 and run_cap >= 1 (AVSR_E_ARG otherwise), both below 2^31. */
int avsr_summary_index(const uint8_t* d_mask, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets, int nvideos,
                       const int32_t* d_tiles, int64_t ntiles, int64_t* d_work, int64_t* d_frame_index, int64_t frame_cap,
                       int64_t* d_frame_offsets, int64_t* d_runs, int64_t run_cap, int64_t* d_run_offsets,
                       int64_t* d_totals, avsr_stream_t stream);

/* Section 2.  d_bgr uint8 [n, h, w, 3] (h, w those of h_surface, the DESTINATION's description over d_dst; its n is the
 * frames d_dst holds).  Destination frame i < count is BGR frame d_index[i] converted (frame i when d_index is NULL, and
 * then count <= n).  An index outside [0, n) is skipped: its destination frame is left as it was.  count at most the
 * destination's frames. */
int avsr_bgr_to_yuv_u8(const uint8_t* d_bgr, int64_t n, uint8_t* d_dst, const int64_t* h_surface, const int* h_forward,
                       const int64_t* d_index, int64_t count, avsr_stream_t stream);

/* Section 2.  Destination frame i < count is source frame d_index[i] (frame i when d_index is NULL, and then count <=
 * the source's frames), sample for sample.  An index outside the source's frames is skipped. */
int avsr_repack_u8(const uint8_t* d_src, const int64_t* h_src_surface, uint8_t* d_dst, const int64_t* h_dst_surface,
                   const int64_t* d_index, int64_t count, avsr_stream_t stream);

/* Section 3.  sr > 0, every fps finite and > 0 is the caller's to see to (d_fps is device memory); fade >= 0,
 * run_cap >= 1 and sample_cap >= 1 (AVSR_E_ARG otherwise). */
int avsr_audio_cut(const float* d_wave, const int64_t* h_wave_offsets, const int64_t* d_wave_offsets, int nvideos,
                   const double* d_fps, double sr, int64_t fade, const int64_t* d_runs, int64_t run_cap,
                   const int64_t* d_run_offsets, int64_t* d_work, float* d_audio, int64_t sample_cap,
                   int64_t* d_audio_offsets, int64_t* d_totals, avsr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_RENDER_H */
