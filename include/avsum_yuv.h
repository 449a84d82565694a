/*
 * avsum_yuv.h — C-ABI of libavsum_yuv.so: planar, semi-planar and 10-bit YUV 4:2:0 frames (I420 / YV12, NV12 / NV21,
 * P010, yuv420p10le) read where they lie on the MI355X (gfx950).  A seventh, self-contained library: it shares no
 * symbol and no state with the other six, libavsum_ingest.so (NV12 only, unchanged) included.
 *
 *   avsy_to_bgr_u8             dense BGR of (gathered) frames: the definition the two fused entry points are held to
 *   avsy_resize_gather2_u8     avs_resize_bilinear_gather2_u8 of the converted frames, one launch, no BGR copy
 *   avsy_hsv_diff_batch_u8     avs_hsv_frame_diff_batch_u8 of the converted frames, one launch, no BGR copy
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSY_OK (0) or a negative AVSY_E_* code; never
 *     throws.  avsy_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller, h_* is HOST memory read before the call returns;
 *     nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside.
 *
 * ONE surface description for every 4:2:0 layout: d_src and h_surface, a host int64_t[AVSY_SURFACE_INTS] holding, in
 * this order (the AVSY_S_* indices),
 *   n, h, w          frames; h and w even, at least 2
 *   sample_bytes     1 or 2
 *   shift            0 or 6; 0 when sample_bytes is 1
 *   pitch_y, pitch_c the bytes from one luma row to the next, from one chroma row to the next
 *   chroma_step      the bytes from one U sample to the next U sample of a chroma row (and from V to V)
 *   u_offset, v_offset   where the first U and the first V sample of a frame lie
 *   frame_stride     the bytes from one frame to the next
 * all offsets in bytes from the first byte f of a frame.  A one-byte sample S(a) is the byte at a: depth d = 8.  A
 * two-byte sample is S(a) = (w16 >> shift) & 1023 with w16 the little-endian 16-bit word at a: depth d = 10; whatever
 * the other six bits of the word hold is ignored.  Pixel (y, x) has, with the nearest chroma sample and no
 * interpolation (the definition of avsum_ingest.h kept),
 *   Y = S(f + y * pitch_y + x * sample_bytes)
 *   U = S(f + u_offset + (y >> 1) * pitch_c + (x >> 1) * chroma_step)
 *   V = S(f + v_offset + (y >> 1) * pitch_c + (x >> 1) * chroma_step)
 * The layouts are settings of these fields:
 *   layout          sample_bytes  chroma_step  v_offset                                shift
 *   NV12            1             2            u_offset + 1                            0
 *   NV21            1             2            u_offset - 1                            0
 *   I420 / YV12     1             1            its own plane (YV12: the two exchanged) 0
 *   P010            2             4            u_offset + 2                            6
 *   planar 10-bit   2             2            its own plane                           0
 * Refused (AVSY_E_SHAPE) before any HIP call: extents that are odd or below 2; a sample_bytes, shift or step outside
 * the above; a pitch shorter than its row of samples; a plane whose last sample ends past frame_stride; Y, U and V
 * sample sets of a frame that share a byte; and, for two-byte samples, an odd d_src, offset, pitch, chroma_step or
 * frame_stride.  For one-byte samples any base alignment is accepted.  Bytes that belong to no sample (pitch padding,
 * gaps between planes, spare rows) never enter a result.
 *
 * The conversion is h_matrix = (y_off, cy, cub, cug, cvg, cvr), the six ints of avsum_ingest.h under the same limits:
 * 0 <= y_off <= 255, every |coefficient| at most AVSY_MAX_COEF = 2^22, in AVSY_SHIFT = 20 fractional bits.  With
 * k = d - 8:
 *   yy = max(Y - (y_off << k), 0) * cy + 2^(19 + k);   uu = U - (128 << k);   vv = V - (128 << k)
 *   B = clamp((yy + cub * uu) >> (20 + k))
 *   G = clamp((yy + cvg * vv + cug * uu) >> (20 + k))
 *   R = clamp((yy + cvr * vv) >> (20 + k))
 * with >> the arithmetic shift (floor) and clamp to 0 .. 255.  For d = 8 this is avsum_ingest.h's definition, integer
 * for integer, and no sum leaves int32.  For d = 10 the sums do leave int32 even for the two named matrices
 * (Y = U = 1023 under "bt709": 1023 * 1220542 + 2214593 * 511 is about 2.38e9), so the definition is stated in 64-bit
 * integers; a kernel may compute it any way that yields these integers.  Two consequences: a 10-bit surface whose every
 * sample is 4 * s converts to the bytes the 8-bit definition gives for s, and any surface that holds the samples of an
 * NV12 surface converts to the bytes of avsi_nv12_to_bgr_u8.
 *
 * The output stays uint8 BGR because every consumer (the resize, the shot scan, the trunks' normalisation) takes
 * bytes.  The two extra bits of a 10-bit sample are not dropped beforehand: they enter the matrix and the ONE rounding
 * to a grey level, where truncating to 8 bits first would round twice.
 */
#ifndef AVSUM_YUV_H
#define AVSUM_YUV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSY_ABI_VERSION 1

#define AVSY_SHIFT 20              /* fractional bits of the matrix (at depth 8; 20 + k at depth 8 + k)           */
#define AVSY_MAX_COEF 4194304      /* 2^22: the largest |coefficient|                                            */
#define AVSY_MATRIX_INTS 6         /* ints of h_matrix                                                           */
#define AVSY_SURFACE_INTS 11       /* int64s of h_surface                                                        */
#define AVSY_MAX_DIFF_FRAMES 16777216 /* 2^24: frames of one avsy_hsv_diff_batch_u8 call at most                  */
#define AVSY_RESIZE_BAND 8         /* output rows of one workgroup of the resize, halved until its rows fit LDS  */
#define AVSY_RESIZE_LDS_BYTES 65536 /* the dynamic LDS one workgroup of the resize may ask for                    */

enum {                             /* the order of h_surface */
  AVSY_S_N = 0,
  AVSY_S_H = 1,
  AVSY_S_W = 2,
  AVSY_S_SAMPLE_BYTES = 3,
  AVSY_S_SHIFT = 4,
  AVSY_S_PITCH_Y = 5,
  AVSY_S_PITCH_C = 6,
  AVSY_S_CHROMA_STEP = 7,
  AVSY_S_U_OFFSET = 8,
  AVSY_S_V_OFFSET = 9,
  AVSY_S_FRAME_STRIDE = 10
};

enum {
  AVSY_OK = 0,
  AVSY_E_ARG = -1,         /* null pointer / coefficient or count out of range   */
  AVSY_E_SHAPE = -2,       /* sizes inconsistent with what the kernel assumes    */
  AVSY_E_HIP = -4,         /* the HIP runtime reported an error at launch        */
  AVSY_E_UNSUPPORTED = -6  /* this entry point does not take the shape           */
};

typedef void* avsy_stream_t;

int avsy_abi_version(void);
const char* avsy_last_error(void);

/* d_bgr uint8 [count, h, w, 3]: row i is frame d_index[i] converted (frame i when d_index is NULL, and then
 * count <= n).  An index outside [0, n) is skipped: its destination is left as it was.  count < 2^31. */
int avsy_to_bgr_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix, const int64_t* d_index,
                   int64_t count, uint8_t* d_bgr, avsy_stream_t stream);

/* cv2.resize(..., INTER_LINEAR) of the converted frames d_index[0 .. count) to dh0 x dw0 (d_dst0 uint8
 * [count, dh0, dw0, 3]) and, where d_dst1 is not NULL, to dh1 x dw1 as well, in one launch: the bytes of
 * avs_resize_bilinear_gather2_u8 on avsy_to_bgr_u8's output.  A workgroup stages the luma rows y_lo .. y_hi and the
 * chroma rows y_lo >> 1 .. y_hi >> 1 (one row of U, V pairs where the chroma is interleaved, a U row and a V row where
 * it is planar) its band of output rows reads into LDS, converts per tap, and leaves through an LDS image of its
 * output rows.  A two-byte row takes twice the LDS.  An index outside [0, n) is skipped.  AVSY_E_UNSUPPORTED: w or an
 * output height above 65535, or the rows of one output row do not fit AVSY_RESIZE_LDS_BYTES. */
int avsy_resize_gather2_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix, const int64_t* d_index,
                           int64_t count, uint8_t* d_dst0, int dh0, int dw0, uint8_t* d_dst1, int dh1, int dw1,
                           avsy_stream_t stream);

/* The band (output rows per workgroup: AVSY_RESIZE_BAND, 4, 2 or 1) avsy_resize_gather2_u8 takes for a destination of
 * dh x dw from frames of h_surface; 0 when it refuses the shape; AVSY_E_SHAPE for a description or extents it rejects.
 * Host only. */
int avsy_resize_band(const int64_t* h_surface, int dh, int dw);

/* d_sums uint32 [n, 3]: the sums of |dH|, |dS|, |dV| (OpenCV's 8-bit HSV of the converted pixels) of every frame
 * against the previous frame of its video over the pixels range(0, h, step) x range(0, w, step); zeros at every
 * video's first frame.  The integers of avs_hsv_frame_diff_batch_u8 on avsy_to_bgr_u8's output.  d_offsets int64
 * [nvideos + 1], starts at 0, increases strictly, ends at n.  n <= AVSY_MAX_DIFF_FRAMES; the strided pixels of a frame
 * times 255 must fit uint32. */
int avsy_hsv_diff_batch_u8(const uint8_t* d_src, const int64_t* h_surface, const int* h_matrix, int step,
                           const int64_t* d_offsets, int nvideos, uint32_t* d_sums, avsy_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_YUV_H */
