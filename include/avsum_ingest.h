/*
 * avsum_ingest.h — C-ABI of libavsum_ingest.so: NV12 frames (what hardware decoders and ffmpeg deliver) read where
 * they lie on the MI355X (gfx950).  A third, self-contained library beside libavsum_hip.so and libavsum_optim.so: it
 * shares no symbol and no state with either.
 *
 *   avsi_nv12_to_bgr_u8            dense BGR of (gathered) frames: the compatibility path and the definition the two
 *                                  fused entry points are held to
 *   avsi_nv12_resize_gather2_u8    avs_resize_bilinear_gather2_u8 of the converted frames, one launch, no BGR copy
 *   avsi_nv12_hsv_diff_batch_u8    avs_hsv_frame_diff_batch_u8 of the converted frames, one launch, no BGR copy
 *
 * Conventions (all entry points), those of avsum_hip.h:
 *   - `extern "C"`, plain pointers and sizes; returns int status: AVSI_OK (0) or a negative AVSI_E_* code; never
 *     throws.  avsi_last_error() returns a thread-local message for the last failure.
 *   - every argument is validated before any HIP call.
 *   - every pointer named d_* is DEVICE memory owned by the caller, h_* is HOST memory read before the call returns;
 *     nothing is allocated or freed.
 *   - asynchronous on the caller's `stream` (a hipStream_t cast to void*; NULL = the null stream); no host
 *     synchronisation inside.
 *
 * A batch of NV12 frames is (d_src, n, h, w, pitch, frame_stride, uv_offset), all offsets in bytes, any base alignment:
 *   h, w            even, at least 2
 *   pitch           >= w: the bytes from one row to the next, of the luma plane and of the chroma plane
 *   uv_offset       >= h * pitch: where the chroma plane of a frame begins
 *   frame_stride    >= uv_offset + (h / 2 - 1) * pitch + w: the bytes from one frame to the next
 * With f the first byte of a frame, pixel (y, x) has
 *   Y = f[y * pitch + x],  U = f[uv_offset + (y >> 1) * pitch + (x & ~1)],  V = the byte after U
 * (the nearest chroma sample, no interpolation).  Bytes of a row past w and rows between the planes are never read.
 *
 * The conversion is h_matrix = (y_off, cy, cub, cug, cvg, cvr), six ints, 0 <= y_off <= 255, every |coefficient| at
 * most AVSI_MAX_COEF = 2^22, in AVSI_SHIFT = 20 fractional bits, all of it in 32-bit integers:
 *   yy = max(Y - y_off, 0) * cy + 2^19;   uu = U - 128;   vv = V - 128
 *   B = clamp((yy + cub * uu) >> 20)
 *   G = clamp((yy + cvg * vv + cug * uu) >> 20)
 *   R = clamp((yy + cvr * vv) >> 20)
 * with >> the arithmetic shift (floor) and clamp to 0 .. 255.  No accumulator leaves int32 under these limits: the
 * largest is 255 * 2^22 + 2^19 + 2 * 128 * 2^22 = 511 * 2^22 + 2^19 < 2^31, and 2^22 is the largest power of two for
 * which that holds (the blue coefficients of BT.601 and BT.709, 2.018 and 2.112, lie above 2^21).
 * (16, 1220542, 2116026, -409993, -852492, 1673527) are OpenCV's COLOR_YUV2BGR_NV12 constants [recalled from memory:
 * the cv2 sources are absent here, so byte parity with cv2 is NOT pinned].
 */
#ifndef AVSUM_INGEST_H
#define AVSUM_INGEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSI_ABI_VERSION 1

#define AVSI_SHIFT 20              /* fractional bits of the matrix                                              */
#define AVSI_MAX_COEF 4194304      /* 2^22: the largest |coefficient|                                            */
#define AVSI_MATRIX_INTS 6         /* ints of h_matrix                                                           */
#define AVSI_MAX_DIFF_FRAMES 16777216 /* 2^24: frames of one avsi_nv12_hsv_diff_batch_u8 call at most             */
#define AVSI_RESIZE_BAND 8         /* output rows of one workgroup of the resize, halved until its rows fit LDS  */
#define AVSI_RESIZE_LDS_BYTES 65536 /* the dynamic LDS one workgroup of the resize may ask for                    */

enum {
  AVSI_OK = 0,
  AVSI_E_ARG = -1,         /* null pointer / coefficient or count out of range   */
  AVSI_E_SHAPE = -2,       /* sizes inconsistent with what the kernel assumes    */
  AVSI_E_HIP = -4,         /* the HIP runtime reported an error at launch        */
  AVSI_E_UNSUPPORTED = -6  /* this entry point does not take the shape           */
};

typedef void* avsi_stream_t;

int avsi_abi_version(void);
const char* avsi_last_error(void);

/* d_bgr uint8 [count, h, w, 3]: row i is frame d_index[i] converted (frame i when d_index is NULL, and then
 * count <= n).  An index outside [0, n) is skipped: its destination is left as it was.  count < 2^31. */
int avsi_nv12_to_bgr_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                        int64_t uv_offset, const int* h_matrix, const int64_t* d_index, int64_t count,
                        uint8_t* d_bgr, avsi_stream_t stream);

/* cv2.resize(..., INTER_LINEAR) of the converted frames d_index[0 .. count) to dh0 x dw0 (d_dst0 uint8
 * [count, dh0, dw0, 3]) and, where d_dst1 is not NULL, to dh1 x dw1 as well, in one launch: the bytes of
 * avs_resize_bilinear_gather2_u8 on avsi_nv12_to_bgr_u8's output.  A workgroup stages the luma rows y_lo .. y_hi and
 * the chroma rows y_lo >> 1 .. y_hi >> 1 its band of output rows reads (1.5 bytes per pixel) into LDS, converts per
 * tap, and leaves through an LDS image of its output rows.  An index outside [0, n) is skipped.  AVSI_E_UNSUPPORTED:
 * w or an output height above 65535, or the rows of one output row do not fit AVSI_RESIZE_LDS_BYTES. */
int avsi_nv12_resize_gather2_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                                int64_t uv_offset, const int* h_matrix, const int64_t* d_index, int64_t count,
                                uint8_t* d_dst0, int dh0, int dw0, uint8_t* d_dst1, int dh1, int dw1,
                                avsi_stream_t stream);

/* The band (output rows per workgroup: AVSI_RESIZE_BAND, 4, 2 or 1) avsi_nv12_resize_gather2_u8 takes for a
 * destination of dh x dw from frames of h x w; 0 when it refuses the shape; AVSI_E_SHAPE for extents it rejects.
 * Host only. */
int avsi_nv12_resize_band(int h, int w, int dh, int dw);

/* d_sums uint32 [n, 3]: the sums of |dH|, |dS|, |dV| (OpenCV's 8-bit HSV of the converted pixels) of every frame
 * against the previous frame of its video over the pixels range(0, h, step) x range(0, w, step); zeros at every
 * video's first frame.  The integers of avs_hsv_frame_diff_batch_u8 on avsi_nv12_to_bgr_u8's output.  d_offsets int64
 * [nvideos + 1], starts at 0, increases strictly, ends at n.  n <= AVSI_MAX_DIFF_FRAMES; the strided pixels of a frame
 * times 255 must fit uint32. */
int avsi_nv12_hsv_diff_batch_u8(const uint8_t* d_src, int64_t n, int h, int w, int pitch, int64_t frame_stride,
                                int64_t uv_offset, const int* h_matrix, int step, const int64_t* d_offsets,
                                int nvideos, uint32_t* d_sums, avsi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AVSUM_INGEST_H */
