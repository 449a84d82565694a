"""NV12 frames read where they lie: the launch wrappers of libavsum_ingest.so (include/avsum_ingest.h) and the numpy
restatements of its pixel definition.

A hardware decoder (or ffmpeg without swscale) delivers NV12: a pitched luma plane, then an interleaved half-resolution
chroma plane, 1.5 bytes per pixel.  ``Nv12Frames`` describes a batch of such surfaces in ONE device tensor; the three
wrappers convert it (``nv12_to_bgr``, the compatibility path and the definition), resize sampled frames of it
(``nv12_resize_gather``, the bytes of ops.resize_gather on the converted frames) and scan it for shot boundaries
(``nv12_hsv_frame_diff_batch``, the integers of ops.hsv_frame_diff_batch on the converted frames) without a dense BGR
copy.  Host tensors are refused: there is no CPU fallback.  ``nv12_to_bgr_host`` / ``nv12_to_bgr_f64`` are the integer
definition and the float formula it approximates, in numpy, for tests and studies.
"""
import ctypes

import numpy as np
import torch

from ._ingest_abi import MAX_COEF, MATRIX_INTS, SHIFT, check, lib
from .ops import ShotTables, _device_arg, _p, _stream, _tables_arg

__all__ = ["Nv12Frames", "MATRICES", "MATRICES_F64", "nv12_to_bgr", "nv12_resize_gather", "nv12_hsv_frame_diff_batch",
           "nv12_to_bgr_host", "nv12_to_bgr_f64", "yuv_to_bgr_host", "yuv_to_bgr_f64"]

# (y_off, cy, cub, cug, cvg, cvr) in SHIFT = 20 fractional bits.  "bt601": OpenCV's COLOR_YUV2BGR_NV12 constants
# [recalled from memory: byte parity with cv2 is not pinned]; "bt709": round(c * 2^20) of the coefficients below
MATRICES = {
    "bt601": (16, 1220542, 2116026, -409993, -852492, 1673527),
    "bt709": (16, 1220542, 2214593, -223347, -558891, 1880097),
}
# the three-decimal formulas the integers stand for, same order
MATRICES_F64 = {
    "bt601": (16, 1.164, 2.018, -0.391, -0.813, 1.596),
    "bt709": (16, 1.164, 2.112, -0.213, -0.533, 1.793),
}


def _matrix(matrix, what):
    """The six integers of ``matrix``: a name of MATRICES or a sequence (y_off, cy, cub, cug, cvg, cvr)."""
    if isinstance(matrix, str):
        if matrix not in MATRICES:
            raise ValueError(f"{what}: matrix must be one of {sorted(MATRICES)} or six integers, got '{matrix}'")
        matrix = MATRICES[matrix]
    m = tuple(int(c) for c in matrix)
    if len(m) != MATRIX_INTS or not 0 <= m[0] <= 255 or any(abs(c) > MAX_COEF for c in m[1:]):
        raise ValueError(f"{what}: a matrix is (y_off in 0..255, five coefficients of magnitude <= 2^22), got {m}")
    return m


def _matrix_arg(matrix, what):
    return (ctypes.c_int * MATRIX_INTS)(*_matrix(matrix, what))


class Nv12Frames:
    """N NV12 surfaces of ``height`` x ``width`` pixels in one uint8 tensor ``data`` [N, rows, pitch]: the luma plane in
    rows 0 .. height - 1, the interleaved chroma plane (U, V, U, V, ...) in rows uv_row .. uv_row + height / 2 - 1, the
    first ``width`` bytes of each row; what lies beyond (the pitch padding, rows between and after the planes) is never
    read.  ``uv_row`` defaults to ``height``.  height and width are even and at least 2, pitch >= width,
    uv_row >= height, rows >= uv_row + height / 2.  Only the tensor's metadata is looked at here, so a description can be
    validated for a host or meta tensor; the launch wrappers insist on a device tensor."""

    def __init__(self, data, height, width, uv_row=None):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 3:
            raise ValueError("Nv12Frames: data must be a uint8 tensor [N, rows, pitch]")
        if not data.is_contiguous():
            raise ValueError(f"Nv12Frames: data must be contiguous, got strides {list(data.stride())}")
        height, width = int(height), int(width)
        uv_row = height if uv_row is None else int(uv_row)
        n, rows, pitch = data.shape
        if height < 2 or width < 2 or height % 2 or width % 2:
            raise ValueError(f"Nv12Frames: height and width must be even and at least 2, got {height}x{width}")
        if pitch < width:
            raise ValueError(f"Nv12Frames: pitch {pitch} below the width {width}")
        if uv_row < height:
            raise ValueError(f"Nv12Frames: uv_row {uv_row} lies inside the luma plane of {height} rows")
        if rows < uv_row + height // 2:
            raise ValueError(f"Nv12Frames: {rows} rows, the chroma plane ends at row {uv_row + height // 2}")
        self.data, self.height, self.width, self.uv_row = data, height, width, uv_row
        self.frames, self.rows, self.pitch = int(n), int(rows), int(pitch)
        self.frame_stride = self.rows * self.pitch
        self.uv_offset = self.uv_row * self.pitch

    @property
    def device(self):
        return self.data.device

    @property
    def nbytes(self):
        return self.frames * self.frame_stride

    @property
    def shape(self):
        """The shape of the BGR tensor these frames stand for."""
        return (self.frames, self.height, self.width, 3)

    def pinned_like(self):
        """An uninitialised pinned host tensor of data's shape: fill it with decoded surfaces, then
        ``ops.pull_copy(pinned, frames.data)`` uploads them - 1.5 bytes per pixel over PCIe instead of 3."""
        return torch.empty(self.data.shape, dtype=torch.uint8, pin_memory=True)

    def _args(self):
        return (_p(self.data), self.frames, self.height, self.width, self.pitch, self.frame_stride, self.uv_offset)


def _frames_arg(frames, what, device=None):
    if not isinstance(frames, Nv12Frames):
        raise ValueError(f"{what}: frames must be an Nv12Frames")
    _device_arg(frames.data, "frames.data", what, (torch.uint8,), ndim=3, device=device)
    return frames


# --------------------------------------------------------------------------- launch wrappers
def nv12_to_bgr(frames, index=None, count=None, matrix="bt601", out=None):
    """uint8 [count, h, w, 3] BGR: row i is frame index[i] of ``frames`` converted (frame i without an index; count
    defaults to every entry of the index, or every frame).  ``index`` int64 device vector of at least ``count`` entries;
    ``count`` a host integer; ``out`` [at least count, h, w, 3] (allocated when None): its rows from ``count`` on and the
    row of an index outside the frames are left as they were.  The integer definition of include/avsum_ingest.h =
    nv12_to_bgr_host."""
    _frames_arg(frames, "nv12_to_bgr")
    dev = frames.device
    if index is not None:
        _device_arg(index, "index", "nv12_to_bgr", (torch.int64,), ndim=1, device=dev)
    limit = frames.frames if index is None else index.numel()
    count = limit if count is None else int(count)
    if not 0 <= count <= limit:
        raise ValueError(f"nv12_to_bgr: count {count} outside 0 .. {limit}")
    if out is None:
        out = torch.empty((count, frames.height, frames.width, 3), dtype=torch.uint8, device=dev)
    else:
        _device_arg(out, "out", "nv12_to_bgr", (torch.uint8,), shape=(None, frames.height, frames.width, 3), device=dev)
        if out.shape[0] < count:
            raise ValueError(f"nv12_to_bgr: out holds {out.shape[0]} frames, count is {count}")
    check(lib().avsi_nv12_to_bgr_u8(*frames._args(), _matrix_arg(matrix, "nv12_to_bgr"), _p(index), count, _p(out),
                                    _stream()), "avsi_nv12_to_bgr_u8")
    return out


def nv12_resize_gather(frames, index, count, sizes, matrix="bt601", outs=None):
    """ops.resize_gather(nv12_to_bgr(frames), index, count, sizes) byte for byte, in ONE launch and without the BGR
    frames: a workgroup stages the luma and chroma rows its output rows read and converts per tap.  ``sizes``: one or
    two (dh, dw).  Returns a list of uint8 [count, dh, dw, 3] tensors, ``outs`` where given."""
    _frames_arg(frames, "nv12_resize_gather")
    dev = frames.device
    _device_arg(index, "index", "nv12_resize_gather", (torch.int64,), ndim=1, device=dev)
    count = int(count)
    if not 0 <= count <= index.numel():
        raise ValueError(f"nv12_resize_gather: count {count} outside 0 .. {index.numel()}, the entries of index")
    sizes = [(int(dh), int(dw)) for dh, dw in sizes]
    if len(sizes) not in (1, 2) or any(dh < 1 or dw < 1 for dh, dw in sizes):
        raise ValueError(f"nv12_resize_gather: sizes must be one or two (dh, dw) of positive extents, got {sizes}")
    if outs is None:
        outs = [torch.empty((count, dh, dw, 3), dtype=torch.uint8, device=dev) for dh, dw in sizes]
    elif len(outs) != len(sizes):
        raise ValueError(f"nv12_resize_gather: {len(outs)} outs for {len(sizes)} sizes")
    for k, ((dh, dw), out) in enumerate(zip(sizes, outs)):
        _device_arg(out, f"outs[{k}]", "nv12_resize_gather", (torch.uint8,), shape=(count, dh, dw, 3), device=dev)
    (dh0, dw0), (dh1, dw1) = sizes[0], sizes[1] if len(sizes) == 2 else (0, 0)
    check(lib().avsi_nv12_resize_gather2_u8(*frames._args(), _matrix_arg(matrix, "nv12_resize_gather"), _p(index), count,
                                            _p(outs[0]), dh0, dw0, _p(outs[1]) if len(sizes) == 2 else None, dh1, dw1,
                                            _stream()), "avsi_nv12_resize_gather2_u8")
    return list(outs)


def nv12_hsv_frame_diff_batch(frames, tables, step=1, raw=False, matrix="bt601"):
    """ops.hsv_frame_diff_batch(nv12_to_bgr(frames), tables, step, raw) integer for integer, without the BGR frames:
    ``frames`` the videos of ``tables`` (an ops.ShotTables) concatenated."""
    _tables_arg(tables, ShotTables, "nv12_hsv_frame_diff_batch")
    _frames_arg(frames, "nv12_hsv_frame_diff_batch", tables.device)
    if frames.frames != tables.frames:
        raise ValueError(f"nv12_hsv_frame_diff_batch: {frames.frames} frames, the tables hold {tables.frames}")
    if int(step) < 1:
        raise ValueError(f"nv12_hsv_frame_diff_batch: step must be >= 1, got {step}")
    sums = torch.empty((frames.frames, 3), dtype=torch.int32, device=frames.device)
    check(lib().avsi_nv12_hsv_diff_batch_u8(*frames._args(), _matrix_arg(matrix, "nv12_hsv_frame_diff_batch"), int(step),
                                            _p(tables.offsets_t), tables.nvideos, _p(sums), _stream()),
          "avsi_nv12_hsv_diff_batch_u8")
    return sums if raw else sums.to(torch.int64) & 0xFFFFFFFF


# --------------------------------------------------------------------------- the definition, in numpy
def yuv_to_bgr_host(y, u, v, matrix="bt601"):
    """uint8 [..., 3] BGR of integer arrays Y, U, V (0 .. 255, one shape): the definition of include/avsum_ingest.h in
    32-bit integers (numpy's >> on int32 is the arithmetic shift)."""
    y_off, cy, cub, cug, cvg, cvr = (np.int32(c) for c in _matrix(matrix, "yuv_to_bgr_host"))
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    yy = np.maximum(y - y_off, 0) * cy + np.int32(1 << (SHIFT - 1))
    uu, vv = u - np.int32(128), v - np.int32(128)
    bgr = np.stack([(yy + cub * uu) >> SHIFT, (yy + cvg * vv + cug * uu) >> SHIFT, (yy + cvr * vv) >> SHIFT], axis=-1)
    assert bgr.dtype == np.int32
    return np.clip(bgr, 0, 255).astype(np.uint8)


def yuv_to_bgr_f64(y, u, v, matrix="bt601"):
    """float64 [..., 3] BGR by the three-decimal formula of MATRICES_F64[matrix] (or six numbers), clipped to 0 .. 255,
    not rounded: what the integers approximate to within 0.5 + 493 * 2^-21."""
    y_off, cy, cub, cug, cvg, cvr = MATRICES_F64[matrix] if isinstance(matrix, str) else matrix
    y, u, v = (np.asarray(a, dtype=np.float64) for a in (y, u, v))
    yy, uu, vv = np.maximum(y - y_off, 0.0) * cy, u - 128.0, v - 128.0
    return np.clip(np.stack([yy + cub * uu, yy + cvg * vv + cug * uu, yy + cvr * vv], axis=-1), 0.0, 255.0)


def _planes(data, height, width, uv_row):
    """(Y, U, V), each [N, height, width], of a numpy uint8 [N, rows, pitch]: the nearest chroma sample per pixel."""
    data = np.asarray(data)
    uv_row = height if uv_row is None else uv_row
    rows, cols = np.arange(height), np.arange(width)
    y = data[:, :height, :width]
    c_rows = (uv_row + (rows >> 1))[:, None]
    return y, data[:, c_rows, (cols & ~1)[None, :]], data[:, c_rows, (cols & ~1)[None, :] + 1]


def nv12_to_bgr_host(data, height, width, uv_row=None, matrix="bt601"):
    """uint8 [N, height, width, 3]: nv12_to_bgr of a numpy uint8 [N, rows, pitch], by the integer definition."""
    return yuv_to_bgr_host(*_planes(data, height, width, uv_row), matrix)


def nv12_to_bgr_f64(data, height, width, uv_row=None, matrix="bt601"):
    """float64 [N, height, width, 3]: the float formula on the same pixels."""
    return yuv_to_bgr_f64(*_planes(data, height, width, uv_row), matrix)
