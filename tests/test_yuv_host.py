"""CPU-side checks of the YUV 4:2:0 ingest path (libavsum_yuv.so, avsum_amd/yuv.py): the seventh header and the binding
derived from it, the library's exports, every refusal of the surface description before any launch, the two host
definitions against each other on every layout, the planted mistakes at the committed cases, the depth-10 integers
against the depth-8 ones and against the float formula, the resize plan against its restatement, and YuvFrames'
refusals on metadata alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nv12_inputs as ni
import pixel_f64_inputs as pfi
import yuv_inputs as yi
from avsum_amd import _header, _ingest_abi, _yuv_abi, ingest, yuv

PKG = os.path.dirname(os.path.dirname(_yuv_abi.LIB_PATH))

_FRAMES = ["uint8_t*", "int64_t*", "int*"]                                   # d_src, h_surface, h_matrix
PINNED = {
    "avsy_abi_version": ("int", []),
    "avsy_last_error": ("char*", []),
    "avsy_to_bgr_u8": ("int", _FRAMES + ["int64_t*", "int64_t", "uint8_t*", "avsy_stream_t"]),
    "avsy_resize_gather2_u8": ("int", _FRAMES + ["int64_t*", "int64_t", "uint8_t*", "int", "int", "uint8_t*", "int", "int",
                                                 "avsy_stream_t"]),
    "avsy_resize_band": ("int", ["int64_t*", "int", "int"]),
    "avsy_hsv_diff_batch_u8": ("int", _FRAMES + ["int", "int64_t*", "int", "uint32_t*", "avsy_stream_t"]),
}
SURFACE_ORDER = ("n", "h", "w", "sample_bytes", "shift", "pitch_y", "pitch_c", "chroma_step", "u_offset", "v_offset",
                 "frame_stride")
E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -6
OTHER_PREFIXES = r"avs[aiodl]?_"                 # the six other libraries' symbols


def _frames(L, data=None):
    """yuv.YuvFrames of a Layout over a meta tensor (or over ``data``)."""
    if data is None:
        data = torch.empty((L.n, L.frame_stride), dtype=torch.uint8, device="meta")
    return yuv.YuvFrames(data, L.h, L.w, **yi.fields(L))


# --------------------------------------------------------------------------- header, binding, library
def test_yuv_header_parses_and_signatures_are_pinned():
    header = _yuv_abi.load_header()
    assert header.prototypes == PINNED
    assert _yuv_abi.declared_symbols() == sorted(PINNED)
    c = header.constants
    assert (c["AVSY_ABI_VERSION"], c["AVSY_SHIFT"], c["AVSY_MAX_COEF"], c["AVSY_MATRIX_INTS"]) == (1, 20, 1 << 22, 6)
    assert (c["AVSY_SURFACE_INTS"], c["AVSY_MAX_DIFF_FRAMES"], c["AVSY_RESIZE_BAND"], c["AVSY_RESIZE_LDS_BYTES"]) == (
        11, 1 << 24, yi.RESIZE_BAND, yi.RESIZE_LDS_BYTES)
    assert (c["AVSY_OK"], c["AVSY_E_ARG"], c["AVSY_E_SHAPE"], c["AVSY_E_HIP"], c["AVSY_E_UNSUPPORTED"]) == (0, -1, -2, -4, -6)
    assert [c["AVSY_S_" + f.upper()] for f in SURFACE_ORDER] == list(range(11))      # the order of section 1
    assert _yuv_abi.SURFACE_FIELDS == SURFACE_ORDER
    # the limits of the matrix are those of the NV12 header
    i = _ingest_abi.load_header().constants
    assert (c["AVSY_SHIFT"], c["AVSY_MAX_COEF"], c["AVSY_MATRIX_INTS"]) == (i["AVSI_SHIFT"], i["AVSI_MAX_COEF"], i["AVSI_MATRIX_INTS"])
    sig = header.signatures()
    assert sig["avsy_last_error"] == (ctypes.c_char_p, [])
    assert sig["avsy_to_bgr_u8"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
    # no name of another header is defined again
    main = _header.load()
    assert not [n for n in list(main.prototypes) + list(main.constants) if n.lower().startswith("avsy_")]
    assert not set(c) & (set(main.constants) | set(i))
    for path in (_yuv_abi.HEADER_PATH, os.path.join(PKG, "csrc", "yuv.hip")):
        assert not re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AVS_\w+|AVSI_\w+)", open(path).read(), flags=re.M), path
    # the header's comment is the definition, and says why the output is bytes
    text = open(_yuv_abi.HEADER_PATH).read()
    for phrase in ("(w16 >> shift) & 1023", "2^(19 + k)", ">> (20 + k)", "64-bit", "ONE rounding"):
        assert phrase in text, phrase


def test_yuv_library_exports_exactly_the_headers_functions():
    lib = _yuv_abi.lib()
    assert lib.avsy_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _yuv_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(avsy_[a-z0-9_]+)\b", out)) == set(PINNED)
    assert not re.findall(rf"\b({OTHER_PREFIXES}[a-z0-9_]+)\b", out)          # nothing of the six others is defined ...
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _yuv_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined
    assert not re.findall(r"\b(avs[a-z]?_[a-z0-9_]+)\b", undefined)           # ... and nothing of them is wanted
    for name, (res, args) in _yuv_abi._SIGNATURES.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name
    # the NV12 library is as it was: its symbols do not mention this one
    out = subprocess.run(["nm", "-D", _ingest_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert not re.findall(r"\bavsy_", out)


def test_yuv_source_is_outside_srcs_and_built_with_the_same_flags():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "yuv.hip" not in srcs and "ingest.hip" not in srcs and len(srcs) == 21
    assert re.search(r"^all: \$\(YUV_LIB\)$", make, flags=re.M)
    rule = re.search(r"^\.\./build/yuv\.o:.*\n(?:\t.*\n)*", make, flags=re.M).group(0)
    assert "$(HIPCC) $(CXXFLAGS) -c" in rule and "pixel_bodies.h" in rule and "avsum_yuv.h" in rule
    assert "$(YUV_LIB)" in re.search(r"^clean:\n\t(.*)$", make, flags=re.M).group(1)
    text = open(os.path.join(PKG, "csrc", "yuv.hip")).read()
    assert re.search(r"^static thread_local char g_err\[", text, flags=re.M)
    assert not re.search(r"\bavs_set_error\b|\bAVS_REQUIRE\b|\bAVS_CHECK_LAUNCH\b|\bavsi_\w+\(|\bAVSI_REQUIRE\b", text)
    assert '#include "avs_internal.h"' in text and '#include "pixel_bodies.h"' in text
    assert "hsv_diff_body<" in text and "stage_out<" in text and "cv_blend(" in text
    # the HSV pixel arithmetic keeps its single definition
    sources = [open(os.path.join(PKG, "csrc", f)).read() for f in sorted(os.listdir(os.path.join(PKG, "csrc")))]
    assert sum(len(re.findall(r"void bgr2hsv_u8\(", s)) for s in sources) == 1
    # compiled per (sample_bytes, planar or interleaved chroma)
    for kernel in ("yuv_to_bgr_kernel", "yuv_resize_gather2_kernel", "yuv_hsv_diff_batch_kernel"):
        assert re.search(rf"template <int SB, bool PLANAR>\n__global__ [^\n]*{kernel}\(", text), kernel
    ignored = subprocess.run(["git", "-C", os.path.dirname(PKG), "check-ignore", "-q", _yuv_abi.LIB_PATH], capture_output=True)
    assert ignored.returncode in (0, 128)                            # ignored (128: not a git work tree)


# --------------------------------------------------------------------------- validation before any launch
def _surface(**changes):
    """h_surface of 2 I420 frames of 4 x 6 with pitches 8 and 4, one spare row after every plane; ``changes`` by field."""
    base = dict(n=2, h=4, w=6, sample_bytes=1, shift=0, pitch_y=8, pitch_c=4, chroma_step=1, u_offset=40, v_offset=52,
                frame_stride=64)
    base.update(changes)
    return (ctypes.c_int64 * 11)(*[base[f] for f in SURFACE_ORDER])


def _surface16(**changes):
    """h_surface of 2 P010 frames of 4 x 6: pitch 16, the pairs at 64."""
    base = dict(n=2, h=4, w=6, sample_bytes=2, shift=6, pitch_y=16, pitch_c=16, chroma_step=4, u_offset=64, v_offset=66,
                frame_stride=96)
    base.update(changes)
    return (ctypes.c_int64 * 11)(*[base[f] for f in SURFACE_ORDER])


def test_yuv_validation_before_launch_needs_no_gpu():
    """Every refusal of the surface description comes before any HIP call (no call here could launch: each has a fault the
    checks find first, and the pointers are made-up addresses)."""
    lib = _yuv_abi.lib()
    m = (ctypes.c_int * 6)(*ingest.MATRICES["bt601"])

    def calls(surface, matrix=m, src=64):
        return [("to_bgr", lambda: lib.avsy_to_bgr_u8(src, surface, matrix, None, 1, 64, None)),
                ("resize", lambda: lib.avsy_resize_gather2_u8(src, surface, matrix, 64, 1, 64, 8, 8, None, 0, 0, None)),
                ("hsv", lambda: lib.avsy_hsv_diff_batch_u8(src, surface, matrix, 1, 64, 1, 64, None))]

    def refused(surface, code, word, matrix=m, src=64):
        for name, call in calls(surface, matrix, src):
            assert call() == code, (name, list(surface), lib.avsy_last_error())
            assert word in lib.avsy_last_error(), (name, lib.avsy_last_error())
        if code == E_SHAPE and matrix is m and src == 64:
            assert lib.avsy_resize_band(surface, 8, 8) == E_SHAPE          # the host-only entry point checks the same

    # the extents
    refused(_surface(h=3), E_SHAPE, b"even")
    refused(_surface(w=5), E_SHAPE, b"even")
    refused(_surface(h=0), E_SHAPE, b"even")
    refused(_surface(n=-1), E_SHAPE, b"n=-1")
    refused(_surface(sample_bytes=3), E_SHAPE, b"sample_bytes")
    refused(_surface(sample_bytes=0), E_SHAPE, b"sample_bytes")
    refused(_surface(shift=6), E_SHAPE, b"shift")                           # a shift with one-byte samples
    refused(_surface16(shift=4), E_SHAPE, b"shift")
    refused(_surface(pitch_y=5), E_SHAPE, b"pitch_y")
    refused(_surface16(pitch_y=10), E_SHAPE, b"pitch_y")                    # six two-byte samples are 12 bytes
    refused(_surface(pitch_c=2), E_SHAPE, b"pitch_c")
    refused(_surface(chroma_step=0), E_SHAPE, b"chroma_step")
    refused(_surface16(chroma_step=1), E_SHAPE, b"chroma_step")
    refused(_surface(u_offset=-1), E_SHAPE, b"negative")
    # each plane's last sample inside frame_stride
    refused(_surface(frame_stride=58), E_SHAPE, b"frame_stride")           # V ends at 52 + 4 + 3 = 59
    refused(_surface(u_offset=58, v_offset=40), E_SHAPE, b"frame_stride")  # U ends at 65
    refused(_surface(frame_stride=29, u_offset=0, v_offset=0), E_SHAPE, b"frame_stride")     # the luma ends at 30
    # the sample sets of a frame do not overlap
    refused(_surface(v_offset=40), E_SHAPE, b"U and V")                    # one plane twice
    refused(_surface(v_offset=42), E_SHAPE, b"U and V")                    # V's first sample is U's third
    refused(_surface(v_offset=45), E_SHAPE, b"U and V")                    # ... or the second of U's second row
    refused(_surface(u_offset=29), E_SHAPE, b"luma")                       # U's first byte is the luma's last
    refused(_surface(v_offset=8), E_SHAPE, b"luma")
    refused(_surface16(v_offset=65), E_SHAPE, b"even")                     # (odd: refused for that first)
    refused(_surface16(v_offset=68), E_SHAPE, b"U and V")                  # V on the second U sample
    refused(_surface16(chroma_step=2, v_offset=66), E_SHAPE, b"U and V")   # planar step with the interleaved offset
    # two-byte samples: the base pointer, every offset, both pitches, the step and frame_stride are even
    for odd in (dict(pitch_y=17), dict(pitch_c=17), dict(u_offset=65, v_offset=67), dict(v_offset=67), dict(frame_stride=97),
                dict(chroma_step=5)):
        refused(_surface16(**odd), E_SHAPE, b"even")
    refused(_surface16(), E_SHAPE, b"even", src=65)
    # ... and what lies inside those limits passes the description: the next check (the pointers) refuses
    for ok in (_surface(), _surface(frame_stride=59), _surface(u_offset=52, v_offset=40), _surface(u_offset=30, v_offset=52),
               _surface(w=4, pitch_c=8, u_offset=6),                        # U in the luma's pitch padding: no byte shared
               _surface(chroma_step=2, pitch_c=6, v_offset=41, frame_stride=64),                  # NV12's pairs
               _surface16(), _surface16(shift=0), _surface16(chroma_step=2, pitch_c=8, v_offset=80)):
        refused(ok, E_ARG, b"null", src=None)
        assert lib.avsy_resize_band(ok, 8, 8) == 8
    refused(_surface(), E_ARG, b"null", matrix=(ctypes.c_int * 6)(*ingest.MATRICES["bt709"]), src=None)
    # the matrix
    refused(_surface(), E_ARG, b"h_matrix", matrix=None)
    for k in range(1, 6):
        for value in ((1 << 22) + 1, -(1 << 22) - 1):
            bad = list(ingest.MATRICES["bt709"])
            bad[k] = value
            refused(_surface(), E_ARG, b"2^22", matrix=(ctypes.c_int * 6)(*bad))
            refused(_surface16(), E_ARG, b"2^22", matrix=(ctypes.c_int * 6)(*bad))
    refused(_surface(), E_ARG, b"y_off", matrix=(ctypes.c_int * 6)(256, 1, 1, 1, 1, 1))
    edge = (ctypes.c_int * 6)(255, 1 << 22, -(1 << 22), 1 << 22, -(1 << 22), 1 << 22)       # the limits themselves pass
    refused(_surface16(), E_ARG, b"null", matrix=edge, src=None)
    assert lib.avsy_to_bgr_u8(64, None, m, None, 1, 64, None) == E_ARG and b"h_surface" in lib.avsy_last_error()
    # counts, sizes and the other pointers
    ok = _surface()
    assert lib.avsy_to_bgr_u8(64, ok, m, None, 1, None, None) == E_ARG
    assert lib.avsy_to_bgr_u8(64, ok, m, None, 3, 64, None) == E_SHAPE and b"no index" in lib.avsy_last_error()
    assert lib.avsy_to_bgr_u8(64, ok, m, None, -1, 64, None) == E_SHAPE
    assert lib.avsy_to_bgr_u8(64, ok, m, None, 0, None, None) == 0                        # nothing to do
    assert lib.avsy_resize_gather2_u8(64, ok, m, None, 1, 64, 8, 8, None, 0, 0, None) == E_ARG
    assert lib.avsy_resize_gather2_u8(64, ok, m, 64, 1, None, 8, 8, None, 0, 0, None) == E_ARG
    assert lib.avsy_resize_gather2_u8(64, ok, m, 64, 1, 64, 0, 8, None, 0, 0, None) == E_SHAPE
    assert lib.avsy_resize_gather2_u8(64, ok, m, 64, 1, 64, 8, 8, 64, 8, 0, None) == E_SHAPE
    assert lib.avsy_resize_gather2_u8(64, ok, m, 64, 1, 64, 65536, 8, None, 0, 0, None) == E_UNSUPPORTED
    assert lib.avsy_resize_band(ok, 0, 8) == E_SHAPE
    assert lib.avsy_hsv_diff_batch_u8(64, ok, m, 1, None, 1, 64, None) == E_ARG
    assert lib.avsy_hsv_diff_batch_u8(64, ok, m, 1, 64, 1, None, None) == E_ARG
    assert lib.avsy_hsv_diff_batch_u8(64, ok, m, 0, 64, 1, 64, None) == E_SHAPE
    assert lib.avsy_hsv_diff_batch_u8(64, ok, m, 1, 64, 0, 64, None) == E_SHAPE and b"no video" in lib.avsy_last_error()
    many = _surface(n=(1 << 24) + 1)
    assert lib.avsy_hsv_diff_batch_u8(64, many, m, 1, 64, 1, 64, None) == E_SHAPE and b"16777216" in lib.avsy_last_error()
    assert lib.avsy_hsv_diff_batch_u8(64, _surface(n=0), m, 1, None, 0, None, None) == 0
    # the shape the resize refuses: its status is the header's UNSUPPORTED, before any launch
    fmt, args, (dh, dw) = yi.REFUSED_CASE
    wide = (ctypes.c_int64 * 11)(*yi.surface_ints(yi.layout(fmt, 1, *args)))
    assert lib.avsy_resize_gather2_u8(64, wide, m, 64, 1, 64, dh, dw, None, 0, 0, None) == E_UNSUPPORTED
    assert b"LDS" in lib.avsy_last_error() and lib.avsy_resize_band(wide, dh, dw) == 0
    with pytest.raises(_yuv_abi.AvsyError, match="status -2.*pitch_y"):
        _yuv_abi.check(lib.avsy_to_bgr_u8(64, _surface(pitch_y=5), m, None, 1, 64, None), "avsy_to_bgr_u8")


# --------------------------------------------------------------------------- the definitions
@pytest.mark.parametrize("fmt", yi.FORMATS)
def test_the_two_host_definitions_agree_on_every_layout(fmt):
    for name in yi.LAYOUTS:
        data, L = yi.layout_case(fmt, name)
        frames = _frames(L)
        for matrix in sorted(ingest.MATRICES):
            want = yuv.frames_to_bgr_host(data, frames, matrix)
            assert want.shape == (yi.LAYOUT_FRAMES, L.h, L.w, 3) and want.dtype == np.uint8
            assert np.array_equal(yi.restatement(data, L, matrix), want), (fmt, name, matrix)
            err = np.abs(want - yuv.frames_to_bgr_f64(data, frames, matrix)).max()
            assert err <= (ni.BOUND if L.sample_bytes == 1 else yi.BOUND_10)
        # the sentinel bytes are exactly the bytes no sample owns, and every layout but the tight one has some
        mask = yi.sample_mask(L)
        assert (data[:, ~mask] == yi.SENTINEL_U8).all() and ((~mask).any() or name == "2x2")
        # other garbage in the six unused bits of a word: other bytes, the same samples
        if L.sample_bytes == 2:
            other, _ = yi.layout_case(fmt, name, garbage_seed=1)
            assert not np.array_equal(other, data)
            assert all(np.array_equal(a, b) for a, b in zip(yuv.yuv_samples_host(other, frames), yuv.yuv_samples_host(data, frames)))


def test_one_byte_formats_are_the_nv12_definition():
    """Any surface holding the samples of an NV12 surface converts to the bytes of ingest.nv12_to_bgr_host."""
    h, w, pitch, uv_row = ni.LAYOUTS[2]
    nv12 = ni.layout_case(ni.LAYOUTS[2])
    for matrix in sorted(ingest.MATRICES):
        want = ingest.nv12_to_bgr_host(nv12, h, w, uv_row, matrix)
        same = yuv.YuvFrames.from_nv12(ingest.Nv12Frames(torch.from_numpy(np.array(nv12)), h, w, uv_row))
        assert np.array_equal(yuv.frames_to_bgr_host(nv12, same, matrix), want)
        for fmt in ("i420", "yv12", "nv21", "p010", "i010"):
            data, L = yi.repack(fmt, nv12, h, w, uv_row, pitch_y=72, gap=2)
            assert np.array_equal(yuv.frames_to_bgr_host(data, _frames(L), matrix), want), (fmt, matrix)


def test_planted_mistakes_are_noticed_at_their_committed_case():
    assert set(yi.NOTICED_BY) == set(yi.MISTAKES) and len(yi.MISTAKES) == 11
    for mistake, (fmt, name) in yi.NOTICED_BY.items():
        assert fmt in yi.FORMATS and name in yi.LAYOUTS
        data, L = yi.layout_case(fmt, name)
        want = yuv.frames_to_bgr_host(data, _frames(L))
        wrong = yi.restatement(data, L, mistake=mistake)
        print(f"{mistake}: {int((wrong != want).sum())} of {want.size} bytes differ at {fmt} {name}")
        assert (wrong != want).any(), mistake
    # what hides a mistake: a shift of 6 leaves nothing for the mask to remove, and the 8-bit formats have neither
    data, L = yi.layout_case("p010", "36x70")
    assert np.array_equal(yi.restatement(data, L, mistake="mask_dropped"), yuv.frames_to_bgr_host(data, _frames(L)))
    data, L = yi.layout_case("i420", "36x70")
    for mistake in ("shift_dropped", "mask_dropped", "y_off_unscaled", "round_8bit", "int32_wrap"):
        assert np.array_equal(yi.restatement(data, L, mistake=mistake), yuv.frames_to_bgr_host(data, _frames(L)))


def test_ten_bit_samples_of_four_s_give_the_eight_bit_bytes_on_every_triple():
    """All 2^24 (Y, U, V): yuv_to_bgr_host of 4 * s at depth 10 == ingest.yuv_to_bgr_host of s == the depth-8 form here."""
    for matrix in sorted(ingest.MATRICES):
        for lo in range(0, 256, 32):
            y, u, v = ni.all_triples(lo, lo + 32)
            want = ingest.yuv_to_bgr_host(y, u, v, matrix)
            assert np.array_equal(yuv.yuv_to_bgr_host(4 * y, 4 * u, 4 * v, matrix, depth=10), want), (matrix, lo)
            if lo == 64:
                assert np.array_equal(yuv.yuv_to_bgr_host(y, u, v, matrix, depth=8), want)
    with pytest.raises(ValueError, match="depth"):
        yuv.yuv_to_bgr_host(0, 0, 0, depth=12)


@pytest.mark.parametrize("matrix", sorted(ingest.MATRICES))
def test_depth_ten_integers_within_the_bound_of_the_float_formula(matrix):
    """On the exhaustive case (every chroma pair with 16 lumas: 16.7 M pixels) and on 2^22 seeded triples."""
    data, L = yi.exhaustive_case()
    worst, wrapped = 0.0, 0
    y_off, cy, cub, cug, cvg, cvr = ingest.MATRICES[matrix]
    one = yuv.YuvFrames(torch.empty((1, L.frame_stride), dtype=torch.uint8, device="meta"), L.h, L.w, **yi.fields(L))
    for k in range(L.n):
        y, u, v = yuv.yuv_samples_host(data[k:k + 1], one)
        if k == 0 and matrix == "bt601":       # every chroma pair once per 2 x 2 block, the frame's four lumas in each
            codes = (u[0, ::2, ::2].astype(np.int64) << 10 | v[0, ::2, ::2]).reshape(-1)
            assert np.array_equal(np.sort(codes), np.arange(1 << 20))
        assert sorted(np.unique(y).tolist()) == sorted(yi.EXHAUSTIVE_LUMAS[4 * k:4 * k + 4])
        got = yuv.yuv_to_bgr_host(y, u, v, matrix, depth=10)
        worst = max(worst, float(np.abs(got - yuv.yuv_to_bgr_f64(y, u, v, matrix, depth=10)).max()))
        blue = np.maximum(y.astype(np.int64) - (y_off << 2), 0) * cy + (1 << 21) + cub * (u.astype(np.int64) - 512)
        wrapped += int((blue >= 1 << 31).sum())
    assert wrapped > 0                                              # it contains the triples at which int32 sums wrap
    y, u, v = yi.seeded_triples(1 << 22)
    got = yuv.yuv_to_bgr_host(y, u, v, matrix, depth=10)
    worst = max(worst, float(np.abs(got - yuv.yuv_to_bgr_f64(y, u, v, matrix, depth=10)).max()))
    print(f"{matrix}: depth 10 max |integer - float| = 0.5 + {worst - 0.5:.3e}; bound 0.5 + {yi.BOUND_10 - 0.5:.3e}; "
          f"{wrapped} blue sums of the exhaustive case past int32")
    assert 0.49 < worst <= yi.BOUND_10
    assert yi.BOUND_10 == 0.5 + (959 + 512 + 512) / 2 / 2 ** 22


# --------------------------------------------------------------------------- the plan, the committed cases
def test_resize_plan_restatement_equals_the_librarys_on_the_committed_shapes():
    lib = _yuv_abi.lib()
    halved_two_byte = False
    for name, (fmt, args, frames, index, sizes) in yi.RESIZE_CASES.items():
        L = yi.layout(fmt, frames, *args)
        surface = (ctypes.c_int64 * 11)(*yi.surface_ints(L))
        for dh, dw in sizes:
            band, total, nl, nc = yi.resize_plan(L, dh, dw)
            assert band == lib.avsy_resize_band(surface, dh, dw) == yuv.yuv_resize_band(_frames(L), dh, dw), (name, dh, dw)
            assert 0 < total <= yi.RESIZE_LDS_BYTES
            assert (band < yi.RESIZE_BAND) == (name in yi.HALVED), (name, band)
            halved_two_byte |= band == 4 and L.sample_bytes == 2
    assert halved_two_byte
    # the same frame in one-byte samples keeps the full band: a two-byte row takes twice the LDS
    fmt, args = yi.RESIZE_CASES["halved_p010"][:2]
    assert yi.resize_plan(yi.layout("nv12", 1, *args), 224, 224)[0] == 8 == yi.resize_plan(yi.layout("i420", 1, *args), 224, 224)[0]
    assert yi.resize_plan(yi.layout("i010", 1, *args), 224, 224)[0] == 4
    # an NV12 description plans as the NV12 library does
    for h, w, dh, dw in ((448, 2560, 224, 224), (360, 640, 299, 299), (36, 70, 224, 224)):
        assert yi.resize_plan(yi.layout("nv12", 1, h, w), dh, dw)[:2] == ni.resize_plan(h, w, dh, dw)[:2]
    fmt, args, (dh, dw) = yi.REFUSED_CASE
    assert yi.resize_plan(yi.layout(fmt, 1, *args), dh, dw)[0] == 0
    # the gather index: a repeat, a descending run, one entry outside the three frames
    assert sorted(i for i in yi.GATHER_INDEX if not 0 <= i < 3) == [3] and yi.GATHER_INDEX[yi.GATHER_SKIPPED] == 3
    assert len(set(yi.GATHER_INDEX)) < len(yi.GATHER_INDEX) and list(yi.GATHER_INDEX[1:4]) == [2, 1, 0]


@pytest.mark.parametrize("fmt", yi.E2E_FORMATS)
def test_scene_batch_has_its_cuts_where_the_scenes_change(fmt):
    from avsum_amd.features.shots import cuts_from_scores
    data, L, offsets = yi.scene_batch(fmt)
    bgr = yuv.frames_to_bgr_host(data, _frames(L))
    sums = pfi.hsv_sums(bgr, 1, offsets)
    scores = sums.sum(1) / (3.0 * L.h * L.w)
    for v, want in enumerate(yi.scene_cuts()):
        part = scores[offsets[v]:offsets[v + 1]]
        cuts = cuts_from_scores(part)
        assert [(a, b) for a, b in zip([0] + cuts, cuts + [len(part)])] == want
        assert all(part[c] > 40.0 for c in cuts) and np.delete(part, cuts).max() < 10.0


# --------------------------------------------------------------------------- YuvFrames
def test_yuvframes_describes_and_refuses_on_metadata_alone():
    meta = torch.empty((3, 31, 80), dtype=torch.uint8, device="meta")
    f = yuv.YuvFrames.i420(meta, 20, 70)
    assert f.surface() == (3, 20, 70, 1, 0, 80, 40, 1, 1600, 2000, 31 * 80) and f.planar and f.depth == 8
    assert (f.shape, f.nbytes, f.device.type) == ((3, 20, 70, 3), 3 * 31 * 80, "meta")
    g = yuv.YuvFrames.yv12(meta, 20, 70)
    assert (g.u_offset, g.v_offset) == (2000, 1600)
    assert yuv.YuvFrames.i420(meta, 20, 70, pitch_c=36, v_offset=2040).surface()[6:10] == (36, 1, 1600, 2040)
    flat = torch.empty((3, 20 * 70 * 3 // 2), dtype=torch.uint8, device="meta")
    assert yuv.YuvFrames.i420(flat, 20, 70).surface() == (3, 20, 70, 1, 0, 70, 35, 1, 1400, 1750, 2100)
    assert yuv.YuvFrames.nv12(meta, 20, 70).surface() == (3, 20, 70, 1, 0, 80, 80, 2, 1600, 1601, 2480)
    assert yuv.YuvFrames.nv21(meta, 20, 70, uv_offset=1680).surface()[7:10] == (2, 1681, 1680)
    wide = torch.empty((3, 31, 160), dtype=torch.uint8, device="meta")
    p = yuv.YuvFrames.p010(wide, 20, 70)
    assert p.surface() == (3, 20, 70, 2, 6, 160, 160, 4, 3200, 3202, 31 * 160) and not p.planar and p.depth == 10
    q = yuv.YuvFrames.i010(wide, 20, 70)
    assert q.surface() == (3, 20, 70, 2, 0, 160, 80, 2, 3200, 4000, 31 * 160) and q.planar
    n = ingest.Nv12Frames(torch.zeros((3, 31, 80), dtype=torch.uint8), 20, 70, uv_row=21)
    assert yuv.YuvFrames.from_nv12(n).surface() == (3, 20, 70, 1, 0, 80, 80, 2, 1680, 1681, 2480)
    assert yuv.YuvFrames.from_nv12(n).data is n.data
    big = yuv.YuvFrames.p010(torch.empty((45000, 540, 1280), dtype=torch.uint8, device="meta"), 360, 640)
    assert big.nbytes == 45000 * 360 * 640 * 3                        # the bytes of the BGR batch, in ten bits
    assert yuv.YuvFrames(meta, 20, 70, **yi.fields(yi.layout("i420", 3, 20, 70, 80, 40))).surface() == f.surface()
    assert f.like(torch.zeros((3, 31, 80), dtype=torch.uint8)).surface() == f.surface()
    for make, bad, word in ((yuv.YuvFrames.i420, (19, 70), "even"), (yuv.YuvFrames.p010, (20, 69), "even"),
                            (yuv.YuvFrames.i420, (0, 70), "even"), (yuv.YuvFrames.i420, (20, 82), "pitch_y"),
                            (yuv.YuvFrames.p010, (20, 70), "pitch_y"),           # 140 bytes of samples in a pitch of 80
                            (yuv.YuvFrames.i420, (22, 70), "plane ends"), (yuv.YuvFrames.nv12, (22, 70), "plane ends")):
        with pytest.raises(ValueError, match=f"YuvFrames.*{word}"):
            make(meta, *bad)
    for kw, word in ((dict(u_offset=1589), "luma"), (dict(v_offset=1600), "U and V"), (dict(v_offset=1634), "U and V"),
                     (dict(pitch_c=34), "pitch_c"), (dict(u_offset=-2), "negative")):
        with pytest.raises(ValueError, match=f"YuvFrames.*{word}"):
            yuv.YuvFrames.i420(meta, 20, 70, **kw)
    for kw in (dict(pitch_y=141), dict(uv_offset=3201)):
        with pytest.raises(ValueError, match="YuvFrames.*even"):
            yuv.YuvFrames.p010(wide, 20, 70, **{("pitch" if k == "pitch_y" else k): v for k, v in kw.items()})
    with pytest.raises(ValueError, match="YuvFrames.*even"):                 # an odd base under two-byte samples
        yuv.YuvFrames.p010(torch.zeros(3 * 31 * 160 + 1, dtype=torch.uint8)[1:].view(3, 31, 160), 20, 70)
    with pytest.raises(ValueError, match="YuvFrames.*shift"):
        yuv.YuvFrames(meta, 20, 70, sample_bytes=1, shift=6, pitch_c=40, chroma_step=1, u_offset=1600, v_offset=2000)
    with pytest.raises(ValueError, match="YuvFrames.*must be given"):
        yuv.YuvFrames(meta, 20, 70)
    with pytest.raises(ValueError, match="pitch_c must be given"):
        yuv.YuvFrames.i420(torch.empty((3, 40, 71), dtype=torch.uint8, device="meta"), 20, 70)
    for other in (meta.to(torch.int8), meta[0][0], meta.transpose(1, 2), np.zeros((3, 31, 80), dtype=np.uint8)):
        with pytest.raises(ValueError, match="YuvFrames"):
            yuv.YuvFrames.i420(other, 20, 70)
    with pytest.raises(ValueError, match="from_nv12"):
        yuv.YuvFrames.from_nv12(meta)
    # python's overlap checks are the library's: the same verdict on a sweep of offsets
    lib = _yuv_abi.lib()
    for v_offset in range(0, 64):
        for make in (_surface, _surface16):
            if make is _surface16 and v_offset % 2:
                continue
            s = make(v_offset=v_offset, frame_stride=128)
            d = dict(zip(SURFACE_ORDER, s))
            try:
                yuv.YuvFrames(torch.empty((2, 128), dtype=torch.uint8, device="meta"), d["h"], d["w"], d["sample_bytes"], d["shift"],
                              d["pitch_y"], d["pitch_c"], d["chroma_step"], d["u_offset"], d["v_offset"])
                verdict = 8
            except ValueError:
                verdict = E_SHAPE
            assert lib.avsy_resize_band(s, 8, 8) == verdict, list(s)
    # the launch wrappers take device tensors only, and say so before anything else
    host = f.like(torch.zeros((3, 31, 80), dtype=torch.uint8))
    for call in (lambda: yuv.yuv_to_bgr(host), lambda: yuv.yuv_resize_gather(host, None, 0, [(8, 8)]),
                 lambda: yuv.yuv_to_bgr(host.data), lambda: yuv.yuv_to_bgr(n)):
        with pytest.raises(ValueError, match="yuv_"):
            call()
    from avsum_amd.features.shots import detect_shots_batch
    with pytest.raises(ValueError, match="detect_shots_batch"):
        detect_shots_batch(host, [0, 3])
    with pytest.raises(ValueError, match="matrix must be one of"):
        yuv._matrix_arg("bt2020", "yuv_to_bgr")
