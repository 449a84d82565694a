"""CPU-side checks of the NV12 ingest path (libavsum_ingest.so, avsum_amd/ingest.py): the third header and the binding
derived from it, the library's exports, validation before any launch, the integer definition against the float formula
on every (Y, U, V), the planted mistakes at the committed cases, the properties the committed resize cases are meant to
have (by the kernel's own plan), and Nv12Frames' refusals on metadata alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nv12_inputs as ni
import pixel_f64_inputs as pfi
from avsum_amd import _header, _ingest_abi, ingest

PKG = os.path.dirname(os.path.dirname(_ingest_abi.LIB_PATH))

_FRAMES = ["uint8_t*", "int64_t", "int", "int", "int", "int64_t", "int64_t", "int*"]      # d_src .. h_matrix
PINNED = {
    "avsi_abi_version": ("int", []),
    "avsi_last_error": ("char*", []),
    "avsi_nv12_to_bgr_u8": ("int", _FRAMES + ["int64_t*", "int64_t", "uint8_t*", "avsi_stream_t"]),
    "avsi_nv12_resize_gather2_u8": ("int", _FRAMES + ["int64_t*", "int64_t", "uint8_t*", "int", "int", "uint8_t*", "int",
                                                      "int", "avsi_stream_t"]),
    "avsi_nv12_resize_band": ("int", ["int", "int", "int", "int"]),
    "avsi_nv12_hsv_diff_batch_u8": ("int", _FRAMES + ["int", "int64_t*", "int", "uint32_t*", "avsi_stream_t"]),
}
E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -6


# --------------------------------------------------------------------------- header, binding, library
def test_ingest_header_parses_and_signatures_are_pinned():
    header = _ingest_abi.load_header()
    assert header.prototypes == PINNED
    assert _ingest_abi.declared_symbols() == sorted(PINNED)
    c = header.constants
    assert (c["AVSI_ABI_VERSION"], c["AVSI_SHIFT"], c["AVSI_MAX_COEF"], c["AVSI_MATRIX_INTS"]) == (1, 20, 1 << 22, 6)
    assert (c["AVSI_MAX_DIFF_FRAMES"], c["AVSI_RESIZE_BAND"], c["AVSI_RESIZE_LDS_BYTES"]) == (
        1 << 24, ni.RESIZE_BAND, ni.RESIZE_LDS_BYTES)
    assert (c["AVSI_OK"], c["AVSI_E_ARG"], c["AVSI_E_SHAPE"], c["AVSI_E_HIP"], c["AVSI_E_UNSUPPORTED"]) == (0, -1, -2, -4, -6)
    sig = header.signatures()
    assert sig["avsi_last_error"] == (ctypes.c_char_p, [])
    assert sig["avsi_nv12_to_bgr_u8"] == (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
    # no AVS_* name of the main header is defined again, and the main header's reader knows no avsi_ name
    main = _header.load()
    assert len(main.prototypes) == 96 and main.constants["AVS_ABI_VERSION"] == 5
    assert not [n for n in list(main.prototypes) + list(main.constants) if n.lower().startswith("avsi_")]
    assert not set(c) & set(main.constants)
    for path in (_ingest_abi.HEADER_PATH, os.path.join(PKG, "csrc", "ingest.hip")):
        assert not re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AVS_\w+)", open(path).read(), flags=re.M), path
    # the python side takes its limits from the header
    assert (ingest.SHIFT, ingest.MAX_COEF, ingest.MATRIX_INTS) == (20, 1 << 22, 6)


def test_ingest_library_exports_exactly_the_headers_functions():
    lib = _ingest_abi.lib()
    assert lib.avsi_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _ingest_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(avsi_[a-z0-9_]+)\b", out)) == set(PINNED)
    assert not re.findall(r"\b(avso?_[a-z0-9_]+)\b", out)              # nothing of the other two libraries is defined ...
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _ingest_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined
    assert not re.findall(r"\b(avs[io]?_[a-z0-9_]+)\b", undefined)     # ... and nothing of them is wanted
    for name, (res, args) in _ingest_abi._SIGNATURES.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name


def test_ingest_source_is_outside_srcs_and_built_with_the_same_flags():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "ingest.hip" not in srcs and len(srcs) == 21
    assert re.search(r"^all: \$\(LIB\) \$\(OPTIM_LIB\)$", make, flags=re.M)
    assert re.search(r"^all: \$\(INGEST_LIB\)$", make, flags=re.M)
    rule = re.search(r"^\.\./build/ingest\.o:.*\n(?:\t.*\n)*", make, flags=re.M).group(0)
    assert "$(HIPCC) $(CXXFLAGS) -c" in rule
    assert "$(INGEST_LIB)" in re.search(r"^clean:\n\t(.*)$", make, flags=re.M).group(1)
    text = open(os.path.join(PKG, "csrc", "ingest.hip")).read()
    assert re.search(r"^static thread_local char g_err\[", text, flags=re.M)
    assert not re.search(r"\bavs_set_error\b|\bAVS_REQUIRE\b|\bAVS_CHECK_LAUNCH\b", text)
    # the HSV pixel arithmetic keeps its single definition
    sources = [open(os.path.join(PKG, "csrc", f)).read() for f in sorted(os.listdir(os.path.join(PKG, "csrc")))]
    assert sum(len(re.findall(r"void bgr2hsv_u8\(", s)) for s in sources) == 1
    ignored = subprocess.run(["git", "-C", os.path.dirname(PKG), "check-ignore", "-q", _ingest_abi.LIB_PATH], capture_output=True)
    assert ignored.returncode in (0, 128)                            # ignored (128: not a git work tree)


# --------------------------------------------------------------------------- validation before any launch
def _frames(h=4, w=6, pitch=8, uv_row=4, rows=6, n=2):
    return [64, n, h, w, pitch, rows * pitch, uv_row * pitch]


def test_ingest_validation_before_launch_needs_no_gpu():
    """Every refusal comes before any HIP call (no call here could launch: each has a fault the checks find first).  The
    coefficient limit is 2^22: the blue coefficients of both named matrices (2 116 026, 2 214 593) lie above 2^21, and
    2^22 is the largest power of two that keeps every accumulator inside int32."""
    lib = _ingest_abi.lib()
    m = (ctypes.c_int * 6)(*ingest.MATRICES["bt601"])

    def calls(frames, matrix=m):
        """The three entry points on one frame description, every other argument fine."""
        return [("to_bgr", lambda: lib.avsi_nv12_to_bgr_u8(*frames, matrix, None, 1, 64, None)),
                ("resize", lambda: lib.avsi_nv12_resize_gather2_u8(*frames, matrix, 64, 1, 64, 8, 8, None, 0, 0, None)),
                ("hsv", lambda: lib.avsi_nv12_hsv_diff_batch_u8(*frames, matrix, 1, 64, 1, 64, None))]

    def refused(frames, code, word, matrix=m):
        for name, call in calls(frames, matrix):
            assert call() == code, (name, frames)
            assert word in lib.avsi_last_error(), (name, lib.avsi_last_error())

    refused(_frames(h=3), E_SHAPE, b"even")
    refused(_frames(w=5), E_SHAPE, b"even")
    refused(_frames(h=0), E_SHAPE, b"even")
    refused(_frames(pitch=4), E_SHAPE, b"pitch")
    refused(_frames(uv_row=3), E_SHAPE, b"uv_offset")                      # inside the luma plane
    refused(_frames(n=-1), E_SHAPE, b"n=-1")
    short = _frames()
    short[5] = 4 * 8 + 1 * 8 + 5                                           # one byte short of the last chroma row's w bytes
    refused(short, E_SHAPE, b"frame_stride")
    short[5] += 1                                                          # exactly enough: the description passes,
    short[0] = None                                                        # and the next check (the pointers) refuses
    refused(short, E_ARG, b"null")
    refused(short, E_ARG, b"null", matrix=(ctypes.c_int * 6)(*ingest.MATRICES["bt709"]))   # both named matrices pass
    refused(_frames(), E_ARG, b"h_matrix", matrix=None)
    for k in range(1, 6):
        for value in ((1 << 22) + 1, -(1 << 22) - 1):
            bad = list(ingest.MATRICES["bt709"])
            bad[k] = value
            refused(_frames(), E_ARG, b"2^22", matrix=(ctypes.c_int * 6)(*bad))
    refused(_frames(), E_ARG, b"y_off", matrix=(ctypes.c_int * 6)(256, 1, 1, 1, 1, 1))
    edge = (ctypes.c_int * 6)(255, 1 << 22, -(1 << 22), 1 << 22, -(1 << 22), 1 << 22)       # the limits themselves pass
    # null pointers: source, destination, index, offsets, sums
    ok = _frames()
    null_src = [None] + ok[1:]
    for matrix in (m, edge):
        assert lib.avsi_nv12_to_bgr_u8(*null_src, matrix, None, 1, 64, None) == E_ARG and b"null" in lib.avsi_last_error()
    assert lib.avsi_nv12_to_bgr_u8(*ok, m, None, 1, None, None) == E_ARG
    assert lib.avsi_nv12_to_bgr_u8(*ok, m, None, 3, 64, None) == E_SHAPE and b"no index" in lib.avsi_last_error()
    assert lib.avsi_nv12_to_bgr_u8(*ok, m, None, -1, 64, None) == E_SHAPE
    assert lib.avsi_nv12_to_bgr_u8(*ok, m, None, 0, None, None) == 0                        # nothing to do
    assert lib.avsi_nv12_resize_gather2_u8(*null_src, m, 64, 1, 64, 8, 8, None, 0, 0, None) == E_ARG
    assert lib.avsi_nv12_resize_gather2_u8(*ok, m, None, 1, 64, 8, 8, None, 0, 0, None) == E_ARG
    assert lib.avsi_nv12_resize_gather2_u8(*ok, m, 64, 1, None, 8, 8, None, 0, 0, None) == E_ARG
    assert lib.avsi_nv12_resize_gather2_u8(*ok, m, 64, 1, 64, 0, 8, None, 0, 0, None) == E_SHAPE
    assert lib.avsi_nv12_resize_gather2_u8(*ok, m, 64, 1, 64, 8, 8, 64, 8, 0, None) == E_SHAPE
    assert lib.avsi_nv12_resize_gather2_u8(*ok, m, 64, 1, 64, 65536, 8, None, 0, 0, None) == E_UNSUPPORTED
    wide = _frames(h=2, w=30000, pitch=30000, uv_row=2, rows=3)
    assert lib.avsi_nv12_resize_gather2_u8(*wide, m, 64, 1, 64, 8, 8, None, 0, 0, None) == E_UNSUPPORTED
    assert b"LDS" in lib.avsi_last_error() and lib.avsi_nv12_resize_band(2, 30000, 8, 8) == 0
    assert lib.avsi_nv12_resize_band(3, 8, 8, 8) == E_SHAPE
    assert lib.avsi_nv12_hsv_diff_batch_u8(*null_src, m, 1, 64, 1, 64, None) == E_ARG
    assert lib.avsi_nv12_hsv_diff_batch_u8(*ok, m, 1, None, 1, 64, None) == E_ARG
    assert lib.avsi_nv12_hsv_diff_batch_u8(*ok, m, 1, 64, 1, None, None) == E_ARG
    assert lib.avsi_nv12_hsv_diff_batch_u8(*ok, m, 0, 64, 1, 64, None) == E_SHAPE
    assert lib.avsi_nv12_hsv_diff_batch_u8(*ok, m, 1, 64, 0, 64, None) == E_SHAPE and b"no video" in lib.avsi_last_error()
    many = _frames(n=(1 << 24) + 1)
    assert lib.avsi_nv12_hsv_diff_batch_u8(*many, m, 1, 64, 1, 64, None) == E_SHAPE and b"16777216" in lib.avsi_last_error()
    assert lib.avsi_nv12_hsv_diff_batch_u8(*_frames(n=0), m, 1, None, 0, None, None) == 0
    with pytest.raises(_ingest_abi.AvsiError, match="status -2.*pitch"):
        _ingest_abi.check(lib.avsi_nv12_to_bgr_u8(*_frames(pitch=4), m, None, 1, 64, None), "avsi_nv12_to_bgr_u8")


# --------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("matrix", sorted(ingest.MATRICES))
def test_integer_definition_within_the_bound_of_the_float_formula_on_every_triple(matrix):
    """All 2^24 (Y, U, V): |nv12_to_bgr_host - nv12_to_bgr_f64| <= 0.5 + 493 * 2^-21, and no accumulator near int32's end."""
    worst = 0.0
    for lo in range(0, 256, 32):
        y, u, v = ni.all_triples(lo, lo + 32)
        got = ingest.yuv_to_bgr_host(y, u, v, matrix)
        worst = max(worst, float(np.abs(got.astype(np.float64) - ingest.yuv_to_bgr_f64(y, u, v, matrix)).max()))
    print(f"{matrix}: max |integer - float| = 0.5 + {worst - 0.5:.3e}; bound 0.5 + {ni.BOUND - 0.5:.3e}")
    assert 0.5 <= worst <= ni.BOUND
    y_off, cy, cub, cug, cvg, cvr = ingest.MATRICES[matrix]
    top = (255 - y_off) * abs(cy) + (1 << 19) + 128 * max(abs(cub), abs(cug) + abs(cvg), abs(cvr))
    assert top < 0.54 * 2 ** 30
    # the integers are the rounded three-decimal coefficients
    assert ingest.MATRICES[matrix][1:] == tuple(int(round(c * 2 ** 20)) for c in ingest.MATRICES_F64[matrix][1:])


def test_the_two_restatements_agree_at_every_committed_conversion_case():
    for layout in ni.LAYOUTS:
        h, w, pitch, uv_row = layout
        data = ni.layout_case(layout)
        for matrix in sorted(ingest.MATRICES):
            want = ingest.nv12_to_bgr_host(data, h, w, uv_row, matrix)
            assert want.shape == (ni.LAYOUT_FRAMES, h, w, 3) and want.dtype == np.uint8
            assert np.array_equal(ni.restatement(data, h, w, uv_row, matrix), want)
            err = np.abs(want - ingest.nv12_to_bgr_f64(data, h, w, uv_row, matrix)).max()
            assert err <= ni.BOUND
        # the sentinel bytes are exactly the bytes outside the planes
        mask = ni.planes_mask(h, w, pitch, uv_row, data.shape[1])
        assert (data[:, ~mask] == ni.SENTINEL_U8).all() and (~mask).any()
    cube = ni.exhaustive_case()
    y, u, v = ingest._planes(cube, 512, 512, 512)
    codes = (y.astype(np.int64) << 16 | u.astype(np.int64) << 8 | v).reshape(-1)
    assert codes.size == 1 << 24 and np.array_equal(np.sort(codes), np.arange(1 << 24))     # every triple exactly once


def test_planted_mistakes_are_noticed_at_a_committed_case():
    assert set(ni.NOTICED_BY) | set(ni.INERT) == set(ni.MISTAKES) and not set(ni.NOTICED_BY) & set(ni.INERT)
    for mistake, layout in ni.NOTICED_BY.items():
        h, w, pitch, uv_row = layout
        data = ni.layout_case(layout)
        want = ingest.nv12_to_bgr_host(data, h, w, uv_row)
        wrong = ni.restatement(data, h, w, uv_row, mistake=mistake)
        print(f"{mistake}: {int((wrong != want).sum())} of {want.size} bytes differ at {layout}")
        assert (wrong != want).any(), mistake
    # pitch == w hides the pitch mistake: the case that notices it must have padding
    assert np.array_equal(ni.restatement(ni.layout_case((2, 2, 2, 2)), 2, 2, 2, mistake="w_for_pitch"),
                          ingest.nv12_to_bgr_host(ni.layout_case((2, 2, 2, 2)), 2, 2, 2))


def test_truncation_of_negative_sums_cannot_reach_a_byte():
    """The issue's seventh planted mistake, rounding a negative sum towards zero instead of down: after the clamp it is
    the same byte for every (Y, U, V) and both matrices - no case, committed or not, can notice it in the output.  It IS
    a different integer before the clamp (shown here on the exhaustive planes), which is where the restatements and
    the kernel are written to floor."""
    assert list(ni.INERT) == ["trunc_negative"]
    for layout in ni.LAYOUTS:
        h, w, pitch, uv_row = layout
        data = ni.layout_case(layout)
        assert np.array_equal(ni.restatement(data, h, w, uv_row, mistake="trunc_negative"),
                              ingest.nv12_to_bgr_host(data, h, w, uv_row))
    data = ni.exhaustive_case()[:4]                                    # lumas 0 .. 15 with every chroma pair
    for matrix in sorted(ingest.MATRICES):
        floor = ni.restatement(data, 512, 512, 512, matrix, clamp=False)
        trunc = ni.restatement(data, 512, 512, 512, matrix, mistake="trunc_negative", clamp=False)
        differ = floor != trunc
        assert differ.any() and (floor[differ] < 0).all() and (trunc[differ] == floor[differ] + 1).all()
        assert np.array_equal(np.clip(floor, 0, 255), np.clip(trunc, 0, 255))


# --------------------------------------------------------------------------- the committed resize and scan cases
def test_resize_cases_have_the_properties_they_are_committed_for():
    lib = _ingest_abi.lib()
    odd_start = straddle_low = straddle_high = split_rows = False
    for name, (h, w, pitch, uv_row, frames, index, sizes) in ni.RESIZE_CASES.items():
        for dh, dw in sizes:
            band, total, nl, nc = ni.resize_plan(h, w, dh, dw)
            assert band == lib.avsi_nv12_resize_band(h, w, dh, dw) and 0 < total <= ni.RESIZE_LDS_BYTES, (name, dh, dw)
            assert (band < ni.RESIZE_BAND) == (name == "halved"), (name, band)
            for y_lo, y_hi in ni.band_rows(h, dh, band):
                odd_start |= y_lo % 2 == 1                             # the band's first chroma row also serves y_lo - 1
                straddle_low |= y_lo % 2 == 1 and y_lo > 0
                straddle_high |= y_hi % 2 == 0 and y_hi < h - 1        # its last chroma row also serves y_hi + 1
                split_rows |= y_hi - y_lo + 1 < 2 * ((y_hi >> 1) - (y_lo >> 1) + 1)
    assert odd_start and straddle_low and straddle_high and split_rows
    # the BGR kernel's plan of the same frames halves earlier: 3 bytes per pixel against 1.5
    assert pfi.gather_plan(448, 2560, 224, 224)[0] < ni.resize_plan(448, 2560, 224, 224)[0] == 4
    assert ni.resize_plan(360, 640, 299, 299)[0] == 8 == pfi.gather_plan(360, 640, 299, 299)[0]
    assert sorted(i for i in ni.GATHER_INDEX if not 0 <= i < 3) == [3] and ni.GATHER_INDEX[ni.GATHER_SKIPPED] == 3


def test_scene_batch_has_its_cuts_where_the_scenes_change():
    """detect_shots' host rule on the converted frames of the end-to-end batch: the planted cuts, with margin."""
    from avsum_amd.features.shots import cuts_from_scores
    data, offsets = ni.scene_batch()
    h, w, pitch, uv_row = ni.E2E_LAYOUT
    bgr = ingest.nv12_to_bgr_host(data, h, w, uv_row)
    sums = pfi.hsv_sums(bgr, 1, offsets)
    scores = sums.sum(1) / (3.0 * h * w)
    for v, want in enumerate(ni.scene_cuts()):
        part = scores[offsets[v]:offsets[v + 1]]
        cuts = cuts_from_scores(part)
        assert [(a, b) for a, b in zip([0] + cuts, cuts + [len(part)])] == want
        assert all(part[c] > 40.0 for c in cuts) and np.delete(part, cuts).max() < 10.0


# --------------------------------------------------------------------------- Nv12Frames
def test_nv12frames_describes_and_refuses_on_metadata_alone():
    data = torch.zeros((3, 31, 80), dtype=torch.uint8, device="cpu")
    f = ingest.Nv12Frames(data, 20, 70, uv_row=21)
    assert (f.frames, f.height, f.width, f.pitch, f.uv_row) == (3, 20, 70, 80, 21)
    assert (f.frame_stride, f.uv_offset, f.nbytes, f.shape) == (31 * 80, 21 * 80, 3 * 31 * 80, (3, 20, 70, 3))
    assert ingest.Nv12Frames(data, 20, 70).uv_offset == 20 * 80
    meta = ingest.Nv12Frames(torch.empty((45000, 540, 640), dtype=torch.uint8, device="meta"), 360, 640)
    assert meta.nbytes == 45000 * 360 * 640 * 3 // 2                  # half the bytes of the BGR batch
    for bad, word in (((19, 70), "even"), ((20, 69), "even"), ((0, 70), "even"), ((20, 82), "pitch"), ((22, 70), "rows")):
        with pytest.raises(ValueError, match=f"Nv12Frames.*{word}"):
            ingest.Nv12Frames(data, *bad)
    with pytest.raises(ValueError, match="luma plane"):
        ingest.Nv12Frames(data, 20, 70, uv_row=19)
    with pytest.raises(ValueError, match="rows"):
        ingest.Nv12Frames(data, 20, 70, uv_row=22)
    for other in (data.to(torch.int8), data[0], data.transpose(1, 2), np.zeros((3, 31, 80), dtype=np.uint8)):
        with pytest.raises(ValueError, match="Nv12Frames"):
            ingest.Nv12Frames(other, 20, 70)
    # the launch wrappers take device tensors only, and say so before anything else
    for call in (lambda: ingest.nv12_to_bgr(f), lambda: ingest.nv12_resize_gather(f, None, 0, [(8, 8)]),
                 lambda: ingest.nv12_to_bgr(data)):
        with pytest.raises(ValueError, match="nv12_"):
            call()
    with pytest.raises(ValueError, match="matrix must be one of"):
        ingest._matrix("bt2020", "nv12_to_bgr")
    with pytest.raises(ValueError, match="2\\^22"):
        ingest._matrix((16, (1 << 22) + 1, 0, 0, 0, 0), "nv12_to_bgr")
    assert ingest._matrix([16, 1, 2, 3, 4, 5], "x") == (16, 1, 2, 3, 4, 5)
