"""CPU-side checks of the summary rendering (libavsum_render.so, avsum_amd/render.py): the eighth header and the binding
derived from it, the library's exports, every refusal before any launch, RenderTables on the host, the numpy definitions
against their restatements on every committed case, the planted mistakes, and the round trip through
yuv.yuv_to_bgr_host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import render_inputs as ri
import yuv_inputs as yi
from avsum_amd import _header, _render_abi, _yuv_abi, ops, render, yuv

PKG = os.path.dirname(os.path.dirname(_render_abi.LIB_PATH))
PINNED = {
    "avsr_abi_version": ("int", []),
    "avsr_last_error": ("char*", []),
    "avsr_summary_index": ("int", ["uint8_t*", "int64_t", "int64_t*", "int64_t*", "int", "int32_t*", "int64_t", "int64_t*",
                                   "int64_t*", "int64_t", "int64_t*", "int64_t*", "int64_t", "int64_t*", "int64_t*",
                                   "avsr_stream_t"]),
    "avsr_bgr_to_yuv_u8": ("int", ["uint8_t*", "int64_t", "uint8_t*", "int64_t*", "int*", "int64_t*", "int64_t",
                                   "avsr_stream_t"]),
    "avsr_repack_u8": ("int", ["uint8_t*", "int64_t*", "uint8_t*", "int64_t*", "int64_t*", "int64_t", "avsr_stream_t"]),
    "avsr_audio_cut": ("int", ["float*", "int64_t*", "int64_t*", "int", "double*", "double", "int64_t", "int64_t*", "int64_t",
                               "int64_t*", "int64_t*", "float*", "int64_t", "int64_t*", "int64_t*", "avsr_stream_t"]),
}
E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -6
ISSUE_INTEGERS = {
    "bt601": (16, 102760, 528482, 269484, 460325, -305136, -155189, -74449, -385876, 460325),
    "bt709": (16, 65012, 643826, 191889, 460325, -355467, -105906, -41943, -418382, 460325),
}


def _frames(L, data=None):
    if data is None:
        data = torch.empty((L.n, L.frame_stride), dtype=torch.uint8, device="meta")
    return yuv.YuvFrames(data, L.h, L.w, **yi.fields(L))


# --------------------------------------------------------------------------- header, binding, library
def test_render_header_parses_and_signatures_are_pinned():
    header = _render_abi.load_header()
    assert header.prototypes == PINNED
    assert _render_abi.declared_symbols() == sorted(PINNED)
    c = header.constants
    assert (c["AVSR_ABI_VERSION"], c["AVSR_TILE"], c["AVSR_TILE_COLS"], c["AVSR_MAX_FRAMES"]) == (1, ri.TILE, 2, 1 << 24)
    assert (c["AVSR_SHIFT"], c["AVSR_MAX_ROW_SUM"], c["AVSR_FORWARD_INTS"], c["AVSR_SURFACE_INTS"]) == (20, 1 << 20, 10, 11)
    assert (c["AVSR_TOTAL_COLS"], c["AVSR_AUDIO_COLS"]) == (3, 3) and c["AVSR_AUDIO_TILE"] % 256 == 0
    assert (c["AVSR_OK"], c["AVSR_E_ARG"], c["AVSR_E_SHAPE"], c["AVSR_E_HIP"], c["AVSR_E_UNSUPPORTED"]) == (0, -1, -2, -4, -6)
    # one surface description for both pixel libraries
    assert _render_abi.SURFACE_FIELDS == _yuv_abi.SURFACE_FIELDS
    sig = header.signatures()
    assert sig["avsr_last_error"] == (ctypes.c_char_p, [])
    assert sig["avsr_repack_u8"] == (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p])
    # no name of another header is defined again
    main, other = _header.load(), _yuv_abi.load_header()
    assert not [n for n in list(main.prototypes) + list(main.constants) if n.lower().startswith("avsr_")]
    assert not set(c) & (set(main.constants) | set(other.constants))
    # the header's comment is the definition
    text = open(_render_abi.HEADER_PATH).read()
    for phrase in ("2^(19 - k)", ">> (20 - k)", "2^(21 - k)", ">> (22 - k)", "sample << shift", "min(fade, L / 2)",
                   "(double)s / fps_v * (double)sr", "No\n * atomic operation", "never crosses a video boundary"):
        assert phrase in text, phrase
    # the plan takes its tile from the header
    from avsum_amd import ragged
    assert ragged.RENDER_TILE == c["AVSR_TILE"] and ops.RenderTables is ragged.RenderTables is render.RenderTables


def test_render_library_exports_exactly_the_headers_functions():
    lib = _render_abi.lib()
    assert lib.avsr_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _render_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(avsr_[a-z0-9_]+)\b", out)) == set(PINNED)
    assert not re.findall(r"\b(avs[aiodly]?_[a-z0-9_]+)\b", out)              # nothing of the seven others is defined ...
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _render_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined
    assert not re.findall(r"\b(avs[a-z]?_[a-z0-9_]+)\b", undefined)           # ... and nothing of them is wanted
    for name, (res, args) in _render_abi._SIGNATURES.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name
    out = subprocess.run(["nm", "-D", _yuv_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert not re.findall(r"\bavsr_", out)                                    # the YUV library is as it was


def test_render_source_is_a_library_of_its_own_without_atomics_or_waiting():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "render.hip" not in srcs and len(srcs) == 21
    assert re.search(r"^all: \$\(RENDER_LIB\)$", make, flags=re.M)
    rule = re.search(r"^\.\./build/render\.o:.*\n(?:\t.*\n)*", make, flags=re.M).group(0)
    assert "$(HIPCC) $(CXXFLAGS) -c" in rule and "avsum_render.h" in rule
    assert "$(RENDER_LIB)" in re.search(r"^clean:\n\t(.*)$", make, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS = (.*)$", make, flags=re.M).group(1)
    text = open(os.path.join(PKG, "csrc", "render.hip")).read()
    assert re.search(r"^static thread_local char g_err\[", text, flags=re.M)
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\batomic\w*\(|\b__hip_atomic|\bwhile\s*\(\s*\*|volatile", code)   # no atomics, no spin on a flag
    assert not re.search(r"hipMalloc|hipFree|hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy", code)
    assert code.count("hipLaunchKernelGGL(index_") == 3 and code.count("hipLaunchKernelGGL(audio_") == 2
    ignored = subprocess.run(["git", "-C", os.path.dirname(PKG), "check-ignore", "-q", _render_abi.LIB_PATH], capture_output=True)
    assert ignored.returncode in (0, 128)


# --------------------------------------------------------------------------- validation before any launch
SURFACE_ORDER = _render_abi.SURFACE_FIELDS


def _surface(**changes):
    """h_surface of 2 I420 frames of 4 x 6 with pitches 8 and 4, one spare row after every plane; ``changes`` by field."""
    base = dict(n=2, h=4, w=6, sample_bytes=1, shift=0, pitch_y=8, pitch_c=4, chroma_step=1, u_offset=40, v_offset=52,
                frame_stride=64)
    base.update(changes)
    return (ctypes.c_int64 * 11)(*[base[f] for f in SURFACE_ORDER])


def _surface16(**changes):
    base = dict(n=2, h=4, w=6, sample_bytes=2, shift=6, pitch_y=16, pitch_c=16, chroma_step=4, u_offset=64, v_offset=66,
                frame_stride=96)
    base.update(changes)
    return (ctypes.c_int64 * 11)(*[base[f] for f in SURFACE_ORDER])


def test_render_pixel_validation_before_launch_needs_no_gpu():
    """Every refusal comes before any HIP call (no call here could launch: each has a fault the checks find first, and
    the pointers are made-up addresses)."""
    lib = _render_abi.lib()
    fwd = (ctypes.c_int * 10)(*render.FORWARD_MATRICES["bt601"])
    SRC, DST = 1 << 20, 1 << 24                                   # made-up, far apart

    def forward(surface, matrix=fwd, src=SRC, dst=DST, n=2, count=1):
        return lib.avsr_bgr_to_yuv_u8(src, n, dst, surface, matrix, None, count, None)

    def refused(call, code, word):
        assert call() == code, lib.avsr_last_error()
        assert word in lib.avsr_last_error(), lib.avsr_last_error()

    # odd extents and the rest of the description, for the forward conversion and for both sides of a repack
    for bad, word in ((_surface(h=3), b"even"), (_surface(w=5), b"even"), (_surface(h=0), b"even"), (_surface(sample_bytes=3), b"sample_bytes"),
                      (_surface(shift=6), b"shift"), (_surface(pitch_y=5), b"pitch_y"), (_surface(pitch_c=2), b"pitch_c"),
                      (_surface(chroma_step=0), b"chroma_step"), (_surface(frame_stride=58), b"frame_stride"),
                      # an overlapping destination: one plane twice, V on U's third sample, U on the luma's last byte
                      (_surface(v_offset=40), b"U and V"), (_surface(v_offset=42), b"U and V"), (_surface(u_offset=29), b"luma"),
                      (_surface16(v_offset=68), b"U and V"), (_surface16(pitch_y=17), b"even")):
        refused(lambda: forward(bad), E_SHAPE, word)
        refused(lambda: lib.avsr_repack_u8(SRC, bad, DST, _surface(), None, 1, None), E_SHAPE, word)
        refused(lambda: lib.avsr_repack_u8(SRC, _surface(), DST, bad, None, 1, None), E_SHAPE, word)
    refused(lambda: forward(_surface16(), dst=DST + 1), E_SHAPE, b"even")            # a two-byte destination at an odd byte
    # a destination whose bytes overlap the source's: 2 BGR frames of 4 x 6 are 144 bytes
    refused(lambda: forward(_surface(), dst=SRC + 143), E_SHAPE, b"overlaps the source")
    refused(lambda: forward(_surface(), dst=SRC - 127), E_SHAPE, b"overlaps the source")
    refused(lambda: lib.avsr_repack_u8(SRC, _surface(), SRC + 64, _surface(), None, 1, None), E_SHAPE, b"overlaps the source")
    # ... what merely touches passes on to the next check: the null stream is fine, so the pointers must be refused first
    refused(lambda: forward(_surface(), src=None), E_ARG, b"null")
    refused(lambda: forward(_surface(), dst=None), E_ARG, b"null")
    # counts
    refused(lambda: forward(_surface(), count=3), E_SHAPE, b"destination holds 2")
    refused(lambda: forward(_surface(), n=1, count=2), E_SHAPE, b"no index")
    refused(lambda: forward(_surface(), count=-1), E_SHAPE, b"count")
    # the forward matrix: y_off, and every row's sum of magnitudes at most 2^20
    refused(lambda: forward(_surface(), matrix=None), E_ARG, b"h_forward")
    refused(lambda: forward(_surface(), matrix=(ctypes.c_int * 10)(256, *[0] * 9)), E_ARG, b"y_off")
    refused(lambda: forward(_surface(), matrix=(ctypes.c_int * 10)(-1, *[0] * 9)), E_ARG, b"y_off")
    for row in range(3):
        for signs in ((1, 1, 1), (-1, 1, -1)):
            over = [16] + [0] * 9
            over[1 + 3 * row:4 + 3 * row] = [signs[0] * (1 << 19), signs[1] * (1 << 18), signs[2] * ((1 << 18) + 1)]
            refused(lambda: forward(_surface(), matrix=(ctypes.c_int * 10)(*over)), E_ARG, b"2^20")     # 2^20 + 1
            over[3 + 3 * row] = signs[2] * (1 << 18)                                                  # 2^20: accepted ...
            refused(lambda: forward(_surface(), matrix=(ctypes.c_int * 10)(*over), src=None), E_ARG, b"null")   # ... (next check)
    refused(lambda: forward(_surface(), matrix=(ctypes.c_int * 10)(*ri.CUSTOM), src=None), E_ARG, b"null")
    with pytest.raises(ValueError, match="forward matrix"):
        render._forward((16, 1 << 19, 1 << 18, (1 << 18) + 1, 0, 0, 0, 0, 0, 0), "test")
    assert render._forward(ri.CUSTOM, "test") == ri.CUSTOM
    # repack: differing extents, differing depths
    refused(lambda: lib.avsr_repack_u8(SRC, _surface(), DST, _surface(h=6, u_offset=56, v_offset=72, frame_stride=96), None, 1, None),
            E_SHAPE, b"4x6")
    refused(lambda: lib.avsr_repack_u8(SRC, _surface(), DST, _surface16(), None, 1, None), E_UNSUPPORTED, b"depth")
    refused(lambda: lib.avsr_repack_u8(SRC, _surface16(), DST, _surface(), None, 1, None), E_UNSUPPORTED, b"depth")
    refused(lambda: lib.avsr_repack_u8(SRC, _surface16(), DST, _surface16(shift=0), None, 3, None), E_SHAPE, b"destination holds 2")
    refused(lambda: lib.avsr_repack_u8(None, _surface16(), DST, _surface16(shift=0), None, 1, None), E_ARG, b"null")
    # count = 0 is nothing to do
    assert forward(_surface(), src=None, dst=None, count=0) == 0


def test_render_index_and_audio_validation_before_launch_needs_no_gpu():
    lib = _render_abi.lib()
    P = 1 << 20
    off = (ctypes.c_int64 * 3)(0, 5, 1030)

    def index(n=1030, offsets=off, nv=2, ntiles=3, frame_cap=10, run_cap=10, mask=P):
        return lib.avsr_summary_index(mask, n, offsets, P, nv, P, ntiles, P, P, frame_cap, P, P, run_cap, P, P, None)

    def refused(call, code, word):
        assert call() == code, lib.avsr_last_error()
        assert word in lib.avsr_last_error(), lib.avsr_last_error()

    for caps in (dict(frame_cap=0), dict(run_cap=0), dict(frame_cap=-3), dict(run_cap=1 << 31)):      # capacities < 1
        refused(lambda: index(**caps), E_ARG, b"capacities")
    refused(lambda: index(n=0), E_SHAPE, b"n=0")
    refused(lambda: index(n=(1 << 24) + 1), E_SHAPE, b"frames")
    refused(lambda: index(nv=0), E_SHAPE, b"nvideos=0")
    refused(lambda: index(offsets=None), E_ARG, b"h_offsets")
    refused(lambda: index(n=1031), E_SHAPE, b"offsets run")
    refused(lambda: index(offsets=(ctypes.c_int64 * 3)(1, 5, 1030)), E_SHAPE, b"offsets run")
    refused(lambda: index(offsets=(ctypes.c_int64 * 3)(0, 0, 1030)), E_SHAPE, b"empty")
    refused(lambda: index(ntiles=2), E_SHAPE, b"give 3 tiles")                        # 5 -> 1 tile, 1025 -> 2 tiles
    refused(lambda: index(mask=None), E_ARG, b"null")

    woff = (ctypes.c_int64 * 3)(0, 100, 300)

    def audio(wave_offsets=woff, nv=2, sr=16000.0, fade=0, run_cap=4, sample_cap=300, wave=P):
        return lib.avsr_audio_cut(wave, wave_offsets, P, nv, P, sr, fade, P, run_cap, P, P, P, sample_cap, P, P, None)

    for caps in (dict(run_cap=0), dict(sample_cap=0), dict(sample_cap=-1)):
        refused(lambda: audio(**caps), E_ARG, b"capacities")
    refused(lambda: audio(fade=-1), E_ARG, b"fade")
    refused(lambda: audio(sr=0.0), E_ARG, b"sr")
    refused(lambda: audio(sr=float("nan")), E_ARG, b"sr")
    refused(lambda: audio(nv=0), E_SHAPE, b"nvideos")
    refused(lambda: audio(wave_offsets=None), E_ARG, b"h_wave_offsets")
    refused(lambda: audio(wave_offsets=(ctypes.c_int64 * 3)(0, 100, 50)), E_SHAPE, b"decrease")
    refused(lambda: audio(wave_offsets=(ctypes.c_int64 * 3)(4, 100, 300)), E_SHAPE, b"start")
    refused(lambda: audio(wave=None), E_ARG, b"null")


# --------------------------------------------------------------------------- RenderTables on the host
def test_render_tables_on_the_host():
    t = ops.RenderTables(ri.INDEX_OFFSETS, device="cpu")
    n, nv = ri.INDEX_OFFSETS[-1], len(ri.INDEX_LENGTHS)
    assert (t.nvideos, t.frames, t.frame_cap, t.run_cap, t.bare) == (nv, n, n, -(-n // 2) + nv, True)
    assert t.tiles.dtype == np.int32 and t.tiles_t.device.type == "cpu" and not t.has_audio and t.sample_cap is None
    assert t.tiles.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]] and t.ntiles == 8
    # the default run capacity holds the most runs any mask has
    assert ops.RenderTables([0, 1, 4, 9], device="cpu").run_cap >= 1 + 2 + 3
    small = ops.RenderTables(ri.INDEX_OFFSETS, *ri.SMALL_CAPS, device="cpu")
    assert (small.frame_cap, small.run_cap) == ri.SMALL_CAPS
    # from a keyshot plan: the frames a summary may hold and the shot capacity
    plan = ops.SummaryTables(ri.E2E_OFFSETS, 0.15, 10, device="cpu")
    k = ops.RenderTables.from_keyshots(plan)
    assert plan.capacity.tolist() == [0, 6, 3] and (k.frame_cap, k.run_cap, k.bare) == (9, 10, False)
    assert ops.RenderTables.from_keyshots(ops.SummaryTables([0, 5], 0.15, 1, device="cpu")).frame_cap == 1   # (a buffer needs a row)
    for bad in (dict(frame_cap=0), dict(run_cap=0), dict(capacity=[1, 2]), dict(capacity=[1, -1, 1, 1, 1]),
                dict(wave_offsets=[0, 1, 2, 3, 4, 5]), dict(fps=25.0),
                dict(wave_offsets=[0, 1, 2, 3, 4, 5], fps=0.0), dict(wave_offsets=[0, 1, 2, 3, 4, 5], fps=[25.0, 30.0]),
                dict(wave_offsets=[0, 1, 2, 3], fps=25.0), dict(wave_offsets=[0, 3, 2, 3, 4, 5], fps=25.0),
                dict(wave_offsets=[0, 1, 2, 3, 4, 5], fps=25.0, sr=float("inf"))):
        with pytest.raises(ValueError):
            ops.RenderTables(ri.INDEX_OFFSETS, device="cpu", **bad)
    with pytest.raises(ValueError, match="2\\^24"):
        ops.RenderTables([0, (1 << 24) + 1], device="cpu")
    with pytest.raises(ValueError):
        ops.RenderTables.from_keyshots(t)


def test_render_sample_cap_covers_every_audio_case():
    """sample_cap >= the host definition's true count: for the bare mask (S) and for keyshot-style capacities equal to the
    frames each video really picks - the tightest capacities the bound is claimed for."""
    wave, mask = ri.audio_case()
    host = render.summary_index_host(mask, ri.AUDIO_OFFSETS)
    assert host["per_video"] == [list(r) for r in ri.AUDIO_RUNS]
    for fade in ri.AUDIO_FADES:
        audio, offsets = render.summary_audio_host(wave, ri.AUDIO_WAVE_OFFSETS, ri.AUDIO_RUNS, ri.AUDIO_FPS, ri.AUDIO_SR, fade)
        bare = ops.RenderTables(ri.AUDIO_OFFSETS, wave_offsets=ri.AUDIO_WAVE_OFFSETS, fps=ri.AUDIO_FPS, sr=ri.AUDIO_SR, device="cpu")
        assert bare.sample_cap == ri.AUDIO_WAVE_OFFSETS[-1] >= audio.size == offsets[-1]
        tight = ops.RenderTables(ri.AUDIO_OFFSETS, capacity=host["totals"][:, 1], wave_offsets=ri.AUDIO_WAVE_OFFSETS,
                                 fps=ri.AUDIO_FPS, sr=ri.AUDIO_SR, device="cpu")
        assert audio.size <= tight.sample_cap < bare.sample_cap
        per_video = np.minimum(ri.AUDIO_TRACKS, np.ceil(host["totals"][:, 1] * ri.AUDIO_SR / np.array(ri.AUDIO_FPS)) + 1
                               + np.minimum(host["totals"][:, 1], -(-np.array(ri.AUDIO_FRAMES) // 2)))
        assert (np.diff(offsets) <= per_video).all() and tight.sample_cap == int(per_video.sum())
    assert bare.fps.dtype == np.float64 and bare.fps_t.dtype == torch.float64 and bare.fps.tolist() == list(ri.AUDIO_FPS)
    # one fps for every video
    assert ops.RenderTables(ri.AUDIO_OFFSETS, wave_offsets=ri.AUDIO_WAVE_OFFSETS, fps=25, device="cpu").fps.tolist() == [25.0] * 3
    # the clamped, the empty and the one-sample runs are what the case says they are
    _, offsets = render.summary_audio_host(wave, ri.AUDIO_WAVE_OFFSETS, ri.AUDIO_RUNS, ri.AUDIO_FPS, ri.AUDIO_SR, 0)
    assert np.diff(offsets).tolist() == [1920 + (128639 - 6400) + 81 + 0, 1 + 0, 533 + (21354 - 2669) + (64064 - 53386)]


# --------------------------------------------------------------------------- definitions against restatements
@pytest.mark.parametrize("name", ri.INDEX_MASKS)
def test_index_definition_equals_its_restatement(name):
    mask = ri.index_mask(name)
    host = render.summary_index_host(mask, ri.INDEX_OFFSETS)
    runs, picked = ri.index_restatement(mask, ri.INDEX_OFFSETS)
    assert host["per_video"] == runs and host["frame_index"][:len(picked)].tolist() == picked
    assert host["totals"][:, 0].tolist() == [len(r) for r in runs] and host["totals"][:, 1].sum() == len(picked)
    assert all(0 <= s < e <= n for r, n in zip(runs, ri.INDEX_LENGTHS) for s, e in r)     # no run leaves its video
    # at capacities that are too small the first entries are the same and the totals are the true counts
    cut = render.summary_index_host(mask, ri.INDEX_OFFSETS, *ri.SMALL_CAPS)
    assert np.array_equal(cut["frame_index"], np.concatenate([picked, np.full(ri.SMALL_CAPS[0], -1)])[:ri.SMALL_CAPS[0]])
    flat = np.array([r for video in runs for r in video] + [(-1, -1)] * ri.SMALL_CAPS[1], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(cut["runs"], flat[:ri.SMALL_CAPS[1]])
    assert np.array_equal(cut["totals"], host["totals"])


@pytest.mark.parametrize("fmt", ri.FORMATS)
@pytest.mark.parametrize("name", ("2x2", "6x10"))
def test_forward_definition_equals_its_restatement(fmt, name):
    bgr, L = ri.bgr_case(name), ri.dest_layout(fmt, name, len(ri.GATHER))
    sentinel = np.full((L.n, L.frame_stride), ri.SENTINEL_U8, dtype=np.uint8)
    for matrix in ("bt601", "bt709", ri.CUSTOM):
        forward = render._forward(matrix, "test")
        got = render.bgr_to_frames_host(bgr, _frames(L), matrix, ri.GATHER, into=sentinel)
        assert np.array_equal(got, ri.forward_restatement(bgr, L, forward, ri.GATHER)), (fmt, name, matrix)
    # nothing but samples is written, and the skipped rows stay
    mask = yi.sample_mask(L)
    assert (got[:, ~mask] == ri.SENTINEL_U8).all() and (got[[1, 3]] == ri.SENTINEL_U8).all()
    assert (sentinel == ri.SENTINEL_U8).all()                                            # (into is not written in place)
    # back through the ingest definition's sample reader: the samples are those of bgr_to_yuv_host
    y, u, v = render.bgr_to_yuv_host(bgr[[2, 0, 1]], ri.CUSTOM, yi.depth_of(fmt))
    ys, us, vs = yuv.yuv_samples_host(got[[0, 2, 4]], _frames(L._replace(n=3)))
    assert np.array_equal(ys, y) and np.array_equal(us[:, ::2, ::2], u) and np.array_equal(vs[:, 1::2, 1::2], v)
    assert y.max() == (255 << (yi.depth_of(fmt) - 8)) + (3 if yi.depth_of(fmt) == 10 else 0)       # the clamp at the top is reached


@pytest.mark.parametrize("mistake", ri.FORWARD_MISTAKES)
def test_planted_forward_mistakes_are_noticed(mistake):
    fmt, name = ri.NOTICED_BY[mistake]
    bgr, L = ri.bgr_case(name), ri.dest_layout(fmt, name, ri.FRAMES)
    into = np.full((L.n, L.frame_stride), ri.SENTINEL_U8, dtype=np.uint8)
    want = render.bgr_to_frames_host(bgr, _frames(L), "bt601", into=into)
    forward = render.FORWARD_MATRICES["bt601"]
    assert np.array_equal(want, ri.forward_restatement(bgr, L, forward))
    assert not np.array_equal(want, ri.forward_restatement(bgr, L, forward, mistake=mistake)), mistake


def test_planted_run_and_audio_mistakes_are_noticed():
    mask = ri.index_mask(ri.NOTICED_BY["run_across_videos"])
    want = render.summary_index_host(mask, ri.INDEX_OFFSETS)["per_video"]
    assert want == ri.index_restatement(mask, ri.INDEX_OFFSETS)[0]
    merged = ri.index_restatement(mask, ri.INDEX_OFFSETS, "run_across_videos")[0]
    assert merged != want and sum(map(len, merged)) < sum(map(len, want))
    wave, _ = ri.audio_case()
    args = (wave, ri.AUDIO_WAVE_OFFSETS, ri.AUDIO_RUNS, ri.AUDIO_FPS, ri.AUDIO_SR)
    for fade in ri.AUDIO_FADES:
        want = render.summary_audio_host(*args, fade)[0]
        got = ri.audio_restatement(*args, fade)
        assert want.dtype == got.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), fade
    # the fade taken at F instead of min(F, L // 2): the 533-, 81- and 1-sample runs are shorter than 2 * 300
    fade = ri.NOTICED_BY["fade_unclamped"]
    assert not np.array_equal(render.summary_audio_host(*args, fade)[0], ri.audio_restatement(*args, fade, "fade_unclamped"))
    assert np.array_equal(render.summary_audio_host(*args, 8)[0][:1920], ri.audio_restatement(*args, 8, "fade_unclamped")[:1920])
    # int(e / fps * sr) computed as int(e * sr / fps): e = 201 at 25 fps gives 128639 against 128640
    e, fps = ri.REORDER_WITNESS
    assert render.audio_bounds_host(e, fps, ri.AUDIO_SR, 1 << 40) == 128639
    assert int(np.floor(np.float64(e) * np.float64(ri.AUDIO_SR) / np.float64(fps))) == 128640
    assert any(e == end and ri.AUDIO_FPS[v] == fps for v, runs in enumerate(ri.AUDIO_RUNS) for _, end in runs)
    wrong = ri.audio_restatement(*args, 0, "bounds_reordered")
    assert not np.array_equal(render.summary_audio_host(*args, 0)[0][:len(wrong)], wrong)
    one_run = (((10, 201),), (), ())
    assert render.summary_audio_host(wave, ri.AUDIO_WAVE_OFFSETS, one_run, ri.AUDIO_FPS, ri.AUDIO_SR)[0].size + 1 == \
        ri.audio_restatement(wave, ri.AUDIO_WAVE_OFFSETS, one_run, ri.AUDIO_FPS, ri.AUDIO_SR, 0, "bounds_reordered").size


@pytest.mark.parametrize("pair", ri.REPACK_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_repack_definition_copies_samples(pair):
    src_fmt, dst_fmt = pair
    data, S = yi.layout_case(src_fmt, "6x10")
    D = ri.dest_layout(dst_fmt, "6x10", 4)
    into = np.full((D.n, D.frame_stride), ri.SENTINEL_U8, dtype=np.uint8)
    got = render.repack_host(data, _frames(S), _frames(D), (2, -1, 0, 1), into=into)
    assert (got[:, ~yi.sample_mask(D)] == ri.SENTINEL_U8).all() and (got[1] == ri.SENTINEL_U8).all()
    ys, us, vs = yuv.yuv_samples_host(data, _frames(S))
    yd, ud, vd = yuv.yuv_samples_host(got[[0, 2, 3]], _frames(D._replace(n=3)))
    assert np.array_equal(yd, ys[[2, 0, 1]]) and np.array_equal(ud, us[[2, 0, 1]]) and np.array_equal(vd, vs[[2, 0, 1]])
    if D.sample_bytes == 2:                                      # the spare bits of every destination word are zero
        words = got[[0, 2, 3]][:, yi.sample_mask(D)].reshape(3, -1, 2).astype(np.int64)
        words = words[..., 0] | (words[..., 1] << 8)
        assert (words & ~(1023 << D.shift) == 0).all()
    with pytest.raises(ValueError, match="depths"):
        render.repack_host(data, _frames(S), _frames(ri.dest_layout("i010" if S.sample_bytes == 1 else "i420", "6x10", 4)))


# --------------------------------------------------------------------------- round trip: facts about the two definitions
def _uniform_blocks(colours):
    """uint8 [len, 2, 2, 3]: one 2x2-uniform frame per (B, G, R)."""
    return np.broadcast_to(np.asarray(colours, dtype=np.uint8)[:, None, None, :], (len(colours), 2, 2, 3))


def _round_trip(bgr, name, depth):
    y, u, v = render.bgr_to_yuv_host(bgr, name, depth)
    back = yuv.yuv_to_bgr_host(y, np.repeat(np.repeat(u, 2, -1), 2, -2), np.repeat(np.repeat(v, 2, -1), 2, -2), name, depth)
    return y, u, v, np.abs(back.astype(np.int64) - bgr).max()


@pytest.mark.parametrize("name", ("bt601", "bt709"))
def test_round_trip_through_the_ingest_definition(name):
    assert render.FORWARD_MATRICES[name] == ISSUE_INTEGERS[name]
    assert render.FORWARD_MATRICES[name][1:] == tuple(int(np.rint(c * 2 ** 20)) for c in render.FORWARD_MATRICES_F64[name][1:])
    assert max(sum(abs(c) for c in render.FORWARD_MATRICES[name][1 + 3 * r:4 + 3 * r]) for r in range(3)) <= 921698 < 1 << 20
    greys = _uniform_blocks([(g, g, g) for g in range(256)])
    y, u, v, worst = _round_trip(greys, name, 8)
    assert (u == 128).all() and (v == 128).all() and y.min() == 16 and y.max() == 235 and worst <= 1
    levels = list(range(0, 255, 5)) + [255]
    assert len(levels) == 52
    lattice = _uniform_blocks(np.stack(np.meshgrid(levels, levels, levels, indexing="ij"), -1).reshape(-1, 3))
    assert _round_trip(lattice, name, 8)[3] <= 2
    assert _round_trip(lattice, name, 10)[3] <= 1
