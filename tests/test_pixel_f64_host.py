"""Host checks of the references, restatements and bounds test_gpu_pixel_f64.py holds the uint8 pixel kernels to (no GPU):

  * oracle.cnn.cv_resize_linear_u8 equals the 32-bit restatement and lies within the derived ``resize_bound`` of the
    float64 definition at every case the device tests run; oracle.shots.bgr2hsv_u8 equals its restatement and lies within
    the derived HSV bounds on all 2^24 colours;
  * every planted mistake is noticed at the case NOTICED_BY names, the ‡ resize mistakes (REFERENCE_CATCHES) by the
    float64 reference alone; the "mistakes" of INERT change no byte at any case, so they are not planted;
  * the launch constants the cases rely on stand in the source text of their launchers, and the cases reach the second
    grid-stride trip, several workgroups per frame and a halved band;
  * the refusals that need no device hold.

Measured here (the asserts below hold them):
  resize   largest |oracle - float64 definition| over 12 pairs x 4 contents x 3 frames: 0.8026 grey levels, of a bound
           of 0.8818 + 1.5e-5 (sh + sw + 1) (0.8904 at 240 x 320); smallest excess of a ‡ mistake over the bound at its
           case: 0.40 levels (plus2_dropped, 240 x 320 -> 224 x 224 noise; the others exceed it by 58 or more)
  HSV      over all 2^24 colours V exact, largest |S - definition| 0.5215 of a bound of 0.5311, largest circular
           |H - definition| 0.6400 of 0.6556"""
import re
from pathlib import Path

import numpy as np
import pytest

import pixel_f64_inputs as pfi
from oracle import cnn as ocnn, shots as osh

F32 = np.float32
ARG, SHAPE, ALIGN = -1, -2, -3      # AVS_E_ARG, AVS_E_SHAPE, AVS_E_ALIGN
CSRC = Path(__file__).resolve().parent.parent / "audiovidsum-a-multi-modal-approach-to-video-summarization_amd" / "csrc"


def _oracle_resize(frames, dh, dw):
    return np.stack([ocnn.cv_resize_linear_u8(f, dh, dw) for f in frames])


# --------------------------------------------------------------------------- resize
def test_resize_oracle_equals_the_restatement_and_lies_within_the_bound():
    """Measured: the oracle's largest distance from the float64 definition is 0.8026 levels (37 x 53 -> 36 x 300, noise)."""
    worst = 0.0
    for (sh, sw), (dh, dw) in pfi.RESIZE_PAIRS:
        for dn, sn in ((dh, sh), (dw, sw)):
            s0, s1, c0, c1 = pfi.resize_coefs(dn, sn)
            assert ((c0 + c1) == 2048).all() and (s0 >= 0).all() and (s1 <= sn - 1).all()     # step 2 of the derivation
        for content in pfi.CONTENTS:
            frames = pfi.resize_case((sh, sw), content)
            ref = pfi.resize_reference(frames, dh, dw)
            got = _oracle_resize(frames, dh, dw)
            assert ref.shape == got.shape == (pfi.RESIZE_FRAMES, dh, dw, 3)
            assert np.array_equal(got, pfi.resize_restatement(frames, dh, dw)), ((sh, sw), (dh, dw), content)
            dist = float(np.abs(got - ref).max())
            assert dist <= pfi.resize_bound(sh, sw), ((sh, sw), (dh, dw), content, dist)
            worst = max(worst, dist)
    assert 0.80 < worst < 0.81                      # the bound (0.88) is neither slack nor tight
    big = pfi.RESIZE_BIG
    frames = pfi.resize_case(big.src, "noise", big.base)
    assert np.abs(_oracle_resize(frames, *big.dst) - pfi.resize_reference(frames, *big.dst)).max() <= pfi.resize_bound(*big.src)


def test_the_reference_is_a_bilinear_resize():
    """Known answers of the definition itself: a constant stays, an identity stays, an exact 2 x downscale is the mean of
    the 2 x 2 block, a ramp is resampled linearly away from the clamps, and an upscale repeats the edge beyond the last
    centres."""
    const = np.full((1, 5, 7, 3), 93, dtype=np.uint8)
    assert (pfi.resize_reference(const, 11, 3) == 93.0).all()
    noise = pfi.resize_case((64, 64), "noise")
    assert np.array_equal(pfi.resize_reference(noise, 64, 64), noise.astype(np.float64))
    x = pfi.resize_case((8, 12), "noise")[:1].astype(np.float64)
    want = (x[:, 0::2, 0::2] + x[:, 1::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 1::2]) / 4
    assert np.abs(pfi.resize_reference(x, 4, 6) - want).max() < 1e-12
    ramp = (np.arange(10.0)[None, None, :, None] * 20 + np.zeros((1, 1, 10, 3)))
    up = pfi.resize_reference(ramp, 1, 40)[0, 0, :, 0]
    assert np.allclose(up[2:38], 20 * ((np.arange(2, 38) + 0.5) / 4 - 0.5)) and (up[:2] == 0).all() and (up[38:] == 180).all()


RESIZE_PLANTED = [m for m in pfi.RESIZE_MISTAKES if m not in pfi.INERT]


@pytest.mark.parametrize("mistake", RESIZE_PLANTED)
def test_resize_mistakes_are_noticed(mistake):
    """Measured excess over the bound at the named case: no_half_pixel 58.96, clamp_at_smax_s1_unclamped 149.1,
    plus2_dropped 0.40, scale_swapped 216.0 levels; coef_truncated, clamp_at_smax and shift4_skipped are held by the bit
    comparison (shift4_skipped does NOT overflow 32 bits: 255 * 2^11 * 2^11 < 2^31 - it is 16 times too bright)."""
    pair, content = pfi.NOTICED_BY[mistake]
    assert pair in pfi.RESIZE_PAIRS and content in pfi.CONTENTS
    (sh, sw), (dh, dw) = pair
    frames = pfi.resize_case((sh, sw), content)
    wrong = pfi.resize_restatement(frames, dh, dw, mistake)
    assert (wrong != pfi.resize_restatement(frames, dh, dw)).any()
    excess = float(np.abs(wrong - pfi.resize_reference(frames, dh, dw)).max()) - pfi.resize_bound(sh, sw)
    if mistake in pfi.REFERENCE_CATCHES:
        assert excess >= 0.40, (mistake, excess)
        if mistake == "scale_swapped":
            assert sh * dw != sw * dh                # a non-square pair: the two scales differ
    if mistake == "shift4_skipped":
        assert int(frames.max()) * 2048 * 2048 < 2 ** 31 and excess > 100


def test_inert_mistakes_change_nothing():
    """s1 left unclamped reads past the row only where its weight is 0: no byte differs at any case.  (g_before_r: the
    sweep over all colours below.)"""
    assert set(pfi.INERT) == {"s1_unclamped", "g_before_r"}
    for (sh, sw), (dh, dw) in pfi.RESIZE_PAIRS:
        for dn, sn in ((dh, sh), (dw, sw)):
            s0, s1, c0, c1 = pfi.resize_coefs(dn, sn, mistake="s1_unclamped")
            assert (c1[s1 > sn - 1] == 0).all()
        for content in pfi.CONTENTS:
            frames = pfi.resize_case((sh, sw), content)
            assert np.array_equal(pfi.resize_restatement(frames, dh, dw, "s1_unclamped"), pfi.resize_restatement(frames, dh, dw))


# --------------------------------------------------------------------------- HSV
def test_hsv_oracle_within_the_bounds_on_all_colours():
    """All 2^24 colours, one blue value per slab.  Measured: V exact; largest |S - definition| 0.5215 of a bound of
    0.5311; largest circular |H - definition| 0.6400 of 0.6556.  The restatement equals the oracle, and taking the
    v == g branch before v == r changes no value (INERT)."""
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst_s = worst_h = 0.0
    for b in range(256):
        slab = np.stack([np.full_like(g, b), g, r], -1)
        got = osh.bgr2hsv_u8(slab)
        h, s, v = pfi.hsv_restatement(slab)
        assert np.array_equal(got[..., 0], h) and np.array_equal(got[..., 1], s) and np.array_equal(got[..., 2], v)
        assert h.min() >= 0 and h.max() < 180 and s.max() <= 255
        for a, c in zip(pfi.hsv_restatement(slab, "g_before_r"), (h, s, v)):
            assert np.array_equal(a, c)
        rh, rs, rv = pfi.hsv_reference(slab)
        assert np.array_equal(v, rv)
        worst_s = max(worst_s, float(np.abs(s - rs).max()))
        worst_h = max(worst_h, float(pfi.circular(h, rh).max()))
    assert worst_s <= pfi.HSV_S_BOUND and worst_h <= pfi.HSV_H_BOUND
    assert worst_s > 0.52 and worst_h > 0.63        # the bounds are not slack


def test_hsv_known_answers_of_the_definition():
    px = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [7, 7, 7], [0, 0, 0], [255, 0, 255], [1, 0, 255]],
                  dtype=np.uint8)
    h, s, v = pfi.hsv_reference(px)
    assert h[:7].tolist() == [0, 60, 120, 30, 0, 0, 150] and s[:7].tolist() == [255, 255, 255, 255, 0, 0, 255]
    assert v.tolist() == [255, 255, 255, 255, 7, 0, 255, 255] and abs(h[7] - (180 - 30 / 255)) < 1e-12     # just below 180


def test_hsv_sums_restatement_equals_the_oracle():
    for size in pfi.HSV_SIZES[:4]:
        frames = pfi.hsv_case(size)
        for step in pfi.HSV_STEPS:
            hsv = [osh.bgr2hsv_u8(f[::step, ::step]).astype(np.int64) for f in frames]
            want = np.zeros((len(frames), 3), dtype=np.int64)
            for i in range(1, len(frames)):
                want[i] = np.abs(hsv[i] - hsv[i - 1]).reshape(-1, 3).sum(0)
            assert np.array_equal(pfi.hsv_sums(frames, step), want)
            cut = pfi.hsv_sums(frames, step, pfi.HSV_VIDEOS)
            starts = list(pfi.HSV_VIDEOS[:-1])
            assert not cut[starts].any() and np.array_equal(np.delete(cut, starts, 0), np.delete(want, starts, 0))


@pytest.mark.parametrize("mistake", [m for m in pfi.HSV_MISTAKES if m not in pfi.INERT])
def test_hsv_mistakes_are_noticed(mistake):
    size, step = pfi.NOTICED_BY[mistake]
    assert size in pfi.HSV_SIZES and step in pfi.HSV_STEPS
    frames = pfi.hsv_case(size)
    good = pfi.hsv_sums(frames, step, pfi.HSV_VIDEOS)
    wrong = pfi.hsv_sums(frames, step, pfi.HSV_VIDEOS, mistake)
    assert (wrong != good).any()
    if mistake == "prev_across_videos":
        assert (wrong[list(pfi.HSV_VIDEOS[1:-1])] != 0).all()
    if mistake == "last_workgroup_dropped":
        rows = [2, 4, 5, 7]                                  # the frames with a predecessor in their video
        assert pfi.hsv_grid(*size, step)[1] == 2 and (0 < wrong[rows]).all() and (wrong[rows] < good[rows]).all()
    if mistake == "step_rows_only":
        assert step > 1 and size[1] % step


# --------------------------------------------------------------------------- normalise
def _norm_cases():
    return [(aff, denom, pad) for aff in (False, True) for denom in (255.0, 1.0) for pad in pfi.NORM_PADS]


def test_normalize_restatement_within_compare_of_float64():
    frames = pfi.norm_case()
    for c in range(3):
        assert set(frames[0, ..., c].ravel().tolist()) == set(range(256))        # every byte value in every channel
    for aff, denom, (pt, pl) in _norm_cases():
        oh, ow = pfi.norm_geometry(pt, pl)
        assert oh > pfi.NORM_SRC[0] + pt and ow > pfi.NORM_SRC[1] + pl and ow % 2 == 0
        args = (frames, denom, pfi.NORM_AFFINE if aff else None, oh, ow, pt, pl)
        r32, r64 = pfi.normalize_eval(*args), pfi.normalize_eval(*args, dtype=np.float64)
        assert r32.dtype == F32 and r64.dtype == np.float64
        ok, err, e32, bound = pfi.compare(r32, r64, r64.astype(F32))
        assert ok, (aff, denom, pt, pl, err, bound)
        assert (r32[:, :pt] == 0).all() and (r32[:, :, :pl] == 0).all() and (r32[..., 3] == 0).all()
        assert (r32[:, pt + pfi.NORM_SRC[0]:] == 0).all() and (r32[:, :, pl + pfi.NORM_SRC[1]:] == 0).all()
    # the float64 form is the definition: one pixel by hand
    mean, std = pfi.NORM_STATS[255.0]
    v = float(frames[0, 0, 0, 1])
    want = (v / 255.0 - float(F32(mean[1]))) / float(F32(std[1])) * float(F32(pfi.NORM_AFFINE[1])) + float(F32(pfi.NORM_AFFINE[4]))
    got = pfi.normalize_eval(frames, 255.0, pfi.NORM_AFFINE, *pfi.norm_geometry(2, 3), 2, 3, dtype=np.float64)[0, 2, 3, 1]
    assert abs(got - want) < 1e-15


@pytest.mark.parametrize("mistake", pfi.NORM_MISTAKES)
def test_normalize_mistakes_are_noticed(mistake):
    aff, denom, (pt, pl) = pfi.NOTICED_BY[mistake]
    assert (aff, denom, (pt, pl)) in _norm_cases()
    oh, ow = pfi.norm_geometry(pt, pl)
    args = (pfi.norm_case(), denom, pfi.NORM_AFFINE if aff else None, oh, ow, pt, pl)
    good = pfi.normalize_eval(*args)
    if mistake.startswith("h2_"):
        base, wrong = pfi.h2_words(good), pfi.h2_words(good, mistake)
        assert (wrong != base).any()
        if mistake == "h2_lo_from_pixel0":
            assert (wrong[:, 0] == base[:, 0]).all()         # only the lo halves: invisible to a comparison at fp16 precision
            assert pl % 2 == 1                               # a pair that straddles the image's left edge
    else:
        wrong = pfi.normalize_eval(*args, mistake=mistake)
        assert (wrong.view(np.int32) != good.view(np.int32)).any()
        r64 = pfi.normalize_eval(*args, dtype=np.float64)
        assert not pfi.compare(wrong, r64, r64.astype(F32))[0]           # and the float64 reference alone catches it


# --------------------------------------------------------------------------- pull copy
def _pull_cases():
    return [(wg, k, tail) for wg in pfi.PULL_WORKGROUPS for k in range(8) for tail in pfi.PULL_TAILS] + \
        [(pfi.PULL_BIG_WORKGROUPS, 6, tail) for tail in pfi.PULL_TAILS[:1]]


def test_pull_copy_restatement_copies_every_unit_once():
    for wg, k, tail in _pull_cases():
        n16 = pfi.pull_units(wg)[k]
        src = pfi.pull_source(n16 * 16 + tail)
        dst, copies = pfi.pull_copy_restatement(src, wg)
        assert np.array_equal(dst, src) and (copies == 1).all(), (wg, k, tail)


@pytest.mark.parametrize("mistake", pfi.PULL_MISTAKES)
def test_pull_copy_mistakes_are_noticed(mistake):
    wg, k, tail = pfi.NOTICED_BY[mistake]
    assert (wg, k, tail) in _pull_cases()
    src = pfi.pull_source(pfi.pull_units(wg)[k] * 16 + tail)
    assert (pfi.pull_copy_restatement(src, wg, mistake)[0] != src).any()


# --------------------------------------------------------------------------- launch constants and reach
def _launcher(text, name):
    """The body of the extern "C" entry point ``name``."""
    m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", text, re.S)
    assert m, name
    return m.group(0)


def test_launch_constants_match_the_sources():
    visual, stage1, shots = ((CSRC / f).read_text() for f in ("visual.hip", "stage1_batch.hip", "shots_batch.hip"))
    capped = f"avs_cdiv(total, {pfi.THREADS}) < {pfi.GRID_CAP} ? avs_cdiv(total, {pfi.THREADS}) : {pfi.GRID_CAP}"
    resize, norm = _launcher(visual, "avs_resize_bilinear_u8"), _launcher(visual, "avs_frames_normalize_u8")
    assert capped in resize and f"dim3(grid), dim3({pfi.THREADS})" in resize
    assert capped in norm and f"dim3(grid < {pfi.GRID_CAP_H2} ? grid : {pfi.GRID_CAP_H2}), dim3({pfi.THREADS})" in norm
    assert norm.count(f"dim3(grid), dim3({pfi.THREADS})") == 2                  # fp32 and bf16
    hsv = _launcher(visual, "avs_hsv_frame_diff_u8")
    assert pfi.HSV_WG_PIXELS == 256 * 8 and "avs_cdiv((long long)ph * pw, 256 * 8)" in hsv
    assert f"if (bx > {pfi.HSV_WG_CAP}) bx = {pfi.HSV_WG_CAP};" in hsv and f"dim3(bx, n - 1), dim3({pfi.THREADS})" in hsv
    assert f"n - 1 <= {pfi.HSV_MAX_FRAMES - 1}" in hsv
    assert hsv.index("n - 1 <= 65535") < hsv.index("hipMemsetAsync")            # a refused call writes nothing
    batch = _launcher(shots, "avs_hsv_frame_diff_batch_u8")
    assert f"#define SB_THREADS {pfi.THREADS}\n" in shots and "avs_cdiv((long long)ph * pw, SB_THREADS * 8)" in batch
    assert f"if (by > {pfi.HSV_WG_CAP}) by = {pfi.HSV_WG_CAP};" in batch
    assert f"#define RG_THREADS {pfi.RG_THREADS}\n" in stage1 and re.search(rf"#define RG_BAND {pfi.RG_BAND}\s", stage1)
    assert pfi.RG_LDS_BYTES == 64 * 1024 and re.search(r"#define RG_LDS_BYTES \(64 \* 1024\)\s", stage1)
    gather = _launcher(stage1, "avs_resize_bilinear_gather2_u8")
    assert "dim3((unsigned)count, (unsigned)bands, (unsigned)ndst), dim3(RG_THREADS), lds" in gather
    pull = _launcher(visual, "avs_pull_copy_u8")
    assert f"workgroups <= {pfi.PULL_MAX_WORKGROUPS}" in pull and f"dim3((unsigned)workgroups), dim3({pfi.THREADS})" in pull
    assert "const long long stride = (long long)gridDim.x * 256;" in visual and "i + 3 * stride < n16; i += 4 * stride" in visual


def test_the_pixel_arithmetic_has_one_text():
    """The resize arithmetic and the shot scan stand once, in pixel_bodies.h, and the kernels call them: no file of csrc/
    holds a copy of its own.  (Sharing took csrc/ from 13 310 lines to 13 275; the count is not asserted, since the next
    kernel added there would trip it.)"""
    sources = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.is_file()}
    once = {"source position": r"\(d \+ 0\.5\) \* scale - 0\.5", "blend": r">> 16\) \+ 2\) >> 2",
            "wave reduction": r"__shfl_xor\(a0", "stage_out": r"^[^/\n]*\bvoid \w*stage_out\("}
    for what, pattern in once.items():
        found = {name: len(re.findall(pattern, text, flags=re.M)) for name, text in sources.items()}
        assert {name: n for name, n in found.items() if n} == {"pixel_bodies.h": 1}, (what, found)
    hips = ("visual.hip", "stage1_batch.hip", "shots_batch.hip", "ingest.hip")
    assert all('#include "pixel_bodies.h"' in sources[f] for f in hips)
    assert sources["pixel_bodies.h"].count("#pragma once") == 1 and '#include "avs_internal.h"' in sources["pixel_bodies.h"]
    assert all(re.search(r"\bcv_blend\(", sources[f]) for f in ("visual.hip", "stage1_batch.hip", "ingest.hip"))
    assert all(len(re.findall(r"\bhsv_diff_body<", sources[f])) == 1 for f in ("visual.hip", "shots_batch.hip", "ingest.hip"))
    for name, plan in (("stage1_batch.hip", "rg_plan"), ("ingest.hip", "ni_plan")):
        body = re.search(r"^static size_t " + plan + r"\(.*?\n}\n", sources[name], flags=re.S | re.M)
        assert body and "cv_band_rows(" in body.group(0), plan
    # nothing in the header has external linkage: every function at file scope is force-inlined
    starts = [ln for ln in sources["pixel_bodies.h"].splitlines() if "(" in ln and re.match(r"[A-Za-z_]", ln)]
    assert len(starts) >= 8 and all(re.match(r"(__host__ )?__device__ __forceinline__ ", ln) for ln in starts), starts


def test_the_cases_reach_every_path():
    # resize: one trip at every pair, the second at the 65 537-frame case and not one frame earlier
    big = pfi.RESIZE_BIG
    px = big.dst[0] * big.dst[1]
    assert pfi.grid_trips(big.frames * px, pfi.GRID_CAP) == (pfi.GRID_CAP, 2)
    assert pfi.grid_trips((big.frames - 1) * px, pfi.GRID_CAP) == (pfi.GRID_CAP, 1) and big.frames * px * 3 < 14_000_000
    assert all(pfi.grid_trips(pfi.RESIZE_FRAMES * dh * dw, pfi.GRID_CAP)[1] == 1 for _, (dh, dw) in pfi.RESIZE_PAIRS)
    # gather: the band of each destination; halved where 8 output rows need more than 64 KiB of LDS
    bands = {pair: pfi.gather_plan(*pair[0], *pair[1])[0] for pair in pfi.RESIZE_PAIRS}
    second = {pair: pfi.gather_plan(*pair[0], *pfi.GATHER_SECOND)[0] for pair in pfi.RESIZE_PAIRS}
    assert {p for p, b in bands.items() if b < pfi.RG_BAND} == {((20, 2200), (16, 40))} and bands[((20, 2200), (16, 40))] == 4
    assert {p[0]: b for p, b in second.items() if b < pfi.RG_BAND} == {(240, 320): 2, (20, 2200): 2}
    assert min(bands.values()) >= 1 and min(second.values()) >= 1
    spans = {pair: pfi.gather_plan(*pair[0], *pair[1])[2] for pair in pfi.RESIZE_PAIRS}
    assert spans[((1, 1), (3, 5))] == spans[((1, 9), (4, 20))] == 1           # a band that reads a single source row
    assert spans[((150, 11), (16, 9))] > 64                                   # 8 output rows over more than 64 source rows
    dws = {dw for _, (_, dw) in pfi.RESIZE_PAIRS}
    assert min(dws) == 1 and max(dws) > 256 and any(dh < 8 for _, (dh, _) in pfi.RESIZE_PAIRS) and pfi.GATHER_SECOND[1] == 65
    assert pfi.GATHER_INDEX[pfi.GATHER_SKIPPED] == pfi.RESIZE_FRAMES and pfi.GATHER_INDEX[:4] == (2, 2, 1, 0)
    # HSV: (strided pixels, workgroups, trips).  A frame takes cdiv(pixels, 2048) workgroups, 64 at the most, so the pixel
    # loop runs up to 8 trips below 131 072 strided pixels and more beyond
    grids = {(size, step): pfi.hsv_grid(*size, step) for size in pfi.HSV_SIZES for step in pfi.HSV_STEPS}
    assert grids[((1, 1), 1)] == (1, 1, 1) and grids[((1, 300), 1)] == (300, 1, 2) and grids[((1, 300), 3)] == (100, 1, 1)
    assert grids[((130, 127), 1)] == (16510, 9, 8) and grids[((47, 45), 1)] == (2115, 2, 5)      # 67 pixels in workgroup 1's
    assert grids[((47, 45), 2)] == (552, 1, 3) and grids[((130, 127), 3)] == (1892, 1, 8)        # ... first trip past 2048
    assert grids[((363, 364), 1)] == (132132, 64, 9)                                              # the cap, and a ninth trip
    assert pfi.hsv_grid(256, 256, 1) == (65536, 32, 8)
    assert {g[1] for g in grids.values()} >= {1, 2, 3, 8, 9, 17, 64}
    assert all(size[0] % step or size[1] % step for size in pfi.HSV_SIZES[2:] for step in (2, 3))     # a cut last row or column
    assert pfi.HSV_VIDEOS == (0, 1, 3, 6, 8) and pfi.HSV_FRAMES == 8
    # normalise: one trip at every geometry; the second with 2 x 2 frames into 4 x 4
    for fmt, frames in pfi.NORM_BIG.items():
        items, cap = (frames * 4 * 2, pfi.GRID_CAP_H2) if fmt == "f16x2" else (frames * 16, pfi.GRID_CAP)
        per = items // frames
        assert pfi.grid_trips(items, cap) == (cap, 2) and pfi.grid_trips(items - per, cap) == (cap, 1)
        assert frames * 16 * 4 * (2 if fmt == "bf16" else 4) < 100_000_000
    assert {pl % 2 for _, pl in pfi.NORM_PADS} == {0, 1} and pfi.NORM_SRC[1] % 2 == 1
    # pull copy: (trips of the 4-way loop, trips of the remainder loop) of thread 0 and of the last thread
    def walk(t, n16, s):
        i = t4 = rem = 0
        i = t
        while i + 3 * s < n16:
            i, t4 = i + 4 * s, t4 + 1
        while i < n16:
            i, rem = i + s, rem + 1
        return t4, rem

    for wg in pfi.PULL_WORKGROUPS:
        s = pfi.THREADS * wg
        units = pfi.pull_units(wg)
        assert [walk(0, n16, s) for n16 in units] == [(0, 0), (0, 1), (0, 1), (0, 3), (1, 0), (1, 0), (1, 1), (2, 0)], wg
        assert [walk(s - 1, n16, s) for n16 in units] == [(0, 0), (0, 0), (0, 0), (0, 3), (0, 3), (1, 0), (1, 0), (1, 3)], wg
    assert (4 * pfi.THREADS * pfi.PULL_BIG_WORKGROUPS + 1) * 16 < 17_000_000


# --------------------------------------------------------------------------- refusals: nothing is launched
A = 1 << 20         # a 256-byte aligned non-null address; never read: every call below returns before any HIP call


def _lib():
    from avsum_amd import _abi
    return _abi.lib(), _abi


def test_refusals_launch_nothing():
    import ctypes
    lib, abi = _lib()
    unsupported = abi.E_UNSUPPORTED
    rs = lib.avs_resize_bilinear_u8
    assert rs(A, -1, 4, 4, A, 4, 4, None) == SHAPE and rs(A, 1, 0, 4, A, 4, 4, None) == SHAPE
    assert rs(A, 1, 4, 4, A, 4, 0, None) == SHAPE and rs(None, 1, 4, 4, A, 4, 4, None) == ARG
    assert rs(None, 0, 4, 4, None, 4, 4, None) == 0
    rg = lib.avs_resize_bilinear_gather2_u8
    assert rg(A, 2, 4, 4, A, 1, A, 0, 4, None, 0, 0, None) == SHAPE and rg(A, 2, 4, 4, A, -1, A, 4, 4, None, 0, 0, None) == SHAPE
    assert rg(A, 2, 4, 4, A, 1, A, 4, 4, A, 4, 0, None) == SHAPE                     # the second size, where it is given
    assert rg(A, 2, 4, 65536, A, 1, A, 4, 4, None, 0, 0, None) == unsupported        # the 16-bit column table
    assert rg(A, 2, 4, 4, A, 1, A, 65536, 4, None, 0, 0, None) == unsupported        # the bands on grid y
    assert rg(A, 2, 4, 12000, A, 1, A, 4, 4, None, 0, 0, None) == unsupported        # two source rows: 72 000 bytes of LDS
    assert rg(A, 2, 4, 4, None, 1, A, 4, 4, None, 0, 0, None) == ARG and rg(None, 2, 4, 4, None, 0, None, 4, 4, None, 0, 0, None) == 0
    hs = lib.avs_hsv_frame_diff_u8
    assert hs(A, pfi.HSV_MAX_FRAMES + 1, 1, 1, 1, A, None) == SHAPE and b"65536 frames" in lib.avs_last_error()
    assert hs(A, 2, 4105, 4105, 1, A, None) == SHAPE and b"too large" in lib.avs_last_error()      # 4105^2 * 255 >= 2^32
    assert 4104 * 4104 * 255 < 2 ** 32 <= 4105 * 4105 * 255
    assert hs(A, 2, 4, 4, 0, A, None) == SHAPE and hs(A, 2, 4, 4, 1, None, None) == ARG and hs(None, 0, 4, 4, 1, None, None) == 0
    hb = lib.avs_hsv_frame_diff_batch_u8
    assert hb(A, 2, 4105, 4105, 1, A, 1, A, None) == SHAPE and hb(A, 2, 4, 4, 1, A, 0, A, None) == SHAPE
    assert hb(A, 2, 4, 4, 1, None, 1, A, None) == ARG and hb(None, 0, 4, 4, 1, None, 0, None, None) == 0
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def nm(dtype=0, src=A, n=1, h=4, w=4, denom=255.0, mean=f3, std=f3, out=A, oh=4, ow=4, pt=0, pl=0):
        return lib.avs_frames_normalize_u8(dtype, src, n, h, w, denom, mean, std, None, out, oh, ow, pt, pl, None)

    assert nm(dtype=7) == ARG and nm(dtype=abi.AVS_F16X2, ow=5) == ALIGN and nm(dtype=abi.AVS_F16X2, out=A + 16) == ALIGN
    assert nm(oh=3) == SHAPE and nm(ow=4, pl=1) == SHAPE and nm(pt=-1) == SHAPE and nm(n=-1) == SHAPE
    assert nm(denom=0.0) == ARG and nm(mean=None) == ARG and nm(src=None) == ARG and nm(n=0, src=None, out=None) == 0
    pc = lib.avs_pull_copy_u8
    assert pc(A, A, 64, 0, None) == SHAPE and pc(A, A, 64, pfi.PULL_MAX_WORKGROUPS + 1, None) == SHAPE and pc(A, A, -1, 1, None) == SHAPE
    assert pc(A + 1, A, 64, 1, None) == ALIGN and pc(A, A + 8, 64, 1, None) == ALIGN and pc(None, A, 64, 1, None) == ARG
    assert pc(None, None, 0, 1, None) == 0
