"""The summary-rendering kernels on the GPU (libavsum_render.so through avsum_amd/render.py), bit for bit against
render.py's numpy definitions: the index (frame list, runs, offsets, totals) at the tile edges and at capacities that are
too small; BGR -> YUV 4:2:0 into every committed layout of every format, off every alignment, and on every (B, G, R);
the repack between every ordered pair of same-depth formats; the audio cut with clamped, empty and one-sample runs and
three fades; and the pipeline's render_device end to end.  Cases come from render_inputs.py, which test_render_host.py
checks on the host."""
import ctypes

import numpy as np
import pytest
import torch

import render_inputs as ri
import yuv_inputs as yi

pytestmark = pytest.mark.gpu

FILL = 7                      # what destinations hold before a launch
GUARD = 8                     # sentinel entries after every buffer


def _yuv_frames(dev, L, data=None, base_offset=0, fill=ri.SENTINEL_U8):
    """YuvFrames of Layout L on the device, its first byte ``base_offset`` bytes into an allocation: holding ``data``
    (numpy [n, frame_stride]) or ``fill`` in every byte."""
    from avsum_amd.yuv import YuvFrames
    flat = torch.full((L.n * L.frame_stride + base_offset,), fill, dtype=torch.uint8, device=dev)
    view = flat[base_offset:].view(L.n, L.frame_stride)
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data)))
    return YuvFrames(view, L.h, L.w, **yi.fields(L))


def _bgr(dev, bgr, base_offset=0):
    flat = torch.zeros(bgr.size + base_offset, dtype=torch.uint8, device=dev)
    view = flat[base_offset:].view(bgr.shape)
    view.copy_(torch.from_numpy(np.array(bgr)))
    return view


# --------------------------------------------------------------------------- index
def _guarded(dev, entries, dtype=torch.int64):
    return torch.full((entries + GUARD,), -77, dtype=dtype, device=dev)


def _index_raw(dev, mask, tables):
    """avsr_summary_index into buffers with GUARD sentinel entries after each; returns them as numpy, guards included."""
    from avsum_amd import _render_abi
    from avsum_amd.ops import _p, _stream
    nv = tables.nvideos
    bufs = {"work": _guarded(dev, 2 * tables.ntiles), "frame_index": _guarded(dev, tables.frame_cap),
            "frame_offsets": _guarded(dev, nv + 1), "runs": _guarded(dev, 2 * tables.run_cap),
            "run_offsets": _guarded(dev, nv + 1), "totals": _guarded(dev, 3 * nv)}
    _render_abi.check(_render_abi.lib().avsr_summary_index(
        _p(mask), tables.frames, tables.offsets.ctypes.data_as(ctypes.c_void_p), _p(tables.offsets_t), nv, _p(tables.tiles_t),
        tables.ntiles, _p(bufs["work"]), _p(bufs["frame_index"]), tables.frame_cap, _p(bufs["frame_offsets"]), _p(bufs["runs"]),
        tables.run_cap, _p(bufs["run_offsets"]), _p(bufs["totals"]), _stream()), "avsr_summary_index")
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _check_index(raw, want, tables):
    nv = tables.nvideos
    for name, entries in (("work", 2 * tables.ntiles), ("frame_index", tables.frame_cap), ("frame_offsets", nv + 1),
                          ("runs", 2 * tables.run_cap), ("run_offsets", nv + 1), ("totals", 3 * nv)):
        assert (raw[name][entries:] == -77).all() and raw[name].size == entries + GUARD, name     # the sentinels stay
    assert np.array_equal(raw["frame_index"][:tables.frame_cap], want["frame_index"])            # -1 past the count
    assert np.array_equal(raw["runs"][:2 * tables.run_cap].reshape(-1, 2), want["runs"])
    assert np.array_equal(raw["frame_offsets"][:nv + 1], want["frame_offsets"])
    assert np.array_equal(raw["run_offsets"][:nv + 1], want["run_offsets"])
    assert np.array_equal(raw["totals"][:3 * nv].reshape(nv, 3), want["totals"])


@pytest.mark.parametrize("name", ri.INDEX_MASKS)
def test_index_at_the_tile_edges(dev, name):
    """Videos of 1, TILE - 1, TILE, TILE + 1 and 2 TILE + 3 frames in one batch."""
    from avsum_amd import ops, render
    mask = ri.index_mask(name)
    tables = ops.RenderTables(ri.INDEX_OFFSETS, device=dev)
    want = render.summary_index_host(mask, ri.INDEX_OFFSETS, tables.frame_cap, tables.run_cap)
    mask_t = torch.from_numpy(np.array(mask)).to(dev)
    _check_index(_index_raw(dev, mask_t, tables), want, tables)
    # the wrapper, and its one download
    index = render.summary_index(mask_t, tables)
    assert np.array_equal(index.frame_index.cpu().numpy(), want["frame_index"]) and int(index.count.item()) == int(mask.sum())
    host = index.host()
    assert host["runs"] == want["per_video"] and host["frames"].tolist() == want["totals"][:, 1].tolist()
    assert host["run_counts"].tolist() == want["totals"][:, 0].tolist() and index.host() is host


def test_index_capacities_too_small(dev):
    """The first ``cap`` entries are right, nothing beyond is written, totals holds the true counts, host() raises."""
    from avsum_amd import ops, render
    mask = ri.index_mask("alternating")
    tables = ops.RenderTables(ri.INDEX_OFFSETS, *ri.SMALL_CAPS, device=dev)
    want = render.summary_index_host(mask, ri.INDEX_OFFSETS, *ri.SMALL_CAPS)
    assert want["totals"][:, 1].sum() > ri.SMALL_CAPS[0] and want["totals"][:, 0].sum() > ri.SMALL_CAPS[1]
    assert (want["frame_index"] >= 0).all() and (want["runs"] >= 0).all()
    mask_t = torch.from_numpy(np.array(mask)).to(dev)
    _check_index(_index_raw(dev, mask_t, tables), want, tables)
    with pytest.raises(RuntimeError, match="exceed the capacities"):
        render.summary_index(mask_t, tables).host()
    # one capacity at a time
    for caps in ((ri.SMALL_CAPS[0], None), (None, ri.SMALL_CAPS[1])):
        tables = ops.RenderTables(ri.INDEX_OFFSETS, *caps, device=dev)
        _check_index(_index_raw(dev, mask_t, tables), render.summary_index_host(mask, ri.INDEX_OFFSETS, tables.frame_cap, tables.run_cap),
                     tables)


def test_index_wrapper_refusals(dev):
    from avsum_amd import ops, render
    tables = ops.RenderTables(ri.E2E_OFFSETS, device=dev)
    n = ri.E2E_OFFSETS[-1]
    for bad in (torch.zeros(n, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.uint8, device=dev),
                torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros((2, n), dtype=torch.uint8, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            render.summary_index(bad, tables)
    with pytest.raises(ValueError, match="row"):
        render.summary_index(torch.zeros((2, n), dtype=torch.uint8, device=dev), tables, row=2)
    with pytest.raises(ValueError):
        render.summary_index(torch.zeros(n, dtype=torch.uint8, device=dev), ops.RenderTables(ri.E2E_OFFSETS, device="cpu"))


# --------------------------------------------------------------------------- BGR -> YUV
@pytest.mark.parametrize("base", ri.BASES, ids=["base0", "base_off"])
@pytest.mark.parametrize("name", list(ri.LAYOUTS))
@pytest.mark.parametrize("fmt", ri.FORMATS)
def test_bgr_to_yuv_layouts(dev, fmt, name, base):
    """Every format x every layout, the destination at byte 0 and one sample into its allocation (the BGR source then one
    byte into its own): both matrices and a custom one at the row limit; gathered with a skipped and an out-of-range
    index; every byte outside the samples unchanged, the spare bits of two-byte words zero."""
    from avsum_amd import render
    bgr = ri.bgr_case(name)
    L = ri.dest_layout(fmt, name, len(ri.GATHER))
    offset = base * L.sample_bytes
    src = _bgr(dev, bgr, base)
    sentinel = np.full((L.n, L.frame_stride), ri.SENTINEL_U8, dtype=np.uint8)
    mask = yi.sample_mask(L)
    for matrix in ("bt601", "bt709", ri.CUSTOM):
        out = _yuv_frames(dev, L, base_offset=offset)
        assert out.data.data_ptr() % 4 == offset and src.data_ptr() % 4 == base
        got = render.bgr_to_yuv(src, out, count=ri.FRAMES, matrix=matrix)
        assert got is out
        got = out.data.cpu().numpy()
        want = render.bgr_to_frames_host(bgr, out, matrix, count=ri.FRAMES, into=sentinel)
        assert np.array_equal(got, want), (fmt, name, matrix, int((got != want).sum()))
        assert (got[:, ~mask] == ri.SENTINEL_U8).all() and (got[ri.FRAMES:] == ri.SENTINEL_U8).all()
    if L.sample_bytes == 2:
        words = got[:ri.FRAMES][:, mask].reshape(ri.FRAMES, -1, 2).astype(np.int64)
        assert ((words[..., 0] | (words[..., 1] << 8)) & ~(1023 << L.shift) == 0).all()
    # gathered: rows 1 (index -1) and 3 (index 7 of 3 frames) are left as they were
    index = torch.tensor(ri.GATHER, dtype=torch.int64, device=dev)
    out = _yuv_frames(dev, L, base_offset=offset)
    got = render.bgr_to_yuv(src, out, index, matrix="bt709").data.cpu().numpy()
    want = render.bgr_to_frames_host(bgr, out, "bt709", ri.GATHER, into=sentinel)
    assert np.array_equal(got, want) and (got[[1, 3]] == ri.SENTINEL_U8).all() and not (got[4] == ri.SENTINEL_U8).all()


@pytest.fixture(scope="module")
def every_colour(dev):
    bgr = ri.exhaustive_bgr()
    return bgr, torch.from_numpy(np.array(bgr)).to(dev)


@pytest.mark.parametrize("fmt", ("nv12", "p010"))
def test_bgr_to_yuv_every_colour(dev, every_colour, fmt):
    """One 4096 x 4096 frame holding every (B, G, R) once: exhaustive for Y; every block sum it produces is checked."""
    from avsum_amd import render
    bgr, bgr_t = every_colour
    L = yi.layout(fmt, 1, 4096, 4096)
    out = _yuv_frames(dev, L, fill=FILL)
    got = render.bgr_to_yuv(bgr_t, out, matrix="bt601").data.cpu().numpy()
    want = render.bgr_to_frames_host(bgr, out, "bt601")
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


def test_bgr_to_yuv_refusals(dev):
    from avsum_amd import render
    src = _bgr(dev, ri.bgr_case("6x10"))
    out = _yuv_frames(dev, ri.dest_layout("i420", "6x10", 3))
    with pytest.raises(ValueError):
        render.bgr_to_yuv(src.cpu(), out)
    with pytest.raises(ValueError):
        render.bgr_to_yuv(src, _yuv_frames(dev, ri.dest_layout("i420", "2x2", 3)))
    with pytest.raises(ValueError, match="count"):
        render.bgr_to_yuv(src, out, count=4)
    with pytest.raises(ValueError, match="forward matrix"):
        render.bgr_to_yuv(src, out, matrix=(16, 1 << 20, 1, 0, 0, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="matrix"):
        render.bgr_to_yuv(src, out, matrix="bt2020")


# --------------------------------------------------------------------------- repack
@pytest.mark.parametrize("name", ri.REPACK_LAYOUTS)
@pytest.mark.parametrize("pair", ri.REPACK_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_repack_pairs(dev, pair, name):
    """Every ordered pair of same-depth formats: the destination holds the source's samples and nothing else changes;
    garbage in a 10-bit source's spare bits does not reach it; yuv_to_bgr of it equals yuv_to_bgr of the source."""
    from avsum_amd import render, yuv
    src_fmt, dst_fmt = pair
    data, S = yi.layout_case(src_fmt, name)
    D = ri.dest_layout(dst_fmt, name, 4)
    src = _yuv_frames(dev, S, data, base_offset=S.sample_bytes)
    out = _yuv_frames(dev, D, base_offset=0 if name == "6x10" else D.sample_bytes)
    sentinel = np.full((D.n, D.frame_stride), ri.SENTINEL_U8, dtype=np.uint8)
    index = (2, -1, 0, 1)
    got = render.repack(src, out, torch.tensor(index, dtype=torch.int64, device=dev)).data.cpu().numpy()
    want = render.repack_host(data, src, out, index, into=sentinel)
    assert np.array_equal(got, want), (pair, name, int((got != want).sum()))
    assert (got[:, ~yi.sample_mask(D)] == ri.SENTINEL_U8).all() and (got[1] == ri.SENTINEL_U8).all()
    if S.sample_bytes == 2:
        other, _ = yi.layout_case(src_fmt, name, garbage_seed=1)
        assert not np.array_equal(other, data)
        again = _yuv_frames(dev, D, base_offset=0 if name == "6x10" else D.sample_bytes)
        render.repack(_yuv_frames(dev, S, other, base_offset=2), again, torch.tensor(index, dtype=torch.int64, device=dev))
        assert np.array_equal(again.data.cpu().numpy(), want)
    # the picture is the same
    plain = render.repack(src, _yuv_frames(dev, D._replace(n=3)))
    assert torch.equal(yuv.yuv_to_bgr(plain, matrix="bt709"), yuv.yuv_to_bgr(src, matrix="bt709"))


def test_repack_refuses_a_differing_depth(dev):
    from avsum_amd import render
    data, S = yi.layout_case("i420", "6x10")
    with pytest.raises(ValueError, match="tone mapping"):
        render.repack(_yuv_frames(dev, S, data), _yuv_frames(dev, ri.dest_layout("p010", "6x10", 3)))
    with pytest.raises(ValueError):
        render.repack(_yuv_frames(dev, S, data), _yuv_frames(dev, ri.dest_layout("nv12", "2x2", 3)))


# --------------------------------------------------------------------------- audio
@pytest.fixture(scope="module")
def audio_index(dev):
    from avsum_amd import ops, render
    wave, mask = ri.audio_case()
    tables = ops.RenderTables(ri.AUDIO_OFFSETS, device=dev)
    return torch.from_numpy(np.array(wave)).to(dev), render.summary_index(torch.from_numpy(np.array(mask)).to(dev), tables)


@pytest.mark.parametrize("fade", ri.AUDIO_FADES)
def test_audio_cut(dev, audio_index, fade):
    """3 tracks of different lengths at 25, 30 and 30000 / 1001 fps; a run clamped at its track's end, one wholly beyond
    it, one of ONE sample; fade 0 (the concatenated slices), 8 and one above half a run."""
    from avsum_amd import render
    wave_t, index = audio_index
    wave, _ = ri.audio_case()
    assert index.host()["runs"] == [list(r) for r in ri.AUDIO_RUNS]
    want, want_offsets = render.summary_audio_host(wave, ri.AUDIO_WAVE_OFFSETS, ri.AUDIO_RUNS, ri.AUDIO_FPS, ri.AUDIO_SR, fade)
    cap = ri.AUDIO_WAVE_OFFSETS[-1]
    out = torch.full((cap + GUARD,), 5.0, dtype=torch.float32, device=dev)
    audio, offsets = render.summary_audio(wave_t, ri.AUDIO_WAVE_OFFSETS, index, ri.AUDIO_FPS, ri.AUDIO_SR, fade, out=out[:cap])
    got = out.cpu().numpy()
    assert audio.data_ptr() == out.data_ptr() and np.array_equal(offsets.cpu().numpy(), want_offsets)
    assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32)), fade
    assert (got[want.size:] == 5.0).all()                                       # nothing past the count, or the buffer
    assert np.array_equal(index.totals.cpu().numpy()[:, 2], np.diff(want_offsets))
    if fade == 0:
        slices = [wave[ri.AUDIO_WAVE_OFFSETS[v]:ri.AUDIO_WAVE_OFFSETS[v + 1]][
            render.audio_bounds_host(s, ri.AUDIO_FPS[v], ri.AUDIO_SR, ri.AUDIO_TRACKS[v]):
            render.audio_bounds_host(e, ri.AUDIO_FPS[v], ri.AUDIO_SR, ri.AUDIO_TRACKS[v])]
            for v, runs in enumerate(ri.AUDIO_RUNS) for s, e in runs]
        assert [len(s) for s in slices][:7] == [1920, 122239, 81, 0, 1, 0, 533]
        assert np.array_equal(got[:want.size], np.concatenate(slices))


def test_audio_capacity_too_small(dev, audio_index):
    """A sample capacity below the count: the first samples are right, nothing beyond is written, host() raises."""
    from avsum_amd import render
    wave_t, index = audio_index
    wave, _ = ri.audio_case()
    want, want_offsets = render.summary_audio_host(wave, ri.AUDIO_WAVE_OFFSETS, ri.AUDIO_RUNS, ri.AUDIO_FPS, ri.AUDIO_SR, 0)
    cap = 5000
    out = torch.full((cap + GUARD,), 5.0, dtype=torch.float32, device=dev)
    audio, offsets = render.summary_audio(wave_t, ri.AUDIO_WAVE_OFFSETS, index, ri.AUDIO_FPS, ri.AUDIO_SR, out=out[:cap])
    got = out.cpu().numpy()
    assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == 5.0).all()
    assert np.array_equal(offsets.cpu().numpy(), want_offsets)                   # the TRUE numbers
    with pytest.raises(RuntimeError, match="samples exceed"):
        render.SummaryRender(index, None, audio, offsets).host()


# --------------------------------------------------------------------------- the routes of summary_frames
def test_summary_frames_same_format_is_gather_rows(dev, monkeypatch):
    """BGR -> BGR and YUV -> the same description are ops.gather_rows on the rows and nothing else."""
    from avsum_amd import ops, render
    bgr, _ = ri.e2e_case()
    mask = np.zeros(ri.E2E_OFFSETS[-1], dtype=np.uint8)
    mask[[0, 4, 5, 6, 30, 44, 45, 67]] = 1
    index = render.summary_index(torch.from_numpy(mask).to(dev), ops.RenderTables(ri.E2E_OFFSETS, device=dev))
    calls = []

    def recording(src, idx, count, out=None):
        calls.append((src.shape, idx.data_ptr(), count.data_ptr()))
        return ops.gather_rows(src, idx, count, out)

    def forbidden(*a, **k):
        raise AssertionError("a conversion kernel was launched for a same-format gather")

    monkeypatch.setattr(render, "gather_rows", recording)
    for name in ("bgr_to_yuv", "repack"):
        monkeypatch.setattr(render, name, forbidden)
    monkeypatch.setattr(render._yuv, "yuv_to_bgr", forbidden)
    frames = torch.from_numpy(np.array(bgr)).to(dev)
    picked = np.flatnonzero(mask)
    for out in (None, "bgr"):
        got = render.summary_frames(frames, index, out).cpu().numpy()
        assert got.shape[0] == index.plan.frame_cap and np.array_equal(got[:picked.size], bgr[picked]) and not got[picked.size:].any()
    L = ri.dest_layout("i420", "6x10", ri.E2E_OFFSETS[-1])
    data = render.bgr_to_frames_host(bgr, _meta(L), "bt601")
    src = _yuv_frames(dev, L, data)
    same = render.summary_frames(src, index)
    assert render._layout(same) == render._layout(src) and np.array_equal(same.data.cpu().numpy()[:picked.size], data[picked])
    own = _yuv_frames(dev, L._replace(n=index.plan.frame_cap + 2), fill=FILL)
    assert render.summary_frames(src, index, own) is own
    got = own.data.cpu().numpy()
    assert np.array_equal(got[:picked.size], data[picked]) and (got[picked.size:] == FILL).all()
    assert len(calls) == 4 and all(c[1] == index.frame_index.data_ptr() and c[2] == index.count.data_ptr() for c in calls)
    assert [c[0] for c in calls][2:] == [(ri.E2E_OFFSETS[-1], L.frame_stride)] * 2


def _meta(L):
    from avsum_amd.yuv import YuvFrames
    return YuvFrames(torch.empty((L.n, L.frame_stride), dtype=torch.uint8, device="meta"), L.h, L.w, **yi.fields(L))


# --------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def keyshots(dev):
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    bgr, scores = ri.e2e_case()
    result = keyshot_summaries_device(torch.from_numpy(np.array(scores)).to(dev), list(ri.E2E_OFFSETS), [list(s) for s in ri.E2E_SHOTS])
    return bgr, torch.from_numpy(np.array(bgr)).to(dev), result


def _picked_frames(picks):
    """The global frames of one row of KeyshotResult.host()."""
    return np.array([ri.E2E_OFFSETS[v] + f for v, shots in enumerate(picks) for s, e in shots for f in range(s, e)], dtype=np.int64)


@pytest.mark.parametrize("row", (0, 1))
def test_render_device_from_keyshots(dev, keyshots, row):
    """3 videos of (5, 40, 23) frames of 6 x 10 pixels with host shot lists: keyshot_summaries_device -> render_device.
    The frames are the host gather of KeyshotResult.host()'s picks (row 1 renders row 1); the runs are the picks with
    adjacent shots merged; the audio is the host cut of those runs."""
    from avsum_amd import render
    from avsum_amd.pipeline import FrameScoringPipeline
    bgr, frames, result = keyshots
    picks = result.host()[row]
    want = _picked_frames(picks)
    assert want.size and not np.array_equal(want, _picked_frames(result.host()[1 - row]))
    wave_offsets = [0, 3200, 28800, 43520]
    wave = np.random.default_rng(3).standard_normal(wave_offsets[-1]).astype(np.float32)
    rendered = FrameScoringPipeline.render_device(frames, list(ri.E2E_OFFSETS), result, torch.from_numpy(wave).to(dev), wave_offsets,
                                                  25, fade=8, row=row)
    assert (rendered.index.plan.frame_cap, rendered.index.plan.run_cap) == (9, result.plan.shot_cap)
    got = rendered.frames.cpu().numpy()
    assert got.shape == (9, 6, 10, 3) and np.array_equal(got[:want.size], bgr[want]) and not got[want.size:].any()
    assert np.array_equal(rendered.index.frame_index.cpu().numpy(), np.concatenate([want, np.full(9 - want.size, -1)]))
    host = rendered.host()
    mask = np.zeros(ri.E2E_OFFSETS[-1], dtype=np.uint8)
    mask[want] = 1
    runs = render.summary_index_host(mask, ri.E2E_OFFSETS)["per_video"]
    assert host["runs"] == runs and host["frames"].tolist() == [sum(e - s for s, e in shots) for shots in picks]
    cut, cut_offsets = render.summary_audio_host(wave, wave_offsets, runs, 25, 16000, 8)
    assert np.array_equal(host["audio_offsets"], cut_offsets) and host["samples"].sum() == cut.size > want.size * 639
    assert rendered.audio.numel() == rendered.index.plan.sample_cap >= cut.size
    assert np.array_equal(rendered.audio.cpu().numpy()[:cut.size].view(np.uint32), cut.view(np.uint32))


def test_render_device_i420_to_nv12_and_bgr(dev, keyshots):
    """The same batch as I420, rendered to NV12, equals repack_host of the gather; rendered to BGR, yuv_to_bgr of it; BGR
    frames rendered to NV12 equal the forward definition of the gather."""
    from avsum_amd import render, yuv
    from avsum_amd.pipeline import FrameScoringPipeline
    bgr, frames, result = keyshots
    want = _picked_frames(result.host()[0])
    S, D = ri.dest_layout("i420", "6x10", ri.E2E_OFFSETS[-1]), ri.dest_layout("nv12", "6x10", 10)
    data = render.bgr_to_frames_host(bgr, _meta(S), "bt601")
    src = _yuv_frames(dev, S, data)
    filled = np.full((D.n, D.frame_stride), FILL, dtype=np.uint8)
    index = np.concatenate([want, np.full(9 - want.size, -1)])
    out = _yuv_frames(dev, D, fill=FILL)
    rendered = FrameScoringPipeline.render_device(src, list(ri.E2E_OFFSETS), result, out=out)
    assert rendered.frames is out and rendered.audio is None and "audio_offsets" not in rendered.host()
    assert np.array_equal(out.data.cpu().numpy(), render.repack_host(data, src, out, index, into=filled))
    as_bgr = FrameScoringPipeline.render_device(src, list(ri.E2E_OFFSETS), result, out="bgr", matrix="bt709").frames.cpu().numpy()
    assert np.array_equal(as_bgr[:want.size], yuv.frames_to_bgr_host(data, src, "bt709")[want]) and not as_bgr[want.size:].any()
    out = _yuv_frames(dev, D, fill=FILL)
    FrameScoringPipeline.render_device(frames, list(ri.E2E_OFFSETS), result, out=out, matrix="bt709")
    assert np.array_equal(out.data.cpu().numpy(), render.bgr_to_frames_host(bgr, out, "bt709", index, into=filled))
    with pytest.raises(ValueError, match="tone mapping"):
        FrameScoringPipeline.render_device(src, list(ri.E2E_OFFSETS), result, out=_yuv_frames(dev, ri.dest_layout("p010", "6x10", 9)))
    with pytest.raises(ValueError, match="other video offsets"):
        FrameScoringPipeline.render_device(src, [0, 6, 45, 68], result)


def test_render_device_from_a_selection_mask(dev, keyshots):
    """A select_mask_device mask renders the frames select selects (the reference's mean-threshold rule)."""
    from avsum_amd.pipeline import FrameScoringPipeline
    bgr, frames, _ = keyshots
    scores = torch.from_numpy(np.array(ri.e2e_case()[1][0])).to(dev)
    mask = FrameScoringPipeline.select_device(scores, list(ri.E2E_OFFSETS))
    selected = FrameScoringPipeline.select(scores, list(ri.E2E_OFFSETS))
    want = np.concatenate([ri.E2E_OFFSETS[v] + np.asarray(s, dtype=np.int64) for v, s in enumerate(selected)])
    rendered = FrameScoringPipeline.render_device(frames, list(ri.E2E_OFFSETS), mask)
    assert 0 < want.size < ri.E2E_OFFSETS[-1] and rendered.index.plan.frame_cap == ri.E2E_OFFSETS[-1]
    got = rendered.frames.cpu().numpy()
    assert np.array_equal(got[:want.size], bgr[want]) and not got[want.size:].any()
    assert rendered.host()["frames"].tolist() == [len(s) for s in selected]
