"""The NV12 ingest kernels on the GPU (libavsum_ingest.so through avsum_amd/ingest.py).  nv12_to_bgr is held to the integer
definition (ingest.nv12_to_bgr_host) on every (Y, U, V) and on the committed layouts; the two fused kernels are held,
byte for byte and integer for integer, to the BGR kernels of libavsum_hip.so applied to nv12_to_bgr's output; the three
batched layers give for an Nv12Frames what they give for its converted frames.  Cases come from nv12_inputs.py, which
test_nv12_host.py checks on the host."""
import numpy as np
import pytest
import torch

import nv12_inputs as ni

pytestmark = pytest.mark.gpu

MATRIX_NAMES = ("bt601", "bt709")
FILL = 7                     # what destinations hold before a launch


def _frames(dev, data, h, w, uv_row, base_offset=0):
    """Nv12Frames of a numpy [N, rows, pitch] on the device, its first byte ``base_offset`` bytes into an allocation."""
    from avsum_amd.ingest import Nv12Frames
    flat = torch.full((data.size + base_offset,), ni.SENTINEL_U8, dtype=torch.uint8, device=dev)
    view = flat[base_offset:].view(data.shape)
    view.copy_(torch.from_numpy(np.array(data)))
    return Nv12Frames(view, h, w, uv_row)


# --------------------------------------------------------------------------- to_bgr
@pytest.mark.parametrize("matrix", MATRIX_NAMES)
def test_to_bgr_every_triple(dev, matrix):
    from avsum_amd import ingest
    data = ni.exhaustive_case()
    frames = _frames(dev, data, 512, 512, 512)
    got = ingest.nv12_to_bgr(frames, matrix=matrix).cpu().numpy()
    want = ingest.nv12_to_bgr_host(data, 512, 512, 512, matrix)
    assert got.shape == want.shape == (64, 512, 512, 3)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("base_offset", [0, 1])
@pytest.mark.parametrize("layout", ni.LAYOUTS, ids=["x".join(map(str, l)) for l in ni.LAYOUTS])
def test_to_bgr_layouts(dev, layout, base_offset):
    from avsum_amd import ingest
    h, w, pitch, uv_row = layout
    data = ni.layout_case(layout)
    frames = _frames(dev, data, h, w, uv_row, base_offset)
    assert frames.data.data_ptr() % 2 == base_offset
    for matrix in MATRIX_NAMES:
        want = ingest.nv12_to_bgr_host(data, h, w, uv_row, matrix)
        assert np.array_equal(ingest.nv12_to_bgr(frames, matrix=matrix).cpu().numpy(), want)
    # a custom matrix goes the same way
    custom = (3, -700001, 4194304, -4194304, 123457, -1)
    assert np.array_equal(ingest.nv12_to_bgr(frames, matrix=custom).cpu().numpy(),
                          ingest.nv12_to_bgr_host(data, h, w, uv_row, custom))
    want = ingest.nv12_to_bgr_host(data, h, w, uv_row)
    # gathered, into a destination that is itself off every alignment; rows past count and the skipped row stay
    index = torch.tensor(ni.GATHER_INDEX, dtype=torch.int64, device=dev)
    count = len(ni.GATHER_INDEX) - 1
    buf = torch.full((len(ni.GATHER_INDEX) * h * w * 3 + 1,), FILL, dtype=torch.uint8, device=dev)
    out = buf[1:].view(len(ni.GATHER_INDEX), h, w, 3)
    assert ingest.nv12_to_bgr(frames, index, count, out=out) is out
    got = out.cpu().numpy()
    for i, r in enumerate(ni.GATHER_INDEX):
        if i >= count or i == ni.GATHER_SKIPPED:
            assert (got[i] == FILL).all(), i
        else:
            assert np.array_equal(got[i], want[r]), i
    assert buf[0].item() == FILL
    with pytest.raises(ValueError, match="nv12_to_bgr: out holds"):
        ingest.nv12_to_bgr(frames, index, count, out=out[:count - 1])
    # the source is as it was, padding and all
    assert np.array_equal(frames.data.cpu().numpy(), data)


# --------------------------------------------------------------------------- resize_gather
@pytest.mark.parametrize("name", sorted(ni.RESIZE_CASES))
def test_resize_gather_equals_convert_then_resize(dev, name):
    from avsum_amd import ingest, ops
    h, w, pitch, uv_row, nframes, index, sizes = ni.RESIZE_CASES[name]
    frames = _frames(dev, ni.resize_case(name), h, w, uv_row, base_offset=1 if name == "index" else 0)
    idx = torch.tensor(index, dtype=torch.int64, device=dev)
    count = len(index)
    skipped = [i for i, r in enumerate(index) if not 0 <= r < nframes]
    for matrix in MATRIX_NAMES if name == "up_both" else MATRIX_NAMES[:1]:
        bgr = ingest.nv12_to_bgr(frames, matrix=matrix)
        want = [torch.full((count, dh, dw, 3), FILL, dtype=torch.uint8, device=dev) for dh, dw in sizes]
        ops.resize_gather(bgr, idx, count, sizes, want)
        outs = [torch.full((count, dh, dw, 3), FILL, dtype=torch.uint8, device=dev) for dh, dw in sizes]
        got = ingest.nv12_resize_gather(frames, idx, count, sizes, matrix, outs)
        assert all(g is o for g, o in zip(got, outs))
        for size, g, wnt in zip(sizes, got, want):
            assert torch.equal(g, wnt), (name, size, matrix, int((g != wnt).sum().item()))
            for i in skipped:
                assert (g[i] == FILL).all()
            assert g[[i for i in range(count) if i not in skipped]].float().std().item() > 10.0    # (pictures, not FILL)
    # one launch for two sizes = one launch per size; outs allocated by the call; a count below the index length
    if len(sizes) == 2 and not skipped:
        for size, both in zip(sizes, got):
            assert torch.equal(ingest.nv12_resize_gather(frames, idx, count, [size], matrix)[0], both)
        part = ingest.nv12_resize_gather(frames, idx, 1, sizes, matrix)
        assert all(p.shape[0] == 1 and torch.equal(p[0], both[0]) for p, both in zip(part, got))


def test_resize_gather_refusals(dev):
    from avsum_amd import ingest
    h, w, pitch, uv_row = ni.LAYOUTS[1]
    frames = _frames(dev, ni.layout_case(ni.LAYOUTS[1]), h, w, uv_row)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    for bad in (lambda: ingest.nv12_resize_gather(frames, idx, 3, [(8, 8)]),
                lambda: ingest.nv12_resize_gather(frames, idx.cpu(), 1, [(8, 8)]),
                lambda: ingest.nv12_resize_gather(frames, idx, 1, []),
                lambda: ingest.nv12_resize_gather(frames, idx, 1, [(8, 8)], outs=[torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=dev)]),
                lambda: ingest.nv12_resize_gather(frames.data, idx, 1, [(8, 8)])):
        with pytest.raises(ValueError, match="nv12_resize_gather"):
            bad()
    with pytest.raises(ValueError, match="matrix must be one of"):
        ingest.nv12_resize_gather(frames, idx, 1, [(8, 8)], matrix="rec2020")
    assert ingest.nv12_resize_gather(frames, idx, 0, [(8, 8)])[0].shape == (0, 8, 8, 3)


# --------------------------------------------------------------------------- hsv_diff
@pytest.mark.parametrize("step", ni.HSV_STEPS)
def test_hsv_diff_equals_convert_then_scan(dev, step):
    from avsum_amd import ingest, ops
    h, w, pitch, uv_row = ni.HSV_LAYOUT
    offsets = list(ni.HSV_OFFSETS)
    frames = _frames(dev, ni.hsv_case(ni.HSV_LAYOUT, offsets[-1]), h, w, uv_row, base_offset=1)
    tables = ops.ShotTables(offsets, 15, dev)
    for matrix in MATRIX_NAMES:
        want = ops.hsv_frame_diff_batch(ingest.nv12_to_bgr(frames, matrix=matrix), tables, step, raw=True)
        got = ingest.nv12_hsv_frame_diff_batch(frames, tables, step, raw=True, matrix=matrix)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        firsts = got[offsets[:-1]]
        assert not firsts.any() and got[[1 + o for o in offsets[1:-1]]].all()      # zeros at the first frames only
        wide = ingest.nv12_hsv_frame_diff_batch(frames, tables, step, matrix=matrix)
        assert wide.dtype == torch.int64 and torch.equal(wide, want.to(torch.int64) & 0xFFFFFFFF)


def test_hsv_diff_several_workgroups_per_frame(dev):
    from avsum_amd import ingest, ops
    layout, offsets = ni.HSV_BIG
    h, w, pitch, uv_row = layout
    frames = _frames(dev, ni.hsv_case(layout, offsets[-1]), h, w, uv_row)
    tables = ops.ShotTables(list(offsets), 15, dev)
    for step in (1, 2):
        want = ops.hsv_frame_diff_batch(ingest.nv12_to_bgr(frames), tables, step, raw=True)
        assert torch.equal(ingest.nv12_hsv_frame_diff_batch(frames, tables, step, raw=True), want)
    with pytest.raises(ValueError, match="nv12_hsv_frame_diff_batch"):
        ingest.nv12_hsv_frame_diff_batch(frames, ops.ShotTables([0, 3], 15, dev))           # another frame count
    with pytest.raises(ValueError, match="nv12_hsv_frame_diff_batch"):
        ingest.nv12_hsv_frame_diff_batch(frames, tables, 0)


# --------------------------------------------------------------------------- end to end
def test_detect_shots_batch_takes_nv12(dev):
    from avsum_amd import ingest
    from avsum_amd.features.shots import detect_shots_batch
    data, offsets = ni.scene_batch()
    h, w, pitch, uv_row = ni.E2E_LAYOUT
    frames = _frames(dev, data, h, w, uv_row)
    for matrix in MATRIX_NAMES:
        from_bgr = detect_shots_batch(ingest.nv12_to_bgr(frames, matrix=matrix), offsets)
        from_nv12 = detect_shots_batch(frames, offsets, matrix=matrix)
        assert torch.equal(from_nv12.sums, from_bgr.sums)
        assert from_nv12.host() == from_bgr.host()
        assert torch.equal(from_nv12.sample_index, from_bgr.sample_index)
    assert detect_shots_batch(frames, offsets).host() == ni.scene_cuts()
    with pytest.raises(ValueError, match="detect_shots_batch"):
        detect_shots_batch(ingest.Nv12Frames(frames.data.cpu(), h, w, uv_row), offsets)


@pytest.fixture(scope="module")
def proc(dev):
    from avsum_amd.features.extractors import AVProcessor
    torch.manual_seed(13)
    p = AVProcessor(torch.float32, "batch")
    p.visual_extractor.to(dev)
    return p


def _embed_batch(dev):
    h, w, pitch, uv_row = ni.E2E_LAYOUT
    data = ni.surface(h, w, pitch, uv_row, frames=sum(ni.EMBED_LENGTHS), seed=3)
    return _frames(dev, data, h, w, uv_row), ni.offsets_of(ni.EMBED_LENGTHS)


def test_embed_shots_takes_nv12(dev, proc):
    """2 videos, 3 shots, 7 sampled frames of 36 x 70, the default arithmetic: the rows of the converted frames, exactly."""
    from avsum_amd import ingest, ops
    frames, offsets = _embed_batch(dev)
    plan = ops.StageOneTables(offsets, list(ni.EMBED_SHOTS), device=dev)
    assert plan.nsamples == 7 and plan.nshots == 3
    want = proc.visual_extractor.embed_shots(ingest.nv12_to_bgr(frames), plan)
    got = proc.visual_extractor.embed_shots(frames, plan)
    assert got.shape == (3, 4096) and got.dtype == torch.float32 and torch.isfinite(got).all() and got.any(dim=1).all()
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="embed_shots"):
        proc.visual_extractor.embed_shots(ingest.Nv12Frames(frames.data[1:], frames.height, frames.width, frames.uv_row), plan)


def test_embed_shots_nv12_frames_of_a_trunks_size(dev, proc):
    """224 x 224 surfaces: the ResNet input is nv12_to_bgr of the pass index, where BGR frames take gather_rows."""
    from avsum_amd import ingest, ops
    data = ni.surface(224, 224, 256, 224, frames=6, seed=4)
    frames = _frames(dev, data, 224, 224, 224)
    plan = ops.StageOneTables([0, 6], [[(0, 6)]], device=dev)
    got = proc.visual_extractor.embed_shots(frames, plan, matrix="bt709")
    want = proc.visual_extractor.embed_shots(ingest.nv12_to_bgr(frames, matrix="bt709"), plan)
    assert got.shape == (1, 4096) and torch.equal(got, want)


def test_process_decoded_batch_takes_nv12(dev, proc):
    from avsum_amd import ingest
    frames, offsets = _embed_batch(dev)
    waves = [np.zeros(int(n / 30 * 16000), dtype=np.float32) for n in ni.EMBED_LENGTHS]
    shots = list(ni.EMBED_SHOTS)
    want = proc.process_decoded_batch(ingest.nv12_to_bgr(frames), offsets, waves, 30.0, shots)
    got = proc.process_decoded_batch(frames, offsets, waves, 30.0, shots)
    assert len(got) == len(want) == 2
    for (vis, aud), (rvis, raud) in zip(got, want):
        assert vis.shape == rvis.shape and vis.dtype == rvis.dtype == np.float32 and vis.any(axis=1).all()
        assert np.array_equal(vis, rvis) and aud.shape == raud.shape and np.array_equal(aud, raud)
    with pytest.raises(ValueError, match="process_decoded_batch"):
        proc.process_decoded_batch(ingest.Nv12Frames(frames.data.cpu(), frames.height, frames.width, frames.uv_row),
                                   offsets, waves, 30.0, shots)


def test_process_decoded_batch_detects_on_nv12(dev, proc):
    """shots=None: the shot scan reads the surfaces too, and the cuts planted in the scene batch come back."""
    from avsum_amd import ingest
    data, offsets = ni.scene_batch()
    h, w, pitch, uv_row = ni.E2E_LAYOUT
    frames = _frames(dev, data, h, w, uv_row)
    waves = [np.zeros(int((b - a) / 30 * 16000), dtype=np.float32) for a, b in zip(offsets[:-1], offsets[1:])]
    got = proc.process_decoded_batch(frames, offsets, waves, 30.0)
    want = proc.process_decoded_batch(ingest.nv12_to_bgr(frames), offsets, waves, 30.0)
    assert [g[0].shape for g in got] == [(len(c), 4096) for c in ni.scene_cuts()]
    for (vis, aud), (rvis, raud) in zip(got, want):
        assert np.array_equal(vis, rvis) and np.array_equal(aud, raud)


def test_pinned_surfaces_upload_with_pull_copy(dev):
    from avsum_amd import ingest, ops
    h, w, pitch, uv_row = ni.LAYOUTS[2]
    data = ni.layout_case(ni.LAYOUTS[2])
    frames = ingest.Nv12Frames(torch.zeros(data.shape, dtype=torch.uint8, device=dev), h, w, uv_row)
    pinned = frames.pinned_like()
    assert pinned.is_pinned() and pinned.shape == frames.data.shape and pinned.numel() == frames.nbytes
    pinned.copy_(torch.from_numpy(np.array(data)))
    ops.pull_copy(pinned, frames.data)
    assert np.array_equal(ingest.nv12_to_bgr(frames).cpu().numpy(), ingest.nv12_to_bgr_host(data, h, w, uv_row))
