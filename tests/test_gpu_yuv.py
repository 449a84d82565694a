"""The YUV 4:2:0 ingest kernels on the GPU (libavsum_yuv.so through avsum_amd/yuv.py).  yuv_to_bgr is held to the int64
definition (yuv.frames_to_bgr_host) on the exhaustive ten-bit case and on every committed layout of every format; it
agrees with the NV12 library on the same picture; the two fused kernels are held, byte for byte and integer for integer,
to the BGR kernels of libavsum_hip.so applied to yuv_to_bgr's output; the three batched layers give for a YuvFrames what
they give for its converted frames.  Cases come from yuv_inputs.py, which test_yuv_host.py checks on the host."""
import numpy as np
import pytest
import torch

import nv12_inputs as ni
import yuv_inputs as yi

pytestmark = pytest.mark.gpu

MATRIX_NAMES = ("bt601", "bt709")
FILL = 7                     # what destinations hold before a launch


def _frames(dev, data, L, base_offset=0):
    """YuvFrames of a flat numpy [n, frame_stride] on the device, its first byte ``base_offset`` bytes into an allocation."""
    from avsum_amd.yuv import YuvFrames
    flat = torch.full((data.size + base_offset,), yi.SENTINEL_U8, dtype=torch.uint8, device=dev)
    view = flat[base_offset:].view(data.shape)
    view.copy_(torch.from_numpy(np.array(data)))
    return YuvFrames(view, L.h, L.w, **yi.fields(L))


# --------------------------------------------------------------------------- to_bgr
@pytest.fixture(scope="module")
def exhaustive(dev):
    data, L = yi.exhaustive_case()
    return data, L, _frames(dev, data, L)


@pytest.mark.parametrize("matrix", MATRIX_NAMES)
def test_to_bgr_every_chroma_pair_at_ten_bits(dev, exhaustive, matrix):
    """4 P010 frames of 2048 x 2048: every (U, V) with 16 lumas, the triples whose sums leave int32 among them."""
    from avsum_amd import yuv
    data, L, frames = exhaustive
    got = yuv.yuv_to_bgr(frames, matrix=matrix).cpu().numpy()
    assert got.shape == (4, 2048, 2048, 3)
    for k in range(L.n):
        want = yuv.frames_to_bgr_host(data[k:k + 1], frames.like(torch.empty((1, L.frame_stride), dtype=torch.uint8, device="meta")), matrix)
        assert np.array_equal(got[k], want[0]), f"frame {k}: {int((got[k] != want[0]).sum())} bytes differ"


@pytest.mark.parametrize("misaligned", [False, True], ids=["base0", "base_off"])
@pytest.mark.parametrize("name", list(yi.LAYOUTS))
@pytest.mark.parametrize("fmt", yi.FORMATS)
def test_to_bgr_layouts(dev, fmt, name, misaligned):
    """Every layout x every format, at base offsets 0 and 1 (one-byte formats) or 0 and 2 (two-byte formats)."""
    from avsum_amd import yuv
    data, L = yi.layout_case(fmt, name)
    base_offset = L.sample_bytes if misaligned else 0
    frames = _frames(dev, data, L, base_offset)
    assert frames.data.data_ptr() % 4 == base_offset
    h, w = L.h, L.w
    for matrix in MATRIX_NAMES:
        want = yuv.frames_to_bgr_host(data, frames, matrix)
        assert np.array_equal(yuv.yuv_to_bgr(frames, matrix=matrix).cpu().numpy(), want), (fmt, name, matrix)
    # a custom matrix at the coefficient limits goes the same way
    custom = (3, -700001, 4194304, -4194304, 123457, -1)
    assert np.array_equal(yuv.yuv_to_bgr(frames, matrix=custom).cpu().numpy(), yuv.frames_to_bgr_host(data, frames, custom))
    edge = (255, 4194304, -4194304, 4194304, -4194304, 4194304)
    assert np.array_equal(yuv.yuv_to_bgr(frames, matrix=edge).cpu().numpy(), yuv.frames_to_bgr_host(data, frames, edge))
    want = yuv.frames_to_bgr_host(data, frames)
    # other garbage in the unused bits of every word changes nothing
    if L.sample_bytes == 2:
        other, _ = yi.layout_case(fmt, name, garbage_seed=1)
        assert not np.array_equal(other, data)
        assert np.array_equal(yuv.yuv_to_bgr(_frames(dev, other, L, base_offset)).cpu().numpy(), want)
    # gathered, into a destination that is itself off every alignment; rows past count and the skipped row stay
    index = torch.tensor(yi.GATHER_INDEX, dtype=torch.int64, device=dev)
    count = yi.GATHER_COUNT
    buf = torch.full((len(yi.GATHER_INDEX) * h * w * 3 + 1,), FILL, dtype=torch.uint8, device=dev)
    out = buf[1:].view(len(yi.GATHER_INDEX), h, w, 3)
    assert yuv.yuv_to_bgr(frames, index, count, out=out) is out
    got = out.cpu().numpy()
    for i, r in enumerate(yi.GATHER_INDEX):
        if i >= count or i == yi.GATHER_SKIPPED:
            assert (got[i] == FILL).all(), i
        else:
            assert np.array_equal(got[i], want[r]), i
    assert buf[0].item() == FILL
    with pytest.raises(ValueError, match="yuv_to_bgr: out holds"):
        yuv.yuv_to_bgr(frames, index, count, out=out[:count - 1])
    # the source is as it was, padding and all
    assert np.array_equal(frames.data.cpu().numpy(), data)


def test_same_picture_through_both_libraries(dev):
    """yuv_to_bgr(YuvFrames.from_nv12(f)) == ingest.nv12_to_bgr(f), and so does an I420, a YV12, an NV21, a P010 and a planar
    ten-bit (samples << 2) repacking of the same picture."""
    from avsum_amd import ingest, ops, yuv
    h, w, pitch, uv_row = ni.LAYOUTS[2]
    nv12 = ni.layout_case(ni.LAYOUTS[2])
    f = ingest.Nv12Frames(torch.from_numpy(np.array(nv12)).to(dev), h, w, uv_row)
    for matrix in MATRIX_NAMES:
        want = ingest.nv12_to_bgr(f, matrix=matrix)
        assert torch.equal(yuv.yuv_to_bgr(yuv.YuvFrames.from_nv12(f), matrix=matrix), want)
        for fmt in ("i420", "yv12", "nv21", "p010", "i010"):
            data, L = yi.repack(fmt, nv12, h, w, uv_row, pitch_y=72, gap=2)
            assert torch.equal(yuv.yuv_to_bgr(_frames(dev, data, L), matrix=matrix), want), (fmt, matrix)
    # ... and through the fused kernels
    idx = torch.tensor([2, 0], dtype=torch.int64, device=dev)
    tables = ops.ShotTables([0, 3], 15, dev)
    for fmt in ("nv12", "i420", "p010"):
        data, L = yi.repack(fmt, nv12, h, w, uv_row)
        frames = _frames(dev, data, L)
        for a, b in zip(yuv.yuv_resize_gather(frames, idx, 2, [(224, 224), (299, 299)]),
                        ingest.nv12_resize_gather(f, idx, 2, [(224, 224), (299, 299)])):
            assert torch.equal(a, b), fmt
        assert torch.equal(yuv.yuv_hsv_frame_diff_batch(frames, tables), ingest.nv12_hsv_frame_diff_batch(f, tables)), fmt


# --------------------------------------------------------------------------- resize_gather
@pytest.mark.parametrize("name", sorted(yi.RESIZE_CASES))
def test_resize_gather_equals_convert_then_resize(dev, name):
    from avsum_amd import ops, yuv
    fmt, args, nframes, index, sizes = yi.RESIZE_CASES[name]
    data, L = yi.resize_case(name)
    frames = _frames(dev, data, L, base_offset=L.sample_bytes if name.startswith("index") else 0)
    idx = torch.tensor(index, dtype=torch.int64, device=dev)
    count = len(index)
    skipped = [i for i, r in enumerate(index) if not 0 <= r < nframes]
    for matrix in MATRIX_NAMES if name.startswith("up_both") else MATRIX_NAMES[:1]:
        bgr = yuv.yuv_to_bgr(frames, matrix=matrix)
        want = [torch.full((count, dh, dw, 3), FILL, dtype=torch.uint8, device=dev) for dh, dw in sizes]
        ops.resize_gather(bgr, idx, count, sizes, want)
        outs = [torch.full((count, dh, dw, 3), FILL, dtype=torch.uint8, device=dev) for dh, dw in sizes]
        got = yuv.yuv_resize_gather(frames, idx, count, sizes, matrix, outs)
        assert all(g is o for g, o in zip(got, outs))
        for size, g, wnt in zip(sizes, got, want):
            assert torch.equal(g, wnt), (name, size, matrix, int((g != wnt).sum().item()))
            for i in skipped:
                assert (g[i] == FILL).all()
            assert g[[i for i in range(count) if i not in skipped]].float().std().item() > 10.0    # (pictures, not FILL)
    # one launch for two sizes = one launch per size; outs allocated by the call; a count below the index length
    if len(sizes) == 2 and not skipped:
        for size, both in zip(sizes, got):
            assert torch.equal(yuv.yuv_resize_gather(frames, idx, count, [size], matrix)[0], both)
        part = yuv.yuv_resize_gather(frames, idx, 1, sizes, matrix)
        assert all(p.shape[0] == 1 and torch.equal(p[0], both[0]) for p, both in zip(part, got))
    # the source is as it was
    assert np.array_equal(frames.data.cpu().numpy(), data)


def test_resize_gather_refusals(dev):
    from avsum_amd import _yuv_abi, yuv
    data, L = yi.layout_case("i420", "6x10")
    frames = _frames(dev, data, L)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    for bad in (lambda: yuv.yuv_resize_gather(frames, idx, 3, [(8, 8)]),
                lambda: yuv.yuv_resize_gather(frames, idx.cpu(), 1, [(8, 8)]),
                lambda: yuv.yuv_resize_gather(frames, idx, 1, []),
                lambda: yuv.yuv_resize_gather(frames, idx, 1, [(8, 8)], outs=[torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=dev)]),
                lambda: yuv.yuv_resize_gather(frames.data, idx, 1, [(8, 8)])):
        with pytest.raises(ValueError, match="yuv_resize_gather"):
            bad()
    with pytest.raises(ValueError, match="matrix must be one of"):
        yuv.yuv_resize_gather(frames, idx, 1, [(8, 8)], matrix="rec2020")
    assert yuv.yuv_resize_gather(frames, idx, 0, [(8, 8)])[0].shape == (0, 8, 8, 3)
    # the shape the plan refuses raises with the header's status, and leaves the destination alone
    fmt, args, size = yi.REFUSED_CASE
    wide, LW = yi.surface(fmt, *args, frames=1)
    wide_frames = _frames(dev, wide, LW)
    assert yuv.yuv_resize_band(wide_frames, *size) == 0
    out = torch.full((1,) + size + (3,), FILL, dtype=torch.uint8, device=dev)
    with pytest.raises(_yuv_abi.AvsyError, match=f"status {_yuv_abi.E_UNSUPPORTED}.*LDS"):
        yuv.yuv_resize_gather(wide_frames, idx, 1, [size], outs=[out])
    assert _yuv_abi.E_UNSUPPORTED == -6 and (out == FILL).all()
    # ... while the dense conversion takes it
    assert np.array_equal(yuv.yuv_to_bgr(wide_frames).cpu().numpy(), yuv.frames_to_bgr_host(wide, wide_frames))


# --------------------------------------------------------------------------- hsv_diff
@pytest.mark.parametrize("step", yi.HSV_STEPS)
@pytest.mark.parametrize("fmt", yi.HSV_FORMATS)
def test_hsv_diff_equals_convert_then_scan(dev, fmt, step):
    from avsum_amd import ops, yuv
    offsets = list(yi.HSV_OFFSETS)
    data, L = yi.hsv_case(fmt)
    frames = _frames(dev, data, L, base_offset=L.sample_bytes)
    tables = ops.ShotTables(offsets, 15, dev)
    for matrix in MATRIX_NAMES:
        want = ops.hsv_frame_diff_batch(yuv.yuv_to_bgr(frames, matrix=matrix), tables, step, raw=True)
        got = yuv.yuv_hsv_frame_diff_batch(frames, tables, step, raw=True, matrix=matrix)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        firsts = got[offsets[:-1]]
        assert not firsts.any() and got[[1 + o for o in offsets[1:-1]]].all()      # zeros at the first frames only
        wide = yuv.yuv_hsv_frame_diff_batch(frames, tables, step, matrix=matrix)
        assert wide.dtype == torch.int64 and torch.equal(wide, want.to(torch.int64) & 0xFFFFFFFF)


@pytest.mark.parametrize("fmt", yi.HSV_BIG_FORMATS)
def test_hsv_diff_several_workgroups_per_frame(dev, fmt):
    from avsum_amd import ops, yuv
    offsets = yi.HSV_BIG[1]
    data, L = yi.hsv_case(fmt, big=True)
    frames = _frames(dev, data, L)
    tables = ops.ShotTables(list(offsets), 15, dev)
    bgr = yuv.yuv_to_bgr(frames)
    for step in (1, 2):
        want = ops.hsv_frame_diff_batch(bgr, tables, step, raw=True)
        assert torch.equal(yuv.yuv_hsv_frame_diff_batch(frames, tables, step, raw=True), want)
    with pytest.raises(ValueError, match="yuv_hsv_frame_diff_batch"):
        yuv.yuv_hsv_frame_diff_batch(frames, ops.ShotTables([0, 3], 15, dev))           # another frame count
    with pytest.raises(ValueError, match="yuv_hsv_frame_diff_batch"):
        yuv.yuv_hsv_frame_diff_batch(frames, tables, 0)


# --------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("fmt", yi.E2E_FORMATS)
def test_detect_shots_batch_takes_yuv(dev, fmt):
    from avsum_amd import yuv
    from avsum_amd.features.shots import detect_shots_batch
    data, L, offsets = yi.scene_batch(fmt)
    frames = _frames(dev, data, L)
    for matrix in MATRIX_NAMES:
        from_bgr = detect_shots_batch(yuv.yuv_to_bgr(frames, matrix=matrix), offsets)
        from_yuv = detect_shots_batch(frames, offsets, matrix=matrix)
        assert torch.equal(from_yuv.sums, from_bgr.sums)
        assert from_yuv.host() == from_bgr.host()
        assert torch.equal(from_yuv.sample_index, from_bgr.sample_index)
    assert detect_shots_batch(frames, offsets).host() == yi.scene_cuts()
    with pytest.raises(ValueError, match="detect_shots_batch"):
        detect_shots_batch(frames.like(frames.data.cpu()), offsets)


@pytest.fixture(scope="module")
def proc(dev):
    from avsum_amd.features.extractors import AVProcessor
    torch.manual_seed(13)
    p = AVProcessor(torch.float32, "batch")
    p.visual_extractor.to(dev)
    return p


@pytest.mark.parametrize("fmt", yi.E2E_FORMATS)
def test_embed_shots_takes_yuv(dev, proc, fmt):
    """2 videos, 3 shots, 7 sampled frames of 36 x 70, the default arithmetic: the rows of the converted frames, exactly."""
    from avsum_amd import ops, yuv
    data, L, offsets = yi.embed_batch(fmt)
    frames = _frames(dev, data, L)
    plan = ops.StageOneTables(offsets, list(yi.EMBED_SHOTS), device=dev)
    assert plan.nsamples == 7 and plan.nshots == 3
    want = proc.visual_extractor.embed_shots(yuv.yuv_to_bgr(frames), plan)
    got = proc.visual_extractor.embed_shots(frames, plan)
    assert got.shape == (3, 4096) and got.dtype == torch.float32 and torch.isfinite(got).all() and got.any(dim=1).all()
    assert torch.equal(got, want)
    assert torch.equal(proc.visual_extractor.embed_shots(frames, plan, matrix="bt709"),
                       proc.visual_extractor.embed_shots(yuv.yuv_to_bgr(frames, matrix="bt709"), plan))
    with pytest.raises(ValueError, match="embed_shots"):
        proc.visual_extractor.embed_shots(frames.like(frames.data[1:]), plan)                # another frame count


def test_embed_shots_yuv_frames_of_a_trunks_size(dev, proc):
    """224 x 224 P010 surfaces: the ResNet input is yuv_to_bgr of the pass index, where BGR frames take gather_rows."""
    from avsum_amd import ops, yuv
    data, L = yi.surface("p010", 224, 224, 256, 256, frames=6, seed=4)
    frames = _frames(dev, data, L)
    plan = ops.StageOneTables([0, 6], [[(0, 6)]], device=dev)
    got = proc.visual_extractor.embed_shots(frames, plan, matrix="bt709")
    want = proc.visual_extractor.embed_shots(yuv.yuv_to_bgr(frames, matrix="bt709"), plan)
    assert got.shape == (1, 4096) and torch.equal(got, want)


@pytest.mark.parametrize("fmt", yi.E2E_FORMATS)
def test_process_decoded_batch_takes_yuv(dev, proc, fmt):
    from avsum_amd import yuv
    data, L, offsets = yi.embed_batch(fmt)
    frames = _frames(dev, data, L)
    waves = [np.zeros(int(n / 30 * 16000), dtype=np.float32) for n in yi.EMBED_LENGTHS]
    shots = list(yi.EMBED_SHOTS)
    want = proc.process_decoded_batch(yuv.yuv_to_bgr(frames), offsets, waves, 30.0, shots)
    got = proc.process_decoded_batch(frames, offsets, waves, 30.0, shots)
    assert len(got) == len(want) == 2
    for (vis, aud), (rvis, raud) in zip(got, want):
        assert vis.shape == rvis.shape and vis.dtype == rvis.dtype == np.float32 and vis.any(axis=1).all()
        assert np.array_equal(vis, rvis) and aud.shape == raud.shape and np.array_equal(aud, raud)
    with pytest.raises(ValueError, match="process_decoded_batch"):
        proc.process_decoded_batch(frames.like(frames.data.cpu()), offsets, waves, 30.0, shots)


@pytest.mark.parametrize("fmt", yi.E2E_FORMATS)
def test_process_decoded_batch_detects_on_yuv(dev, proc, fmt):
    """shots=None: the shot scan reads the surfaces too, and the cuts planted in the scene batch come back."""
    from avsum_amd import yuv
    data, L, offsets = yi.scene_batch(fmt)
    frames = _frames(dev, data, L)
    waves = [np.zeros(int((b - a) / 30 * 16000), dtype=np.float32) for a, b in zip(offsets[:-1], offsets[1:])]
    got = proc.process_decoded_batch(frames, offsets, waves, 30.0)
    want = proc.process_decoded_batch(yuv.yuv_to_bgr(frames), offsets, waves, 30.0)
    assert [g[0].shape for g in got] == [(len(c), 4096) for c in yi.scene_cuts()]
    for (vis, aud), (rvis, raud) in zip(got, want):
        assert np.array_equal(vis, rvis) and np.array_equal(aud, raud)


def test_pinned_surfaces_upload_with_pull_copy(dev):
    from avsum_amd import ops, yuv
    data, L = yi.layout_case("p010", "36x70")
    frames = yuv.YuvFrames(torch.zeros(data.shape, dtype=torch.uint8, device=dev), L.h, L.w, **yi.fields(L))
    pinned = frames.pinned_like()
    assert pinned.is_pinned() and pinned.shape == frames.data.shape and pinned.numel() == frames.nbytes
    pinned.copy_(torch.from_numpy(np.array(data)))
    ops.pull_copy(pinned, frames.data)
    assert np.array_equal(yuv.yuv_to_bgr(frames).cpu().numpy(), yuv.frames_to_bgr_host(data, frames))
