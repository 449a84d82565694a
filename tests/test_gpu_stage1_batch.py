"""Batched stage-1 extraction on the GPU: the two glue kernels bit for bit against the kernels they replace, and
AVProcessor.process_decoded_batch against the per-video process_decoded loop and the oracle."""
import numpy as np
import pytest
import torch

import stage1_batch_inputs as s1

pytestmark = pytest.mark.gpu

BAR = 5e-4       # the project's feature bar (test_gpu_configs, smoke()): |d| < BAR * max(1, |ref|.max())


# --------------------------------------------------------------------------- resize_gather
RESIZE_SOURCES = [(5, 37, 53), (4, 240, 320), (3, 224, 224)]     # upscale to both sizes, downscale to both, 299 only


def _resize_case(dev, shape, seed):
    n, h, w = shape
    src = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(dev)
    # repeats, descending order and (entry 2) one row outside src
    idx = torch.tensor([n - 1, n - 1, n, 0, n - 2, 1, 0], dtype=torch.int64, device=dev)
    sizes = [s for s in ((224, 224), (299, 299)) if s != (h, w)]
    return src, idx, sizes


@pytest.mark.parametrize("shape", RESIZE_SOURCES)
def test_resize_gather_equals_gather_then_resize(dev, shape):
    from avsum_amd import ops
    src, idx, sizes = _resize_case(dev, shape, 31)
    count, bad = idx.numel(), 2
    outs = [torch.full((count, dh, dw, 3), 7, dtype=torch.uint8, device=dev) for dh, dw in sizes]
    got = ops.resize_gather(src, idx, count, sizes, outs)
    assert all(g is o for g, o in zip(got, outs))
    valid = [i for i in range(count) if i != bad]
    for (dh, dw), out in zip(sizes, outs):
        want = ops.resize_bilinear(src.index_select(0, idx[valid]), dh, dw)
        assert np.array_equal(out[valid].cpu().numpy(), want.cpu().numpy()), (dh, dw)
        assert (out[bad] == 7).all()                                  # the row outside src: left as it was
    # one launch for two sizes = one launch per size
    for k, size in enumerate(sizes):
        single = torch.full_like(outs[k], 7)
        ops.resize_gather(src, idx, count, [size], [single])
        assert torch.equal(single, outs[k])
    # a count below the index length, outs allocated by the call, and bases that are views into their buffers (a frame of
    # 37 * 53 * 3 bytes is odd: no alignment at all)
    tail = idx[3:]                                                    # rows 0, n - 2, 1, 0
    part = ops.resize_gather(src[1:], tail, 2, sizes[-1:])[0]
    assert torch.equal(part, ops.resize_bilinear(src[1:].index_select(0, tail[:2]), *sizes[-1]))


def test_resize_gather_tall_band(dev):
    """A source whose bands need more LDS than one workgroup may take at 8 output rows: the band is halved."""
    from avsum_amd import ops
    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, 700, 1500, 3), dtype=np.uint8)).to(dev)
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    a, b = ops.resize_gather(src, idx, 1, [(224, 224), (299, 299)])
    assert torch.equal(a, ops.resize_bilinear(src, 224, 224)) and torch.equal(b, ops.resize_bilinear(src, 299, 299))


def test_resize_gather_refusals(dev):
    from avsum_amd import ops
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    size = [(4, 4)]
    for frames, index, count, sizes in [
            (src.cpu(), idx, 2, size), (src, idx.cpu(), 2, size),                       # host tensors
            (src.float(), idx, 2, size), (src, idx.int(), 2, size),                     # wrong dtypes
            (src[..., :2], idx, 2, size), (src[0], idx, 2, size), (src, idx[:, None], 2, size),   # wrong shapes
            (src, idx, 3, size), (src, idx, -1, size),                                  # count outside the index
            (src, idx, 2, []), (src, idx, 2, size * 3), (src, idx, 2, [(0, 4)])]:
        with pytest.raises(ValueError, match="resize_gather"):
            ops.resize_gather(frames, index, count, sizes)
    with pytest.raises(ValueError, match="resize_gather"):
        ops.resize_gather(src, idx, 2, size, [torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=dev)])


# --------------------------------------------------------------------------- segment_mean_perm
def test_segment_mean_perm_equals_segment_mean_of_permuted_rows(dev):
    from avsum_amd import ops
    g = torch.Generator().manual_seed(17)
    wide = torch.randn((23, 64), generator=g).to(dev)
    x = wide[:, 11:51]                                               # [23, 40]: a column slice
    perm = torch.randperm(23, generator=g).to(dev)
    offsets = [0, 0, 1, 13, 23]                                      # an empty segment, one row, 12 rows, 10 rows
    seg = torch.tensor(offsets, dtype=torch.int64, device=dev)
    buf = torch.full((4, 96), -3.0, device=dev)
    got = ops.segment_mean_perm(x, perm, seg, buf[:, 40:80])
    want = ops.segment_mean(x[perm].contiguous(), seg)
    assert got.data_ptr() == buf[:, 40:80].data_ptr()
    assert np.array_equal(buf[:, 40:80].cpu().numpy(), want.cpu().numpy())
    assert not want[0].any() and (buf[:, :40] == -3.0).all() and (buf[:, 80:] == -3.0).all()
    # the offsets as a validated table: the same bytes, and its span is checked against perm
    table = ops.RaggedOffsets(offsets, "test", device=dev, min_length=0)
    assert torch.equal(ops.segment_mean_perm(x, perm, table), want)
    with pytest.raises(ValueError, match="segment_mean_perm"):
        ops.segment_mean_perm(x, perm[:22].contiguous(), table)


def test_segment_mean_perm_refusals(dev):
    from avsum_amd import ops
    x = torch.zeros((6, 8), device=dev)
    perm = torch.arange(6, device=dev)
    seg = torch.tensor([0, 6], dtype=torch.int64, device=dev)
    for a, p, s in [(x.cpu(), perm, seg), (x, perm.cpu(), seg), (x, perm, seg.cpu()),          # host tensors
                    (x.double(), perm, seg), (x, perm.int(), seg), (x, perm, seg.int()),       # wrong dtypes
                    (x[0], perm, seg), (x.t(), perm, seg), (x, perm[:, None], seg), (x, perm, seg[:, None])]:   # shapes
        with pytest.raises(ValueError, match="segment_mean_perm"):
            ops.segment_mean_perm(a, p, s)
    with pytest.raises(ValueError, match="segment_mean_perm"):
        ops.segment_mean_perm(x, perm, seg, torch.zeros((2, 8), device=dev))


# --------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def batch(dev):
    """The three videos, one f32 processor, and the rows of the per-video loop - computed once, left unchanged."""
    from avsum_amd.features.extractors import AVProcessor
    torch.manual_seed(9)
    proc = AVProcessor(torch.float32, "batch")
    rsd = {k: v.clone() for k, v in proc.visual_extractor.resnet.state_dict().items()}
    isd = {k: v.clone() for k, v in proc.visual_extractor.inception.state_dict().items()}
    proc.visual_extractor.to(dev)
    frames, offsets, waves = s1.frames(), s1.offsets_of(s1.LENGTHS), s1.waveforms()
    loop = [proc.process_decoded(frames[offsets[v]:offsets[v + 1]], waves[v], s1.FPS[v], s1.SHOTS[v], batch_audio=True)
            for v in range(3)]
    return {"proc": proc, "rsd": rsd, "isd": isd, "frames": frames, "offsets": offsets, "waves": waves, "loop": loop,
            "frames_t": torch.from_numpy(frames).to(dev)}


def _same_kind(a, b):
    assert type(a) is type(b) and a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)


def test_batch_equals_the_per_video_loop(dev, batch):
    proc = batch["proc"]
    got = proc.process_decoded_batch(batch["frames_t"], batch["offsets"], batch["waves"], s1.FPS, s1.SHOTS)
    assert len(got) == 3
    worst = 0.0
    for v, ((vis, aud), (rvis, raud)) in enumerate(zip(got, batch["loop"])):
        _same_kind(vis, rvis)
        _same_kind(aud, raud)
        assert np.array_equal(aud, raud)                              # strict mode: float64 zeros, or np.array([])
        if not s1.SHOTS[v]:
            assert vis.shape == (0,) and vis.dtype == np.float64 and aud.shape == (0,)
            continue
        assert aud.dtype == np.float64 and aud.shape == (len(s1.SHOTS[v]), 296) and not aud.any()
        zero = ~rvis.any(axis=1)
        assert np.array_equal(vis[zero], rvis[zero])                  # the empty shots: exactly zero rows
        err = np.abs(vis - rvis).max()
        worst = max(worst, err / max(1.0, np.abs(rvis).max()))
        print(f"video {v}: max |batch - loop| = {err:.3e}, |loop|.max() = {np.abs(rvis).max():.3e}")
        assert err < BAR * max(1.0, np.abs(rvis).max())
    assert [int((~r[0].any(axis=1)).sum()) for r in (batch["loop"][0], batch["loop"][2])] == [2, 1]
    # a numpy batch is uploaded by the call; passes of at most 8 frames hold the same groups
    again = proc.process_decoded_batch(batch["frames"], batch["offsets"], batch["waves"], s1.FPS, s1.SHOTS, chunk_frames=8)
    for (vis, aud), (rvis, raud) in zip(again, batch["loop"]):
        _same_kind(vis, rvis)
        assert np.abs(vis - rvis).max(initial=0.0) < BAR * max(1.0, np.abs(rvis).max(initial=0.0))


def test_batch_against_the_oracle(dev, batch):
    """Video 2 - 7 sampled frames in the shots (3, 3) and (0, 20) - against the float oracle, shot by shot."""
    from avsum_amd.features.extractors import sample_shot_indices
    from oracle import cnn as ocnn
    v = 2
    video = batch["frames"][batch["offsets"][v]:batch["offsets"][v + 1]]
    want = np.array([ocnn.visual_forward(batch["rsd"], batch["isd"], [video[i] for i in sample_shot_indices(s, min(e, len(video)))])
                     for s, e in s1.SHOTS[v]])
    got = batch["proc"].process_decoded_batch(video, [0, len(video)], [batch["waves"][v]], s1.FPS[v], [s1.SHOTS[v]])[0][0]
    assert got.shape == want.shape == (2, 4096) and got.dtype == np.float32
    assert not got[0].any()
    err = np.abs(got - want).max()
    print(f"max |batch - oracle| = {err:.3e}, |oracle|.max() = {np.abs(want).max():.3e}")
    assert err < BAR * max(1.0, np.abs(want).max())


def test_frames_already_224(dev, batch):
    """224 x 224 frames go to the ResNet trunk by gather_rows; only the Inception input is resized.  One group of 3."""
    proc = batch["proc"]
    video = np.random.default_rng(23).integers(0, 256, (8, 224, 224, 3), dtype=np.uint8)
    wave = np.zeros(4000, dtype=np.float32)
    want = proc.process_decoded(video, wave, 30.0, [(0, 8)], batch_audio=True)[0]
    got = proc.process_decoded_batch(video, [0, 8], [wave], 30.0, [[(0, 8)]])[0][0]
    _same_kind(got, want)
    err = np.abs(got - want).max()
    print(f"max |batch - loop| = {err:.3e}, |loop|.max() = {np.abs(want).max():.3e}")
    assert want.shape == (1, 4096) and err < BAR * max(1.0, np.abs(want).max())


def test_audio_rows_intent_mode(dev, batch):
    proc = batch["proc"]
    bounds = [[(int(s / f * proc.sr), int(e / f * proc.sr)) for s, e in shots] for shots, f in zip(s1.SHOTS, s1.FPS)]
    proc.audio_extractor.strict_reference = False
    try:
        got = proc.process_decoded_batch(batch["frames_t"], batch["offsets"], batch["waves"], s1.FPS, s1.SHOTS)
        direct = proc.audio_extractor.forward_shots_batch(batch["waves"], bounds)
    finally:
        proc.audio_extractor.strict_reference = True
    assert direct.shape == (6, 296) and direct.dtype == np.float32 and np.isfinite(direct).all() and direct.any()
    assert np.array_equal(got[0][1], direct[:4]) and np.array_equal(got[2][1], direct[4:])
    assert got[0][1].dtype == np.float32 and got[1][1].shape == (0,) and got[1][0].shape == (0,)


def test_detected_shots_and_shot_batch_result(dev, batch):
    """shots=None and a ShotBatchResult give the rows of the host-list call, exactly (two copies of the two-cut video)."""
    from avsum_amd.features.shots import detect_shots_batch
    proc = batch["proc"]
    one = s1.two_cut_video()
    frames = torch.from_numpy(np.concatenate([one, one])).to(dev)
    offsets, waves = [0, 64, 128], [np.zeros(int(64 / 30 * 16000), dtype=np.float32)] * 2
    shots = [(0, 22), (22, 45), (45, 64)]
    by_list = proc.process_decoded_batch(frames, offsets, waves, 30.0, [shots, shots])
    result = detect_shots_batch(frames, offsets)
    assert result.host() == [shots, shots]
    for other in (proc.process_decoded_batch(frames, offsets, waves, 30.0),
                  proc.process_decoded_batch(frames, offsets, waves, [30.0, 30.0], result)):
        for (vis, aud), (rvis, raud) in zip(other, by_list):
            _same_kind(vis, rvis)
            _same_kind(aud, raud)
            assert vis.shape == (3, 4096) and np.array_equal(vis, rvis) and np.array_equal(aud, raud)
    assert by_list[0][0].any(axis=1).all() and not by_list[0][1].any()
    with pytest.raises(ValueError, match="process_decoded_batch"):
        proc.process_decoded_batch(frames, [0, 60, 128], waves, 30.0, result)


def test_embed_shots_f16x2(dev, batch):
    """The headline arithmetic on the same batch, in passes of at most 16 frames, against the f32 embed_shots rows."""
    from avsum_amd import ops
    from avsum_amd.features.extractors import VisualFeatureExtractor
    f32 = batch["proc"].visual_extractor
    h2 = VisualFeatureExtractor(arith="f16x2")
    h2.resnet.load_state_dict(batch["rsd"])
    h2.inception.load_state_dict(batch["isd"])
    h2.to(dev)
    want = f32.embed_shots(batch["frames_t"], ops.StageOneTables(batch["offsets"], s1.SHOTS, device=dev))
    plan = ops.StageOneTables(batch["offsets"], s1.SHOTS, chunk_frames=16, device=dev)
    assert len(plan.passes) > 1
    got = h2.embed_shots(batch["frames_t"], plan)
    assert got.shape == want.shape == (6, 4096) and got.dtype == torch.float32 and got.is_cuda
    assert torch.isfinite(got).all()
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(f"max |f16x2 - f32| = {err:.3e}, |f32|.max() = {scale:.3e}")
    assert err < BAR * scale
    with pytest.raises(ValueError, match="embed_shots"):
        f32.embed_shots(batch["frames_t"][:-1], plan)
    with pytest.raises(ValueError, match="embed_shots"):
        f32.embed_shots(batch["frames_t"], ops.StageOneTables(batch["offsets"], s1.SHOTS, device="cpu"))
