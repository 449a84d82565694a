"""Per-shot audio features in one set of launches (avs_stft_mel_shots_f32 + avs_vggish_examples_f32): every shot is its
own signal - zero padded to 960 samples, clamped to [-1, 1], reflect padded at its own ends, top_db relative to its own
maximum, VGGish framing from its first sample - as features/extractors.py:195-234 compute on waveform[s0:s1]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SR = 16000


def _tones(n, seed, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f = 200.0 + 3000.0 * rng.random(3)
    x = sum(amp * np.sin(2 * np.pi * fi * t) for fi in f) + 0.01 * rng.standard_normal(n)
    return x.astype(np.float32)


def _tracks():
    """3 tracks of different lengths (one not a multiple of 4) with a near-silent run and a run beyond +-1."""
    a = _tones(50003, 1)
    a[20000:30000] = 1e-4 * np.random.default_rng(2).standard_normal(10000).astype(np.float32)   # near silence
    a[40000:43000] *= 4.0                                                                        # beyond +-1
    b = _tones(36000, 3, 0.2)
    c = _tones(20001, 4, 0.5)
    bounds = [[(0, 17000),        # one VGGish example
               (100, 450),        # shorter than 400: padded to 960
               (5, 6),            # one sample
               (700, 700),        # empty
               (45001, 60000),    # clipped by the track end
               (39001, 41500),    # odd offset, overlaps the next one
               (40000, 43000),    # samples beyond +-1
               (21000, 29000)],   # near-silent inside a loud track: the per-shot top_db clamp matters
              [(3, 19000), (10000, 12003)],
              [(0, 20001), (7777, 9001)]]
    return [a, b, c], bounds


def _shot_signal(w, s0, s1):
    x = np.asarray(w[s0:s1], dtype=np.float32)
    if 0 < x.size < 960:
        x = np.pad(x, (0, 960 - x.size))
    return np.clip(x, -1, 1)


@pytest.fixture(scope="module")
def ext():
    from avsum_amd.features.extractors import AudioFeatureExtractor
    torch.manual_seed(7)
    return AudioFeatureExtractor(strict_reference=False)


def test_shots_vs_float64_oracle(dev, ext):
    from oracle import audio as oa, vggish as ov
    waves, bounds = _tracks()
    got = ext.forward_shots_batch(waves, bounds)
    assert got.shape == (sum(len(b) for b in bounds), 296) and got.dtype == np.float32
    sd = {k: v.cpu() for k, v in ext.vggish.state_dict().items()}
    row = 0
    for w, bb in zip(waves, bounds):
        for s0, s1 in bb:
            x = _shot_signal(w, s0, s1)
            g = got[row]
            row += 1
            if x.size == 0:
                assert not g.any()
                continue
            mel = oa.extract_mel_f64(x).mean(0)
            assert np.abs(g[40:168] - mel).max() <= 1e-4, (s0, s1)
            mf = oa.mfcc(torch.from_numpy(x)).double().mean(1).numpy()
            assert np.abs(g[:40] - mf).max() <= 1e-4 * np.abs(mf).max(), (s0, s1)
            if ov.num_examples(x.size) == 0:
                assert not g[168:].any()
            else:
                vg = ov.vggish_forward(sd, x).mean(0).numpy()
                assert np.abs(g[168:] - vg).max() <= 1.0, (s0, s1)


def test_shots_vs_per_shot_path(dev, ext, monkeypatch):
    from avsum_amd import ops
    from avsum_amd.audio import MelPlan
    from avsum_amd.features import extractors
    from avsum_amd.features.extractors import AudioFeatureExtractor
    from avsum_amd.vggish import VGGishFrontEnd
    waves, bounds = _tracks()
    w, bb = waves[0], bounds[0] + [(30001, 47000)]
    got = ext.forward_shots(w, bb)
    want = np.array([ext(w[a:b]) for a, b in bb])
    assert got.shape == want.shape and got.dtype == want.dtype
    # log2-mel means: the same per-frame arithmetic, only the order of the mean's sum differs
    d = np.abs(got[:, 40:168] - want[:, 40:168])
    assert (d <= 2e-5 + 1e-5 * np.abs(want[:, 40:168])).all(), d.max()
    # MFCC means: the DCT of the mean dB row against the mean of the per-frame DCTs (linear; fp32 rounding of either)
    d = np.abs(got[:, :40] - want[:, :40])
    assert (d <= 2e-5 + 1e-5 * np.abs(want[:, :40]).max(1, keepdims=True)).all(), d.max()
    # VGGish: the batched log-mel examples are bit-identical to the per-shot front end's
    tables = MelPlan.shot_tables([w], [bb], dev)
    fe = VGGishFrontEnd.get(dev)
    ex = ops.vggish_examples(tables.waves, tables.ex_start, fe.basis_t, fe.fb, fe.fb_lo, fe.fb_hi)
    seg = tables.ex_seg.tolist()
    assert ex.shape[0] == seg[-1] >= 2
    for s, (a, b) in enumerate(bb):
        one = fe.examples(torch.from_numpy(_shot_signal(w, a, b)).to(dev))
        assert torch.equal(ex[seg[s]:seg[s + 1]], one), (a, b)
    # quantised embeddings: identical up to rare +-1 round-off flips (the bar of test_vggish_vs_oracle)
    d = np.abs(got[:, 168:] - want[:, 168:])
    assert d.max() <= 1 and (d > 0).mean() < 0.01
    # strict mode: the literal zeros (float64 rows, float32 for an empty shot) and no GPU work
    strict = AudioFeatureExtractor()
    ref = np.array([strict(w[a:b]) for a, b in bb])

    def no_gpu(*a, **k):
        raise AssertionError("strict mode launched GPU work")
    monkeypatch.setattr(extractors, "_device", no_gpu)
    monkeypatch.setattr(ops, "stft_mel_shots", no_gpu)
    monkeypatch.setattr(ops, "vggish_examples", no_gpu)
    z = strict.forward_shots(w, bb)
    assert z.shape == ref.shape and z.dtype == ref.dtype == np.float64 and not z.any()


def test_per_shot_semantics_differ_from_the_whole_track_variant(dev, ext):
    """The whole-track variant (segment_means_batch) pools the track's STFT frames by shot and clamps against the track's
    maximum; per shot, the frames at the boundaries and the quiet shot's MFCC differ by far more than the bars."""
    from avsum_amd.audio import MelPlan
    a = _tones(32000, 9, 0.5)
    a[8000:20000] = 1e-4 * np.random.default_rng(5).standard_normal(12000).astype(np.float32)
    shots = [(0, 8000), (8000, 20000), (20000, 32000)]
    got = ext.forward_shots(a, shots)
    plan = MelPlan.get(SR, 128, 40, dev)
    frames = [0, 40, 100, 1 + 32000 // 200]
    tables = plan.batch_tables([torch.from_numpy(a)], [frames], dev)
    log2, db = (torch.empty((3, 128), device=dev) for _ in range(2))
    plan.segment_means_batch(tables, log2, db)
    from avsum_amd import ops
    mf = ops.linear(db, plan.dct).cpu().numpy()
    d_mel = np.abs(got[:, 40:168] - log2.cpu().numpy()).max(1)
    assert (d_mel > 1e-2).all(), d_mel                      # every shot: boundary frames (bar: 2e-5)
    d_mf = np.abs(got[1, :40] - mf[1]).max()
    assert d_mf > 1e-2 * np.abs(mf[1]).max(), d_mf         # quiet shot: its own top_db clamp (bar: 1e-5 of the scale)


def test_batch_equals_single_and_is_deterministic(dev, ext):
    waves, bounds = _tracks()
    waves.append(_tones(17003, 11))
    bounds.append([(1, 16999), (0, 3)])
    batch = ext.forward_shots_batch(waves, bounds)
    again = ext.forward_shots_batch(waves, bounds)
    assert np.array_equal(batch, again)
    single = np.concatenate([ext.forward_shots(w, b) for w, b in zip(waves, bounds)])
    assert np.array_equal(batch, single)


def test_process_decoded_batch_audio(dev):
    from avsum_amd.features.extractors import AVProcessor
    torch.manual_seed(3)
    proc = AVProcessor(strict_reference=False)
    proc.visual_extractor.to(dev)
    rng = np.random.default_rng(6)
    frames = [rng.integers(0, 256, (64, 80, 3), dtype=np.uint8) for _ in range(45)]
    wave = _tones(16000 * 2, 13)
    shots = [(0, 20), (20, 21), (21, 45), (44, 60)]
    v0, a0 = proc.process_decoded(frames, wave, 25.0, shots)
    v1, a1 = proc.process_decoded(frames, wave, 25.0, shots, batch_audio=True)
    assert np.array_equal(v0, v1)
    assert a1.shape == a0.shape and a1.dtype == a0.dtype
    d = np.abs(a1[:, :168] - a0[:, :168])
    assert (d[:, 40:] <= 2e-5 + 1e-5 * np.abs(a0[:, 40:168])).all()
    assert (d[:, :40] <= 2e-5 + 1e-5 * np.abs(a0[:, :40]).max(1, keepdims=True)).all()
    dv = np.abs(a1[:, 168:] - a0[:, 168:])
    assert dv.max() <= 1 and (dv > 0).mean() < 0.01
