"""Host checks of the references and of the bounds test_gpu_audio_f64.py holds the audio front-end kernels of
csrc/audio.hip to (no GPU):

  * every fp32 restatement of audio_f64_inputs lies within its bound at every case the device tests run - a kernel that
    does what its comments say can pass;
  * every planted mistake lies outside it at the case NOTICED_BY names - the bounds do not pass a wrong kernel;
  * a clamp-engaging case has at least 10 % of its float64 dB values (non-empty bands) on either side of the threshold,
    the idle case under 1 % below;
  * the float64 reference is oracle.audio.extract_mel_f64's, the constants are the package's own;
  * the cases reach every instance the issue lists: n_mels != 128 and > 256, empty filters, nfft % 4 != 0, frames an exact
    multiple of 64, the second grid-stride trip, every shot alignment and length class, every table index in range."""
import numpy as np
import pytest

import audio_f64_inputs as afi
from oracle import audio as oa

F32 = np.float32


def _within(cpu, ref):
    ok, err, e32, bound = afi.compare(cpu, ref, cpu)
    return ok and np.isfinite(np.asarray(cpu)).all()


# --------------------------------------------------------------------------- restatements lie within the bounds
@pytest.mark.parametrize("n_mels", [p[1] for p in afi.PLANS])
def test_fused_restatement_within_the_bounds(n_mels):
    k = afi.mel_constants(afi.SR, n_mels)
    worst = 0.0
    for name in afi.SIGNALS:
        for n in afi.LENGTHS:
            x, ref, cpu = afi.fused_bundle(name, n, n_mels)
            assert ref.log2.shape == (1 + n // afi.HOP, n_mels)
            ok, ratio = afi.power_check(cpu.pow, ref.pow, ref.l1, k)
            assert ok, (name, n, ratio)
            worst = max(worst, ratio)
            assert _within(cpu.log2, ref.log2) and _within(cpu.db, ref.db) and _within(cpu.db_clamped, ref.db_clamped), (name, n)
            assert abs(float(cpu.max) - ref.max) <= afi.power_bound(ref.pow, ref.l1, k).max() + 1e-10 * afi.EPS32
            if name == "zeros":
                assert (ref.pow == 0).all() and (cpu.pow == 0).all() and (ref.db == -100.0).all()
    assert 0.1 < worst < 0.75       # the bound is neither slack nor tight for the arithmetic it describes


@pytest.mark.parametrize("n_mels", [128, 40, 320])
@pytest.mark.parametrize("name", ["tones", "gap", "sine", "noise"])
def test_an_fp32_dft_is_outside_the_power_bound_on_every_signal(n_mels, name):
    k = afi.mel_constants(afi.SR, n_mels)
    x = afi.signal(name, 6601)
    ref = afi.mel_reference(x, k)
    assert afi.power_check(afi.mel_restatement(x, k).pow, ref.pow, ref.l1, k)[0]
    ok, ratio = afi.power_check(afi.mel_restatement(x, k, "fp32_dft").pow, ref.pow, ref.l1, k)
    assert not ok and ratio > 2.0, (name, n_mels, ratio)


def test_segment_batch_and_shot_restatements_within_the_bound():
    for n_mels in (p[1] for p in afi.SEG_PLANS):
        for bounds in (afi.SEG_BOUNDS, afi.SEG_BOUNDS_OFFSET):
            _, k, ref, cpu = afi.seg_bundle(n_mels, bounds)
            assert _within(cpu[0], ref[0]) and _within(cpu[1], ref[1]), (n_mels, bounds)
        _, _, ref, cpu = afi.seg_bundle(n_mels)
        assert (ref[0][2] == 0).all() and (cpu[1][2] == 0).all()       # the empty segment
    tracks, bounds, k, ref, cpu, _ = afi.batch_bundle()
    for r, c in zip(ref, cpu):
        assert _within(c[0], r[0]) and _within(c[1], r[1])
    ref, cpu = afi.shot_bundle()
    for r, c in zip(ref, cpu):
        assert _within(c[0], r[0]) and _within(c[1], r[1])


def test_vggish_power_mel_stft_and_resample_restatements_within_their_bounds():
    x, ref, cpu = afi.vgg_bundle()
    for r, c in zip(ref, cpu):
        assert r.shape == (96, 64) and _within(c, r)
    for frames in afi.PM_FRAMES:
        for nbins in afi.PM_BINS:
            k, spec = afi.pm_constants(nbins), afi.pm_case(frames, nbins)
            for mode in range(4):
                (r, rmax), (c, cmax) = afi.pm_reference(spec, k, mode), afi.pm_restatement(spec, k, mode)
                if mode == 2:
                    assert afi.power_check(c, r, np.zeros(frames), k)[0]
                else:
                    assert _within(c, r), (frames, nbins, mode)
    for shape in afi.STFT_SHAPES:
        case = afi.stft_case(*shape)
        assert (np.abs(case.ref.astype(F32).astype(np.float64) - case.ref) <= afi.stft_bound(case)).all()
        ints = afi.stft_case(*shape, integers=True)
        assert np.array_equal(ints.ref, ints.ref.astype(F32).astype(np.float64))      # exactly representable: equality
    for args in afi.resample_cases():
        case = afi.resample_case(*args)
        assert _within(afi.resample_eval(case, np.float32), afi.resample_eval(case, np.float64)), case.label


def test_elementwise_restatements():
    xt, want = afi.quantize_ties()
    assert np.array_equal(((xt.astype(np.float64) + 2.0) * 64.0) % 1.0, np.full(256, 0.5))     # exact ties in fp32
    assert np.array_equal(afi.quantize_restatement(xt, -2.0, 2.0, 64.0), want)
    q = afi.quantize_restatement(afi.quantize_inputs(1000), *afi.QUANT_VGG)
    assert q.min() == 0.0 and q.max() == 255.0 and np.array_equal(q, np.rint(q))
    for t, pad, out_len in afi.REFLECT_SHAPES:
        x = np.arange(1, t + 1, dtype=F32)
        out = afi.reflect_reference(x, pad, out_len)
        assert out.shape == (out_len,) and (out[t + 2 * pad:] == 0).all() and out[pad] == 1.0 and (pad == 0 or out[0] == pad + 1)
    x, mx = afi.clamp_case(1000)
    r64, r32 = afi.clamp_reference(x, mx, np.float64), afi.clamp_reference(x, mx, F32)
    assert _within(r32, r64) and 0.1 < (r64 > x).mean() < 0.9


# --------------------------------------------------------------------------- planted mistakes lie outside them
def test_every_mistake_has_a_case():
    assert set(afi.NOTICED_BY) == set(afi.MISTAKES) and len(afi.MISTAKES) == 21


@pytest.mark.parametrize("mistake", afi.DFT_MISTAKES + afi.MEL_MISTAKES)
def test_fused_mistakes_are_noticed(mistake):
    name, n, n_mels = afi.NOTICED_BY[mistake]
    assert name in afi.SIGNALS and n in afi.LENGTHS and n_mels in [p[1] for p in afi.PLANS]
    k = afi.mel_constants(afi.SR, n_mels)
    x, ref, cpu = afi.fused_bundle(name, n, n_mels)
    wrong = afi.mel_restatement(x, k, mistake)
    pow_ok = afi.power_check(wrong.pow, ref.pow, ref.l1, k)[0]
    log2_ok = afi.compare(wrong.log2, ref.log2, cpu.log2)[0]
    db_ok = afi.compare(wrong.db, ref.db, cpu.db)[0]
    if mistake == "log2_eps_outside":
        assert not log2_ok and pow_ok and db_ok
        live = np.broadcast_to(k.nonempty, ref.log2.shape)         # not only through the -inf of the empty filters
        assert not afi.compare(wrong.log2[live], ref.log2[live], cpu.log2[live])[0]
    elif mistake == "db_floor_missing":
        assert not db_ok and pow_ok and log2_ok
    else:
        assert not pow_ok and not log2_ok and not db_ok, (mistake, pow_ok, log2_ok, db_ok)


@pytest.mark.parametrize("mistake", afi.SEG_MISTAKES)
def test_segment_mistakes_are_noticed(mistake):
    n_mels = afi.NOTICED_BY[mistake]
    assert n_mels in [p[1] for p in afi.SEG_PLANS]
    _, k, ref, cpu = afi.seg_bundle(n_mels)
    wrong = afi.seg_mistaken(n_mels, mistake)
    noticed = [not afi.compare(w, r, c)[0] for w, r, c in zip(wrong, ref[:2], cpu[:2])]
    assert noticed[1] and (noticed[0] or mistake == "clamp_block_max"), (mistake, noticed)


def test_batch_mistake_is_noticed():
    trk = afi.NOTICED_BY["clamp_prev_track_max"]
    tracks, bounds, k, ref, cpu, prev = afi.batch_bundle()
    assert 0 < trk < len(tracks) - 1 and ref[trk][2] < 1e-4 * min(ref[trk - 1][2], ref[trk + 1][2])     # quiet between two loud
    assert not afi.compare(prev[trk], ref[trk][1], cpu[trk][1])[0]
    assert afi.compare(prev[0], ref[0][1], cpu[0][1])[0]


@pytest.mark.parametrize("mistake", afi.SHOT_MISTAKES)
def test_shot_mistakes_are_noticed(mistake):
    s = afi.NOTICED_BY[mistake]
    ref, cpu = afi.shot_bundle()
    wrong = afi.shot_bundle(128, mistake)[1]
    assert not afi.compare(wrong[s][1], ref[s][1], cpu[s][1])[0], mistake
    if mistake != "clamp_whole_track_max":
        assert not afi.compare(wrong[s][0], ref[s][0], cpu[s][0])[0], mistake


@pytest.mark.parametrize("mistake", afi.VGG_MISTAKES)
def test_vggish_mistakes_are_noticed(mistake):
    e = afi.NOTICED_BY[mistake]
    x, ref, cpu = afi.vgg_bundle()
    assert not afi.compare(afi.vgg_restatement(x, afi.VGG_STARTS[e], mistake), ref[e], cpu[e])[0]


@pytest.mark.parametrize("mistake", afi.RESAMPLE_MISTAKES)
def test_resample_mistakes_are_noticed(mistake):
    args = afi.NOTICED_BY[mistake]
    assert args in afi.resample_cases()
    case = afi.resample_case(*args)
    ref, cpu = afi.resample_eval(case, np.float64), afi.resample_eval(case, np.float32)
    assert not afi.compare(afi.resample_eval(case, np.float32, mistake), ref, cpu)[0]


# --------------------------------------------------------------------------- the clamp is exercised
def test_clamp_share_condition():
    for n_mels in (p[1] for p in afi.PLANS):
        k = afi.mel_constants(afi.SR, n_mels)
        for name, n in afi.CLAMP_ENGAGING:
            below, above = afi.clamp_share(afi.fused_bundle(name, n, n_mels)[1], k)
            assert below >= 0.10 and above >= 0.10, (name, n, n_mels, below)
        for name, n in afi.CLAMP_IDLE:
            assert afi.clamp_share(afi.fused_bundle(name, n, n_mels)[1], k)[0] < 0.01       # (a few bins between the tones)
    for n_mels in (p[1] for p in afi.SEG_PLANS):
        k = afi.mel_constants(afi.SR, n_mels)
        below, above = afi.clamp_share(afi.mel_reference(afi.seg_track(), k), k)
        assert below >= 0.10 and above >= 0.10
    ref = afi.shot_bundle()[0]
    quiet, loud = afi.NOTICED_BY["clamp_whole_track_max"], afi.NOTICED_BY["shot_no_pm1_clamp"]
    assert ref[quiet][2] < 1e-8 * ref[loud][2]                      # a quiet shot inside a loud track


# --------------------------------------------------------------------------- references and constants
def test_the_reference_is_the_oracles_and_the_constants_are_the_packages():
    from avsum_amd import audio as pa, vggish as pv
    for n_mels in (128, 40, 320):
        k = afi.mel_constants(afi.SR, n_mels)
        fb = pa.mel_filterbank(afi.SR, n_mels).astype(F32)
        assert np.array_equal(k.fb, fb)
        nz = fb > 0
        assert np.array_equal(k.lo, np.where(nz.any(0), nz.argmax(0), 0)) and (k.fb[:, ~k.nonempty] == 0).all()
        for m in range(n_mels):         # outside [lo, hi) every weight is 0: the walk over all bins is the kernel's walk
            assert (k.fb[:k.lo[m], m] == 0).all() and (k.fb[k.hi[m]:, m] == 0).all()
    x = afi.signal("tones", 6601)
    for n_mels in (128, 40):
        want = oa.extract_mel_f64(x, afi.SR, n_mels)
        assert np.abs(afi.mel_reference(x, afi.mel_constants(afi.SR, n_mels)).log2 - want).max() < 1e-9
    v = afi.vgg_constants()
    assert np.array_equal(v.fb, pv.vggish_mel_matrix().astype(F32)) and v.n_bins == 257 and v.n_mels == 64
    for o, n in afi.RESAMPLE_RATES[:3]:
        taps, width, down, up = afi.resample_taps(o, n)
        ptaps, pwidth, porig, pnew = pa.resample_taps(o, n)
        assert np.array_equal(taps, ptaps) and (width, down, up) == (pwidth, porig, pnew)


# --------------------------------------------------------------------------- every listed instance is reached
def test_the_cases_reach_every_instance():
    # n_mels: != 128, and > 256 (the SEG form's per-band loop takes a second trip) with 73 empty filters; 4 at 128
    assert [p[1] for p in afi.PLANS] == [128, 40] and [p[1] for p in afi.SEG_PLANS] == [128, 320]
    assert int((~afi.mel_constants(afi.SR, 320).nonempty).sum()) == 73 and int((~afi.mel_constants(afi.SR, 128).nonempty).sum()) == 4
    # fused lengths: two frames with the right reflection reaching sample 1, exactly 32 frames, 33, more than two blocks
    assert [1 + n // afi.HOP for n in afi.LENGTHS] == [2, 2, 3, 32, 33, 34, 66]
    # segment table: a 1-frame, a 33-frame and an empty segment; blocks 34 and 66 wholly inside the quiet run
    blocks = afi.segment_blocks(afi.SEG_BOUNDS)
    assert blocks == [(0, 1, 0), (1, 32, 1), (33, 1, 1), (34, 32, 3), (66, 32, 3), (98, 2, 3), (100, 30, 4)]
    assert 1 + afi.SEG_T // afi.HOP == afi.SEG_BOUNDS[-1] == 130
    for f0 in (34, 66):
        assert (f0 - 1) * afi.HOP >= afi.SEG_RUN[0] and (f0 + 31 + 1) * afi.HOP <= afi.SEG_RUN[1]
    assert afi.SEG_BOUNDS_OFFSET[0] > 0
    # batch: lengths that are no multiple of 4, a zeros track
    tracks = afi.batch_tracks()
    assert len(tracks) == 4 and sum(len(t) % 4 != 0 for t in tracks) >= 2 and not tracks[3].any() and all(len(t) > 200 for t in tracks)
    # shots: every alignment of the first sample, every length class, empty / clipped / loud, every index in range
    shots, tr = afi.shot_list(), afi.shot_tracks()
    offs = [0, (len(tr[0]) + 3) // 4 * 4]
    assert {(offs[t] + a) % 4 for t, a, n in shots if n > 0} == {0, 1, 2, 3}
    assert {1, 350, 959, 960, 961, 7000} <= {n for _, _, n in shots} and 0 in {n for _, _, n in shots}
    assert all(0 <= a and a + n <= len(tr[t]) for t, a, n in shots)
    assert shots[8] == (0, 19000, len(tr[0]) - 19000) and afi.SHOT_BOUNDS[0][8][1] > len(tr[0])       # clipped by the track end
    assert np.abs(tr[0][3001:10001]).max() > 1.0
    # stft: nfft % 4 != 0 three times, frames = 64 exactly, one frame, a third block
    assert [s[2] % 4 for s in afi.STFT_SHAPES] == [0, 2, 2, 2] and afi.STFT_SHAPES[1][0] == 64
    assert [afi.stft_case(*s).ncols_pad for s in afi.STFT_SHAPES] == [128, 192, 64, 64]
    # VGGish: the last legal start, overlapping examples, samples beyond +-1 in three of the four
    x = afi.vgg_waves()
    assert afi.VGG_STARTS[2] + afi.VGG_EX_LEN == len(x) and afi.VGG_STARTS[1] - afi.VGG_STARTS[0] < afi.VGG_EX_LEN
    assert [bool(np.abs(x[s:s + afi.VGG_EX_LEN]).max() > 1) for s in afi.VGG_STARTS] == [True, True, False, True]
    # elementwise: one element past the 8192 x 256 threads of one trip
    assert afi.BIG > 8192 * 256 and afi.BIG * 4 < 9_000_000 and 0 in afi.SMALL_COUNTS
    assert afi.REFLECT_BIG[2] == afi.BIG and afi.REFLECT_BIG[2] > afi.REFLECT_BIG[0] + 2 * afi.REFLECT_BIG[1]
    # resample: every rate pair with 1, 2, 3 channels; clips of 1 sample, shorter than the filter, and 3001
    cases = afi.resample_cases()
    assert {c[:2] for c in cases} == set(afi.RESAMPLE_RATES) and {c[2] for c in cases} == {1, 2, 3}
    for o, n in afi.RESAMPLE_RATES[:3]:
        width = afi.resample_taps(o, n)[1]
        assert {c[3] for c in cases if c[:2] == (o, n)} == {1, width - 1, 3001}
    for c in cases:
        case = afi.resample_case(*c)
        assert (case.out_len - 1) // case.up * case.down - case.width < case.t and case.out_len <= 65536 * 256
