"""The audio front-end kernels (csrc/audio.hip), each on its own against float64: avs_stft_mel_fused_f32 (log2 / dB / power
from one launch and each alone, 128 and 40 mels), avs_stft_mel_segmean_f32 (one pass and two passes, 128 and 320 mels), its
batch form, avs_stft_mel_shots_f32, avs_vggish_examples_f32, avs_stft_f64, avs_power_mel_f32 (modes 0-3), and
avs_clamp_topdb_f32 / avs_fill_f32 / avs_quantize_f32 / avs_reflect_pad_f32 / avs_resample_f32.  Cases, references,
restatements and the bounds come from audio_f64_inputs; test_audio_f64_host.py shows on the host that the bounds pass the
fp32 restatements and fail every planted mistake, and that the cases reach every instance.

Bounds: log-domain outputs are held to scorer_f64_inputs.compare (4 e32 + 8 eps32 max(1, max|ref|)); mel power to the
per-element bound of audio_f64_inputs.power_bound; avs_stft_f64 on float data to stft_bound and on integer data to
equality; reflect_pad, fill, quantize, power_mel mode 2 and the mode-1 maximum to equality with the fp32 restatement.

Every destination is pre-filled with NaN in its window and with a sentinel in its pad columns and beyond its count: the
window must be finite afterwards, everything else bit for bit what it was.  Every call runs twice, into fresh
destinations, and must give the same bits.  Waveforms are followed by sentinel samples, so a read past a clip shows.

Left out on purpose: device tables with out-of-range entries (the kernels clamp them; a wrong clamp would fault a shared
machine); the second trip of resample's grid (its cap of 65 536 blocks needs 67 MB of output); misaligned waveforms
(refusals are covered on the host side).

RATIO lines (printed per check; run with -s).  Measured on an MI355X over all cases of this file: the number of checks,
the largest err / e32 (err / bound for the per-element bounds of mel power and avs_stft_f64), and the check that came
closest to its bound:

  family                        checks  largest ratio     closest to its bound
  fused, 128 mels: power        35      err/bound 0.50    tones t=13000
  fused, 128 mels: log2, dB,    105     err/e32 3.50      tones t=13000 db_clamped: err 8.1e-6, bound 8.0e-5
    dB clamped
  fused, 40 mels: power         35      err/bound 0.41    tones t=6399
  fused, 40 mels: log2, dB,     105     err/e32 3.50      noise t=6399 db: err 5.4e-6, bound 4.3e-5
    dB clamped
  segmean (128 and 320 mels)    8       err/e32 1.26      320 mels, bounds [0, 1, 34, 34, 100, 130] log2: err 6.7e-6, bound 4.0e-5
  batch                         8       err/e32 3.50      track 1 (tones x 1e-3) log2: err 4.3e-6, bound 3.1e-5
  shots                         22      err/e32 1.79      shot 5 (first 3001, L 7000) db: err 1.2e-5, bound 8.9e-5
  vggish                        4       err/e32 1.75      start 0: err 5.9e-7, bound 5.7e-6
  stft_f64 (float data)         4       err/bound 0.50    frames=64 hop=5 nfft=6 ncols=129
  power_mel modes 0, 1, 3       27      err/e32 2.75      1 frame, 1025 bins, mode 3: err 6.0e-7, bound 4.7e-6
  power_mel mode 2              9       err/bound 0.34    13 frames, 201 bins
  clamp_topdb                   5       err/e32 1.00      count 255: err 2.0e-6, bound 6.9e-5
  resample                      31      err/e32 1.00      44100->16000 mono t=3001: err 1.6e-7, bound 1.6e-6

No check uses more than 17 % of a compare bound or more than half of a per-element bound (half: one fp32 rounding of a
value the bound allows two half-ulps for).  err / e32 above 1 comes from the device's log2f / log10f / logf against
numpy's (the 3.50 are log2(0 + 1e-6) of the all-zero signals and of the empty filters: 1.5e-6, 0.8 ulp, on the device
against 4.2e-7 in numpy).  The restatement
equalities of power_mel (mode 2, the mode-1 maximum) hold on the device, as do those of fill, quantize and reflect_pad."""
import numpy as np
import pytest
import torch

import audio_f64_inputs as afi

pytestmark = pytest.mark.gpu

S = afi.SENTINEL
NAN = float("nan")
TAIL = 8
F32 = np.float32


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _plan(dev, n_mels):
    """The package's device constants (window, folded DFT tables, filterbank) for n_mels; the filterbank is the one the
    references use (asserted on the host)."""
    from avsum_amd.audio import MelPlan
    plan = MelPlan.get(afi.SR, n_mels, {128: 40, 40: 13}.get(n_mels, 40), dev)
    k = afi.mel_constants(afi.SR, n_mels)
    assert np.array_equal(plan.fb.cpu().numpy(), k.fb) and np.array_equal(plan.fb_lo.cpu().numpy(), k.lo)
    assert np.array_equal(plan.fb_hi.cpu().numpy(), k.hi)
    return plan, k


def _consts(plan):
    ops, _ = _api()
    return tuple(ops._p(t) for t in (plan.window, plan.cos_t, plan.sin_t, plan.fb, plan.fb_lo, plan.fb_hi))


def _wave(x, dev, pad_to=1):
    """x on the device followed by sentinel samples (a fresh, 16-byte aligned allocation)."""
    n = -(-len(x) // pad_to) * pad_to
    buf = torch.full((n + TAIL,), S, dtype=torch.float32)
    buf[:len(x)] = torch.from_numpy(np.array(x, dtype=F32))      # (a copy: the seeded signals are read-only)
    buf[len(x):n] = 0.0
    return buf.to(dev)


class Dest:
    """A destination [rows, cols] in rows ``ld`` wide, followed by TAIL elements: NaN inside the window, the sentinel in
    the pad columns and in the tail."""

    def __init__(self, rows, cols, dev, ld=None, fill=NAN):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        assert self.ld >= cols
        host = torch.full((rows * self.ld + TAIL,), S, dtype=torch.float32)
        host[:rows * self.ld].view(rows, self.ld)[:, :cols] = fill
        self.before = host
        self.buf = host.to(dev)

    def read(self):
        """The window as numpy, after asserting that nothing outside it changed and that it is finite."""
        after = self.buf.cpu()
        a, b = after.clone().view(torch.int32), self.before.clone().view(torch.int32)
        n = self.rows * self.ld
        a[:n].view(self.rows, self.ld)[:, :self.cols] = 0
        b[:n].view(self.rows, self.ld)[:, :self.cols] = 0
        assert torch.equal(a, b), "a pad column or an element beyond the count was written"
        got = after[:n].view(self.rows, self.ld)[:, :self.cols].contiguous().numpy()
        assert np.isfinite(got).all(), "a destination element was left unwritten or is not finite"
        return got


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ratio(family, label, name, err, yard, bound, kind="err/e32"):
    ratio = err / yard if yard > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO family={family!r} case={label!r} tensor={name} err={err:.3e} yard={yard:.3e} bound={bound:.3e} {kind}={ratio:.2f}")


def _check(family, label, name, got, ref, cpu32):
    ok, err, e32, bound = afi.compare(got, ref, cpu32)
    _ratio(family, label, name, err, e32, bound)
    assert ok, f"{family} {label} {name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"


def _check_power(family, label, got, ref_pow, l1, k):
    ok, ratio = afi.power_check(got, ref_pow, l1, k)
    print(f"RATIO family={family!r} case={label!r} tensor=power err/bound={ratio:.2f}")
    assert ok, f"{family} {label} power: err / bound {ratio:.2f}"


# --------------------------------------------------------------------------- the fused kernel
def _fused(plan, k, wave, t, log2=False, db=False, power=False, gmax=False):
    """avs_stft_mel_fused_f32 through the C ABI into destinations of the caller -> (log2, db, power, max) as numpy."""
    ops, abi = _api()
    frames = 1 + t // afi.HOP
    dev = wave.device
    d = [Dest(frames, k.n_mels, dev) if on else None for on in (log2, db, power)]
    m = Dest(1, 1, dev, fill=0.0) if (db or gmax) else None      # the caller zeroes the maximum
    abi.check(abi.lib().avs_stft_mel_fused_f32(ops._p(wave), t, *_consts(plan), k.n_mels, *(ops._p(x.buf) if x else None for x in d),
                                               ops._p(m.buf) if m else None, ops._stream()), "avs_stft_mel_fused_f32")
    return tuple(x.read() if x else None for x in d) + (m.read()[0, 0] if m else None,)


@pytest.mark.parametrize("name", afi.SIGNALS)
@pytest.mark.parametrize("n_mels", [p[1] for p in afi.PLANS])
def test_fused_front_end(dev, n_mels, name):
    """201 .. 13000 samples (2 frames with the right reflection reaching sample 1; 32, 33, 34 and 66 frames): log2, dB and
    power from one launch against float64, each alone and the maximum alone bit for bit the same, the dB rows again after
    avs_clamp_topdb_f32 at the launch's own maximum (gap and sine: the clamp engages)."""
    ops, abi = _api()
    plan, k = _plan(dev, n_mels)
    for n in afi.LENGTHS:
        x, ref, cpu = afi.fused_bundle(name, n, n_mels)
        label = f"{name} t={n} mels={n_mels}"
        wave = _wave(x, dev)
        log2, db, pw, mx = _fused(plan, k, wave, n, log2=True, db=True, power=True)
        _check_power("fused", label, pw, ref.pow, ref.l1, k)
        _check("fused", label, "log2", log2, ref.log2, cpu.log2)
        _check("fused", label, "db", db, ref.db, cpu.db)
        assert _same(mx, np.maximum(pw, F32(1e-10)).max()), "the maximum is not the maximum of the clamped mel power"
        again = _fused(plan, k, wave, n, log2=True, db=True, power=True)
        assert all(_same(a, b) for a, b in zip((log2, db, pw, mx), again)), "two launches differ"
        assert _same(_fused(plan, k, wave, n, log2=True)[0], log2)
        alone = _fused(plan, k, wave, n, db=True)
        assert _same(alone[1], db) and _same(alone[3], mx)
        assert _same(_fused(plan, k, wave, n, power=True)[2], pw)
        assert _same(_fused(plan, k, wave, n, gmax=True)[3], mx), "avs_stft_mel_max differs from the dB path's maximum"
        # the top_db clamp at this launch's maximum, in place, in a destination with a tail
        d = Dest(db.shape[0], n_mels, dev)
        d.buf[:db.size] = torch.from_numpy(db.reshape(-1)).to(dev)
        abi.check(abi.lib().avs_clamp_topdb_f32(ops._p(d.buf), db.size, ops._p(torch.tensor([float(mx)], dtype=torch.float32, device=dev)), afi.TOP_DB,
                                                ops._stream()), "avs_clamp_topdb_f32")
        _check("fused", label, "db_clamped", d.read(), ref.db_clamped, cpu.db_clamped)


# --------------------------------------------------------------------------- segment means
def _segmean(plan, k, wave, t, bounds, one_pass, top_db=afi.TOP_DB):
    """avs_stft_mel_segmean_f32 into ld_log2 = n_mels + 2, ld_db = n_mels + 5 -> (log2 means, dB means, max).  Two passes:
    the maximum comes from a launch of the fused kernel that writes nothing else."""
    from avsum_amd.audio import MelPlan
    ops, abi = _api()
    dev = wave.device
    blocks, seg_block, seg_frames = MelPlan.segment_table(list(bounds), dev)
    assert blocks.cpu().tolist() == [list(b) for b in afi.segment_blocks(bounds)]
    nblocks, nseg, nmel = blocks.shape[0], len(bounds) - 1, k.n_mels
    if one_pass:
        m = Dest(1, 1, dev)
    else:
        m = Dest(1, 1, dev, fill=0.0)
        abi.check(abi.lib().avs_stft_mel_fused_f32(ops._p(wave), t, *_consts(plan), nmel, None, None, None, ops._p(m.buf),
                                                   ops._stream()), "avs_stft_mel_fused_f32")
    need = int(abi.lib().avs_stft_mel_segmean_workspace_bytes(nblocks, nmel, 1, 1, int(one_pass)))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    o_log2, o_db = Dest(nseg, nmel, dev, ld=nmel + 2), Dest(nseg, nmel, dev, ld=nmel + 5)
    abi.check(abi.lib().avs_stft_mel_segmean_f32(ops._p(wave), t, *_consts(plan), nmel, ops._p(blocks), nblocks, ops._p(seg_block),
                                                 ops._p(seg_frames), nseg, ops._p(m.buf), int(one_pass), top_db, ops._p(o_log2.buf),
                                                 o_log2.ld, ops._p(o_db.buf), o_db.ld, ops._p(ws), need, ops._stream()),
              "avs_stft_mel_segmean_f32")
    return o_log2.read(), o_db.read(), m.read()[0, 0]


@pytest.mark.parametrize("n_mels", [p[1] for p in afi.SEG_PLANS])
def test_segment_means(dev, n_mels):
    """130 frames with 32-frame blocks wholly inside a quiet run; a 1-frame, a 33-frame and an empty segment; 320 mels
    take the per-band loop's second trip.  One pass and two passes give the same bits; a table that does not start at
    frame 0 (two passes only) is clamped at the whole track's maximum."""
    plan, k = _plan(dev, n_mels)
    x, _, ref, cpu = afi.seg_bundle(n_mels)
    wave = _wave(x, dev)
    one = _segmean(plan, k, wave, len(x), afi.SEG_BOUNDS, True)
    label = f"mels={n_mels} bounds={list(afi.SEG_BOUNDS)}"
    _check("segmean", label, "log2", one[0], ref[0], cpu[0])
    _check("segmean", label, "db", one[1], ref[1], cpu[1])
    assert (one[0][2] == 0).all() and (one[1][2] == 0).all()          # the empty segment
    full_max = _fused(plan, k, wave, len(x), gmax=True)[3]
    assert _same(one[2], full_max)
    two = _segmean(plan, k, wave, len(x), afi.SEG_BOUNDS, False)
    assert all(_same(a, b) for a, b in zip(one, two)), "one pass and two passes differ"
    assert all(_same(a, b) for a, b in zip(one, _segmean(plan, k, wave, len(x), afi.SEG_BOUNDS, True))), "two calls differ"
    _, _, ref, cpu = afi.seg_bundle(n_mels, afi.SEG_BOUNDS_OFFSET)
    off = _segmean(plan, k, wave, len(x), afi.SEG_BOUNDS_OFFSET, False)
    label = f"mels={n_mels} bounds={list(afi.SEG_BOUNDS_OFFSET)}"
    _check("segmean", label, "log2", off[0], ref[0], cpu[0])
    _check("segmean", label, "db", off[1], ref[1], cpu[1])
    assert _same(off[2], full_max)


def _batch(plan, k, tables, ntracks, nseg):
    ops, abi = _api()
    cat, toff, tlen, blocks, seg_block, seg_frames = tables
    dev, nmel, nblocks = cat.device, k.n_mels, blocks.shape[0]
    need = int(abi.lib().avs_stft_mel_segmean_workspace_bytes(nblocks, nmel, 1, 1, 1))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    o_log2, o_db, m = Dest(nseg, nmel, dev, ld=nmel + 2), Dest(nseg, nmel, dev, ld=nmel + 5), Dest(1, ntracks, dev)
    abi.check(abi.lib().avs_stft_mel_segmean_batch_f32(ops._p(cat), ops._p(toff), ops._p(tlen), ntracks, *_consts(plan), nmel,
                                                       ops._p(blocks), nblocks, ops._p(seg_block), ops._p(seg_frames), nseg,
                                                       ops._p(m.buf), afi.TOP_DB, ops._p(o_log2.buf), o_log2.ld, ops._p(o_db.buf),
                                                       o_db.ld, ops._p(ws), need, ops._stream()), "avs_stft_mel_segmean_batch_f32")
    return o_log2.read(), o_db.read(), m.read()[0]


def test_segment_means_batch(dev):
    """Four tracks in one set of launches - tones, tones x 1e-3, noise, zeros; two lengths are no multiple of 4: every
    clamp uses its own track's maximum; equal bit for bit to the per-track calls."""
    from avsum_amd.audio import MelPlan
    plan, k = _plan(dev, 128)
    tracks, bounds, _, ref, cpu, _ = afi.batch_bundle()
    tables = MelPlan.batch_tables([torch.from_numpy(np.array(t)) for t in tracks], [list(b) for b in bounds], dev)
    nseg = sum(len(b) - 1 for b in bounds)
    got = _batch(plan, k, tables, len(tracks), nseg)
    assert all(_same(a, b) for a, b in zip(got, _batch(plan, k, tables, len(tracks), nseg))), "two calls differ"
    s0 = 0
    for i, (x, b) in enumerate(zip(tracks, bounds)):
        n = len(b) - 1
        label = f"track {i} t={len(x)}"
        _check("batch", label, "log2", got[0][s0:s0 + n], ref[i][0], cpu[i][0])
        _check("batch", label, "db", got[1][s0:s0 + n], ref[i][1], cpu[i][1])
        single = _segmean(plan, k, _wave(x, dev), len(x), b, True)
        assert _same(single[0], got[0][s0:s0 + n]) and _same(single[1], got[1][s0:s0 + n]) and _same(single[2], got[2][i]), label
        s0 += n


# --------------------------------------------------------------------------- shot form
def _shots(plan, k, tb):
    ops, abi = _api()
    dev, nmel = tb.waves.device, k.n_mels
    nshot, nblocks, ntracks = tb.seg_frames.numel(), tb.blocks.shape[0], tb.track_len.numel()
    need = int(abi.lib().avs_stft_mel_shots_workspace_bytes(nblocks, nmel, 1, 1))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    o_log2, o_db, m = Dest(nshot, nmel, dev, ld=nmel + 2), Dest(nshot, nmel, dev, ld=nmel + 5), Dest(1, nshot, dev)
    abi.check(abi.lib().avs_stft_mel_shots_f32(ops._p(tb.waves), tb.waves.numel(), ops._p(tb.track_off), ops._p(tb.track_len), ntracks,
                                               ops._p(tb.shots), nshot, *_consts(plan), nmel, ops._p(tb.blocks), nblocks,
                                               ops._p(tb.seg_block), ops._p(tb.seg_frames), ops._p(m.buf), afi.TOP_DB,
                                               ops._p(o_log2.buf), o_log2.ld, ops._p(o_db.buf), o_db.ld, ops._p(ws), need,
                                               ops._stream()), "avs_stft_mel_shots_f32")
    return o_log2.read(), o_db.read(), m.read()[0]


def test_shot_means(dev):
    """Two tracks, twelve shots, each its own signal: first samples at every offset mod 4; 1, 350, 959, 960, 961 and 7000
    samples; an empty shot, one clipped by the track end, a loud one (clamped to +-1 at load) and a quiet one inside the
    loud track (its clamp uses its own maximum).  Every table index is in range."""
    from avsum_amd.audio import MelPlan
    plan, k = _plan(dev, 128)
    tb = MelPlan.shot_tables(afi.shot_tracks(), [list(b) for b in afi.SHOT_BOUNDS], dev)
    shots = afi.shot_list()
    assert tb.shots.cpu().tolist() == [list(s) for s in shots] and tb.waves.numel() % 4 == 0
    ref, cpu = afi.shot_bundle()
    got = _shots(plan, k, tb)
    assert all(_same(a, b) for a, b in zip(got, _shots(plan, k, tb))), "two calls differ"
    for s, (trk, first, length) in enumerate(shots):
        label = f"shot {s} track={trk} first={first} L={length}"
        if length == 0:
            assert not got[0][s].any() and not got[1][s].any() and got[2][s] == 0
            continue
        _check("shots", label, "log2", got[0][s], ref[s][0], cpu[s][0])
        _check("shots", label, "db", got[1][s], ref[s][1], cpu[s][1])
        assert abs(float(got[2][s]) - ref[s][2]) <= ref[s][3], label     # the shot's own maximum, within the power bound


# --------------------------------------------------------------------------- VGGish examples
def _vgg(front, waves, n, starts):
    ops, abi = _api()
    dev = waves.device
    nex = len(starts)
    need = int(abi.lib().avs_vggish_examples_workspace_bytes(nex))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    out = Dest(nex * 96, 64, dev)
    abi.check(abi.lib().avs_vggish_examples_f32(ops._p(waves), n, ops._p(torch.tensor(starts, dtype=torch.int64, device=dev)), nex,
                                                ops._p(front.basis_t), front.basis_t.shape[1], ops._p(front.fb), ops._p(front.fb_lo),
                                                ops._p(front.fb_hi), 64, ops._p(out.buf), ops._p(ws), need, ops._stream()),
              "avs_vggish_examples_f32")
    return out.read().reshape(nex, 96, 64)


def test_vggish_examples(dev):
    """Starts 0, 3, the last legal one and 5000 (overlapping examples), a stretch beyond +-1: the EX instance of the dense
    DFT + power_mel mode 3 against the float64 oracle on the clamped slice."""
    from avsum_amd.vggish import VGGishFrontEnd
    front = VGGishFrontEnd.get(dev)
    v = afi.vgg_constants()
    assert np.array_equal(front.fb.cpu().numpy(), v.fb) and np.array_equal(front.fb_lo.cpu().numpy(), v.lo)
    assert np.array_equal(front.fb_hi.cpu().numpy(), v.hi)
    x, ref, cpu = afi.vgg_bundle()
    waves = _wave(x, dev)
    got = _vgg(front, waves, len(x), list(afi.VGG_STARTS))
    assert _same(got, _vgg(front, waves, len(x), list(afi.VGG_STARTS))), "two calls differ"
    for e, start in enumerate(afi.VGG_STARTS):
        _check("vggish", f"start={start}", "logmel", got[e], ref[e], cpu[e])


# --------------------------------------------------------------------------- avs_stft_f64
def _stft(case, dev):
    ops, abi = _api()
    out = Dest(case.frames, case.ncols, dev)
    x = _wave(case.x, dev)
    basis = torch.from_numpy(case.basis).to(dev)
    abi.check(abi.lib().avs_stft_f64(ops._p(x), len(case.x), case.frames, case.hop, case.nfft, ops._p(basis), case.ncols, case.ncols_pad,
                                     ops._p(out.buf), ops._stream()), "avs_stft_f64")
    return out.read()


@pytest.mark.parametrize("shape", afi.STFT_SHAPES, ids=[str(s) for s in afi.STFT_SHAPES])
def test_stft_f64(dev, shape):
    """nfft % 4 != 0 (the k < nfft guards), frames an exact multiple of 64, one frame, a third row block; ncols 64, 70 and
    129: random float data to one fp32 rounding of the fp64 sum, integer data to equality."""
    case = afi.stft_case(*shape)
    got = _stft(case, dev)
    err, bound = np.abs(got.astype(np.float64) - case.ref), afi.stft_bound(case)
    print(f"RATIO family='stft_f64' case={case.label!r} tensor=spec err/bound={(err / bound).max():.2f}")
    assert (err <= bound).all(), (case.label, (err / bound).max())
    assert _same(got, _stft(case, dev)), "two calls differ"
    ints = afi.stft_case(*shape, integers=True)
    assert np.array_equal(_stft(ints, dev).astype(np.float64), ints.ref), case.label


# --------------------------------------------------------------------------- avs_power_mel_f32
def _power_mel(spec, k, mode, dev):
    ops, abi = _api()
    frames = spec.shape[0]
    out, m = Dest(frames, k.n_mels, dev), Dest(1, 1, dev, fill=0.0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sp, fb, lo, hi = dv(spec), dv(k.fb), dv(k.lo), dv(k.hi)
    abi.check(abi.lib().avs_power_mel_f32(ops._p(sp), frames, k.n_bins, ops._p(fb), ops._p(lo), ops._p(hi), k.n_mels, mode, ops._p(out.buf),
                                          ops._p(m.buf) if mode == 1 else None, ops._stream()), "avs_power_mel_f32")
    return out.read(), m.read()[0, 0]


@pytest.mark.parametrize("nbins", afi.PM_BINS)
@pytest.mark.parametrize("frames", afi.PM_FRAMES)
def test_power_mel_modes(dev, frames, nbins):
    """Modes 0 (log2), 1 (dB and the maximum), 2 (power) and 3 (VGGish: magnitude, ln) on a random spectrum; 1, 8 and 13
    frames (one block, a full block, a second partial one), 201, 257 and 1025 bins.  Mode 2 and the mode-1 maximum equal
    the sequential fp32 restatement bit for bit: the spectrum is given, every operation is one rounding in a fixed order."""
    k, spec = afi.pm_constants(nbins), afi.pm_case(frames, nbins)
    label = f"frames={frames} bins={nbins}"
    for mode in range(4):
        (ref, _), (cpu, cmax) = afi.pm_reference(spec, k, mode), afi.pm_restatement(spec, k, mode)
        got, mx = _power_mel(spec, k, mode, dev)
        assert _same(got, _power_mel(spec, k, mode, dev)[0]), "two calls differ"
        if mode == 2:
            _check_power("power_mel", label, got, ref, np.zeros(frames), k)
            assert _same(got, cpu), f"{label}: mode 2 differs from the sequential fp32 restatement"
        else:
            _check("power_mel", label, f"mode{mode}", got, ref, cpu)
        if mode == 1:
            assert _same(mx, cmax), f"{label}: the mode-1 maximum differs from the restatement's"


# --------------------------------------------------------------------------- elementwise kernels
@pytest.mark.parametrize("count", afi.SMALL_COUNTS + (afi.BIG,))
def test_fill_quantize_and_clamp(dev, count):
    """Counts 0 .. 1000 and 2 097 190 (the second grid-stride trip): fill and quantize (the VGGish constants, edge values
    in front) bit for bit the fp32 restatement, clamp_topdb within the bound; nothing beyond the count is written."""
    ops, abi = _api()
    lib = abi.lib()
    d = Dest(1, count, dev)
    abi.check(lib.avs_fill_f32(ops._p(d.buf), count, 0.3, ops._stream()), "avs_fill_f32")
    assert _same(d.read(), np.full((1, count), F32(0.3)))
    x = afi.quantize_inputs(count)
    d = Dest(1, count, dev)
    abi.check(lib.avs_quantize_f32(ops._p(_wave(x, dev)), count, *afi.QUANT_VGG, ops._p(d.buf), ops._stream()), "avs_quantize_f32")
    assert _same(d.read()[0], afi.quantize_restatement(x, *afi.QUANT_VGG))
    x, mx = afi.clamp_case(count)
    d = Dest(1, count, dev)
    d.buf[:count] = torch.from_numpy(x).to(dev)
    abi.check(lib.avs_clamp_topdb_f32(ops._p(d.buf), count, ops._p(torch.tensor([float(mx)], dtype=torch.float32, device=dev)), afi.TOP_DB, ops._stream()),
              "avs_clamp_topdb_f32")
    if count:
        _check("clamp_topdb", f"count={count}", "x", d.read()[0], afi.clamp_reference(x, mx, np.float64), afi.clamp_reference(x, mx, F32))


def test_quantize_ties(dev):
    """scale = 64 on x = -2 + (k + 0.5) / 64: exact ties, rounded half to even."""
    ops, abi = _api()
    x, want = afi.quantize_ties()
    d = Dest(1, len(x), dev)
    abi.check(abi.lib().avs_quantize_f32(ops._p(_wave(x, dev)), len(x), -2.0, 2.0, 64.0, ops._p(d.buf), ops._stream()), "avs_quantize_f32")
    assert _same(d.read()[0], want)


@pytest.mark.parametrize("shape", afi.REFLECT_SHAPES + (afi.REFLECT_BIG,), ids=str)
def test_reflect_pad(dev, shape):
    """np.pad(mode="reflect") followed by zeros up to out_len: pad = t - 1, pad = 0, a zero tail, the second trip."""
    ops, abi = _api()
    t, pad, out_len = shape
    x = afi.signal("noise", t)
    d = Dest(1, out_len, dev)
    abi.check(abi.lib().avs_reflect_pad_f32(ops._p(_wave(x, dev)), t, pad, ops._p(d.buf), out_len, ops._stream()), "avs_reflect_pad_f32")
    assert _same(d.read()[0], afi.reflect_reference(x, pad, out_len))


# --------------------------------------------------------------------------- resample
def _resample(case, dev):
    ops, abi = _api()
    y = Dest(1, case.out_len, dev)
    x = _wave(case.x.reshape(-1), dev)
    taps = torch.from_numpy(case.taps).to(dev)
    abi.check(abi.lib().avs_resample_f32(ops._p(x), case.t, case.channels, ops._p(taps), case.up, case.down, case.taps.shape[1], case.width,
                                         ops._p(y.buf), case.out_len, ops._stream()), "avs_resample_f32")
    return y.read()[0]


@pytest.mark.parametrize("rates", afi.RESAMPLE_RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_resample(dev, rates):
    """48000 / 44100 / 8000 -> 16000 and the 16000 -> 16000 mix-down; 1, 2 and 3 channels; clips of 1 sample, of
    width - 1 samples (shorter than the filter) and of 3001; the float64 reference uses the fp32 taps."""
    for args in afi.resample_cases():
        if args[:2] != rates:
            continue
        case = afi.resample_case(*args)
        got = _resample(case, dev)
        _check("resample", case.label, "y", got, afi.resample_eval(case, np.float64), afi.resample_eval(case, np.float32))
        assert _same(got, _resample(case, dev)), "two calls differ"
