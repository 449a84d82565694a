"""Inputs, float64 references, fp32 restatements, planted mistakes and the bounds of the per-kernel tests of the audio
front end (csrc/audio.hip: avs_reflect_pad_f32, avs_stft_f64, avs_power_mel_f32, avs_stft_mel_fused_f32,
avs_stft_mel_segmean_f32 and its batch form, avs_stft_mel_shots_f32, avs_vggish_examples_f32, avs_clamp_topdb_f32,
avs_fill_f32, avs_quantize_f32, avs_resample_f32): test_audio_f64_host.py on the host, test_gpu_audio_f64.py on the
device.  numpy / torch on the CPU only: both build the same seeded cases from here.

Signals (fp32, 16 kHz): "tones" 0.4 sin 220 Hz + 0.3 sin 1333 Hz + 0.2 sin 5200 Hz + 1e-3 N(0, 1); "gap" = tones with a run
(the middle third unless given) replaced by 1e-5 N(0, 1); "sine" 0.5 sin 440 Hz; "noise" 0.3 N(0, 1); "loud" = tones x 4;
"zeros".

References: the defining formulas in float64 (reflect padding, a dense 400-point DFT, the fp32 values of
torch.hann_window(400) and of the filterbank as constants, log2(mel + 1e-6), 10 log10(max(mel, 1e-10)) clamped at its own
maximum - top_db, time means per segment).  Restatements follow the kernels: the float64 DFT with re and im rounded to
fp32, re*re + im*im in fp32 (every operation rounded: the build does not contract), the mel sum in ascending bin order in
fp32, the fp32 log; segment sums frame by frame within a 32-frame block, blocks in block order, one division by the frame
count.  ``mistake`` plants one deliberate error (MISTAKES); NOTICED_BY names the case at which the host test shows it to
lie outside its bound.

Bounds - none measured on the code under test:
  1. log-domain outputs: scorer_f64_inputs.compare unchanged, 4 * e32 + 8 * eps32 * max(1, max|ref|);
  2. mel power, per element: |got - ref| <= (hi_m - lo_m + 6) 2^-24 ref + 2^-40 (sum_n |w_n x_n|)^2 sum_k fb[k, m]: two
     fp32 roundings of re / im, their squares and sum (6 half-ulps), one product and one add per bin of an all-positive
     sum, and the slack of the fp64 accumulation (``power_bound``);
  3. avs_stft_f64 on float data, per element: |got - ref| <= 2^-23 |ref| + 2^-40 sum_k |a_k b_k| (``stft_bound``);
  4. equality where the arithmetic is fixed (reflect_pad, fill, quantize, power_mel mode 2 and the mode-1 maximum)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import audio as oa, vggish as ov
from scorer_f64_inputs import EPS32, SENTINEL, compare as _compare  # noqa: F401  (one definition of the bound, shared)

SR, N_FFT, HOP, N_BINS, FPB = 16000, 400, 200, 201, 32
TOP_DB = 80.0
SHOT_MIN = 960
PLANS = ((16000, 128, 40), (16000, 40, 13))         # (sample rate, n_mels, n_mfcc) of the fused-kernel cases
SEG_PLANS = ((16000, 128, 40), (16000, 320, 40))    # 320 mels: the per-band loop's second trip, 73 empty filters
SIGNALS = ("tones", "gap", "sine", "noise", "zeros")
LENGTHS = (201, 399, 400, 6399, 6400, 6601, 13000)
F32 = np.float32

DFT_MISTAKES = ("fp32_dft", "drop_n200", "window_partner_399", "right_reflect_about_t", "left_reflect_repeat_0")
MEL_MISTAKES = ("mel_stops_at_hi_minus_1", "log2_eps_outside", "db_floor_missing")
SEG_MISTAKES = ("clamp_block_max", "mean_div_32", "drop_last_partial_block")
BATCH_MISTAKES = ("clamp_prev_track_max",)
SHOT_MISTAKES = ("clamp_whole_track_max", "shot_tail_from_track", "shot_no_pm1_clamp")
VGG_MISTAKES = ("vgg_no_pm1_clamp", "vgg_magnitude_squared")
RESAMPLE_MISTAKES = ("base_without_width", "taps_tap_major", "mean_not_divided", "end_test_j_gt_t")
MISTAKES = DFT_MISTAKES + MEL_MISTAKES + SEG_MISTAKES + BATCH_MISTAKES + SHOT_MISTAKES + VGG_MISTAKES + RESAMPLE_MISTAKES


def compare(got, ref, cpu32, scale=None):
    """scorer_f64_inputs.compare on numpy arrays / torch tensors."""
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return _compare(as_t(got), as_t(ref), as_t(cpu32), scale)


# --------------------------------------------------------------------------- signals and constants
_SEEDS = {"tones": 101, "gap": 202, "sine": 303, "noise": 404, "zeros": 505}


@functools.lru_cache(maxsize=None)
def signal(name, n, run=None, seed=0):
    """fp32 [n] (read-only).  run = (first, last + 1) of the quiet run of "gap" (default: the middle third)."""
    t = np.arange(n, dtype=np.float64) / SR
    if name in ("tones", "gap", "loud"):
        rng = np.random.default_rng(_SEEDS["tones"] + seed)
        x = 0.4 * np.sin(2 * np.pi * 220 * t) + 0.3 * np.sin(2 * np.pi * 1333 * t) + 0.2 * np.sin(2 * np.pi * 5200 * t) \
            + 1e-3 * rng.standard_normal(n)
        if name == "gap":
            a, b = run if run is not None else (n // 3, 2 * n // 3)
            x[a:b] = 1e-5 * np.random.default_rng(_SEEDS["gap"] + seed).standard_normal(b - a)
        if name == "loud":
            x = 4.0 * x
    elif name == "sine":
        x = 0.5 * np.sin(2 * np.pi * 440 * t)
    elif name == "noise":
        x = 0.3 * np.random.default_rng(_SEEDS["noise"] + seed).standard_normal(n)
    else:
        assert name == "zeros", name
        x = np.zeros(n)
    x = x.astype(F32)
    x.setflags(write=False)
    return x


def _lo_hi(fb):
    """[lo, hi) of the non-zero bins of each filter; (0, 0) for an empty one (audio.MelPlan's rule)."""
    nz = fb > 0
    lo = np.where(nz.any(0), nz.argmax(0), 0).astype(np.int32)
    hi = np.where(nz.any(0), fb.shape[0] - nz[::-1].argmax(0), 0).astype(np.int32)
    return lo, hi


@functools.lru_cache(maxsize=None)
def mel_constants(sr, n_mels, n_bins=N_BINS):
    """fb fp32 [n_bins, n_mels] (torchaudio's melscale_fbanks in its own fp32 order), fb_lo / fb_hi int32 [n_mels]."""
    fb = oa.melscale_fbanks(n_bins, 0.0, float(sr // 2), n_mels, sr).numpy().astype(F32)
    lo, hi = _lo_hi(fb)
    return SimpleNamespace(fb=fb, lo=lo, hi=hi, n_mels=n_mels, n_bins=n_bins, nonempty=hi > lo)


@functools.lru_cache(maxsize=None)
def vgg_constants():
    fb = ov.mel_matrix().astype(F32)
    lo, hi = _lo_hi(fb)
    return SimpleNamespace(fb=fb, lo=lo, hi=hi, n_mels=fb.shape[1], n_bins=fb.shape[0], nonempty=hi > lo)


@functools.lru_cache(maxsize=None)
def _dft_tables():
    win = torch.hann_window(N_FFT).double().numpy()     # the fp32 window values ARE the algorithm's constants
    ang = 2.0 * np.pi * ((np.arange(N_FFT)[:, None] * np.arange(N_BINS)[None, :]) % N_FFT) / N_FFT
    return win, np.cos(ang), np.sin(ang)


# --------------------------------------------------------------------------- frames, spectrum, mel
def frames_of(x, mistake=None):
    """float64 [1 + t // 200, 400]: the frames of x reflect padded by 200 samples at both ends."""
    x = np.asarray(x, dtype=np.float64)
    t = len(x)
    j = np.arange(-N_FFT // 2, t + N_FFT // 2)
    left = -j - 1 if mistake == "left_reflect_repeat_0" else -j
    right = np.minimum(2 * t - j, t - 1) if mistake == "right_reflect_about_t" else 2 * (t - 1) - j
    j = np.where(j < 0, left, np.where(j >= t, right, j))
    xp = x[j]
    nf = 1 + t // HOP
    return xp[HOP * np.arange(nf)[:, None] + np.arange(N_FFT)[None, :]]


def spectrum(fr, mistake=None):
    """(re, im) [frames, 201] of the Hann-windowed 400-point DFT: float64 (fp32 under the fp32_dft mistake)."""
    win, c, s = _dft_tables()
    if mistake == "window_partner_399":      # the folded DFT's partner term w[400 - n] x[400 - n] with w[399 - n]
        win = win.copy()
        win[201:] = win[200:399]
    xw = fr * win
    if mistake == "drop_n200":
        xw = xw.copy()
        xw[:, 200] = 0.0
    if mistake == "fp32_dft":
        xw = xw.astype(F32)
        return xw @ c.astype(F32), xw @ s.astype(F32)
    return xw @ c, xw @ s


def window_l1(fr):
    """sum_n |w_n x_n| per frame: the magnitude the fp64 accumulation's slack is relative to."""
    return np.abs(fr * _dft_tables()[0]).sum(1)


def mel_sum32(pw, k, mistake=None):
    """fp32 [frames, n_mels]: a += pw[f, k] * fb[k, m] over the bins in ascending order, product and sum rounded (outside
    [lo, hi) the weights are 0 and the sum does not change, so the walk over all bins is the kernel's walk)."""
    fb = k.fb
    if mistake == "mel_stops_at_hi_minus_1":
        fb = fb.copy()
        fb[np.maximum(k.hi - 1, 0), np.arange(k.n_mels)] = 0.0
    a = np.zeros((pw.shape[0], k.n_mels), dtype=F32)
    for b in range(fb.shape[0]):
        a = a + pw[:, b:b + 1] * fb[b:b + 1, :]
    return a


def _logs(mel, dtype, mistake=None):
    """(log2(mel + 1e-6), 10 log10(max(mel, 1e-10)), max of the clamped mel) in ``dtype``."""
    mel = mel.astype(dtype)
    with np.errstate(divide="ignore"):
        log2 = np.log2(mel) + dtype(1e-6) if mistake == "log2_eps_outside" else np.log2(mel + dtype(1e-6))
        cl = mel if mistake == "db_floor_missing" else np.maximum(mel, dtype(1e-10))
        db = dtype(10.0) * np.log10(cl)
    return log2.astype(dtype), db.astype(dtype), (cl.max() if cl.size else dtype(0.0))


def threshold(mx, dtype, top_db=TOP_DB):
    """10 log10(max) - top_db as the kernels evaluate it."""
    with np.errstate(divide="ignore"):
        return dtype(dtype(10.0) * np.log10(dtype(mx)) - dtype(top_db))


def mel_reference(x, k, mistake=None):
    """float64: pow / log2 / db (unclamped) [frames, n_mels], max, l1 [frames] of the signal x."""
    fr = frames_of(x, mistake if mistake in DFT_MISTAKES else None)
    re, im = spectrum(fr)
    mel = (re * re + im * im) @ k.fb.astype(np.float64)
    log2, db, mx = _logs(mel, np.float64)
    return SimpleNamespace(pow=mel, log2=log2, db=db, max=mx, l1=window_l1(fr), db_clamped=np.maximum(db, threshold(mx, np.float64)))


def mel_restatement(x, k, mistake=None):
    """fp32, in the fused kernel's order of operations."""
    fr = frames_of(x, mistake if mistake in DFT_MISTAKES else None)
    re, im = spectrum(fr, mistake if mistake in DFT_MISTAKES else None)
    re, im = re.astype(F32), im.astype(F32)
    pw = re * re + im * im
    mel = mel_sum32(pw, k, mistake)
    log2, db, mx = _logs(mel, F32, mistake if mistake in MEL_MISTAKES else None)
    with np.errstate(invalid="ignore"):
        dbc = np.maximum(db, threshold(mx, F32))
    return SimpleNamespace(pow=mel, log2=log2, db=db, max=F32(mx), db_clamped=dbc)


def power_bound(ref_pow, l1, k):
    """Bound 2, per element [frames, n_mels]."""
    width = (k.hi - k.lo).astype(np.float64)
    return (width + 6.0)[None, :] * 2.0 ** -24 * ref_pow + 2.0 ** -40 * (np.asarray(l1) ** 2)[:, None] * k.fb.astype(np.float64).sum(0)[None, :]


def power_check(got, ref_pow, l1, k):
    """(ok, largest err / bound) of bound 2; an element whose bound is 0 must be exact."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref_pow)
    bound = power_bound(ref_pow, l1, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return bool(np.isfinite(np.asarray(got)).all() and (err <= bound).all()), float(ratio.max()) if ratio.size else 0.0


@functools.lru_cache(maxsize=None)
def fused_bundle(name, n, n_mels):
    """(x, float64 reference, fp32 restatement) of one fused-kernel case, computed once per process."""
    x, k = signal(name, n), mel_constants(SR, n_mels)
    return x, mel_reference(x, k), mel_restatement(x, k)


def clamp_share(ref, k):
    """Shares of the float64 dB values of the non-empty bands below and above the clamp's threshold."""
    db = ref.db[:, k.nonempty]
    below = float((db < threshold(ref.max, np.float64)).mean())
    return below, 1.0 - below


# at least 10 % of the float64 dB values of the non-empty bands on either side of the threshold, in both plans.  (The long
# sines are clamped too - 87 .. 93 % of their values lie below it, which at 128 mels leaves 9.7 % above - and every case
# is compared after the clamp; they just do not count towards the condition.)
CLAMP_ENGAGING = (("gap", 6601), ("gap", 13000), ("sine", 399), ("sine", 400))
CLAMP_IDLE = (("tones", 6601), ("tones", 13000))


# --------------------------------------------------------------------------- segment means
SEG_T, SEG_RUN = 25801, (6000, 20000)
SEG_BOUNDS = (0, 1, 34, 34, 100, 130)
SEG_BOUNDS_OFFSET = (34, 66, 100, 103)      # a table that does not start at frame 0: the two-pass path


def seg_track():
    return signal("gap", SEG_T, SEG_RUN)


def segment_blocks(bounds):
    """[(first frame, frames <= 32, segment)] in the order of audio.MelPlan.segment_table."""
    return [(f, min(FPB, b - f), s) for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])) for f in range(a, b, FPB)]


def segment_means_reference(rows, bounds):
    """float64 [nseg, n_mels]: the mean of rows[a:b]; zeros for an empty segment."""
    return np.stack([rows[a:b].mean(0) if b > a else np.zeros(rows.shape[1]) for a, b in zip(bounds[:-1], bounds[1:])])


def segment_means_restatement(rows, bounds, mistake=None):
    """fp32: frame by frame within a block, blocks in block order, one division by the frame count."""
    rows = rows.astype(F32)
    out = np.zeros((len(bounds) - 1, rows.shape[1]), dtype=F32)
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        if b <= a:
            continue
        total = np.zeros(rows.shape[1], dtype=F32)
        for f0 in range(a, b, FPB):
            nf = min(FPB, b - f0)
            if mistake == "drop_last_partial_block" and nf < FPB and f0 + nf == b and f0 > a:
                continue
            part = np.zeros(rows.shape[1], dtype=F32)
            for f in range(f0, f0 + nf):
                part = part + rows[f]
            total = total + part
        out[s] = total / F32(FPB if mistake == "mean_div_32" else b - a)
    return out


def clamped_rows32(r32, bounds, mistake=None, thr_max=None):
    """fp32 dB rows clamped as the segment kernels clamp them: at the track's maximum (thr_max overrides it), or - the
    clamp_block_max mistake - at the maximum of the rows of each block."""
    db = r32.db
    if mistake == "clamp_block_max":
        out = db.copy()
        for f0, nf, _ in segment_blocks(bounds):
            blk_max = np.maximum(r32.pow[f0:f0 + nf], F32(1e-10)).max()
            out[f0:f0 + nf] = np.maximum(db[f0:f0 + nf], threshold(blk_max, F32))
        return out
    return np.maximum(db, threshold(r32.max if thr_max is None else thr_max, F32))


@functools.lru_cache(maxsize=None)
def seg_bundle(n_mels, bounds=SEG_BOUNDS):
    """(x, k, ref (log2 means, dB means, max), restatement (same)) of the segment-mean case."""
    x, k = seg_track(), mel_constants(SR, n_mels)
    r64, r32 = mel_reference(x, k), mel_restatement(x, k)
    ref = (segment_means_reference(r64.log2, bounds), segment_means_reference(r64.db_clamped, bounds), r64.max)
    cpu = (segment_means_restatement(r32.log2, bounds), segment_means_restatement(clamped_rows32(r32, bounds), bounds), r32.max)
    return x, k, ref, cpu


def seg_mistaken(n_mels, mistake, bounds=SEG_BOUNDS):
    x, k = seg_track(), mel_constants(SR, n_mels)
    r32 = mel_restatement(x, k)
    return (segment_means_restatement(r32.log2, bounds, mistake),
            segment_means_restatement(clamped_rows32(r32, bounds, mistake), bounds, mistake))


# --------------------------------------------------------------------------- batch form
def batch_tracks():
    """Four tracks: loud, tones x 1e-3 between two loud ones, zeros; two lengths are no multiple of 4."""
    quiet = (signal("tones", 4803, seed=1) * F32(1e-3)).astype(F32)
    return [signal("tones", 6601), quiet, signal("noise", 7002), signal("zeros", 1001)]


def batch_bounds(tracks):
    out = []
    for w in tracks:
        nf = 1 + len(w) // HOP
        out.append((0, 1, nf // 2, nf // 2, nf))
    return out


@functools.lru_cache(maxsize=None)
def batch_bundle(n_mels=128):
    """Per track (ref log2 means, ref dB means, ref max), the same restated; ``prev`` = the restated dB means clamped at
    the PREVIOUS track's maximum (the clamp_prev_track_max mistake)."""
    k = mel_constants(SR, n_mels)
    tracks = batch_tracks()
    bounds = batch_bounds(tracks)
    ref, cpu, prev, last = [], [], [], None
    for x, b in zip(tracks, bounds):
        r64, r32 = mel_reference(x, k), mel_restatement(x, k)
        ref.append((segment_means_reference(r64.log2, b), segment_means_reference(r64.db_clamped, b), r64.max))
        cpu.append((segment_means_restatement(r32.log2, b), segment_means_restatement(clamped_rows32(r32, b), b), r32.max))
        prev.append(segment_means_restatement(clamped_rows32(r32, b, thr_max=r32.max if last is None else last), b))
        last = r32.max
    return tracks, bounds, k, ref, cpu, prev


# --------------------------------------------------------------------------- shot form
SHOT_TRACK0, SHOT_QUIET = 20003, (9000, 12000)
SHOT_BOUNDS = (
    # track 0: loud (tones x 4) around a quiet run; (first, last + 1) in samples, Python slice semantics
    ((0, 1), (1, 351), (402, 1361), (1363, 2323), (2324, 3285), (3001, 10001), (9200, 11800), (5, 5), (19000, 25000)),
    # track 1: tones
    ((0, 9001), (7, 357), (6002, 6964)),
)


def shot_tracks():
    loud = np.array(signal("gap", SHOT_TRACK0, SHOT_QUIET), dtype=F32) * F32(4.0)
    return [loud.astype(F32), signal("tones", 9001, seed=2)]


def shot_list():
    """[(track, first, present length L)] in table order."""
    out = []
    for trk, (w, bounds) in enumerate(zip(shot_tracks(), SHOT_BOUNDS)):
        for s0, s1 in bounds:
            a, b, _ = slice(s0, s1).indices(len(w))
            out.append((trk, a, max(0, b - a)))
    return out


def shot_signal(track, first, length, mistake=None):
    """The shot's own signal: the slice zero padded to 960 samples and clamped to [-1, 1]."""
    lp = max(length, SHOT_MIN)
    x = np.zeros(lp, dtype=F32)
    x[:length] = track[first:first + length]
    if mistake == "shot_tail_from_track":
        tail = track[first + length:first + lp]
        x[length:length + len(tail)] = tail
    return x if mistake == "shot_no_pm1_clamp" else np.clip(x, F32(-1.0), F32(1.0))


@functools.lru_cache(maxsize=None)
def shot_bundle(n_mels=128, mistake=None):
    """Per shot (log2 mean, dB mean, max) [n_mels] in float64 (followed by the largest element of the shot's power_bound:
    a maximum moves by no more than its elements do) and restated; an empty shot gives zeros and a maximum 0."""
    k = mel_constants(SR, n_mels)
    tracks = shot_tracks()
    ref, cpu = [], []
    whole = [mel_restatement(np.clip(t, F32(-1), F32(1)), k).max for t in tracks] if mistake == "clamp_whole_track_max" else None
    for trk, first, length in shot_list():
        if length == 0:
            z = np.zeros(n_mels)
            ref.append((z, z, 0.0, 0.0))
            cpu.append((z.astype(F32), z.astype(F32), F32(0.0)))
            continue
        r64 = mel_reference(shot_signal(tracks[trk], first, length), k)
        r32 = mel_restatement(shot_signal(tracks[trk], first, length, mistake), k)
        b = (0, r64.log2.shape[0])
        ref.append((segment_means_reference(r64.log2, b)[0], segment_means_reference(r64.db_clamped, b)[0], r64.max,
                    power_bound(r64.pow, r64.l1, k).max()))
        dbc =clamped_rows32(r32, b, thr_max=whole[trk] if whole else None)
        cpu.append((segment_means_restatement(r32.log2, b)[0], segment_means_restatement(dbc, b)[0], r32.max))
    return ref, cpu


# --------------------------------------------------------------------------- VGGish examples
VGG_LEN, VGG_EX_LEN, VGG_LOUD = 26000, 15600, (2000, 9000)
VGG_STARTS = (0, 3, VGG_LEN - VGG_EX_LEN, 5000)


@functools.lru_cache(maxsize=None)
def vgg_waves():
    x = np.array(signal("tones", VGG_LEN, seed=3), dtype=F32)
    x[VGG_LOUD[0]:VGG_LOUD[1]] *= F32(4.0)
    x.setflags(write=False)
    return x


def vgg_reference(x, start):
    """float64 [96, 64]: oracle.vggish.log_mel_spectrogram on the clamped slice."""
    return ov.log_mel_spectrogram(np.clip(x[start:start + VGG_EX_LEN], F32(-1), F32(1)))


def vgg_restatement(x, start, mistake=None):
    """fp32: the float64 512-point DFT of the windowed frame with re / im rounded to fp32, the MAGNITUDE spectrum
    sqrtf(re*re + im*im), the mel sum in ascending bin order, logf(mel + 0.01)."""
    k = vgg_constants()
    s = np.asarray(x[start:start + VGG_EX_LEN], dtype=np.float64)
    if mistake != "vgg_no_pm1_clamp":
        s = np.clip(s, -1.0, 1.0)
    idx = np.arange(ov.WINDOW)[None, :] + ov.HOP * np.arange(ov.EXAMPLE_FRAMES)[:, None]
    n = np.arange(ov.WINDOW)
    ang = 2.0 * np.pi * ((n[:, None] * np.arange(ov.NUM_BINS)[None, :]) % ov.FFT_LEN) / ov.FFT_LEN
    xw = s[idx] * ov.periodic_hann()
    re, im = (xw @ np.cos(ang)).astype(F32), (xw @ np.sin(ang)).astype(F32)
    pw = re * re + im * im
    mel = mel_sum32(pw if mistake == "vgg_magnitude_squared" else np.sqrt(pw), k)
    return np.log(mel + F32(0.01)).astype(F32)


@functools.lru_cache(maxsize=None)
def vgg_bundle():
    x = vgg_waves()
    return x, [vgg_reference(x, s) for s in VGG_STARTS], [vgg_restatement(x, s) for s in VGG_STARTS]


# --------------------------------------------------------------------------- avs_stft_f64
STFT_SHAPES = ((75, 12, 40, 70), (64, 5, 6, 129), (1, 7, 42, 64), (130, 3, 10, 64))     # (frames, hop, nfft, ncols)


@functools.lru_cache(maxsize=None)
def stft_case(frames, hop, nfft, ncols, integers=False):
    """x fp32 [(frames - 1) hop + nfft], basis float64 [nfft, ncols_pad] (columns past ncols hold a sentinel the kernel
    may multiply but never store), ref float64 [frames, ncols], mag = sum_k |a_k b_k|."""
    rng = np.random.default_rng(frames * 1000 + nfft + (7 if integers else 0))
    n = (frames - 1) * hop + nfft
    ncols_pad = -(-ncols // 64) * 64
    if integers:
        x = rng.integers(-9, 10, n).astype(F32)
        b = rng.integers(-5, 6, (nfft, ncols)).astype(np.float64)
    else:
        x = rng.standard_normal(n).astype(F32)
        b = rng.standard_normal((nfft, ncols))
    basis = np.full((nfft, ncols_pad), 3.0)
    basis[:, :ncols] = b
    fr = x.astype(np.float64)[hop * np.arange(frames)[:, None] + np.arange(nfft)[None, :]]
    return SimpleNamespace(x=x, basis=basis, ncols_pad=ncols_pad, ref=fr @ b, mag=np.abs(fr) @ np.abs(b), frames=frames, hop=hop,
                           nfft=nfft, ncols=ncols, label=f"frames={frames} hop={hop} nfft={nfft} ncols={ncols}")


def stft_bound(case):
    """Bound 3, per element: one fp32 rounding of an fp64 sum of exact products."""
    return 2.0 ** -23 * np.abs(case.ref) + 2.0 ** -40 * case.mag


# --------------------------------------------------------------------------- avs_power_mel_f32
PM_FRAMES, PM_BINS = (1, 8, 13), (201, 257, 1025)


@functools.lru_cache(maxsize=None)
def pm_constants(nbins):
    return {201: lambda: mel_constants(SR, 128), 257: vgg_constants, 1025: lambda: mel_constants(SR, 80, 1025)}[nbins]()


@functools.lru_cache(maxsize=None)
def pm_case(frames, nbins):
    """spec fp32 [frames, 2 nbins] = (re | im), N(0, 1) scaled per bin so that the bands differ by orders of magnitude."""
    rng = np.random.default_rng(frames * 10000 + nbins)
    spec = rng.standard_normal((frames, 2 * nbins)) * np.tile(10.0 ** rng.uniform(-4, 1, nbins), 2)[None, :]
    return spec.astype(F32)


def pm_reference(spec, k, mode):
    """float64 from the fp32 spectrum given: (out, max of the clamped mel)."""
    s = spec.astype(np.float64)
    nb = k.n_bins
    pw = s[:, :nb] ** 2 + s[:, nb:] ** 2
    mel = (np.sqrt(pw) if mode == 3 else pw) @ k.fb.astype(np.float64)
    log2, db, mx = _logs(mel, np.float64)
    return {0: log2, 1: db, 2: mel, 3: np.log(mel + 0.01)}[mode], mx


def pm_restatement(spec, k, mode):
    nb = k.n_bins
    re, im = spec[:, :nb], spec[:, nb:]
    pw = re * re + im * im
    mel = mel_sum32(np.sqrt(pw) if mode == 3 else pw, k)
    log2, db, mx = _logs(mel, F32)
    return {0: log2, 1: db, 2: mel, 3: np.log(mel + F32(0.01)).astype(F32)}[mode], F32(mx)


# --------------------------------------------------------------------------- elementwise kernels
BIG = 2097153 + 37          # 8192 blocks x 256 threads + 1: the second grid-stride trip
SMALL_COUNTS = (0, 1, 255, 257, 1000)
QUANT_VGG = (-2.0, 2.0, 63.75)
REFLECT_SHAPES = ((201, 200, 601), (5, 0, 5), (7, 3, 20))     # (t, pad, out_len)
REFLECT_BIG = (BIG - 410, 200, BIG)


def reflect_reference(x, pad, out_len):
    out = np.zeros(out_len, dtype=F32)
    out[:len(x) + 2 * pad] = np.pad(x, pad, mode="reflect") if pad else x
    return out


def quantize_restatement(x, lo, hi, scale):
    """rint((clamp(x, lo, hi) - lo) * scale) in fp32, half to even."""
    lo, hi, scale = F32(lo), F32(hi), F32(scale)
    return np.rint((np.minimum(np.maximum(x.astype(F32), lo), hi) - lo) * scale).astype(F32)


def quantize_inputs(count, seed=0):
    """N(0, 1.5) with the edge values in front: below / at / above the clamps, zeros of both signs."""
    x = (np.random.default_rng(900 + seed).standard_normal(count) * 1.5).astype(F32)
    edges = np.array([-5.0, -2.0, np.nextafter(F32(-2.0), F32(0.0)), -0.0, 0.0, np.nextafter(F32(2.0), F32(0.0)), 2.0, 2.5, 1e-8],
                     dtype=F32)
    n = min(count, len(edges))
    x[:n] = edges[:n]
    return x


def quantize_ties():
    """x = -2 + (k + 0.5) / 64 for k = 0 .. 255: (x + 2) * 64 = k + 0.5 exactly; half to even gives k for even k, k + 1
    for odd k."""
    k = np.arange(256)
    return (-2.0 + (k + 0.5) / 64.0).astype(F32), np.where(k % 2 == 0, k, k + 1).astype(F32)


def clamp_case(count, seed=0):
    """dB-like values N(-40, 30) and a maximum of 37.5 (threshold about -64.3: both sides are populated)."""
    x = (np.random.default_rng(700 + seed).standard_normal(count) * 30.0 - 40.0).astype(F32)
    return x, F32(37.5)


def clamp_reference(x, mx, dtype, top_db=TOP_DB):
    return np.maximum(x.astype(dtype), threshold(mx, dtype, top_db))


# --------------------------------------------------------------------------- avs_resample_f32
RESAMPLE_RATES = ((48000, 16000), (44100, 16000), (8000, 16000), (16000, 16000))
RESAMPLE_CHANNELS = (1, 2, 3)


def resample_taps(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(taps fp32 [up, ntaps], width, down, up): the Hann-windowed sinc design of audio.resample_taps, restated; equal
    rates give the single tap 1 of the pure channel mix-down."""
    if orig_freq == new_freq:
        return np.ones((1, 1), dtype=F32), 0, 1, 1
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    kern = np.where(t == 0, 1.0, np.sin(safe) / safe) * window * (base / orig)
    return kern.astype(F32), width, orig, new


def resample_lengths(width):
    return sorted({1, max(1, width - 1), 3001})


@functools.lru_cache(maxsize=None)
def resample_case(orig_freq, new_freq, channels, t):
    taps, width, down, up = resample_taps(orig_freq, new_freq)
    x = (np.random.default_rng(orig_freq + 10 * channels + t).standard_normal((t, channels)) * 0.3 + 0.1).astype(F32)
    return SimpleNamespace(x=x, taps=taps, width=width, down=down, up=up, t=t, channels=channels, out_len=-(-up * t // down),
                           label=f"{orig_freq}->{new_freq} channels={channels} t={t}")


def resample_eval(case, dtype, mistake=None):
    """y[i up + p] = sum_k mono[i down + k - width] taps[p][k], mono = the channel mean (0 outside the clip): float64 the
    defining formula on the fp32 taps; float32 the kernel's order (channels added in order, one multiplication by
    1 / channels, fmaf over the taps in ascending order)."""
    assert mistake is None or mistake in RESAMPLE_MISTAKES
    x, taps, t, ch = case.x, case.taps, case.t, case.channels
    ntaps = taps.shape[1]
    if dtype == np.float64:
        mono = x.astype(np.float64).mean(1)
    else:
        mono = np.zeros(t, dtype=F32)
        for c in range(ch):
            mono = mono + x[:, c]
        if ch > 1 and mistake != "mean_not_divided":
            mono = mono * (F32(1.0) / F32(ch))
    mono = np.concatenate([mono, np.full(1, 1.0, dtype=mono.dtype)])    # the sample one past the clip (end_test_j_gt_t reads it)
    o = np.arange(case.out_len)
    i, ph = o // case.up, o % case.up
    base = i * case.down - (0 if mistake == "base_without_width" else case.width)
    flat = taps.reshape(-1)
    acc = np.zeros(case.out_len, dtype=dtype)
    for kk in range(ntaps):
        j = base + kk
        live = (j >= 0) & ((j <= t) if mistake == "end_test_j_gt_t" else (j < t))
        v = np.where(live, mono[np.clip(j, 0, t)], 0).astype(dtype)
        tp = (flat[(kk * case.up + ph) % flat.size] if mistake == "taps_tap_major" else taps[ph, kk]).astype(dtype)
        if dtype == np.float64:
            acc = acc + v * tp
        else:       # fmaf: the product of two fp32 is exact in float64
            acc = (v.astype(np.float64) * tp.astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return acc


def resample_cases():
    out = []
    for o, n in RESAMPLE_RATES:
        width = resample_taps(o, n)[1]
        for ch in RESAMPLE_CHANNELS:
            if o == n and ch == 1:
                continue            # equal rates, mono: nothing is launched
            for t in resample_lengths(width):
                out.append((o, n, ch, t))
    return out


# --------------------------------------------------------------------------- which case notices which mistake
NOTICED_BY = {
    # fused kernel: (signal, samples, n_mels)
    "fp32_dft": ("tones", 6601, 128),
    "drop_n200": ("tones", 6601, 128),
    "window_partner_399": ("tones", 6601, 128),
    "right_reflect_about_t": ("tones", 201, 128),
    "left_reflect_repeat_0": ("noise", 201, 128),
    "mel_stops_at_hi_minus_1": ("noise", 6601, 40),
    "log2_eps_outside": ("gap", 6601, 128),
    "db_floor_missing": ("zeros", 6601, 128),
    # segment means: n_mels of the SEG_BOUNDS case
    "clamp_block_max": 128,
    "mean_div_32": 128,
    "drop_last_partial_block": 320,
    # batch form: the track
    "clamp_prev_track_max": 1,
    # shot form: the shot's index in shot_list()
    "clamp_whole_track_max": 6,
    "shot_tail_from_track": 1,
    "shot_no_pm1_clamp": 5,
    # VGGish: the example
    "vgg_no_pm1_clamp": 0,
    "vgg_magnitude_squared": 2,
    # resample: (orig, new, channels, t)
    "base_without_width": (48000, 16000, 1, 3001),
    "taps_tap_major": (44100, 16000, 2, 3001),
    "mean_not_divided": (16000, 16000, 2, 3001),
    "end_test_j_gt_t": (8000, 16000, 3, 1),
}
