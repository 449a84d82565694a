"""Seeded cases, restatements and planted mistakes of the summary-rendering tests (libavsum_render.so, avsum_amd/render.py):
test_render_host.py on the host, test_gpu_render.py on the device.  numpy only; both build the same cases from here.

Oracles are avsum_amd.render's numpy definitions (summary_index_host, bgr_to_frames_host, repack_host,
summary_audio_host).  The ``*_restatement`` functions below state the same definitions a second time, by loops and byte
addresses, so that a planted ``mistake`` can go wrong the way a kernel would; without a mistake the host test holds the
two equal on every committed case, and with one it must differ on the case NOTICED_BY names.
"""
import functools

import numpy as np

import yuv_inputs as yi
from pixel_f64_inputs import SENTINEL_U8

TILE = 1024                                   # AVSR_TILE (test_render_host.py holds it to the header)

# --------------------------------------------------------------------------- index cases
INDEX_LENGTHS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
INDEX_OFFSETS = tuple(np.concatenate([[0], np.cumsum(INDEX_LENGTHS)]).tolist())
INDEX_MASKS = ("zeros", "ones", "alternating", "straddle", "boundary", "seeded")
SMALL_CAPS = (100, 7)                         # frame_cap, run_cap of the overflow case (on "alternating")


@functools.lru_cache(maxsize=None)
def index_mask(name):
    n, off = INDEX_OFFSETS[-1], INDEX_OFFSETS
    mask = np.zeros(n, dtype=np.uint8)
    if name == "ones":
        mask[:] = 1
    elif name == "alternating":               # the most runs: every second frame
        mask[::2] = 1
    elif name == "straddle":                  # runs across the tile boundaries inside videos 3 and 4
        mask[off[3] + TILE - 1:off[3] + TILE + 1] = 1
        mask[off[4] + TILE - 5:off[4] + TILE + 5] = 1
        mask[off[4] + 2 * TILE - 1:off[4] + 2 * TILE + 3] = 1
    elif name == "boundary":                  # a video ending in 1 followed by one starting with 1, twice
        mask[0] = 1
        mask[off[1]:off[1] + 2] = 1
        mask[off[2] - 3:off[2]] = 1
        mask[off[2]:off[2] + 2] = 1
    elif name == "seeded":
        mask[:] = np.random.default_rng(41).random(n) < 0.3
    mask.setflags(write=False)
    return mask


def index_restatement(mask, offsets, mistake=None):
    """Per video the list of (start, end) runs and the list of global picked frames, frame by frame."""
    assert mistake in (None, "run_across_videos")
    runs, picked = [[] for _ in offsets[:-1]], []
    video_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    open_run = None                                              # (video, start) of the run being read
    for i, m in enumerate(mask):
        v = int(video_of[i])
        first = i == offsets[v]
        if open_run is not None and (not m or (first and mistake is None)):
            runs[open_run[0]].append((open_run[1], i - offsets[open_run[0]]))
            open_run = None
        if m:
            picked.append(i)
            if open_run is None:
                open_run = (v, i - offsets[v])
    if open_run is not None:
        runs[open_run[0]].append((open_run[1], len(mask) - offsets[open_run[0]]))
    return runs, picked


# --------------------------------------------------------------------------- forward conversion cases
FORMATS, LAYOUTS = yi.FORMATS, yi.LAYOUTS
BASES = (0, 1)                                # the destination starts at byte 0 / one SAMPLE into its allocation
CUSTOM = (200, 1 << 20, 0, 0, -(1 << 19), 1 << 19, 0, 1 << 18, -(1 << 18), 1 << 19)   # every row's sum of |c| is 2^20
FRAMES = 3
GATHER = (2, -1, 0, 7, 1)                     # a skipped (-1) and an out-of-range (7) entry among 3 source frames


@functools.lru_cache(maxsize=None)
def bgr_case(name, seed=0):
    h, w = LAYOUTS[name][:2]
    bgr = np.random.default_rng(7300 + 100 * h + w + seed).integers(0, 256, (FRAMES, h, w, 3), dtype=np.uint8)
    bgr.setflags(write=False)
    return bgr


def dest_layout(fmt, name, frames):
    return yi.layout(fmt, frames, *yi.layout_args(fmt, name))


FORWARD_MISTAKES = ("uv_swapped", "block_rows", "round_dropped", "shift_dropped")


def forward_restatement(bgr, L, forward, index=None, mistake=None):
    """uint8 [L.n, frame_stride] from a SENTINEL_U8-filled buffer: the forward definition by byte addresses."""
    assert mistake is None or mistake in FORWARD_MISTAKES
    k = 0 if L.sample_bytes == 1 else 2
    top = (256 << k) - 1
    y_off, yb, yg, yr, ub, ug, ur, vb, vg, vr = (int(c) for c in forward)
    out = np.full((L.n, L.frame_stride), SENTINEL_U8, dtype=np.uint8)
    shift = 0 if mistake == "shift_dropped" else L.shift

    def put(frame, at, sample):
        if L.sample_bytes == 1:
            out[frame, at] = sample
        else:
            out[frame, at], out[frame, at + 1] = (sample << shift) & 255, (sample << shift) >> 8

    index = range(len(bgr)) if index is None else index
    for i, r in enumerate(index):
        if not 0 <= r < len(bgr) or i >= L.n:
            continue
        px = bgr[r].astype(np.int64)
        for y in range(L.h):
            for x in range(L.w):
                b, g, red = (int(c) for c in px[y, x])
                half = 0 if mistake == "round_dropped" else 1 << (19 - k)
                put(i, y * L.pitch_y + x * L.sample_bytes,
                    min(max(((yb * b + yg * g + yr * red + half) >> (20 - k)) + (y_off << k), 0), top))
        for cy in range(L.h // 2):
            rows = (cy, cy + 1) if mistake == "block_rows" else (2 * cy, 2 * cy + 1)
            for cx in range(L.w // 2):
                sb, sg, sr = (int(px[rows[0]:rows[1] + 1:rows[1] - rows[0], 2 * cx:2 * cx + 2, c].sum()) for c in range(3))
                half = 0 if mistake == "round_dropped" else 1 << (21 - k)
                u = min(max(((ub * sb + ug * sg + ur * sr + half) >> (22 - k)) + (128 << k), 0), top)
                v = min(max(((vb * sb + vg * sg + vr * sr + half) >> (22 - k)) + (128 << k), 0), top)
                if mistake == "uv_swapped":
                    u, v = v, u
                at = cy * L.pitch_c + cx * L.chroma_step
                put(i, L.u_offset + at, u)
                put(i, L.v_offset + at, v)
    return out


@functools.lru_cache(maxsize=None)
def exhaustive_bgr():
    """uint8 [1, 4096, 4096, 3]: every (B, G, R) exactly once, in a seeded order (so that the 2x2 blocks mix colours)."""
    p = np.random.default_rng(99).permutation(1 << 24).astype(np.uint32)
    bgr = np.stack([p & 255, (p >> 8) & 255, p >> 16], axis=-1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    bgr.setflags(write=False)
    return bgr


# --------------------------------------------------------------------------- repack cases
REPACK_FORMATS = {8: ("i420", "yv12", "nv21", "nv12"), 10: ("p010", "i010")}
REPACK_PAIRS = tuple((a, b) for fmts in REPACK_FORMATS.values() for a in fmts for b in fmts if a != b)
REPACK_LAYOUTS = ("6x10", "36x70")


# --------------------------------------------------------------------------- audio cases
AUDIO_FRAMES = (260, 90, 120)
AUDIO_OFFSETS = (0, 260, 350, 470)
AUDIO_FPS = (25.0, 30.0, 30000.0 / 1001.0)
AUDIO_TRACKS = (130000, 32001, 64064)
AUDIO_WAVE_OFFSETS = (0, 130000, 162001, 226065)
AUDIO_SR = 16000
# video 0 (25 fps): (10, 201) ends where int(201 / 25 * 16000) = 128639 and int(201 * 16000 / 25) = 128640 differ - the
# reordered bound is noticed here; (203, 210) is clamped at the track's end (129919 .. 130000), (250, 260) lies wholly
# beyond it (0 samples).  video 1 (30 fps, a track of 32001 samples): (60, 80) begins at 32000 and is clamped to ONE
# sample, (85, 90) is empty.  video 2 (30000 / 1001 fps): a run of one frame (533 samples) and one ending at the track's end
AUDIO_RUNS = (((0, 3), (10, 201), (203, 210), (250, 260)), ((60, 80), (85, 90)), ((0, 1), (5, 40), (100, 120)))
AUDIO_FADES = (0, 8, 300)                     # 300 is above half of the 533-, the 81- and the 1-sample runs
REORDER_WITNESS = (201, 25.0)                 # (e, fps): floor(e / fps * sr) = 128639, floor(e * sr / fps) = 128640


@functools.lru_cache(maxsize=None)
def audio_case():
    """(wave float32 [S], mask uint8 [N]) of the runs above."""
    wave = np.random.default_rng(17).standard_normal(AUDIO_WAVE_OFFSETS[-1]).astype(np.float32)
    mask = np.zeros(AUDIO_OFFSETS[-1], dtype=np.uint8)
    for v, runs in enumerate(AUDIO_RUNS):
        for s, e in runs:
            mask[AUDIO_OFFSETS[v] + s:AUDIO_OFFSETS[v] + e] = 1
    wave.setflags(write=False)
    mask.setflags(write=False)
    return wave, mask


AUDIO_MISTAKES = ("fade_unclamped", "bounds_reordered")


def audio_restatement(wave, wave_offsets, runs_per_video, fps, sr, fade, mistake=None):
    """float32 [samples]: the cut sample by sample."""
    assert mistake is None or mistake in AUDIO_MISTAKES
    out = []
    for v, runs in enumerate(runs_per_video):
        track = wave[wave_offsets[v]:wave_offsets[v + 1]]

        def bound(frame):
            if mistake == "bounds_reordered":
                x = np.float64(frame) * np.float64(sr) / np.float64(fps[v])
            else:
                x = np.float64(frame) / np.float64(fps[v]) * np.float64(sr)
            return min(int(np.floor(x)), len(track))

        for s, e in runs:
            a, b = bound(s), bound(e)
            length = b - a
            f = fade if mistake == "fade_unclamped" else min(fade, length // 2)
            for i in range(length):
                x = np.float32(track[a + i])
                if i < f:
                    x = x * (np.float32(i + 1) / np.float32(f + 1))
                elif i >= length - f:
                    x = x * (np.float32(length - i) / np.float32(f + 1))
                out.append(np.float32(x))
    return np.array(out, dtype=np.float32)


NOTICED_BY = {
    "uv_swapped": ("i420", "2x2"), "block_rows": ("i420", "6x10"), "round_dropped": ("nv21", "6x10"),
    "shift_dropped": ("p010", "2x2"), "run_across_videos": "boundary", "fade_unclamped": 300, "bounds_reordered": 0,
}

# --------------------------------------------------------------------------- end to end
E2E_LENGTHS = (5, 40, 23)
E2E_OFFSETS = (0, 5, 45, 68)
E2E_SHOTS = (((0, 5),), ((0, 6), (6, 9), (9, 12), (12, 20), (20, 23), (23, 40)), ((0, 2), (2, 3), (3, 5), (5, 6), (6, 23)))
E2E_HW = (6, 10)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """(bgr uint8 [68, 6, 10, 3], scores float32 [2, 68]): seeded frames and two rows of scores that pick different shots."""
    rng = np.random.default_rng(23)
    bgr = rng.integers(0, 256, (E2E_OFFSETS[-1],) + E2E_HW + (3,), dtype=np.uint8)
    scores = rng.random((2, E2E_OFFSETS[-1]), dtype=np.float32)
    scores[1] = 1 - scores[0]                                   # the second row prefers what the first does not
    bgr.setflags(write=False)
    scores.setflags(write=False)
    return bgr, scores
