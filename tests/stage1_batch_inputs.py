"""Inputs shared by test_stage1_batch_host.py and test_gpu_stage1_batch.py: the ragged batch of three videos with the shot
lists process_decoded accepts (overlapping, past the video's end, empty, none at all) and the per-shot loops the closed
forms of ops.StageOneTables are checked against."""
import numpy as np

LENGTHS = [45, 31, 20]
# video 0: (0, 20) holds 7 samples (groups of 4 and 3); (20, 21) holds no multiple of 3 - an empty shot between two
# others; (21, 45) holds 8 samples (two groups of 4); (44, 60) reaches past the 45 frames and overlaps the shot before
# it: clipped to (44, 45), empty again.  Video 1 has no shots.  Video 2: (3, 3) is empty, (0, 20) holds 7 samples
COUNTS = [7, 0, 8, 0, 0, 7]      # sampled frames per shot
SHOTS = [[(0, 20), (20, 21), (21, 45), (44, 60)], [], [(3, 3), (0, 20)]]
FPS = [30.0, 25.0, 24.0]
SR = 16000


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def frames(lengths=LENGTHS, h=40, w=56, seed=21):
    """uint8 [sum(lengths), h, w, 3]: seeded noise, the videos concatenated."""
    return np.random.default_rng(seed).integers(0, 256, (int(np.sum(lengths)), h, w, 3), dtype=np.uint8)


def waveforms(lengths=LENGTHS, fps=FPS, seed=22):
    """One mono float32 track per video, as long as the video at its frame rate."""
    rng = np.random.default_rng(seed)
    return [(0.3 * rng.standard_normal(int(n / f * SR))).astype(np.float32) for n, f in zip(lengths, fps)]


def tables_by_loops(lengths, shots_per_video):
    """The tables of ops.StageOneTables from the loops of the per-video path: sample_shot_indices on the clipped shot, as
    process_decoded calls it, and the groups VisualFeatureExtractor.forward builds, range(0, c, MICRO_BATCH)."""
    from avsum_amd.features.extractors import MICRO_BATCH, sample_shot_indices
    base = offsets_of(lengths)
    shot_offsets, sample_offsets, sample_index, group_offsets, group_sizes = [0], [0], [], [], []
    for v, (shots, n) in enumerate(zip(shots_per_video, lengths)):
        for start, end in shots:
            idx = sample_shot_indices(start, min(end, n))
            group_offsets += [len(sample_index) + g for g in range(0, len(idx), MICRO_BATCH)]
            group_sizes += [min(MICRO_BATCH, len(idx) - g) for g in range(0, len(idx), MICRO_BATCH)]
            sample_index += [int(base[v]) + i for i in idx]
            sample_offsets.append(len(sample_index))
        shot_offsets.append(len(sample_offsets) - 1)
    group_offsets.append(len(sample_index))
    i64 = lambda x: np.asarray(x, dtype=np.int64).reshape(-1)
    return {"shot_offsets": i64(shot_offsets), "sample_offsets": i64(sample_offsets), "sample_index": i64(sample_index),
            "group_offsets": i64(group_offsets), "group_sizes": i64(group_sizes)}


def two_cut_video():
    """The 64-frame construction of test_gpu_configs.test_decoded_video_with_detected_shots: 40 x 56 frames that jitter
    around a base image replaced at frames 22 and 45, so the detector cuts there."""
    rng = np.random.default_rng(12)
    n, h, w = 64, 40, 56
    out = np.zeros((n, h, w, 3), dtype=np.uint8)
    base = rng.integers(0, 256, (h, w, 3))
    for f in range(n):
        if f in (22, 45):
            base = rng.integers(0, 256, (h, w, 3))
        out[f] = np.clip(base + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    return out
