"""Inputs shared by test_shots_batch_host.py and test_gpu_shots_batch.py: synthetic videos whose cuts the host rule
decides unambiguously, and the per-shot loops the closed forms are checked against.

A uniform grey frame has H = S = 0, so a jump of dV between two uniform grey frames scores exactly dV / 3: dV = 81 is
exactly the default threshold 27.0 (a cut candidate), dV = 80 is not."""
import numpy as np

SIDE = 8            # frames of 8 x 8 pixels: below the 256-pixel downscale width, so step = 1
JUMP, NEAR = 81, 80


def grey_video(n, jumps, side=SIDE, level=40):
    """uint8 [n, side, side, 3]: uniform grey frames; frame f differs from frame f - 1 by |dV| = jumps[f] (default 0)."""
    out = np.empty((n, side, side, 3), dtype=np.uint8)
    for f in range(n):
        dv = jumps.get(f, 0) if f else 0
        level = level + dv if level + dv <= 255 else level - dv
        out[f] = level
    return out


def noisy_video(n, seed, side=SIDE, change=0.15):
    """uint8 [n, side, side, 3]: torch.randint frames (H and S contribute) held for random runs: the score is 0 inside
    a run and far above the threshold where the frame changes, at irregular places."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, 256, (n, side, side, 3), dtype=torch.uint8, generator=gen).numpy()
    changes = torch.rand(n, generator=gen).numpy() < change
    which = np.cumsum(changes)
    return pool[which]


def batch_videos():
    """The batch of the GPU tests: (list of uint8 videos, what each is there for).  Lengths 1, 2, 14, 16, 17, 31, 70, 401."""
    videos = [
        grey_video(1, {}),                                       # one frame: nothing to compare
        grey_video(2, {1: JUMP}),                                # a candidate at f = 1 < min_scene_len: no cut, no shot
        grey_video(14, {}),                                      # no candidate at all
        grey_video(16, {14: JUMP, 15: JUMP}),                    # f = 14 ignored, f = 15 taken; consecutive candidates
        grey_video(17, {15: NEAR, 16: JUMP}),                    # dV = 80 is no candidate, dV = 81 is: the shot (16, 17)
        grey_video(31, {15: JUMP, 29: JUMP, 30: JUMP}),          # 14 after a cut: ignored; 15 after: taken
        grey_video(70, {20: JUMP, 34: NEAR, 49: JUMP, 63: JUMP, 64: JUMP, 65: JUMP}),   # cuts 49 | 64: both sides of a word
        noisy_video(401, 5),
    ]
    expected = {1: [], 2: [], 3: [(0, 15), (15, 16)], 4: [(0, 16), (16, 17)], 5: [(0, 15), (15, 30), (30, 31)],
                6: [(0, 20), (20, 49), (49, 64), (64, 70)]}
    return videos, expected


def long_video(chunk=4096):
    """One video longer than two LDS chunks of the cut kernel: cuts next to the chunk boundaries, candidates within
    min_scene_len of a cut that lies in the previous chunk, and shots of more than 300 frames (the cap of 100)."""
    n = 2 * chunk + 700
    jumps = {chunk - 6: JUMP, chunk - 1: JUMP, chunk: JUMP, chunk + 4: JUMP, chunk + 9: JUMP, chunk + 30: JUMP,
             2 * chunk - 15: JUMP, 2 * chunk: JUMP, 2 * chunk + 1: JUMP, 2 * chunk + 400: NEAR, 2 * chunk + 650: JUMP}
    expected = [0, chunk - 6, chunk + 9, chunk + 30, 2 * chunk - 15, 2 * chunk, 2 * chunk + 650, n]
    return grey_video(n, jumps), list(zip(expected[:-1], expected[1:]))


def past_65536_videos():
    """(two videos, their cut lists): the first is longer than the 65 536 frames the per-video frame-difference call
    takes and has a cut past that frame; every jump is 15 frames or more after the last, so every jump is a cut."""
    cuts = [[30, 65500, 65536, 65580], [20]]
    return [grey_video(n, dict.fromkeys(c, JUMP)) for n, c in zip((65600, 40), cuts)], cuts


def offsets_of(videos):
    return np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)


def cuts_of(shots):
    """The cut list behind a detect_shots result."""
    return [s for s, _ in shots[1:]]


def tables_by_loops(cuts_per_video, lengths):
    """shot_tables_host's tables from the loops of the per-video path: sample_shot_indices per shot and the groups
    VisualFeatureExtractor.forward builds, list(range(0, c, MICRO_BATCH)) + [c]."""
    from avsum_amd.features.extractors import MICRO_BATCH, sample_shot_indices
    base = np.concatenate([[0], np.cumsum(lengths)])
    shot_offsets, shots, sample_offsets, sample_index, group_offsets, most = [0], [], [0], [], [], 0
    for v, (cuts, n) in enumerate(zip(cuts_per_video, lengths)):
        bounds = [0] + list(cuts) + [int(n)] if len(cuts) else [0]
        for s, e in zip(bounds[:-1], bounds[1:]):
            idx = sample_shot_indices(s, e)
            group_offsets += [len(sample_index) + g for g in range(0, len(idx), MICRO_BATCH)]
            sample_index += [int(base[v]) + i for i in idx]
            shots.append((s, e))
            sample_offsets.append(len(sample_index))
            most = max(most, len(idx))
        shot_offsets.append(len(shots))
    group_offsets.append(len(sample_index))
    i64 = lambda x, shape=(-1,): np.asarray(x, dtype=np.int64).reshape(shape)
    return {"shot_offsets": i64(shot_offsets), "shots": i64(shots, (-1, 2)), "sample_offsets": i64(sample_offsets),
            "sample_index": i64(sample_index), "group_offsets": i64(group_offsets),
            "counts": i64([len(shots), len(sample_index), len(group_offsets) - 1, most])}
