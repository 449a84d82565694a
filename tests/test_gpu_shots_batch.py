"""Batched shot detection and frame sampling on the GPU (ops.hsv_frame_diff_batch / shot_cuts_batch / shot_tables /
gather_rows, features.shots.detect_shots_batch / sample_frames): the integers of the per-video path, exactly."""
import numpy as np
import pytest
import torch

import shots_batch_inputs as sbi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(dev):
    """The batch, its per-video reference (detect_shots, hsv_frame_diff) and the batched result, computed once."""
    from avsum_amd import ops
    from avsum_amd.features.shots import detect_shots, detect_shots_batch, shot_tables_host
    videos, expected = sbi.batch_videos()
    offsets = sbi.offsets_of(videos)
    frames = torch.from_numpy(np.concatenate(videos)).to(dev)
    per_video = [detect_shots(torch.from_numpy(v).to(dev)) for v in videos]
    per_video_sums = [ops.hsv_frame_diff(torch.from_numpy(v).to(dev), 1).cpu().numpy() for v in videos]
    result = detect_shots_batch(frames, offsets)
    want = shot_tables_host([sbi.cuts_of(s) for s in per_video], [len(v) for v in videos])
    return {"videos": videos, "expected": expected, "offsets": offsets, "frames": frames, "per_video": per_video,
            "per_video_sums": per_video_sums, "result": result, "want": want}


def test_inputs_decide_as_designed(batch):
    """The per-video host rule places the cuts the inputs were built for (lengths 1, 2, 14, 16, 17, 31, 70, 401)."""
    assert [len(v) for v in batch["videos"]] == [1, 2, 14, 16, 17, 31, 70, 401]
    for v, shots in batch["expected"].items():
        assert batch["per_video"][v] == shots, v
    assert batch["per_video"][0] == [] and len(batch["per_video"][7]) > 3
    noisy = batch["per_video_sums"][7]
    assert (noisy[:, 0] > 0).any() and (noisy[:, 1] > 0).any()      # H and S contribute


def test_batch_sums_are_the_per_video_integers(batch):
    from avsum_amd import ops
    plan = batch["result"].plan
    got = ops.hsv_frame_diff_batch(batch["frames"], plan, 1)
    assert got.dtype == torch.int64
    got = got.cpu().numpy()
    assert np.array_equal(got, np.concatenate(batch["per_video_sums"]))
    assert not got[batch["offsets"][:-1]].any()                      # zeros at every video's first frame
    raw = batch["result"].sums.cpu().numpy()
    assert raw.dtype == np.int32 and np.array_equal(raw.astype(np.int64) & 0xFFFFFFFF, got)
    # a step that skips pixels, against the per-video call with the same step
    got3 = ops.hsv_frame_diff_batch(batch["frames"], plan, 3).cpu().numpy()
    want3 = np.concatenate([ops.hsv_frame_diff(torch.from_numpy(v).to(batch["frames"].device), 3).cpu().numpy()
                            for v in batch["videos"]])
    assert np.array_equal(got3, want3)


def test_host_lists_equal_detect_shots(batch):
    got = batch["result"].host()
    assert got == batch["per_video"]
    assert all(isinstance(a, int) and isinstance(b, int) for shots in got for a, b in shots)


def test_cut_slots(batch):
    res = batch["result"]
    cuts, totals, plan = res.cuts.cpu().numpy(), res.totals.cpu().numpy(), res.plan
    for v, shots in enumerate(batch["per_video"]):
        want = sbi.cuts_of(shots)
        assert len(want) <= plan.cut_off[v + 1] - plan.cut_off[v] == (len(batch["videos"][v]) - 1) // 15
        assert cuts[plan.cut_off[v]:plan.cut_off[v] + len(want)].tolist() == want
        assert totals[v, 0] == len(shots)


def test_tables_equal_shot_tables_host(batch):
    res, want = batch["result"], batch["want"]
    s, f, g, _ = (int(x) for x in want["counts"])
    assert np.array_equal(res.counts.cpu().numpy(), want["counts"])
    assert np.array_equal(res.shot_offsets.cpu().numpy(), want["shot_offsets"])
    assert np.array_equal(res.shots.cpu().numpy()[:s], want["shots"])
    assert np.array_equal(res.sample_offsets.cpu().numpy()[:s + 1], want["sample_offsets"])
    assert np.array_equal(res.sample_index.cpu().numpy()[:f], want["sample_index"])
    assert np.array_equal(res.group_offsets.cpu().numpy()[:g + 1], want["group_offsets"])
    host = res.host_tables()
    for name in ("counts", "shot_offsets", "shots", "sample_offsets", "group_offsets"):
        assert np.array_equal(host[name], want[name]), name
    # and the closed forms are the loops of the per-video path (the sample list and forward's groups)
    loops = sbi.tables_by_loops([sbi.cuts_of(x) for x in batch["per_video"]], [len(v) for v in batch["videos"]])
    for name in loops:
        assert np.array_equal(want[name], loops[name]), name
    assert (want["sample_offsets"][1:] == want["sample_offsets"][:-1]).any()     # the shot (16, 17): no sampled frame


def test_sample_frames_is_the_indexed_frames(batch):
    from avsum_amd.features.shots import sample_frames
    dense, groups = sample_frames(batch["frames"], batch["result"])
    want = batch["want"]
    assert dense.is_cuda and dense.dtype == torch.uint8 and dense.shape == (int(want["counts"][1]), 8, 8, 3)
    ref = np.concatenate(batch["videos"])[want["sample_index"]]
    assert dense.cpu().numpy().tobytes() == ref.tobytes()
    assert not groups.is_cuda and groups.dtype == torch.int64
    assert np.array_equal(groups.numpy(), want["group_offsets"])
    assert groups[0] == 0 and groups[-1] == dense.shape[0] and (groups[1:] - groups[:-1]).max() <= 4


def test_audio_bounds(batch):
    fps, sr = 29.97, 16000
    got = batch["result"].audio_bounds(fps, sr)
    assert got == [[(int(a / fps * sr), int(b / fps * sr)) for a, b in shots] for shots in batch["per_video"]]


def test_two_runs_give_identical_bytes(batch):
    from avsum_amd.features.shots import detect_shots_batch, sample_frames
    first = batch["result"]
    again = detect_shots_batch(batch["frames"], batch["offsets"])
    a, b = first.host_tables(), again.host_tables()
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    f = int(a["counts"][1])
    assert first.sample_index[:f].cpu().numpy().tobytes() == again.sample_index[:f].cpu().numpy().tobytes()
    assert first.sums.cpu().numpy().tobytes() == again.sums.cpu().numpy().tobytes()
    c1, c2, plan = first.cuts.cpu().numpy(), again.cuts.cpu().numpy(), first.plan
    for v, shots in enumerate(batch["per_video"]):                  # a slot is written up to the video's cuts
        used = slice(plan.cut_off[v], plan.cut_off[v] + max(len(shots) - 1, 0))
        assert c1[used].tobytes() == c2[used].tobytes(), v
    assert first.totals.cpu().numpy().tobytes() == again.totals.cpu().numpy().tobytes()
    d1, d2 = sample_frames(batch["frames"], first)[0], sample_frames(batch["frames"], again)[0]
    assert d1.cpu().numpy().tobytes() == d2.cpu().numpy().tobytes()


def test_video_longer_than_the_lds_chunk(dev):
    """One video of 8892 frames: three chunks of the cut kernel; `last` crosses both boundaries; the cap of 100."""
    from avsum_amd.features.shots import detect_shots, detect_shots_batch, sample_frames, shot_tables_host
    video, expected = sbi.long_video()
    frames = torch.from_numpy(video).to(dev)
    want_shots = detect_shots(frames)
    assert want_shots == expected
    res = detect_shots_batch(frames, [0, len(video)])
    assert res.host() == [want_shots]
    want = shot_tables_host([sbi.cuts_of(want_shots)], [len(video)])
    host = res.host_tables()
    for name in host:
        assert np.array_equal(host[name], want[name]), name
    assert want["counts"][3] == 100
    dense, groups = sample_frames(frames, res)
    assert np.array_equal(res.sample_index.cpu().numpy()[:dense.shape[0]], want["sample_index"])
    assert dense.cpu().numpy().tobytes() == video[want["sample_index"]].tobytes()
    assert np.array_equal(groups.numpy(), want["group_offsets"])


def test_more_than_65536_frames(dev):
    """65 600 + 40 frames in one launch: past the per-video call's 65 536 frames, where only the 64-bit frame index and
    grid x reach.  The reference is the input's construction (the per-video call cannot take the first video)."""
    from avsum_amd import ops
    from avsum_amd.features.shots import detect_shots_batch, sample_frames, shot_tables_host
    videos, cuts = sbi.past_65536_videos()
    lengths = [len(v) for v in videos]
    assert lengths[0] > 65537 and cuts[0][-1] > 65536
    allf = np.concatenate(videos)
    frames = torch.from_numpy(allf).to(dev)
    res = detect_shots_batch(frames, sbi.offsets_of(videos))
    want_sums = np.zeros((len(allf), 3), dtype=np.int64)
    for base, video_cuts in zip((0, lengths[0]), cuts):
        want_sums[base + np.asarray(video_cuts), 2] = sbi.JUMP * sbi.SIDE * sbi.SIDE
    assert np.array_equal(ops.hsv_frame_diff_batch(frames, res.plan, 1).cpu().numpy(), want_sums)
    assert res.host() == [list(zip([0] + c, c + [n])) for c, n in zip(cuts, lengths)]
    want = shot_tables_host(cuts, lengths)
    host = res.host_tables()
    for name in host:
        assert np.array_equal(host[name], want[name]), name
    dense, _ = sample_frames(frames, res)
    assert np.array_equal(res.sample_index.cpu().numpy()[:dense.shape[0]], want["sample_index"])
    assert dense.cpu().numpy().tobytes() == allf[want["sample_index"]].tobytes()


def test_other_threshold_and_scene_length(batch):
    """min_scene_len = 1 takes every candidate; a threshold of 80 / 3 admits the dV = 80 jumps too."""
    from avsum_amd.features.shots import detect_shots, detect_shots_batch
    dev = batch["frames"].device
    for threshold, gap in ((27.0, 1), (80 / 3.0, 15), (26.0, 4)):
        res = detect_shots_batch(batch["frames"], batch["offsets"], threshold, gap)
        want = [detect_shots(torch.from_numpy(v).to(dev), threshold, gap) for v in batch["videos"]]
        assert res.host() == want, (threshold, gap)


@pytest.mark.parametrize("row_shape,dtype,skip_rows", [((8, 8, 3), torch.uint8, 0),     # 192 B: 16-byte units
                                                        ((5, 4), torch.uint8, 0),        # 20 B: 4-byte units
                                                        ((5, 4), torch.uint8, 1),        # 20 B rows from a base at +20
                                                        ((7,), torch.uint8, 0),          # 7 B: single bytes
                                                        ((4352,), torch.float32, 0),     # 1088 units of 16 B: a whole piece and a part
                                                        ((2051,), torch.uint8, 0)])      # two whole pieces of single bytes and 3 more
def test_gather_rows(dev, row_shape, dtype, skip_rows):
    from avsum_amd import ops
    gen = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (37,) + row_shape, generator=gen).to(dtype).to(dev)[skip_rows:]
    index = torch.randint(0, src.shape[0], (23,), generator=gen).to(dev)
    count = torch.tensor([23], dtype=torch.int64, device=dev)
    out = ops.gather_rows(src, index, count)
    assert out.shape == (23,) + row_shape and out.dtype == dtype
    assert out.cpu().numpy().tobytes() == src[index].cpu().numpy().tobytes()


def test_gather_rows_count_below_capacity(dev):
    """The row count comes from device memory: rows past it keep the sentinel, an index outside src is skipped."""
    from avsum_amd import ops
    gen = torch.Generator().manual_seed(12)
    src = torch.randint(0, 256, (10, 8, 8, 3), dtype=torch.uint8, generator=gen).to(dev)
    index = torch.tensor([9, 0, 3, 3, 7, 1, 2, 4, 5], dtype=torch.int64, device=dev)
    counts = torch.tensor([99, 5, 99, 99], dtype=torch.int64, device=dev)
    out = torch.full((9, 8, 8, 3), 0xAB, dtype=torch.uint8, device=dev)
    got = ops.gather_rows(src, index, counts[1:2], out)
    assert got is out
    assert torch.equal(out[:5], src[index[:5]]) and bool((out[5:] == 0xAB).all())
    out.fill_(0xAB)
    ops.gather_rows(src, torch.tensor([2, 10, -1, 5], dtype=torch.int64, device=dev),
                    torch.tensor([4], dtype=torch.int64, device=dev), out[:4])
    assert torch.equal(out[0], src[2]) and torch.equal(out[3], src[5]) and bool((out[1:3] == 0xAB).all())
    with pytest.raises(ValueError):
        ops.gather_rows(src, index, counts)                      # count must be ONE element
    with pytest.raises(ValueError):
        ops.gather_rows(src, index.cpu(), counts[1:2])
