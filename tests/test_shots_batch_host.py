"""Batched shot detection on the host: the closed forms of the sampling rule (features.shots.shot_tables_host) against
the per-shot loops of the per-video path, the capacities ops.ShotTables derives from the frame offsets alone, and the
argument checks that come before any launch.  No GPU needed."""
import numpy as np
import pytest
import torch

import shots_batch_inputs as sbi

# (cuts, length) per video.  Between them: shot starts with s % 3 = 0, 1, 2; the one-frame shot (16, 17) that holds no
# multiple of 3 (0 sampled frames, 0 groups); shots of 330 and 400 frames (the cap of 100); c = 1 (15, 18), c = 4
# (18, 30), c = 5 (30, 45); a video with no cut, so no shot; a one-frame video
CASES = [
    ([15, 18, 30, 45], 60),
    ([16], 17),
    ([], 50),
    ([330], 730),
    ([31, 47, 62], 63),
    ([], 1),
    ([15, 16, 17, 20], 21),
]


def _min_gap(cases):
    return min(int(np.diff([0] + cuts).min()) for cuts, _ in cases if cuts)


def test_cases_cover_what_they_claim():
    from avsum_amd.features.extractors import sample_shot_indices
    shots = [(s, e) for cuts, n in CASES if cuts for s, e in zip([0] + cuts, cuts + [n])]
    assert {s % 3 for s, _ in shots} == {0, 1, 2}
    counts = {(s, e): len(sample_shot_indices(s, e)) for s, e in shots}
    assert counts[(16, 17)] == 0 and counts[(15, 18)] == 1 and counts[(18, 30)] == 4 and counts[(30, 45)] == 5
    assert counts[(0, 330)] == 100 and counts[(330, 730)] == 100     # 110 and 134 multiples of 3, capped


def test_tables_equal_the_per_shot_loops():
    from avsum_amd.features.shots import shot_tables_host
    cuts, lengths = [c for c, _ in CASES], [n for _, n in CASES]
    got, want = shot_tables_host(cuts, lengths), sbi.tables_by_loops(cuts, lengths)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), name
    assert want["counts"][3] == 100 and want["shot_offsets"][3] == want["shot_offsets"][2]   # the cap; a shotless video


@pytest.mark.parametrize("cases", [CASES, CASES[:1], CASES[2:3], CASES[5:6], CASES[1:2] + CASES[3:4]])
def test_tables_of_any_sub_batch(cases):
    from avsum_amd.features.shots import shot_tables_host
    cuts, lengths = [c for c, _ in cases], [n for _, n in cases]
    got, want = shot_tables_host(cuts, lengths), sbi.tables_by_loops(cuts, lengths)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


def test_capacities_bound_every_case():
    """The capacities come from the offsets and min_scene_len alone and hold whatever the cuts are."""
    from avsum_amd import ops
    from avsum_amd.features.shots import shot_tables_host
    for cases in (CASES, CASES[:1], CASES[1:2], CASES[3:4], CASES[6:7]):
        cuts, lengths = [c for c, _ in cases], [n for _, n in cases]
        gap = _min_gap(cases)       # the largest min_scene_len these cuts are possible under
        plan = ops.ShotTables(np.concatenate([[0], np.cumsum(lengths)]), gap, device="cpu")
        t = shot_tables_host(cuts, lengths)
        s, f, g, _ = t["counts"]
        assert s <= plan.shot_cap and f <= plan.sample_cap and g <= plan.group_cap
        slots = np.diff(plan.cut_off)
        assert np.array_equal(slots, (np.asarray(lengths) - 1) // gap)
        assert all(len(c) <= slot for c, slot in zip(cuts, slots))
        assert plan.cut_cap == slots.sum() and plan.shot_cap == (slots + 1).sum()
        assert plan.sample_cap == sum(-(-n // 3) for n in lengths)
        # per video, too: its shots, sampled frames and groups fit its share of each capacity
        for v, n in enumerate(lengths):
            one = shot_tables_host([cuts[v]], [n])["counts"]
            assert one[0] <= slots[v] + 1 and one[1] <= -(-n // 3) and one[2] <= -(-n // 3) // 4 + slots[v] + 1


def test_capacity_is_reached():
    """Cuts every min_scene_len frames fill the cut slot and the shot capacity exactly: the bound is not loose."""
    from avsum_amd import ops
    from avsum_amd.features.shots import shot_tables_host
    for n, gap in ((61, 15), (16, 15), (10, 1), (100, 3)):
        cuts = list(range(gap, n, gap))
        plan = ops.ShotTables([0, n], gap, device="cpu")
        t = shot_tables_host([cuts], [n])
        assert len(cuts) == plan.cut_cap and t["counts"][0] == plan.shot_cap
        assert t["counts"][1] == plan.sample_cap == -(-n // 3) and t["counts"][2] <= plan.group_cap


def test_shot_tables_refuses_bad_offsets():
    from avsum_amd import ops
    for bad in ([0, 5, 3], [0, 5, 5], [0], [], [1, 4], [0, 1 << 31]):
        with pytest.raises(ValueError):
            ops.ShotTables(bad, device="cpu")
    with pytest.raises(ValueError):
        ops.ShotTables([0, 10], 0, device="cpu")
    plan = ops.ShotTables([0, 10, 40], device="cpu")
    assert plan.nvideos == 2 and plan.frames == 40 and plan.min_scene_len == 15
    assert plan.cut_off.tolist() == [0, 0, 1] and plan.shot_cap == 3 and plan.sample_cap == 4 + 10


def test_shot_tables_host_refuses_bad_cuts():
    from avsum_amd.features.shots import shot_tables_host
    for cuts, n in (([0], 10), ([10], 10), ([5, 5], 10), ([6, 5], 10)):
        with pytest.raises(ValueError):
            shot_tables_host([cuts], [n])
    with pytest.raises(ValueError):
        shot_tables_host([[5]], [10, 10])


def test_host_tensors_are_rejected():
    from avsum_amd import ops
    from avsum_amd.features.shots import detect_shots_batch, sample_frames
    frames = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    plan = ops.ShotTables([0, 4], device="cpu")
    with pytest.raises(ValueError):
        detect_shots_batch(frames, [0, 4])
    with pytest.raises(ValueError):
        ops.hsv_frame_diff_batch(frames, plan)
    with pytest.raises(ValueError):
        ops.shot_cuts_batch(plan, torch.zeros((4, 3), dtype=torch.int32), 64.0)
    with pytest.raises(ValueError):
        ops.shot_tables(plan, torch.zeros(0, dtype=torch.int64), torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.gather_rows(frames, torch.zeros(2, dtype=torch.int64), torch.ones(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        sample_frames(frames, None)


def test_entry_points_check_arguments_before_any_launch():
    """The C entries return an error status on bad extents or null pointers without touching the device."""
    from avsum_amd import _abi
    lib = _abi.lib()
    arg, shape = -1, -2   # AVS_E_ARG, AVS_E_SHAPE
    assert lib.avs_hsv_frame_diff_batch_u8(None, 4, 0, 8, 1, None, 1, None, None) == shape
    assert lib.avs_hsv_frame_diff_batch_u8(None, 4, 8, 8, 1, None, 1, None, None) == arg
    assert lib.avs_hsv_frame_diff_batch_u8(None, 0, 8, 8, 1, None, 0, None, None) == 0
    assert lib.avs_shot_cuts_batch(None, 4, None, 1, 64.0, 27.0, 0, None, None, None, None) == shape
    assert lib.avs_shot_cuts_batch(None, 4, None, 1, 64.0, 27.0, 15, None, None, None, None) == arg
    assert lib.avs_shot_tables_fill(None, 0, None, None, None, None, None, 1, None, None, 1, None, 1, None, None) == shape
    assert lib.avs_shot_tables_fill(None, 1, None, None, None, None, None, 1, None, None, 1, None, 1, None, None) == arg
    assert lib.avs_gather_rows_u8(None, 4, 0, None, None, 4, None, None) == shape
    assert lib.avs_gather_rows_u8(None, 4, 16, None, None, 4, None, None) == arg
    assert lib.avs_gather_rows_u8(None, 4, 16, None, None, 0, None, None) == 0
