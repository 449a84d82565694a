"""The host plan of the batched stage-1 extraction, ops.StageOneTables with device="cpu": the sample, group and pass tables
against the per-shot loops of the per-video path, and every refusal.  No GPU needed."""
import numpy as np
import pytest

import stage1_batch_inputs as s1


def _plan(lengths=s1.LENGTHS, shots=s1.SHOTS, **kw):
    from avsum_amd import ops
    return ops.StageOneTables(s1.offsets_of(lengths), shots, device="cpu", **kw)


def _check_passes(plan, want):
    """pass_order a permutation with row_of_sample its inverse; the passes tile 0 .. F in order, each whole groups of one
    size within chunk_frames; a pass row's frame is its sample's frame."""
    f = plan.nsamples
    assert sorted(plan.pass_order.tolist()) == list(range(f))
    assert np.array_equal(plan.row_of_sample[plan.pass_order], np.arange(f))
    assert np.array_equal(plan.pass_frame_index, plan.sample_index[plan.pass_order])
    group_of = np.repeat(np.arange(want["group_sizes"].size), want["group_sizes"])      # sample position -> its group
    assert [lo for _, lo, _ in plan.passes] == [0] + [hi for _, _, hi in plan.passes[:-1]]
    assert (plan.passes[-1][2] if plan.passes else 0) == f
    sizes = [gsz for gsz, _, _ in plan.passes]
    assert sizes == sorted(sizes, reverse=True)                       # the sets follow one another: 4, 3, 2, 1
    for gsz, lo, hi in plan.passes:
        assert 0 < hi - lo <= plan.chunk_frames and (hi - lo) % gsz == 0
        members = plan.pass_order[lo:hi].reshape(-1, gsz)
        assert (np.diff(members, axis=1) == 1).all()                  # a group's frames, adjacent and in order
        assert (want["group_sizes"][group_of[members[:, 0]]] == gsz).all()
        assert (group_of[members] == group_of[members[:, :1]]).all()  # whole groups: never part of one
    assert np.array_equal(plan.pass_counts, [hi - lo for _, lo, hi in plan.passes])
    # inside a set the samples keep the shot order
    for gsz in set(sizes):
        rows = np.concatenate([plan.pass_order[lo:hi] for g, lo, hi in plan.passes if g == gsz])
        assert (np.diff(rows) > 0).all()


def test_tables_equal_the_per_shot_loops():
    plan, want = _plan(chunk_frames=8), s1.tables_by_loops(s1.LENGTHS, s1.SHOTS)
    assert np.diff(want["sample_offsets"]).tolist() == s1.COUNTS
    for name in ("shot_offsets", "sample_offsets", "sample_index", "group_offsets"):
        got = getattr(plan, name)
        assert got.dtype == np.int64 and np.array_equal(got, want[name]), name
    assert (plan.nvideos, plan.nshots, plan.nsamples, plan.frames) == (3, 6, 22, 96)
    assert np.array_equal(plan.shots, [(0, 20), (20, 21), (21, 45), (44, 60), (3, 3), (0, 20)])     # kept unclipped
    assert plan.shot_video.tolist() == [0, 0, 0, 0, 2, 2]
    _check_passes(plan, want)
    assert len(plan.passes) > 2                                       # chunk_frames = 8: several passes exist
    assert plan.passes == [(4, 0, 8), (4, 8, 16), (3, 16, 22)]
    # the device side stays on the host with device="cpu"
    for name in ("pass_frame_index", "row_of_sample", "sample_offsets", "pass_counts"):
        t = getattr(plan, name + "_t")
        assert t.device.type == "cpu" and np.array_equal(t.numpy(), getattr(plan, name))
    assert plan.samples.offsets_t is plan.sample_offsets_t and plan.samples.total == plan.nsamples


def test_every_group_size_and_odd_chunks():
    """Shots of 1, 2, 3, 5, 6 and 9 sampled frames: groups of every size; chunk_frames that no group size divides."""
    lengths = [100, 30]
    shots = [[(0, 1), (1, 6), (5, 13), (30, 45), (45, 63), (63, 90)], [(2, 28), (28, 30)]]
    want = s1.tables_by_loops(lengths, shots)
    assert np.diff(want["sample_offsets"]).tolist() == [1, 1, 3, 5, 6, 9, 9, 0]
    assert set(want["group_sizes"].tolist()) == {1, 2, 3, 4}
    for chunk in (4, 5, 7, 4096):
        plan = _plan(lengths, shots, chunk_frames=chunk)
        for name in ("shot_offsets", "sample_offsets", "sample_index", "group_offsets"):
            assert np.array_equal(getattr(plan, name), want[name]), name
        _check_passes(plan, want)
    assert [p[0] for p in _plan(lengths, shots).passes] == [4, 3, 2, 1]      # default chunk: one pass per set


def test_long_shot_is_capped_at_100():
    from avsum_amd.features.extractors import sample_shot_indices
    plan = _plan([400], [[(0, 400)]])
    assert plan.nsamples == 100 and plan.sample_offsets.tolist() == [0, 100]
    assert np.array_equal(plan.sample_index, sample_shot_indices(0, 400))
    assert np.array_equal(plan.group_offsets, np.arange(0, 101, 4))
    assert plan.passes == [(4, 0, 100)]


def test_tiling_shots_reproduce_shot_tables_host():
    from avsum_amd.features.shots import shot_tables_host
    cuts, lengths = [[15, 18, 30, 45], [16], [], [330], [15, 16, 17, 20]], [60, 17, 50, 730, 21]
    want = shot_tables_host(cuts, lengths)
    shots = [list(zip([0] + c, c + [n])) if c else [] for c, n in zip(cuts, lengths)]
    plan = _plan(lengths, shots)
    for name in ("shot_offsets", "sample_offsets", "sample_index", "group_offsets"):
        assert np.array_equal(getattr(plan, name), want[name]), name
    assert np.array_equal(plan.shots, want["shots"])
    assert (plan.nshots, plan.nsamples, plan.group_offsets.size - 1) == tuple(want["counts"][:3])


def test_batch_without_samples():
    plan = _plan([5, 7], [[], [(1, 3), (4, 4)]])
    assert (plan.nshots, plan.nsamples, plan.passes) == (2, 0, [])
    assert plan.sample_offsets.tolist() == [0, 0, 0] and plan.group_offsets.tolist() == [0]
    assert plan.pass_order.size == 0 and plan.row_of_sample.size == 0


def test_reexported_by_ops():
    from avsum_amd import ops, ragged
    assert ops.StageOneTables is ragged.StageOneTables
    assert {"StageOneTables", "resize_gather", "segment_mean_perm"} <= set(ops.__all__)


@pytest.mark.parametrize("lengths, shots, kw, match", [
    (s1.LENGTHS, [[(0, 20)], [], [(-1, 5)]], {}, "negative"),
    (s1.LENGTHS, s1.SHOTS[:2], {}, "2 shot lists for 3 videos"),
    (s1.LENGTHS, s1.SHOTS + [[]], {}, "4 shot lists for 3 videos"),
    ([(1 << 24) + 1], [[]], {}, "rows"),
    (s1.LENGTHS, s1.SHOTS, {"chunk_frames": 3}, "chunk_frames"),
])
def test_refusals(lengths, shots, kw, match):
    with pytest.raises(ValueError, match=match):
        _plan(lengths, shots, **kw)


def test_2_pow_24_frames_are_taken():
    assert _plan([1 << 24], [[(0, 9)]]).nsamples == 3
