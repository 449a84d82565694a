"""Keyshot summaries on the GPU (ops.shot_value_sums / knapsack_batch / mask_overlap_counts, evaluation.keyshots): the
integers and the fp64 optimum of the numpy oracle, exactly."""
import numpy as np
import pytest
import torch

import keyshots_inputs as ki
import shots_batch_inputs as sbi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(dev):
    """The main batch (V = 5, K = 3), its host oracle and the device result, computed once."""
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    lengths, shots = ki.batch_videos()
    offsets = ki.offsets_of(lengths)
    rows = ki.score_rows(int(offsets[-1]), 1)
    scores = torch.from_numpy(rows).to(dev)
    return {"lengths": lengths, "shots": shots, "offsets": offsets, "rows": rows, "scores": scores,
            "host": ki.host_summaries(rows, lengths, shots), "result": keyshot_summaries_device(scores, offsets, shots)}


def _assert_equals_host(result, host, shots):
    flat = np.concatenate([np.concatenate(p) if len(p) else np.zeros(0, bool) for p in host["picked"]])
    nshots = sum(len(s) for s in shots)
    assert np.array_equal(result.mask.cpu().numpy(), host["mask"])
    assert np.array_equal(result.totals.cpu().numpy(), host["totals"])
    optimum = result.optimum.cpu().numpy()
    assert optimum.dtype == np.float64 and (optimum == host["optimum"]).all()
    picked = result.picked.cpu().numpy()[:, :nshots]
    assert np.array_equal(picked.astype(bool).reshape(-1), flat)
    assert result.host() == host["segments"]


def test_batch_equals_the_host_oracle(batch):
    lengths, host, result = batch["lengths"], batch["host"], batch["result"]
    assert lengths == [40, 47, 430, 6830, 700]
    plan = result.plan
    assert plan.capacity.tolist() == [6, 7, 64, 1024, 105] and plan.words == 17
    assert 150 <= len(batch["shots"][3]) <= 230 and batch["shots"][4][0] == (0, 105)
    assert result.mask.dtype == torch.uint8 and result.mask.shape == (3, sum(lengths))
    assert result.picked.shape == (3, plan.shot_cap) and result.optimum.shape == (3, 5) and result.totals.shape == (3, 5, 3)
    _assert_equals_host(result, host, batch["shots"])
    # the inputs decide as designed: nothing taken in the first two videos, something in the others, in every row, and
    # never more frames than the capacity; in the constant row every shot is worth 2^31, so the optimum counts shots
    totals = host["totals"]
    assert not totals[:, :2, :2].any() and (totals[:, 2:, 0] > 0).all() and (totals[:, :, 1] <= totals[:, :, 2]).all()
    assert (host["optimum"][1] == totals[1, :, 0] * 2.0 ** 31).all()


def test_shot_value_sums_are_exact(batch):
    from avsum_amd import ops
    from avsum_amd.evaluation.keyshots import quantise_scores
    result, off = batch["result"], batch["offsets"]
    got = ops.shot_value_sums(result.plan, batch["scores"], result.shot_offsets, result.shots).cpu().numpy()
    want = []
    for v, shots in enumerate(batch["shots"]):
        q = quantise_scores(batch["rows"][:, off[v]:off[v + 1]])
        want += [q[:, s:e].sum(axis=1) for s, e in shots]
    assert got.dtype == np.int64 and np.array_equal(got, np.stack(want, 1))
    # a row view with a row stride and a misaligned first score
    wide = torch.zeros((3, batch["scores"].shape[1] + 3), dtype=torch.float32, device=batch["scores"].device)
    wide[:, 1:-2] = batch["scores"]
    again = ops.shot_value_sums(result.plan, wide[:, 1:-2], result.shot_offsets, result.shots).cpu().numpy()
    assert np.array_equal(again, got)


def test_full_lds_configuration(dev):
    """Capacities 8190 and 8191 (the largest): 128 words of take bits, both rows of 8192 cells in LDS."""
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    lengths, shots = ki.full_lds_videos()
    rows = np.random.default_rng(5).random((1, sum(lengths)), dtype=np.float32)
    result = keyshot_summaries_device(torch.from_numpy(rows[0]).to(dev), ki.offsets_of(lengths), shots)
    assert result.plan.capacity.tolist() == [8190, 8191] and result.plan.words == 128
    assert [len(s) for s in shots] == [40, 40]
    host = ki.host_summaries(rows, lengths, shots)
    _assert_equals_host(result, host, shots)
    assert (host["totals"][0, :, 0] > 0).all()


def test_shot_batch_result_equals_host_lists(dev):
    """The detector's device tables, used where they lie, against the same shots uploaded from host lists."""
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    from avsum_amd.features.shots import detect_shots_batch
    from avsum_amd.pipeline import FrameScoringPipeline
    videos, _ = sbi.batch_videos()
    offsets = sbi.offsets_of(videos)
    lengths = [len(v) for v in videos]
    detected = detect_shots_batch(torch.from_numpy(np.concatenate(videos)).to(dev), offsets)
    rows = np.random.default_rng(9).random((2, int(offsets[-1])), dtype=np.float32)
    scores = torch.from_numpy(rows).to(dev)
    residents = {ratio: keyshot_summaries_device(scores, offsets, detected, ratio) for ratio in (0.15, 0.6)}
    assert detected._host is None                                       # nothing was downloaded on the way
    lists = detected.host()
    for ratio, resident in residents.items():
        assert resident._host is None
        assert resident.shots.data_ptr() == detected.shots.data_ptr()
        assert resident.picked.shape[1] == detected.plan.shot_cap
        uploaded = FrameScoringPipeline.summarize_device(scores, offsets, lists, ratio)
        nshots = sum(len(s) for s in lists)
        assert uploaded.picked.shape[1] == nshots < detected.plan.shot_cap
        for name in ("mask", "optimum", "totals"):
            assert torch.equal(getattr(resident, name), getattr(uploaded, name)), name
        assert torch.equal(resident.picked[:, :nshots], uploaded.picked)
        assert resident.host() == uploaded.host()
        _assert_equals_host(resident, ki.host_summaries(rows, lengths, lists, ratio), lists)
    assert resident.totals[:, :, 0].sum().item() > 0


def test_video_alone_and_inside_a_batch(batch, dev):
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    off, result = batch["offsets"], batch["result"]
    for v in (2, 3, 4):
        alone = keyshot_summaries_device(batch["scores"][0, off[v]:off[v + 1]].contiguous(), [0, batch["lengths"][v]],
                                         [batch["shots"][v]])
        assert torch.equal(alone.mask[0], result.mask[0, off[v]:off[v + 1]])
        assert alone.optimum[0, 0].item() == result.optimum[0, v].item()
        assert torch.equal(alone.totals[0, 0], result.totals[0, v])
        assert alone.host()[0][0] == result.host()[0][v]


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_keyshot_f1_equals_the_host_pipeline(batch, dev, reduce):
    from avsum_amd.evaluation.keyshots import keyshot_f1_device
    lengths, shots = batch["lengths"], batch["shots"]
    users = ki.user_rows(sum(lengths), 3, 7)
    rows = np.concatenate([batch["rows"][:1], users])
    host = ki.host_summaries(rows, lengths, shots)
    want, table = ki.host_f1(host["segments"][0], host["segments"][1:], lengths, reduce)
    got, mean = keyshot_f1_device(batch["scores"][0], torch.from_numpy(users).to(dev), batch["offsets"], shots,
                                  reduce=reduce)
    assert got.dtype == np.float64 and got.shape == (5,)
    assert np.isnan(want[:2]).all() and not np.isnan(want[2:]).any()      # the two videos with an empty summary
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert (got[2:] == want[2:]).all() and (table[2:] > 0).any()
    assert np.isnan(mean) and np.mean(got[2:]) == np.mean(want[2:])


def test_overlap_counts_are_the_mask_sums(batch):
    from avsum_amd import ops
    mask, off = batch["result"].mask, batch["offsets"]
    got = ops.mask_overlap_counts(off, mask[0], mask[1:]).cpu().numpy()
    assert torch.equal(ops.mask_overlap_counts(batch["result"].plan, mask[0], mask[1:]).cpu(), torch.from_numpy(got))
    host = batch["host"]["mask"].astype(np.int64)
    want = np.array([[[(host[0, a:b] & host[u, a:b]).sum(), host[0, a:b].sum(), host[u, a:b].sum()] for u in (1, 2)]
                     for a, b in zip(off[:-1], off[1:])], dtype=np.int64)
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_every_frame_of_the_mask_is_written(batch, monkeypatch):
    """The wrapper's torch.empty buffers arrive filled with 0xFF: no frame keeps it - shots or no shots, gaps or not."""
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    real_empty = torch.empty

    def poisoned(*args, **kwargs):
        out = real_empty(*args, **kwargs)
        if out.dtype == torch.uint8:
            out.fill_(0xFF)
        return out

    monkeypatch.setattr(torch, "empty", poisoned)
    result = keyshot_summaries_device(batch["scores"], batch["offsets"], batch["shots"])
    monkeypatch.undo()
    mask = result.mask.cpu().numpy()
    assert set(np.unique(mask).tolist()) <= {0, 1}
    assert np.array_equal(mask, batch["host"]["mask"])
    nshots = sum(len(s) for s in batch["shots"])
    assert set(np.unique(result.picked.cpu().numpy()[:, :nshots]).tolist()) <= {0, 1}


def test_argument_refusals(batch, dev):
    from avsum_amd import ops
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    result, scores, offsets, shots = batch["result"], batch["scores"], batch["offsets"], batch["shots"]
    plan = result.plan
    with pytest.raises(ValueError, match="keyshot_summaries_device"):
        keyshot_summaries_device(scores.cpu(), offsets, shots)                   # a host tensor for the scores
    with pytest.raises(ValueError, match="shot_value_sums: scores must be a device tensor"):
        ops.shot_value_sums(plan, scores.cpu(), result.shot_offsets, result.shots)
    with pytest.raises(ValueError, match="shot_value_sums: scores must hold 8047 frames"):
        ops.shot_value_sums(plan, scores[:, :-1], result.shot_offsets, result.shots)
    with pytest.raises(ValueError, match="shot_value_sums: shots must have shape"):
        ops.shot_value_sums(plan, scores, result.shot_offsets, result.shots[:-1])
    sums = ops.shot_value_sums(plan, scores, result.shot_offsets, result.shots)
    with pytest.raises(ValueError, match="knapsack_batch: shots must have shape"):
        ops.knapsack_batch(plan, sums, result.shot_offsets, result.shots[:-1])
    with pytest.raises(ValueError, match="knapsack_batch: sums"):
        ops.knapsack_batch(plan, sums[:, :-1], result.shot_offsets, result.shots)
    overlapping = [list(s) for s in shots]
    overlapping[2] = [(0, 20), (19, 40)]
    with pytest.raises(ValueError, match="keyshot_summaries_device: video 2: the shots must ascend"):
        keyshot_summaries_device(scores, offsets, overlapping)
    with pytest.raises(ValueError, match="keyshot_summaries_device: video 1: every shot"):
        keyshot_summaries_device(scores, offsets, [shots[0], [(0, 48)]] + shots[2:])
    many = torch.zeros((ops.SUMMARY_MAX_ROWS + 1, 40), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="shot_value_sums: 1025 score rows"):
        keyshot_summaries_device(many, [0, 40], [[(0, 5)]])
    with pytest.raises(ValueError, match="knapsack_batch: 1025 score rows"):
        ops.knapsack_batch(plan, torch.zeros((1025, plan.shot_cap), dtype=torch.int64, device=dev), result.shot_offsets,
                           result.shots)
    with pytest.raises(ValueError, match="mask_overlap_counts: the offsets end at"):
        ops.mask_overlap_counts(offsets[:-1], result.mask[0], result.mask[1:])
    with pytest.raises(ValueError, match="mask_overlap_counts: user_masks"):
        ops.mask_overlap_counts(plan, result.mask[0], result.mask[1:, :-1])
    with pytest.raises(ValueError, match="SummaryTables"):
        keyshot_summaries_device(scores, offsets, shots, ratio=0.0)
