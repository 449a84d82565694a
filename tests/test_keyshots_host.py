"""Host side of the keyshot summaries: the SummaryTables plan, the numpy oracle of evaluation/keyshots.py against brute
force, the pinned tie rule, the F1 identity with the reference's segment metric and the quantiser's edge cases."""
import numpy as np
import pytest

import keyshots_inputs as ki


# --------------------------------------------------------------------------- the plan
def test_summary_tables_capacities_and_words():
    from avsum_amd import ops, ragged
    assert ops.SummaryTables is ragged.SummaryTables
    assert ops.SUMMARY_MAX_CAPACITY == ragged.SUMMARY_MAX_CAPACITY == 8191
    lengths = (40, 47, 700, 7000)
    t = ragged.SummaryTables(ki.offsets_of(lengths), 0.15, 300, device="cpu")
    assert t.capacity.dtype == np.int64 and t.capacity.tolist() == [6, 7, 105, 1050]
    assert (t.nvideos, t.frames, t.ratio, t.shot_cap, t.max_capacity) == (4, sum(lengths), 0.15, 300, 1050)
    assert t.lengths.tolist() == list(lengths) and t.offsets.tolist() == ki.offsets_of(lengths).tolist()
    assert t.words == 17 == -(-(1050 + 1) // 64)
    assert t.take_words(21) == 21 * 300 * 17
    assert t.offsets_t.device.type == "cpu" and t.capacity_t.tolist() == [6, 7, 105, 1050]
    # the word count on both sides of a word boundary: 63 + 1 cells fill one word, 64 + 1 need two
    assert ragged.SummaryTables([0, 426], 0.15, 1, device="cpu").words == 1      # C = 63
    assert ragged.SummaryTables([0, 430], 0.15, 1, device="cpu").words == 2      # C = 64
    # shot_cap from a ShotTables
    shots = ragged.ShotTables(ki.offsets_of(lengths), 15, device="cpu")
    assert ragged.SummaryTables(ki.offsets_of(lengths), 0.15, shots, device="cpu").shot_cap == shots.shot_cap
    # the longest video at 0.15, and the rows limit keeps the workspace below 2^31 entries for 2^14 shots
    full = ragged.SummaryTables([0, 54613], 0.15, 1 << 14, device="cpu")
    assert full.max_capacity == 8191 and full.words == 128
    assert full.take_words(ragged.SUMMARY_MAX_ROWS) == 1 << 31 and full.take_words(ragged.SUMMARY_MAX_ROWS - 1) < 1 << 31
    assert ragged.SummaryTables([0, 54606], 0.15, 1, device="cpu").words == 128


@pytest.mark.parametrize("kwargs, fragment", [
    (dict(offsets_host=[0]), "offsets must hold"),
    (dict(offsets_host=[1, 5]), "start at 0"),
    (dict(offsets_host=[0, 5, 5]), "at least 1"),
    (dict(offsets_host=[0, 5, 3]), "decrease"),
    (dict(offsets_host=[0, (1 << 24) + 1]), "rows"),
    (dict(offsets_host=[0, 100], ratio=0.0), "ratio"),
    (dict(offsets_host=[0, 100], ratio=-0.1), "ratio"),
    (dict(offsets_host=[0, 100], ratio=1.5), "ratio"),
    (dict(offsets_host=[0, 100], ratio=float("nan")), "ratio"),
    (dict(offsets_host=[0, 100], ratio=float("inf")), "ratio"),
    (dict(offsets_host=[0, 100], shot_cap=0), "shot_cap"),
    (dict(offsets_host=[0, 40, 54654], ratio=0.15), "video 1 has 54614 frames"),
])
def test_summary_tables_refusals(kwargs, fragment):
    from avsum_amd import ragged
    with pytest.raises(ValueError, match="SummaryTables") as err:
        ragged.SummaryTables(device="cpu", **{"shot_cap": 1, **kwargs})
    assert fragment in str(err.value)


def test_summary_tables_ratio_one_is_allowed():
    from avsum_amd import ragged
    assert ragged.SummaryTables([0, 100], 1.0, 1, device="cpu").capacity.tolist() == [100]


# --------------------------------------------------------------------------- the oracle
def _random_problem(rng, constant):
    s = int(rng.integers(0, 11))
    weights = rng.integers(1, 40, size=s).astype(np.int64)
    if constant:
        sums = weights << 31                                   # every frame 0.5: every shot's value is 2^31, all ties
    else:
        from avsum_amd.evaluation.keyshots import quantise_scores
        sums = np.array([quantise_scores(rng.random(int(w), dtype=np.float32)).sum() for w in weights], dtype=np.int64)
    capacity = int(rng.integers(0, max(2, int(weights.sum()) + 2))) if s else int(rng.integers(0, 50))
    return sums, weights, capacity


def test_knapsack_host_against_brute_force():
    from avsum_amd.evaluation.keyshots import knapsack_host
    rng = np.random.default_rng(2024)
    for case in range(300):
        sums, weights, capacity = _random_problem(rng, constant=case % 3 == 0)
        picked, optimum = knapsack_host(sums, weights, capacity)
        s = weights.size
        subsets = (np.arange(1 << s)[:, None] >> np.arange(s)[None, :]) & 1          # every subset, [2^S, S]
        values = sums.astype(np.float64) / np.maximum(weights, 1).astype(np.float64)
        feasible = subsets @ weights <= capacity
        best = float(np.max((subsets @ values)[feasible]))
        assert picked.dtype == bool and picked.shape == (s,)
        assert int(weights[picked].sum()) <= capacity, case
        assert optimum == pytest.approx(best, rel=1e-12, abs=0.0), case
        assert float(values[picked].sum()) == pytest.approx(best, rel=1e-12, abs=0.0), case


def test_tie_rule_picks_the_first():
    """Two shots of equal weight and equal value, C = that weight: the second's cand > row is false."""
    from avsum_amd.evaluation.keyshots import keyshot_summary_host, knapsack_host
    picked, optimum = knapsack_host([5 << 31, 5 << 31], [5, 5], 5)
    assert picked.tolist() == [True, False] and optimum == 2.0 ** 31
    picked, mask, optimum = keyshot_summary_host(np.full(34, 0.5, np.float32), [(0, 5), (5, 10), (10, 34)], 34)
    assert picked.tolist() == [True, False, False] and mask.tolist() == [1] * 5 + [0] * 29 and optimum == 2.0 ** 31


def test_host_summary_edge_videos():
    """No shot; a shot heavier than the capacity; a shot of exactly the capacity."""
    from avsum_amd.evaluation.keyshots import keyshot_summary_host
    scores = np.linspace(0.1, 0.9, 47, dtype=np.float32)
    picked, mask, optimum = keyshot_summary_host(scores[:40], [], 40)
    assert picked.shape == (0,) and not mask.any() and optimum == 0.0
    picked, mask, optimum = keyshot_summary_host(scores, [(0, 47)], 47)
    assert picked.tolist() == [False] and not mask.any() and optimum == 0.0
    picked, mask, optimum = keyshot_summary_host(scores[:40], [(0, 6), (6, 40)], 40)
    assert picked.tolist() == [True, False] and mask.sum() == 6 and optimum > 0.0
    for bad in ([(0, 48)], [(5, 5)], [(-1, 4)], [(0, 10), (9, 20)], [(10, 20), (0, 5)]):
        with pytest.raises(ValueError, match="keyshot_summary_host"):
            keyshot_summary_host(scores, bad, 47)


def test_quantiser_edge_cases():
    from avsum_amd.evaluation.keyshots import quantise_scores
    x = np.array([0.0, 1.0, 2.0 ** -33, 1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, np.nan, -1.0, 2.0, 0.5], dtype=np.float32)
    got = quantise_scores(x)
    assert got.dtype == np.int64
    assert got.tolist() == [0, 1 << 32, 0, 2, 2, 0, 0, 1 << 32, 1 << 31]      # halves go to the even neighbour


def test_f1_is_the_reference_segment_metric():
    from avsum_amd.evaluation.keyshots import f1_from_overlap
    from avsum_amd.evaluation.metrics import compute_temporal_f1
    lengths, shots = ki.batch_videos()
    rows = np.concatenate([ki.score_rows(sum(lengths), 3)[:1], ki.user_rows(sum(lengths), 3, 4)])
    host = ki.host_summaries(rows, lengths, shots)
    off = ki.offsets_of(lengths)
    compared = 0
    for v, n in enumerate(lengths):
        pred = host["mask"][0, off[v]:off[v + 1]].astype(np.int64)
        for u in range(1, 4):
            user = host["mask"][u, off[v]:off[v + 1]].astype(np.int64)
            counts = np.array([(pred & user).sum(), pred.sum(), user.sum()], dtype=np.int64)
            got = f1_from_overlap(counts)
            if counts[1] == 0 or counts[2] == 0:
                assert np.isnan(got)
                continue
            assert float(got) == compute_temporal_f1(host["segments"][0][v], host["segments"][u][v], n)
            compared += 1
    assert compared >= 9
    table = f1_from_overlap(np.array([[[3, 6, 4], [0, 0, 4]]], dtype=np.int64))
    assert table.shape == (1, 2) and table[0, 0] == compute_temporal_f1([(0, 6)], [(3, 7)], 10) and np.isnan(table[0, 1])
    with pytest.raises(ValueError, match="f1_from_overlap"):
        f1_from_overlap(np.zeros((2, 3), dtype=np.int32))
