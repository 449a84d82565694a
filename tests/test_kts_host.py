"""Host side of kernel temporal segmentation: the numpy oracle of features/kts.py against brute force and on planted
inputs, the pinned tie rule, the flag, the stride / shot conversion, the KtsTables plan and the validation-before-launch
returns of the C entry points."""
import itertools

import numpy as np
import pytest

import kts_inputs as kin

ARG, SHAPE, WORKSPACE = -1, -2, -5   # AVS_E_ARG, AVS_E_SHAPE, AVS_E_WORKSPACE


def _gram(x):
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return x64 @ x64.T


# --------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("lmin", [1, 2])
def test_scores_equal_brute_force(lmin):
    from avsum_amd.features.kts import cpd_auto_host, cpd_nonlin_host, max_change_points, scatter_tables_host
    K = _gram(np.random.default_rng(0).standard_normal((9, 5)).astype(np.float32))
    n = 9
    K1, K2, Jt, flag = scatter_tables_host(K)
    assert flag == 0 and K1.shape == (10,) and K2.shape == Jt.shape == (10, 10)

    def scatter(t, l):                       # the definition, from the samples themselves
        block = K[t:l, t:l]
        return np.trace(block) - block.sum() / (l - t)

    for t, l in itertools.combinations(range(n + 1), 2):
        assert Jt[l, t] == pytest.approx(scatter(t, l), abs=1e-9)
    cps, costs, scores, flag = cpd_auto_host(K, None, 1.0, lmin)
    m_max = max_change_points(n, None, lmin)
    assert m_max == (8 if lmin == 1 else 3) and scores.shape == costs.shape == (m_max + 1,) and flag == 0
    for m in range(m_max + 1):
        best = np.inf
        for cut in itertools.combinations(range(1, n), m):
            b = (0,) + cut + (n,)
            if min(b[i + 1] - b[i] for i in range(m + 1)) >= lmin:
                best = min(best, sum(scatter(b[i], b[i + 1]) for i in range(m + 1)))
        assert abs(best - scores[m]) <= 1e-9, (m, best, scores[m])
        fixed_cps, fixed_scores = cpd_nonlin_host(K, m, lmin)
        assert fixed_cps.shape == (m,) and (fixed_scores == scores[:m + 1]).all()
        b = [0] + fixed_cps.tolist() + [n]
        assert min(np.diff(b)) >= lmin
        assert sum(scatter(b[i], b[i + 1]) for i in range(m + 1)) == pytest.approx(scores[m], abs=1e-9)
    assert cps.tolist() == cpd_nonlin_host(K, int(np.argmin(costs)), lmin)[0].tolist()


@pytest.mark.parametrize("lengths, d, want", [
    ((7, 12, 5, 9), 20, [7, 19, 24]),
    ((40, 23, 64, 31, 50), 64, [40, 63, 127, 158]),
    ((33,), 20, []),
])
def test_planted_change_points_are_recovered(lengths, d, want):
    from avsum_amd.features.kts import cpd_auto_host, kts_host
    x = kin.planted(lengths, d, 0.02, 3)
    cps, costs, scores, flag = cpd_auto_host(_gram(x), min(12, len(x) - 1))
    assert cps.tolist() == want and flag == 0
    ordered = np.sort(costs)
    assert ordered[1] - ordered[0] >= 2e-3
    again, shots, costs2, flag2 = kts_host(x, 1, min(12, len(x) - 1))
    assert again.tolist() == want and (costs2 == costs).all() and flag2 == 0
    assert shots == list(zip([0] + want, want + [len(x)]))


def test_tie_rule_takes_the_smallest_t():
    """K = ones: every J(t, l) is exactly 0, every segmentation ties, and the smallest t wins at every step."""
    from avsum_amd.features.kts import cpd_auto_host, cpd_nonlin_host, scatter_tables_host
    K = np.ones((23, 23))
    Jt = scatter_tables_host(K)[2]
    assert all(Jt[l, t] == 0.0 for l in range(24) for t in range(l))
    cps, scores = cpd_nonlin_host(K, 4, 3)
    assert cps.tolist() == [3, 6, 9, 12] and scores[4] == 0.0 and (scores == 0.0).all()
    cps, costs, _, _ = cpd_auto_host(K, 4, 1.0, 3, select="fixed")
    assert cps.tolist() == [3, 6, 9, 12]
    assert cpd_auto_host(K, 4, 1.0, 3)[0].tolist() == []        # all scores 0: the penalty decides for k = 0
    with pytest.raises(ValueError, match="cpd_nonlin_host"):
        cpd_nonlin_host(K, 7, 3)                                # 8 segments of 3 do not fit 23 samples
    with pytest.raises(ValueError, match="select"):
        cpd_auto_host(K, 4, 1.0, 3, select="best")


def test_non_finite_kernel_sets_the_flag():
    from avsum_amd.features.kts import cpd_auto_host, kts_host, scatter_tables_host
    K = np.ones((23, 23))
    K[5, 7] = np.nan
    assert scatter_tables_host(K)[3] == 1
    K = np.ones((23, 23))
    K[5, 7], K[9, 2] = np.inf, -np.inf
    assert scatter_tables_host(K)[3] == 1
    cps, costs, scores, flag = cpd_auto_host(K, 5)
    assert flag == 1 and cps.shape == (0,) and costs.shape == (6,) and np.isnan(costs).all()
    x = kin.planted((7, 12), 6)
    x[4, 2] = np.nan
    cps, shots, costs, flag = kts_host(x, 2)
    assert flag == 1 and cps.shape == (0,) and shots == [(0, 19)]


def test_stride_and_shot_conversion():
    from avsum_amd.features.kts import cpd_auto_host, kts_host, shots_from_change_points
    x = kin.planted((30, 45, 26), 16, 0.02, 8)                  # N = 101: no multiple of 5
    cps, shots, costs, flag = kts_host(x, 5, 6)
    assert cps.tolist() == [6, 15] and shots == [(0, 30), (30, 75), (75, 101)] and costs.shape == (7,) and flag == 0
    want = cpd_auto_host(_gram(x[::5]), 6)
    assert want[0].tolist() == cps.tolist() and (want[1] == costs).all()
    assert shots_from_change_points([], 101, 5) == [(0, 101)]
    # one sample: nothing to cut, whatever the stride
    cps, shots, costs, flag = kts_host(x[:7], 15)
    assert cps.shape == (0,) and shots == [(0, 7)] and costs.tolist() == [0.0] and flag == 0
    cps, shots, costs, flag = kts_host(x[:1], 1, lmin=3)
    assert cps.shape == (0,) and shots == [(0, 1)] and costs.shape == (1,)


def test_penalties():
    from avsum_amd.features.kts import kts_penalties
    pen = kts_penalties(50, 3, 2.0)
    assert pen.dtype == np.float64 and pen[0] == 0.0
    for k in (1, 2, 3):
        assert pen[k] == (2.0 * k / (2.0 * 50.0)) * (np.log(50.0 / k) + 1.0)
    assert kts_penalties(7, 0).tolist() == [0.0]


# --------------------------------------------------------------------------- the plan
def test_kts_tables_layout():
    from avsum_amd import ops, ragged
    from avsum_amd.features.kts import kts_penalties
    assert ops.KtsTables is ragged.KtsTables and ops.KTS_MAX_SAMPLES == ragged.KTS_MAX_SAMPLES == 2048
    lengths = (7, 100, 31, 1951)
    t = ragged.KtsTables(kin.offsets_of(lengths), 15, None, 1.0, 1, device="cpu")
    assert t.n.tolist() == [1, 7, 3, 131] and t.max_n == 131 and t.m_max.tolist() == [0, 6, 2, 130]
    assert (t.nvideos, t.frames, t.stride, t.lmin, t.vmax) == (4, sum(lengths), 15, 1, 1.0)
    assert t.k_offsets.tolist() == [0, 1, 50, 59, 59 + 131 * 131] and t.k_entries == 59 + 131 * 131
    assert t.k1_offsets.tolist() == [0, 2, 10, 14, 146]
    assert t.jt_offsets.tolist() == [0, 4, 68, 84, 84 + 132 * 132]
    assert t.p_offsets.tolist() == [0, 2, 58, 70, 70 + 131 * 132]
    assert t.cost_offsets.tolist() == [0, 1, 8, 11, 142] and t.cost_cap == t.shot_cap == 142
    assert t.penalties.dtype == np.float64 and t.penalties.shape == (142,)
    assert (t.penalties[11:] == kts_penalties(131, 130, 1.0)).all() and t.penalties[0] == t.penalties[1] == 0.0
    # the upper-triangle tiles of 64 x 64: one for each of the small videos, 3 x 4 / 2 = 6 for n = 131
    assert t.tiles.dtype == np.int32 and t.ntiles == 9
    assert t.tiles.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [3, 0, 1], [3, 0, 2], [3, 1, 1], [3, 1, 2],
                                [3, 2, 2]]
    assert t.videos.shape == (4, 10) and t.videos[3].tolist() == [138, 1951, 131, 130, 59, 14, 84, 70, 11, 0]
    assert t.offsets_t.device.type == t.videos_t.device.type == t.tiles_t.device.type == "cpu"
    assert t.penalties_t.dtype.is_floating_point and t.penalties_t.numel() == 142
    assert t.shots_of(1, [2, 5]) == [(0, 30), (30, 75), (75, 100)]
    # lmin and ncp, one per video (None: n - 1); a video shorter than lmin keeps m_max = 0
    t = ragged.KtsTables(kin.offsets_of((2, 9, 33, 160)), 1, [None, 8, 4, 159], 2.0, 3, device="cpu")
    assert t.n.tolist() == [2, 9, 33, 160] and t.m_max.tolist() == [0, 2, 4, 52] and t.vmax == 2.0
    assert ragged.KtsTables([0, 2048], 1, 3, device="cpu").m_max.tolist() == [3]


@pytest.mark.parametrize("kwargs, fragment", [
    (dict(video_offsets=[0]), "offsets must hold"),
    (dict(video_offsets=[1, 5]), "start at 0"),
    (dict(video_offsets=[0, 5, 5]), "at least 1"),
    (dict(video_offsets=[0, 5, 3]), "decrease"),
    (dict(video_offsets=[0, 100], stride=0), "stride"),
    (dict(video_offsets=[0, 100], lmin=0), "lmin"),
    (dict(video_offsets=[0, 100], ncp=-1), "ncp"),
    (dict(video_offsets=[0, 100, 200], ncp=[3]), "ncp entries"),
    (dict(video_offsets=[0, 100], vmax=0.0), "vmax"),
    (dict(video_offsets=[0, 100], vmax=-1.0), "vmax"),
    (dict(video_offsets=[0, 100], vmax=float("nan")), "vmax"),
    (dict(video_offsets=[0, 100], vmax=float("inf")), "vmax"),
    (dict(video_offsets=[0, 40, 40 + 2049], stride=1), "video 1 has 2049 samples"),
    (dict(video_offsets=[0, 40, 40 + 15 * 2048 + 1], stride=15), "video 1 has 2049 samples"),
    (dict(video_offsets=np.arange(0, 2048 * 513, 2048), stride=1, ncp=0), "packed Gram buffer"),
])
def test_kts_tables_refusals(kwargs, fragment):
    from avsum_amd import ragged
    with pytest.raises(ValueError, match="KtsTables") as err:
        ragged.KtsTables(device="cpu", **kwargs)
    assert fragment in str(err.value)


# --------------------------------------------------------------------------- the C entry points
def test_workspace_bytes_mirror_the_plan():
    from avsum_amd import _abi, ops, ragged
    for lengths, stride, ncp in (((7, 100, 31, 1951), 15, None), ((1,), 1, None), ((2048,), 1, 3), ((33, 160), 1, [32, 5])):
        t = ragged.KtsTables(kin.offsets_of(lengths), stride, ncp, device="cpu")
        got = _abi.lib().avs_kts_workspace_bytes(t.k1_entries, t.k_entries, t.jt_entries, t.p_entries)
        assert got == t.workspace_bytes == ops.kts_workspace(t) and got % 256 == 0
        assert got >= 8 * (t.k1_entries + t.k_entries + t.jt_entries) + 2 * t.p_entries
    assert _abi.lib().avs_kts_workspace_bytes(1, 1 << 31, 1, 1) == 0
    assert _abi.lib().avs_kts_workspace_bytes(0, 1, 1, 1) == 0
    with pytest.raises(ValueError, match="kts_workspace"):
        ops.kts_workspace(None)


def test_entry_points_check_arguments_before_any_launch():
    """The C entries return an error status on bad extents, null pointers or a short workspace without touching the
    device."""
    from avsum_amd import _abi
    lib = _abi.lib()
    gram = lambda **k: lib.avs_kts_gram_f64(*[k.get(a, d) for a, d in (   # noqa: E731
        ("x", None), ("rows", 8), ("d", 4), ("ld", 4), ("stride", 1), ("videos", None), ("nvideos", 1), ("tiles", None),
        ("ntiles", 1), ("gram", None), ("k_entries", 64), ("stream", None))])
    assert gram() == ARG
    for bad in (dict(rows=0), dict(d=0), dict(ld=3), dict(stride=0), dict(nvideos=0), dict(nvideos=65536), dict(ntiles=0),
                dict(k_entries=0), dict(k_entries=1 << 31)):
        assert gram(**bad) == SHAPE, bad
    entries = (3, 4, 9, 6)
    assert lib.avs_kts_scatters_f64(None, None, 1, 2, None, 1 << 20, *entries, None, None) == ARG
    assert lib.avs_kts_scatters_f64(None, None, 0, 2, None, 1 << 20, *entries, None, None) == SHAPE
    assert lib.avs_kts_scatters_f64(None, None, 1, 2049, None, 1 << 20, *entries, None, None) == SHAPE
    assert lib.avs_kts_scatters_f64(None, None, 1, 2, None, 1 << 20, 3, 4, 1 << 31, 6, None, None) == SHAPE
    dp = lambda **k: lib.avs_kts_dp_f64(*[k.get(a, d) for a, d in (       # noqa: E731
        ("videos", None), ("nvideos", 1), ("max_n", 2), ("lmin", 1), ("stride", 1), ("fixed", 0), ("pen", None),
        ("ws", None), ("ws_bytes", 1 << 20), ("k1", 3), ("k", 4), ("jt", 9), ("p", 6), ("cost_cap", 2), ("flags", None),
        ("scores", None), ("costs", None), ("cps", None), ("shot_offsets", None), ("shots", None), ("totals", None),
        ("stream", None))])
    assert dp() == ARG
    for bad in (dict(nvideos=0), dict(max_n=0), dict(max_n=2049), dict(lmin=0), dict(stride=0), dict(cost_cap=0),
                dict(cost_cap=1 << 31), dict(p=0), dict(jt=1 << 31)):
        assert dp(**bad) == SHAPE, bad
    # a short workspace is refused once the pointers are there (host memory stands in: nothing is launched)
    import ctypes
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.avs_kts_scatters_f64(ptr, ptr, 1, 2, ptr, 255, *entries, ptr, None) == WORKSPACE
    assert dp(videos=ptr, pen=ptr, ws=ptr, ws_bytes=255, flags=ptr, scores=ptr, costs=ptr, cps=ptr, shot_offsets=ptr,
              shots=ptr, totals=ptr) == WORKSPACE
