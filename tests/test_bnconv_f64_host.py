"""The case table of the float64 tests of the BatchNorm convolution entry points (avs_conv2d_nhwc_bnstats, _bnstats_xin,
_bnlocal, _affine), checked on the host (no GPU): the restated plan pinned LIVE on the library's two host queries, the
instances the cases reach against REACHABLE, the thresholds read from the source, the float64 reference against the plain
tests' loop over taps, every restatement inside and every planted mistake outside the bounds, the measured constants,
the tall family's map from device rows to the distinct groups, and the entry points' refusals with pointers that are
never dereferenced (bnconv_f64_inputs; the device side is test_gpu_bnconv_f64.py)."""
import ctypes
import re

import pytest
import torch

import bnconv_f64_inputs as bfi
import conv_f64_inputs as cfi
import convbn_f64_inputs as cbi
import gemm_f64_inputs as gfi

F16X2, F32, SPLIT = bfi.F16X2, bfi.F32, bfi.SPLIT
# the forms a mistake can be made in: the input affine rides in the statistics form only, the residual's affine and the
# AVS_F16P8 residual in the given-affine form (an AVS_F16P8 input: the statistics form), Chan's merge and the short last
# group in the statistics form
ONE_FORM = {"in_affine_on_padding", "in_relu_ignored", "in_affine_of_group0", "res_affine_of_group0", "chan_equal_counts",
            "short_last_group_divides_by_rpg", "no_eps"}


def _lib():
    from avsum_amd import _abi
    return _abi.lib(), _abi


def _desc(abi, case):
    c = case.conv
    ho, wo = cfi.extent(c)
    x_img, x_row, x_px, _ = cfi.strides(c)
    formats = (abi.X_F16P8 if case.x_p8 else 0) | (abi.Y_F16P8 if case.y_p8 else 0) | (abi.RES_F16P8 if case.res == "p8" else 0)
    return abi.ConvDesc(c.dtype, c.n, c.h, c.w, c.cin, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, ho, wo, c.cout, x_img, x_row, x_px,
                        c.kh * c.kw * c.cin, c.cout + c.ypad, bfi.RELU if case.relu else 0, 1.0, c.w_layout, c.variant, formats)


# --------------------------------------------------------------------------- the plan
def test_the_cases_reach_every_instance_the_batchnorm_forms_can():
    reached = {bfi.instance(c) for c in bfi.CASES}
    want = bfi.REACHABLE - set(bfi.LEFT_OUT)
    assert reached == want, (sorted(want - reached, key=repr), sorted(reached - want, key=repr))
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in bfi.LEFT_OUT.values())
    assert len(bfi.REACHABLE) == 180 and len(bfi.LEFT_OUT) == 0
    for f, values in enumerate(bfi.FIELDS):         # every field's every value is reached
        assert {t[f] for t in reached} == set(values), bfi.FIELD_NAMES[f]
    by = lambda **kw: {t for t in reached if all(t[bfi.FIELD_NAMES.index(k)] == v for k, v in kw.items())}
    assert {t[0] for t in by(epi="stats")} == {F32, SPLIT, F16X2} and {t[0] for t in by(epi="bnlocal") | by(epi="affine")} == {F16X2}
    assert {t[1] for t in by(epi="stats", tap9=True, xin=True)} == {64, 128} == {t[1] for t in by(epi="stats", tap9=True, xin=False)}
    assert {t[6] for t in by(ap8=True)} == {2, 4} and {t[6] for t in by(groupw=True)} == {2, 4} and by(epi="bnlocal", tap9=True)
    assert {t[13] for t in by(epi="bnlocal")} == {None, "spatial", "point"}
    # both branches of p.xin_table: groups of at least 384 rows with cin <= 128, smaller groups, cin = 144
    xin = [(bfi.case_plan(c).xin_table, c.rpg, c.conv.cin) for c in bfi.CASES if c.xin is not None]
    assert {t for t, _, _ in xin} == {True, False}
    assert [1 for t, rpg, cin in xin if not t and rpg < 384] and [1 for t, rpg, cin in xin if not t and rpg >= 384 and cin == 144]
    assert {c.xin for c in bfi.CASES} == {None, 0, 1}


def test_the_workspace_query_answers_as_the_restated_plan():
    """avs_conv2d_bnstats_workspace_bytes == ceil256(tiles_m * stat_slots * 2 * cout * 4) with the restated tile_rows, for
    every statistics case: this pins the 128 / 256 / by-rule tile choice under `stats` (and the AVS_F16P8 requirements)."""
    lib, abi = _lib()
    rows = set()
    for case in (c for c in bfi.CASES if c.form == "stats"):
        p = bfi.case_plan(case)
        want = (p.tiles_m * ((p.tile_rows + case.rpg - 2) // case.rpg + 1) * 2 * case.conv.cout * 4 + 255) // 256 * 256
        assert want == p.ws_bytes
        got = lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(_desc(abi, case)), case.rpg)
        assert got == want, (case.name, got, want, lib.avs_last_error())
        rows.add((case.conv.dtype, p.tile_rows, case.conv.variant & 3))
    assert rows >= {(F16X2, 256, 0), (F16X2, 128, 0), (F16X2, 256, 2), (F16X2, 128, 1), (SPLIT, 256, 2), (SPLIT, 128, 0), (F32, 128, 2)}


def test_the_tile_rows_query_answers_as_the_restated_plan():
    """avs_conv2d_bnlocal_tile_rows == 256 // rpg * rpg, or the refusal, for every tile-local case and for every group size
    of 30 .. 259 rows at one 1x1 shape; the smallest group it takes is the one the case table starts from."""
    lib, abi = _lib()
    for case in (c for c in bfi.CASES if c.form == "bnlocal"):
        p = bfi.case_plan(case)
        assert p.tile_rows == 256 // case.rpg * case.rpg
        assert lib.avs_conv2d_bnlocal_tile_rows(ctypes.byref(_desc(abi, case)), case.rpg) == p.tile_rows, case.name
    taken = []
    for rpg in range(30, 260):
        d = abi.ConvDesc(*bfi.desc_fields(dtype=F16X2, n=12 * rpg, h=1, w=1, cin=48, kh=1, kw=1, ph=0, pw=0, cout=64))
        want = bfi.bnlocal_tile_rows(F16X2, 12 * rpg, 64, 48, rpg, 64)
        got = lib.avs_conv2d_bnlocal_tile_rows(ctypes.byref(d), rpg)
        assert got == (bfi.E_UNSUPPORTED if want is None else want), (rpg, got, want)
        if got > 0:
            taken.append(rpg)
    # six groups of 37 .. 42 rows fill 222 .. 252 of a tile's 256 rows (BNLOCAL_MAX_GROUPS = 6, 3/4 of the tile = 192 rows)
    assert taken[0] == bfi.BNLOCAL_MIN_RPG == 37 and taken[-1] == 256
    assert taken == [r for r in range(37, 257) if 256 // r * r >= 192]
    assert any(c.rpg == taken[0] for c in bfi.CASES if c.form == "bnlocal")


def _edges(rules):
    """One shape either side of each threshold this module adds to the rules."""
    g = lambda cin, cout=128, n=6: (n, 16, 4, cin, 1, 1, 1, 1, 0, 0, cout)
    pl = lambda *a, **kw: bfi.plan(*a, rules=rules, **kw)
    return (pl(F16X2, g(128), "affine", 64).wr, pl(F16X2, g(136), "affine", 64).wr,                    # AVS_RULE_AFFINE_128_MAX_K
            pl(F16X2, g(48), "stats", 63).refusal is None, pl(F16X2, g(48), "stats", 64).refusal is None,   # STATS_MIN_GROUP_ROWS
            bfi.bnlocal_tile_rows(F16X2, 6 * 36, 64, 48, 36, 64, rules), bfi.bnlocal_tile_rows(F16X2, 6 * 37, 64, 48, 37, 64, rules),
            [bfi.case_plan(c, rules).xin_table for c in bfi.CASES if c.xin is not None])                # the two XIN_TABLE constants


def test_the_thresholds_are_read_from_the_source(tmp_path):
    assert _edges(None)[:6] == (2, 4, False, True, None, 222)
    src, hdr = open(gfi._source()).read(), open(bfi._params_source()).read()
    for name, where, pattern, factor in (("affine_128_max_k", "src", r"(AVS_RULE_AFFINE_128_MAX_K = )\d+", 2),
                                         ("stats_min_group_rows", "hdr", r"(STATS_MIN_GROUP_ROWS = )\d+", 0.5),
                                         ("bnlocal_max_groups", "hdr", r"(BNLOCAL_MAX_GROUPS = )\d+", 2),
                                         ("xin_table_min_group_rows", "hdr", r"(XIN_TABLE_MIN_GROUP_ROWS = )\d+", 2),
                                         ("xin_table_max_cin", "hdr", r"(XIN_TABLE_MAX_CIN = )\d+", 2)):
        value = int(bfi.RULES[name] * factor)
        edited = tmp_path / f"{name}.txt"
        text, n = re.subn(pattern, lambda m: m.group(1) + str(value), src if where == "src" else hdr)
        assert n == 1, name
        edited.write_text(text)
        rules = bfi.read_rules(**({"path": str(edited)} if where == "src" else {"params_path": str(edited)}))
        assert rules[name] == value and rules["tall_min_tiles"] == bfi.RULES["tall_min_tiles"]
        assert _edges(rules) != _edges(None), name


def test_the_table_has_the_issues_families():
    by = lambda **kw: [c for c in bfi.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    rows = bfi.rows_of
    for dtype in bfi.DTYPES:
        st = [c for c in by(form="stats") if c.conv.dtype == dtype and not c.conv.period]
        assert {c.rpg for c in st} >= {64, 65, 100, 196, 200, 300, 600}
        assert {rows(c) for c in st} >= {127, 128, 129, 255, 256, 257} and {c.conv.cout for c in st} >= {8, 64, 72, 128, 136}
        assert {c.conv.variant & 3 for c in st} == {0, 1, 2} and {c.regime for c in st} == set(bfi.REGIMES)
        assert [c for c in st if c.conv.ypad and c.conv.yc0] and [c for c in st if rows(c) % c.rpg] and [c for c in st if rows(c) % 256]
        spans = [len(bfi._tiles_of_group(r0, r1, bfi.case_plan(c).tile_rows)) for c in st
                 for r0, r1 in zip(bfi.offsets_of(c)[:-1], bfi.offsets_of(c)[1:])]
        assert max(spans) >= 3                                          # Chan's merge runs more than once
    tall = [c for c in bfi.CASES if c.conv.period]
    assert len(tall) == 8 and {c.xin for c in tall} == {None, 0, 1} and {c.conv.cin for c in tall} == {16, 32, 144}
    for c in tall:
        p, lay = bfi.case_plan(c), bfi.layout(c)
        assert p.tap9 and p.wr == 4 and c.conv.variant == 0 and c.conv.period == cfi.TALL_PERIOD and c.conv.w <= 63
        assert p.tiles_m * p.tiles_n >= bfi.RULES["tall_min_tiles"] > (p.tiles_m - 40) * p.tiles_n
        assert len(lay.keys) == cfi.TALL_PERIOD * (bfi.AFF_PERIOD if c.xin is not None else 1) or c.xin is None
        assert lay.groups <= cfi.TALL_PERIOD * bfi.AFF_PERIOD + 1 and lay.rows % c.rpg != 0
    loc = by(form="bnlocal")
    assert {c.rpg for c in loc} >= {37, 42, 43, 49, 64, 85, 100, 128, 192, 196, 224, 225, 256}
    assert {bfi.case_plan(c).local224 for c in loc if c.rpg in (196, 224)} == {None, "spatial", "point"}
    assert {(c.conv.kh, c.conv.sh) for c in loc} == {(3, 1), (3, 2), (1, 1), (1, 2)} and {c.relu for c in loc} == {False, True}
    assert [c for c in loc if c.res and c.res_pad] and [c for c in loc if bfi.has_moments(c)]
    for c in loc:                                                       # a last tile with fewer groups than the first
        per_tile = 256 // c.rpg
        assert per_tile == 1 or (rows(c) // c.rpg) % per_tile != 0, c.name
    aff = by(form="affine")
    assert {c.rpg for c in aff} >= {32, 33, 64, 100, 192, 600} and {c.conv.cin for c in aff} >= {40, 48, 136}
    assert {c.res for c in aff} == {None, "h2", "p8"} and {c.y_p8 for c in aff} == {False, True} and {c.relu for c in aff} == {False, True}
    assert {c.res_affine for c in aff if c.res} == {False, True} and {c.conv.sh for c in aff} == {1, 2}
    gw = [c for c in aff if bfi.case_plan(c).groupw]
    assert [c for c in gw if rows(c) % 64] and [c for c in gw if rows(c) % c.rpg]
    assert {(c.conv.cin * 1 <= bfi.RULES["affine_128_max_k"], c.conv.variant & 3) for c in aff} == {(a, v) for a in (False, True) for v in (0, 1, 2)}
    for c in aff:                                                       # scale of both signs, with an exact zero
        sc = bfi.reference(c).given[0]
        assert bool((sc > 0).any()) and bool((sc < 0).any()) and bool((sc[:, 1] == 0).all())


# --------------------------------------------------------------------------- reference, restatements, mistakes
def test_the_reference_is_the_plain_tests_loop_over_taps():
    plain = [c for c in cfi.CASES if c.epi == "plain" and c.n > 0 and not c.period and not c.split and
             (c.crop or c.xwide > c.cin or c.sh != c.sw or c.ph != c.pw or c.kh != c.kw)]
    assert len(plain) >= 8 and {c.dtype for c in plain} >= {F32, SPLIT, F16X2}
    for case in plain[::max(1, len(plain) // 8)]:
        o = cfi.operands(case, "a")
        mine = bfi.tap_conv(case, o.x.double(), o.wv.double())
        assert bool(((mine - cfi.explicit_reference(case, "a")).abs() <= 2.0 ** -45 * cfi.magnitude(case, "a")).all()), case.name


def test_the_regimes_are_what_they_say():
    for case in bfi.CASES:
        ref, o = bfi.reference(case), bfi.operands(case)
        if case.form == "affine":
            continue
        assert bool((ref.scale[:, 1] == 0).all()) and bool((ref.scale[:, 0] > 0).all()) and bool((ref.scale[:, 2] < 0).all())
        off = bfi.offsets_of(case)
        g = o.const_group
        blk = ref.acc[off[g]:off[g + 1]]
        if case.regime == "const":          # variance exactly 0: the output is beta
            assert bool((blk[:, cbi.CONST_CH] == blk[0, cbi.CONST_CH]).all()), case.name
            assert ref.shift[g, cbi.CONST_CH].item() == pytest.approx(0.75 - blk[0, cbi.CONST_CH].item() * ref.scale[g, cbi.CONST_CH].item())
            if case.form == "bnlocal" and case.res is None:
                assert bool(((ref.y[off[g]:off[g + 1], cbi.CONST_CH] - 0.75).abs() < 1e-12).all()), case.name
        assert case.regime != "mean40" or not case.conv.period
        if case.regime == "mean40" and case.conv.cout > 5:      # |mean| / std about 40 in every group
            ch = 5
            ratios = [(ref.acc[a:b, ch].mean().abs() / ref.acc[a:b, ch].std()).item() for a, b in zip(off[:-1], off[1:])]
            assert min(ratios) > 20.0, (case.name, ratios)


def test_group_bound_is_compare_groups_bound():
    case = next(c for c in bfi.CASES if c.form == "bnlocal" and c.rpg == 64 and c.res is not None)
    b = bfi.bundle(case)
    lay = bfi.layout(case)
    mine = bfi.group_bound(b.ref.y, b.rs.y, b.offsets)
    ok, (err, e32, bound, gi, ci) = cbi.compare_groups(b.rs.y, b.ref.y, b.rs.y, lay.groups, case.rpg)
    assert ok and mine[gi * case.rpg, ci].item() == pytest.approx(bound, rel=1e-12)


@pytest.mark.parametrize("form", bfi.FORMS)
def test_restatements_lie_within_the_bounds_and_mistakes_outside(form):
    worst = {SPLIT: 0.0, F16X2: 0.0}
    for case in (c for c in bfi.CASES if c.form == form):
        b = bfi.bundle(case)
        lay = bfi.layout(case)
        assert b.ref.acc.shape == b.rs.acc.shape == (lay.rows, case.conv.cout)
        out = bfi.outside(case, b.rs)
        assert out and not any(out.values()), (case.name, out)
        if b.raw_slack is not None:
            assert bool(((b.rs.raw - b.ref.acc).abs() <= b.raw_slack).all()), case.name
            worst[case.conv.dtype] = max(worst[case.conv.dtype], bfi.restatement_ratio(case))
        hit = 0
        for mistake in bfi.MISTAKES:
            if bfi.applies(case, mistake):
                hit += 1
                assert any(bfi.outside(case, bfi.restatement(case, mistake)).values()), (case.name, mistake)
        assert hit >= (1 if form == "affine" else 4), case.name
    if form == "stats":
        print(f"restatement ratios: split {worst[SPLIT]:.4f}, f16x2 {worst[F16X2]:.4f}")
        assert 0.9 * bfi.SPLIT_RATIO_MEASURED <= worst[SPLIT] <= 1.001 * bfi.SPLIT_RATIO_MEASURED <= cfi.SPLIT_C_MEASURED
        assert 0.9 * bfi.F16X2_RATIO_MEASURED <= worst[F16X2] <= 1.001 * bfi.F16X2_RATIO_MEASURED <= cfi.F16X2_C_MEASURED


def test_every_mistake_has_cases_in_two_forms():
    for mistake in bfi.MISTAKES:
        on = [c for c in bfi.CASES if bfi.applies(c, mistake)]
        assert len(on) >= 2, mistake
        kinds = {(c.form, c.conv.dtype) for c in on}
        assert len(kinds) >= (1 if mistake in ONE_FORM else 2), (mistake, kinds)
    # the mistakes the issue names are all here
    assert set(bfi.MISTAKES) >= {"unbiased", "drop_last_row", "first_row_of_next_group", "no_eps", "wave_takes_first_rows_group",
                                 "third_group_takes_second", "chan_equal_counts", "short_last_group_divides_by_rpg",
                                 "in_affine_on_padding", "in_relu_ignored", "in_affine_of_group0", "res_affine_of_group0",
                                 "relu_before_residual", "p8_remainder_dropped", "residual_stride_ignored", "beta_without_mean"}


def test_the_tall_family_maps_device_rows_to_the_distinct_groups():
    for case in (c for c in bfi.CASES if c.conv.period):
        lay, c = bfi.layout(case), case.conv
        hrow, hgroup = bfi.device_maps(case, "cpu")
        r = torch.arange(bfi.rows_of(case))
        frames = torch.tensor(lay.frames)
        assert torch.equal(frames[hrow // 63], (r // 63) % c.period) and torch.equal(hrow % 63, r % 63)      # the same base frame
        assert torch.equal(hrow // case.rpg, hgroup[r // case.rpg])                                        # in the mapped group
        g = torch.arange(bfi.groups_of(case))
        assert torch.equal(torch.tensor(lay.aff)[hgroup], g % bfi.AFF_PERIOD)                              # the same affine row
        sizes = torch.bincount(r // case.rpg)
        host_sizes = torch.tensor(bfi.offsets_of(case)).diff()
        assert torch.equal(host_sizes[hgroup], sizes) and set(hgroup.tolist()) == set(range(lay.groups))


# --------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("label,entry,status,changes,kw", bfi.refusals(), ids=[r[0] for r in bfi.refusals()])
def test_refusals_launch_nothing(label, entry, status, changes, kw):
    """Every refusal comes before any launch, so pointers that are never dereferenced do (test_gpu_bnconv_f64.py makes the
    same calls with device buffers and looks at the destinations)."""
    lib, abi = _lib()
    d = abi.ConvDesc(*bfi.desc_fields(**changes))
    a = {name: 4096 * (i + 1) for i, name in enumerate(bfi.POINTERS[entry])}
    for name in kw.get("null", ()):
        a[name] = None
    for name in kw.get("misalign", ()):
        a[name] += 8
    rpg = kw.get("rpg", 64)
    ws = lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(d), rpg) if entry.startswith("bnstats") else 0
    args = bfi.entry_args(entry, a, rpg, ldr=kw.get("ldr", changes.get("cout", 64)), ws_bytes=max(ws, 0) - (1 if kw.get("ws_short") else 0))
    got = getattr(lib, bfi.ENTRY_POINTS[entry])(ctypes.byref(d), *args)
    assert got == status, (got, lib.avs_last_error())
    assert bfi.ENTRY_POINTS[entry].encode() in lib.avs_last_error()
