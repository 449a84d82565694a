"""Host checks of the references and of the bound test_gpu_convbn_f64.py holds the bf16 convolution + BatchNorm kernels to
(no GPU):

  * every restatement of convbn_f64_inputs lies within the bound at every case the device tests run, the moments check
    included - a correct kernel of this arithmetic can pass;
  * every planted mistake lies outside it at the case a NOTICED_BY table names - the bound is not slack enough to pass a
    wrong kernel;
  * the case list reaches all 12 instances of conv1x1_bn_kernel and all 4 of bn_gram_affine_kernel (the launchers' rules
    restated in convbn_f64_inputs), the three branches of ``live``, grids that are no multiple of 8, the K tail, partial
    column slabs, padded strides and every option on and off;
  * the float64 references equal oracle.cnn.bn_batch where that applies;
  * the entry points refuse bad shapes, strides, null pairs and misaligned pointers before launching anything."""
import pytest
import torch

import convbn_f64_inputs as cfi

ARG, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -5      # AVS_E_ARG, _SHAPE, _ALIGN, _WORKSPACE (AVS_E_UNSUPPORTED: from _abi)
LOCAL_RUNS = (("normal", False, False), ("mean40", False, False), ("const", True, True))


# --------------------------------------------------------------------------- restatements lie within the bound
@pytest.mark.parametrize("form", cfi.FORMS)
def test_conv1x1_restatement_within_the_bound(form):
    for si in range(len(cfi.CONV_SHAPES)):
        for regime in cfi.REGIMES:
            case, ref, cpu32 = cfi.conv_bundle(si, form, regime)
            assert torch.isfinite(ref).all() and torch.isfinite(cpu32).all(), case.label
            ok, (err, _, bound, _, _) = cfi.compare_groups(cpu32, ref, cpu32, case.groups, case.rpg)
            assert ok, (case.label, err, bound)
            if cfi.has_moments(case):
                assert cfi.compare_moments(cpu32, ref, cpu32, case.groups, case.rpg)[0], case.label
            # the regimes are what they say
            sc, _ = cfi.conv_stats_reference(case)
            assert (sc[:, 1] == 0).all() and (sc[:, 0] > 0).all() and (sc[:, 2] < 0).all()
            y = cfi._per_group(case.a.double() @ case.w.double().t(), case.groups, case.rpg)
            if regime == "mean40" and case.rpg > 1:
                r = y.mean(1).abs() / y.var(1, unbiased=False).sqrt()
                assert (r[:, list(cfi.MEAN40_CH)] > 15).all() and (r[:, list(cfi.MEAN40_CH)] < 120).all(), case.label
            if regime == "const":
                yc = y[case.const_group, :, cfi.CONST_CH]
                assert (yc == yc[0]).all() and yc[0] != 0, case.label
                assert sc[case.const_group, cfi.CONST_CH] == case.gamma[cfi.CONST_CH].double() / torch.sqrt(cfi.eps32().double())
            if case.xf:     # scales of both signs; one input column entirely rectified to zero
                assert (case.isc > 0).any() and (case.isc < 0).any() and (case.a[:, cfi.DEAD_COL] == 0).all()


def test_rows_per_group_1_gives_beta():
    """Variance exactly 0 in every channel: the float64 output is beta (+ residual, ReLU)."""
    case, ref, cpu32 = cfi.conv_bundle(0, "two_pass", "normal")
    assert case.rpg == 1 and case.res is None and not case.relu
    assert torch.allclose(ref, case.beta.double().expand_as(ref), rtol=0, atol=1e-12)
    assert torch.equal(cpu32[:, 1], cfi.bf(case.beta[1]).expand(case.rows))


def test_conv1x1_reference_is_the_oracles_batchnorm():
    from oracle import cnn as ocnn
    case, ref, _ = cfi.conv_bundle(2, "two_pass", "normal")
    assert case.res is None and not case.relu
    y = (case.a.double() @ case.w.double().t()).view(case.groups, case.rpg, case.n)
    for g in range(case.groups):
        want = ocnn.bn_batch(y[g].t().reshape(1, case.n, case.rpg, 1).permute(2, 1, 0, 3), case.gamma.double(),
                             case.beta.double(), cfi.BN_EPS)
        got = ref[g * case.rpg:(g + 1) * case.rpg]
        assert (want.reshape(case.rpg, case.n) - got).abs().max().item() < 1e-9


def test_gram_restatement_within_the_bound():
    for key in cfi.gram_case_keys():
        case, ref, cpu32 = cfi.gram_bundle(*key)
        for r, c in zip(ref, cpu32):
            assert torch.isfinite(c).all() and cfi.compare(c, r, c)[0], case.label
        assert (cpu32[0][:, 1] == 0).all() and (ref[0][:, 1] == 0).all()
        if case.regime == "mean40" and case.rpg > 1:
            a = cfi._per_group(case.a.double(), case.groups, case.rpg)
            ratio = a.mean(1) ** 2 / a.var(1, unbiased=False).clamp_min(1e-30)
            assert (ratio[:, 8:16] > 400).all(), case.label


@pytest.mark.parametrize("shape", cfi.LOCAL_SHAPES, ids=[str(s).replace(" ", "") for s in cfi.LOCAL_SHAPES])
def test_bnlocal_restatement_within_the_bound(shape):
    for regime, with_res, relu in LOCAL_RUNS:
        case = cfi.conv2d_case("local", shape, regime, with_res, relu)
        ref, cpu32 = cfi.local_reference(case), cfi.local_restatement(case)
        groups = case.ge.rows // case.ge.rpg
        assert cfi.compare_groups(cpu32, ref, cpu32, groups, case.ge.rpg)[0], case.label
        if not with_res and not relu:
            assert cfi.compare_moments(cpu32, ref, cpu32, groups, case.ge.rpg)[0], case.label


@pytest.mark.parametrize("shape", cfi.STATS_SHAPES, ids=[str(s).replace(" ", "") for s in cfi.STATS_SHAPES])
def test_bnstats_restatement_within_the_bound(shape):
    for regime in cfi.REGIMES:
        case = cfi.conv2d_case("stats", shape, regime)
        off = cfi.stats_groups(case.ge.rows, case.ge.rpg)
        for r0, r1 in zip(off[:-1], off[1:]):
            raw = cfi.bf(case.acc32[r0:r1])
            assert cfi.compare_groups(raw, case.acc64[r0:r1], raw, 1, r1 - r0)[0], case.label
        ref = cfi.ragged_stats(case.acc64, off, case.gamma, case.beta, torch.float64)
        cpu32 = cfi.ragged_stats(case.acc32, off, case.gamma, case.beta, torch.float32)
        for r, c in zip(ref, cpu32):
            assert cfi.compare(c, r, c)[0], case.label


@pytest.mark.parametrize("n,fpg", cfi.STEM_CASES)
def test_stem_restatement_within_the_bound(n, fpg):
    case, acc64, _, ref, cpu32 = cfi.stem_bundle(n, fpg)
    for r, c in zip(ref, cpu32):
        assert all(cfi.compare(c[g], r[g], c[g])[0] for g in range(case.groups)), case.label
    assert (cpu32[0][:, 1] == 0).all() and (case.gamma < 0).any() and (case.gamma > 0).any()
    inner = acc64[cfi.CONST_FRAME, :, 2:-2, 2:-2]         # a single colour: constant away from the borders
    assert (inner.amax((1, 2)) - inner.amin((1, 2))).max().item() < 1e-9
    for apply in (0, 1):
        for relu in (0, 1):
            y, r = cfi.stem_restatement(n, fpg, apply, relu), cfi.stem_reference(n, fpg, apply, relu)
            assert cfi.compare_groups(y, r, y, case.groups, fpg * 56 * 56)[0], (case.label, apply, relu)


def test_normalize_table():
    """bf16((v / denom - mean) / std) against float64, for denom 1 and 255: half a bf16 step."""
    for denom in (1.0, 255.0):
        lut = cfi.normalize_lut(denom)
        v = torch.arange(256, dtype=torch.float64)
        for c in range(3):
            ref = (v / denom - cfi.STEM_MEAN[c]) / cfi.STEM_STD[c]
            assert ((lut[c].double() - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-30).all()
    f = cfi.all_bytes_frame()
    assert all(sorted(f[0, :, :, c].reshape(-1).tolist()) == list(range(256)) for c in range(3))


# --------------------------------------------------------------------------- planted mistakes lie outside it
@pytest.mark.parametrize("mistake", cfi.CONV_MISTAKES)
def test_conv1x1_mistakes_are_noticed(mistake):
    key, check = cfi.NOTICED_BY[mistake]
    assert key in cfi.conv_case_keys()
    case, ref, cpu32 = cfi.conv_bundle(*key)
    wrong = cfi.conv_restatement(case, mistake)[0]
    if check == "moments":
        assert cfi.has_moments(case)
        ok, err, _, bound, _ = cfi.compare_moments(wrong, ref, cpu32, case.groups, case.rpg)
    else:
        ok, (err, _, bound, _, _) = cfi.compare_groups(wrong, ref, cpu32, case.groups, case.rpg)
    assert not ok, (case.label, mistake, err, bound)


def test_unbiased_variance_is_noticed_at_49_row_groups():
    """By the moments check alone, at every 49-row case of the tile-local form that runs it."""
    shape, regime = cfi.NOTICED_BY_LOCAL["unbiased"]
    assert shape in cfi.LOCAL_SHAPES and cfi.conv2d_geometry(shape).rpg == 49 and (regime, False, False) in LOCAL_RUNS
    seen = 0
    for shape in cfi.LOCAL_SHAPES:
        if cfi.conv2d_geometry(shape).rpg != 49:
            continue
        for regime, with_res, relu in LOCAL_RUNS:
            if with_res or relu:
                continue
            case = cfi.conv2d_case("local", shape, regime, False, False)
            ref, cpu32 = cfi.local_reference(case), cfi.local_restatement(case)
            ok, err, _, bound, _ = cfi.compare_moments(cfi.local_restatement(case, "unbiased"), ref, cpu32, case.ge.rows // 49, 49)
            assert not ok, (case.label, err, bound)
            seen += 1
    assert seen == 6


STAT_MISTAKES = ("unbiased", "drop_last_row", "first_row_of_next_group")


def test_the_moments_check_alone_notices_statistics_mistakes_at_every_group_size():
    """unbiased (1 / (2 R) of the spread), a group's last row left out and the next group's first row taken in (1 / R of
    it), by compare_moments alone: at every conv1x1 case that runs it with more than one row per group - the 161-, 196-
    and 257-row groups included - and at every tile-local case that runs it (49, 64, 100 and 196 rows)."""
    sizes = set()
    for key in cfi.conv_case_keys():
        case, ref, cpu32 = cfi.conv_bundle(*key)
        if not cfi.has_moments(case) or case.rpg == 1:
            continue
        sizes.add(case.rpg)
        for mistake in STAT_MISTAKES:
            ok, err, _, bound, _ = cfi.compare_moments(cfi.conv_restatement(case, mistake)[0], ref, cpu32, case.groups, case.rpg)
            assert not ok, (case.label, mistake, err, bound)
    assert sizes == {33, 130, 161, 196, 257}
    sizes = set()
    for shape in cfi.LOCAL_SHAPES:
        for regime, with_res, relu in LOCAL_RUNS:
            if with_res or relu:
                continue
            case = cfi.conv2d_case("local", shape, regime, False, False)
            ref, cpu32 = cfi.local_reference(case), cfi.local_restatement(case)
            sizes.add(case.ge.rpg)
            for mistake in STAT_MISTAKES:
                ok, err, _, bound, _ = cfi.compare_moments(cfi.local_restatement(case, mistake), ref, cpu32,
                                                           case.ge.rows // case.ge.rpg, case.ge.rpg)
                assert not ok, (case.label, mistake, err, bound)
    assert sizes == {49, 64, 100, 196}


def test_moments_floor_is_below_the_mistakes_and_above_a_few_flipped_roundings():
    """The floor against the sizes it is derived from: below the unbiased variance's 1 / (2 R) of a spread that is a third
    of the magnitude, at least two outputs of a bf16 step rounding the other way, at every group size of the cases."""
    for r in (33, 49, 64, 100, 130, 161, 196, 257):
        assert 2 * 2.0 ** -7 / r <= cfi.moments_floor(r) < 1.0 / (2 * r) / 3


@pytest.mark.parametrize("mistake", cfi.AFFINE_MISTAKES)
def test_the_affine_comparison_notices_statistics_mistakes(mistake):
    """The comparison of returned (scale, shift) - the whole tensor for the Gram kernel and bnstats, per group for the stem -
    rejects the unbiased variance and a group's last row left out: at every Gram case with more than one row per group,
    at every bnstats case (mean40 and const included), and in every stem group but the single-colour frame's own, whose
    variance is all cancellation (it still rejects the missing row there)."""
    def rejected(wrong, ref, cpu32):
        return any(not cfi.compare(w, r, c)[0] for w, r, c in zip(wrong, ref, cpu32))

    for key in cfi.gram_case_keys():
        case, ref, cpu32 = cfi.gram_bundle(*key)
        if case.rpg > 1:
            assert rejected(cfi.gram_restatement(case, mistake), ref, cpu32), (case.label, mistake)
    for shape in cfi.STATS_SHAPES:
        for regime in cfi.REGIMES:
            case = cfi.conv2d_case("stats", shape, regime)
            off = cfi.stats_groups(case.ge.rows, case.ge.rpg)
            ref = cfi.ragged_stats(case.acc64, off, case.gamma, case.beta, torch.float64)
            cpu32 = cfi.ragged_stats(case.acc32, off, case.gamma, case.beta, torch.float32)
            wrong = cfi.ragged_stats(case.acc32, off, case.gamma, case.beta, torch.float32, mistake)
            assert rejected(wrong, ref, cpu32), (case.label, mistake)
    for n, fpg in cfi.STEM_CASES:
        case, _, acc32, ref, cpu32 = cfi.stem_bundle(n, fpg)
        wrong = cfi.stem_fold(acc32, fpg, case.gamma, case.beta, mistake=mistake)
        for g in range(case.groups):
            single_colour = fpg == 1 and g == cfi.CONST_FRAME
            if single_colour and mistake == "unbiased":
                continue
            assert rejected([w[g] for w in wrong], [r[g] for r in ref], [c[g] for c in cpu32]), (case.label, g, mistake)


@pytest.mark.parametrize("mistake", cfi.STEM_MISTAKES)
def test_stem_mistakes_are_noticed(mistake):
    (n, fpg), apply, relu = cfi.NOTICED_BY_STEM[mistake]
    assert (n, fpg) in cfi.STEM_CASES
    ref, cpu32 = cfi.stem_reference(n, fpg, apply, relu), cfi.stem_restatement(n, fpg, apply, relu)
    wrong = cfi.stem_restatement(n, fpg, apply, relu, mistake)
    ok, (err, _, bound, _, _) = cfi.compare_groups(wrong, ref, cpu32, n // fpg, fpg * 56 * 56)
    assert not ok, (mistake, err, bound)


def test_the_old_bar_would_not_notice_them():
    """What the 3 % bar of test_gpu_models.py lets through: the unbiased variance at 33-row groups and statistics of the
    rounded output."""
    for mistake in ("unbiased", "stats_of_rounded_output"):
        case, ref, _ = cfi.conv_bundle(*cfi.NOTICED_BY[mistake][0])
        wrong = cfi.conv_restatement(case, mistake)[0]
        scale = max(1.0, ref.abs().max().item())
        assert (wrong.double() - ref).abs().max().item() < 3e-2 * scale


# --------------------------------------------------------------------------- the cases reach every instance and path
def test_cases_reach_every_instance_and_path():
    cases = [cfi.conv_case(*k) for k in cfi.conv_case_keys()]
    inst = {cfi.kernel_instance(c.n, c.xf, c.form) for c in cases}
    assert inst == {(bn, xf, pre, ra) for bn in (64, 128) for xf in (False, True)
                    for pre, ra in ((False, False), (True, False), (True, True))} and len(inst) == 12
    live = set().union(*(cfi.live_branches(c.rpg, c.form) for c in cases))
    assert live == {"le0", "1_32", "33_64"}
    assert cfi.live_branches(161, "affine") == {"33_64", "le0"} and cfi.live_branches(130, "affine") >= {"1_32", "le0"}
    assert cfi.live_branches(257, "affine_ra") >= {"1_32", "le0"} and cfi.live_branches(33, "two_pass") == set()
    # every option on and off, in every form it exists in; every (shape, form) with and without an input affine
    for form in cfi.FORMS:
        fc = [c for c in cases if c.form == form]
        assert {c.xf for c in fc} == {False, True} and {c.padded for c in fc} == {False, True}
        assert {c.relu for c in fc} == {False, True}
        assert {c.res is not None for c in fc} == ({True} if form == "affine_ra" else {False, True})
        for si in range(len(cfi.CONV_SHAPES)):
            assert {c.xf for c in fc if c.si == si} == {False, True}
    assert any(cfi.has_moments(c) for c in cases if c.regime == "mean40")
    # the K tail, partial slabs, groups below a tile, grids that are no multiple of 8, k at the input affine's limit
    shapes = cfi.CONV_SHAPES
    assert any(k % 32 for _, k, _, _ in shapes) and any(n % 128 and n > 64 for _, _, n, _ in shapes)
    assert any(n > 128 and n % 128 for _, _, n, _ in shapes) and any(r < 128 for r, _, _, _ in shapes)
    assert any(k == cfi.MAX_K and c.xf for c in cases for k in [c.k])
    for r, k, n, g in shapes:
        nwg = g * -(-n // (64 if n <= 64 else 128))
        assert sorted(cfi.remapped_workgroups(nwg)) == list(range(nwg))       # the remap is a permutation
    assert any((g * -(-n // (64 if n <= 64 else 128))) % 8 for _, _, n, g in shapes)
    assert cfi.remapped_workgroups(9) == [0, 2, 3, 4, 5, 6, 7, 8, 1]
    # padded operands differ from the dense ones and stay 16-byte aligned
    for c in cases:
        if c.padded:
            assert (c.lin_stride, c.ldc, c.ldr, c.off_y) == (c.k + 8, c.n + 16, c.n + 8, 8)
        assert c.lin_stride % 8 == 0 and c.ldc % 8 == 0 and c.ldr % 8 == 0 and c.off_y % 8 == 0
    # the Gram kernel: both k, with and without an input affine; every n, group size, group count, regime and store mode
    keys = cfi.gram_case_keys()
    assert {(k, xf) for k, _, _, _, _, xf, _ in keys} == {(64, False), (64, True), (128, False), (128, True)}
    for k in cfi.GRAM_K:
        kk = [key for key in keys if key[0] == k]
        assert {key[1] for key in kk} == set(cfi.GRAM_N) and {key[2] for key in kk} == set(cfi.GRAM_RPG)
        assert {key[3] for key in kk} == set(cfi.GRAM_GROUPS) and {key[4] for key in kk} == set(cfi.GRAM_REGIMES)
        assert {key[6] for key in kk} == set(cfi.GRAM_STORES)
    # the tile-local groups: 49, 64, 100 and 196 rows, a last tile with fewer groups; statistics groups of >= 64 rows that
    # straddle the row tiles, with a shorter last group
    geo = [cfi.conv2d_geometry(s) for s in cfi.LOCAL_SHAPES]
    assert {g.rpg for g in geo} == {49, 64, 100, 196}
    assert any((g.rows // g.rpg) % (256 // g.rpg) for g in geo)
    assert {g.k for g in geo} == {1, 3} and {g.s for g in geo} == {1, 2}
    sgeo = [cfi.conv2d_geometry(s) for s in cfi.STATS_SHAPES]
    assert all(g.rpg >= 64 for g in sgeo) and any(g.rows % g.rpg for g in sgeo) and any(g.rpg % 128 for g in sgeo)
    assert any(g.cin == 72 for g in sgeo) and any(g.cout == 136 for g in sgeo) and any(g.rpg == 64 for g in sgeo)


def test_shapes_are_taken_by_the_forms():
    """The host-only queries: every tile-local shape is taken with tiles of floor(256 / rows) groups, every statistics shape
    by avs_conv2d_nhwc_bnstats."""
    from avsum_amd import ops
    code = ops.dtype_code(torch.bfloat16)
    for s in cfi.LOCAL_SHAPES:
        g = cfi.conv2d_geometry(s)
        assert ops.conv_bnlocal_tile_rows(code, *g.geom, *g.xs, g.k * g.k * g.cin, g.cout, g.rpg) == 256 // g.rpg * g.rpg, s
    for s in cfi.STATS_SHAPES:
        g = cfi.conv2d_geometry(s)
        assert ops.conv_bnstats_ok(code, *g.geom, *g.xs, g.k * g.k * g.cin, g.cout, g.rpg), s


# --------------------------------------------------------------------------- refusals: nothing is launched
A = 1 << 20         # a 256-byte aligned non-null address; never read: every call below returns before any HIP call


def _lib():
    from avsum_amd import _abi
    return _abi.lib(), _abi.E_UNSUPPORTED


def test_conv1x1_refusals():
    lib, unsupported = _lib()

    def bn(x=A, ls=64, k=64, w=A, ldb=64, n=64, rpg=8, groups=2, ga=A, be=A, res=None, ldr=0, relu=1, y=A, ldc=64):
        return lib.avs_conv1x1_bn_bf16(x, ls, k, w, ldb, n, rpg, groups, ga, be, 1e-5, res, ldr, relu, y, ldc, None)

    def bn_in(isc=A, ish=A, k=64, ls=None, ldb=None):
        return lib.avs_conv1x1_bn_in_bf16(A, ls or k, k, isc, ish, A, ldb or k, 64, 8, 2, A, A, 1e-5, None, 0, 1, A, 64, None)

    def aff(isc=None, ish=None, sc=A, sh=A, res=None, ldr=0, rsc=None, rsh=None, k=64, n=64, y=A, ldc=64, ls=None):
        return lib.avs_conv1x1_affine_bf16(A, ls or k, k, isc, ish, A, k, n, 8, 2, sc, sh, res, ldr, rsc, rsh, 1, y, ldc, None)

    assert bn(k=0) == SHAPE and bn(n=0) == SHAPE and bn(rpg=0) == SHAPE and bn(groups=-1) == SHAPE
    assert bn(groups=0, x=None, w=None, y=None) == 0
    assert bn(x=None) == ARG and bn(w=None) == ARG and bn(y=None) == ARG and bn(ga=None) == ARG and bn(be=None) == ARG
    assert bn(k=60, ls=60, ldb=60) == SHAPE and bn(n=60, ldc=64) == SHAPE and bn(ls=68) == SHAPE and bn(ldb=56) == SHAPE
    assert bn(ls=56) == SHAPE and bn_in(k=64, ls=56) == SHAPE and aff(ls=56) == SHAPE          # lin_stride < k
    assert bn(ldc=56) == SHAPE and bn(ldc=68) == SHAPE and bn(res=A, ldr=56) == SHAPE and bn(res=A, ldr=68) == SHAPE
    for kw in (dict(x=A + 8), dict(w=A + 8), dict(y=A + 8), dict(res=A + 8, ldr=64)):
        assert bn(**kw) == ALIGN, kw
    assert bn_in(isc=None) == ARG and bn_in(ish=None) == ARG
    assert bn_in(k=cfi.MAX_K + 8) == unsupported                                  # k = 520 with an input affine
    assert bn_in(isc=A + 8) == ALIGN and bn_in(ish=A + 4) == ALIGN
    assert aff(sc=None) == ARG and aff(sh=None) == ARG
    assert aff(res=A, ldr=64, rsc=A, rsh=None) == ARG and aff(res=A, ldr=64, rsc=None, rsh=A) == ARG     # a null pair
    assert aff(rsc=A, rsh=A) == ARG                                               # a residual affine without a residual
    assert aff(res=A, ldr=64, rsc=A + 8, rsh=A) == ALIGN and aff(res=A, ldr=64, rsc=A, rsh=A + 4) == ALIGN
    assert aff(isc=A, ish=None) == ARG and aff(isc=A, ish=A, k=cfi.MAX_K + 8) == unsupported
    assert aff(y=A + 8) == ALIGN and aff(n=60) == SHAPE


def test_gram_refusals():
    lib, unsupported = _lib()

    def gram(x=A, ls=64, k=64, isc=None, ish=None, w=A, ldb=64, n=64, rpg=8, groups=2, ga=A, be=A, sc=A, sh=A, a_out=None, lda=0):
        return lib.avs_bn_gram_affine_bf16(x, ls, k, isc, ish, w, ldb, n, rpg, groups, ga, be, 1e-5, sc, sh, a_out, lda, None)

    assert gram(k=72, ls=72, ldb=72) == unsupported and gram(n=40) == unsupported and gram(n=0) == unsupported
    assert gram(rpg=0) == SHAPE and gram(groups=-1) == SHAPE and gram(groups=0, x=None) == 0
    assert gram(x=None) == ARG and gram(ga=None) == ARG and gram(sc=None) == ARG and gram(sh=None) == ARG
    assert gram(isc=A) == ARG and gram(ish=A) == ARG                              # a null pair
    assert gram(ls=56) == SHAPE and gram(ls=68) == SHAPE and gram(ldb=56) == SHAPE
    assert gram(x=A + 8) == ALIGN and gram(w=A + 8) == ALIGN
    assert gram(a_out=A + 4096, lda=64) == ARG                                    # d_a_out without an input affine
    assert gram(isc=A, ish=A, a_out=A, lda=72, ls=64) == ARG                      # in place with lda != lin_stride
    assert gram(isc=A, ish=A, a_out=A + 4096, lda=56) == ALIGN and gram(isc=A, ish=A, a_out=A + 4104, lda=64) == ALIGN


def test_stem_refusals():
    import ctypes
    lib, unsupported = _lib()
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def stem(fr=A, n=2, denom=1.0, mean=m3, std=m3, w=A, ldw=224, fpg=1, ga=A, be=A, y=A, sc=A, sh=A, ws=A, wsb=1 << 30):
        return lib.avs_stem_conv_bn_pool_bf16(fr, n, denom, mean, std, w, ldw, fpg, ga, be, 1e-5, 1, 1, y, sc, sh, ws, wsb, None)

    assert stem(n=-1) == SHAPE and stem(fpg=0) == SHAPE and stem(n=0, fr=None) == 0
    assert stem(n=3, fpg=2) == unsupported
    assert stem(fr=None) == ARG and stem(ga=None) == ARG and stem(ws=None) == ARG and stem(denom=0.0) == ARG
    assert stem(ldw=216) == SHAPE and stem(ldw=228) == SHAPE
    assert stem(w=A + 8) == ALIGN and stem(y=A + 8) == ALIGN and stem(sc=A + 8) == ALIGN
    assert stem(wsb=16) == WORKSPACE and stem(n=2, wsb=2 * 49 * 2 * 64 * 4 - 1) == WORKSPACE
