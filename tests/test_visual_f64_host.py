"""Host checks of the references and of the bound test_gpu_visual_f64.py holds the BatchNorm and pooling kernels of
csrc/visual.hip to (no GPU):

  * every fp32 restatement of visual_f64_inputs lies within the bound (or equals the reference, where the device test asks
    for equality) at every case the device tests run - a correct fp32-class kernel can pass;
  * every planted mistake lies outside it, in every instance it applies to, at the case NOTICED_BY names - the bound is not
    slack enough to pass a wrong kernel;
  * the float64 BatchNorm reference equals oracle.cnn.bn_batch, the pooling references F.max_pool2d / F.avg_pool2d;
  * the case list reaches every kernel instance the launchers can pick (their rules restated in visual_f64_inputs) and
    stays inside the documented alignment;
  * the six C entry points refuse bad shapes, strides, dtypes and misaligned pointers before launching anything."""
import pytest
import torch
import torch.nn.functional as F

import visual_f64_inputs as vfi
from oracle import cnn as ocnn

INSTANCES = vfi.INSTANCES
IDS = [vfi.iname(*i) for i in INSTANCES]
ARG, SHAPE, ALIGN = -1, -2, -3      # AVS_E_ARG, AVS_E_SHAPE, AVS_E_ALIGN


def _pool_cases(fmt, narrow):
    return [vfi.pool_case(fmt, narrow, base_c, mode, fl, ksp, hw) for base_c in vfi.pool_bases(fmt, narrow)
            for mode, fls in vfi.POOL_FLAVOURS.items() for fl in fls for ksp in vfi.POOL_KSP for hw in vfi.POOL_MAPS]


def _bmp_cases(fmt, narrow):
    base_c = vfi.pool_bases(fmt, narrow)[0]
    return [vfi.bnmaxpool_case(fmt, narrow, base_c, ksp, relu) for ksp in vfi.BMP_KSP for relu in (False, True)] + \
        [vfi.bnmaxpool_case(fmt, narrow, base_c, vfi.BMP_KSP[0], True, grouped=False)]


# --------------------------------------------------------------------------- restatements lie within the bound
@pytest.mark.parametrize("fmt", vfi.STATS_FORMATS)
def test_statistics_restatement_within_the_bound(fmt):
    for c, regime in vfi.stats_cases(fmt):
        case, ref, cpu32 = vfi.stats_bundle(fmt, c, regime)
        for name, r, y in zip(("scale", "shift"), ref, cpu32):
            ok, err, e32, bound = vfi.compare(y, r, y)
            assert ok and torch.isfinite(y).all(), (case.label, name, err, bound)
        empty = [g for g in range(7) if case.group_rows[g] == case.group_rows[g + 1]]
        assert empty == [1] and (ref[0][1] == 0).all() and (ref[1][1] == 0).all() and (cpu32[0][1] == 0).all()
        if regime == "const":       # variance exactly 0: scale = gamma / sqrt(eps), three roundings
            want = case.gamma.double() / torch.sqrt(vfi.eps32().double())
            assert torch.equal(ref[0][vfi.CONST_GROUP], want)
            assert ((cpu32[0][vfi.CONST_GROUP].double() - want).abs() <= 4 * vfi.EPS32 * want.abs()).all()
        assert ref[0][:, 1].abs().max() == 0 and (ref[0][0, 0] > 0) and (ref[0][0, 2] < 0)     # gamma: 0 and both signs


@pytest.mark.parametrize("fmt,narrow", INSTANCES, ids=IDS)
def test_apply_restatement_within_the_bound(fmt, narrow):
    for base_c in vfi.APPLY_BASE_C:
        for variant in vfi.APPLY_VARIANTS:
            case, ref, mag, cpu32 = vfi.apply_bundle(fmt, narrow, base_c, variant)
            ok, err, e32, bound = vfi.compare(cpu32, ref, cpu32, mag)
            assert ok, (case.label, err, bound)
            if fmt != "f32":
                assert e32 > 0      # the yardstick carries the format's rounding
            if variant != "nogroups":
                assert (case.gidx[-vfi.TAIL_ROWS:] == -1).all() and case.max_group_rows >= 1


@pytest.mark.parametrize("fmt,narrow", INSTANCES, ids=IDS)
def test_pool_and_bn_maxpool_restatements_within_the_bound(fmt, narrow):
    for case in _pool_cases(fmt, narrow):
        ok, err, e32, bound = vfi.pool_check(case, vfi.pool_restatement(case))
        assert ok, (case.label, err, bound)
        assert torch.isfinite(vfi.pool_eval(case, torch.float64)).all(), case.label     # every window holds an in-image tap
    for case in _bmp_cases(fmt, narrow):
        ref, mag = vfi.bnmaxpool_eval(case, torch.float64)
        y = vfi.bnmaxpool_restatement(case)
        ok, err, e32, bound = vfi.compare(y, ref, y, mag)
        assert ok and torch.isfinite(ref).all(), (case.label, err, bound)


@pytest.mark.parametrize("fmt", vfi.STATS_FORMATS)
def test_global_average_and_segment_mean_restatements(fmt):
    for n, hw, c in vfi.gap_shapes(fmt):
        case = vfi.gap_case(fmt, n, hw, c)
        y = vfi.gap_restatement(case)
        assert vfi.compare(y, vfi.gap_reference(case), y)[0], case.label
    for d, seg in vfi.SEGMENT_CASES:
        case = vfi.segment_case(d, seg)
        y = vfi.segment_mean_sequential(case.x, seg)
        ref = torch.stack([case.x[a:b].double().mean(0) if b > a else torch.zeros(d, dtype=torch.float64)
                           for a, b in zip(seg[:-1], seg[1:])])
        assert vfi.compare(y, ref, y)[0] and (y.double() - ref).abs().max().item() <= 41 * vfi.EPS32 * 4


# --------------------------------------------------------------------------- planted mistakes lie outside it
@pytest.mark.parametrize("fmt", vfi.STATS_FORMATS)
@pytest.mark.parametrize("mistake", vfi.STATS_MISTAKES)
def test_statistics_mistakes_are_noticed(fmt, mistake):
    c, regime = vfi.NOTICED_BY[mistake]
    assert (c, regime) in vfi.stats_cases(fmt)
    case, ref, cpu32 = vfi.stats_bundle(fmt, c, regime)
    wrong = vfi.stats_restatement(case.x, case.group_rows, case.gamma, case.beta, case.tr, mistake=mistake)
    noticed = [not vfi.compare(w, r, y)[0] for w, r, y in zip(wrong, ref, cpu32)]
    assert any(noticed), (case.label, mistake)


@pytest.mark.parametrize("fmt,narrow", INSTANCES, ids=IDS)
@pytest.mark.parametrize("mistake", vfi.APPLY_MISTAKES)
def test_apply_mistakes_are_noticed(fmt, narrow, mistake):
    base_c, variant = vfi.NOTICED_BY[mistake]
    assert base_c in vfi.APPLY_BASE_C and variant in vfi.APPLY_VARIANTS
    case, ref, mag, cpu32 = vfi.apply_bundle(fmt, narrow, base_c, variant)
    ok, err, e32, bound = vfi.compare(vfi.apply_restatement(case, mistake), ref, cpu32, mag)
    assert not ok, (case.label, mistake, err, bound)


@pytest.mark.parametrize("fmt,narrow", INSTANCES, ids=IDS)
@pytest.mark.parametrize("mistake", vfi.POOL_MISTAKES)
def test_pool_mistakes_are_noticed(fmt, narrow, mistake):
    mode, flavour, ksp, hw = vfi.NOTICED_BY[mistake]
    case = vfi.pool_case(fmt, narrow, vfi.pool_bases(fmt, narrow)[0], mode, flavour, ksp, hw)
    assert any(c is case for c in _pool_cases(fmt, narrow))
    ok, err, e32, bound = vfi.pool_check(case, vfi.pool_restatement(case, mistake))
    assert not ok, (case.label, mistake, err, bound)


@pytest.mark.parametrize("fmt,narrow", INSTANCES, ids=IDS)
@pytest.mark.parametrize("mistake", vfi.BNMAXPOOL_MISTAKES)
def test_bn_maxpool_mistakes_are_noticed(fmt, narrow, mistake):
    ksp, relu = vfi.NOTICED_BY[mistake]
    case = vfi.bnmaxpool_case(fmt, narrow, vfi.pool_bases(fmt, narrow)[0], ksp, relu)
    assert any(c is case for c in _bmp_cases(fmt, narrow))
    ref, mag = vfi.bnmaxpool_eval(case, torch.float64)
    ok, err, e32, bound = vfi.compare(vfi.bnmaxpool_restatement(case, mistake), ref, vfi.bnmaxpool_restatement(case), mag)
    assert not ok, (case.label, mistake, err, bound)


@pytest.mark.parametrize("fmt", vfi.STATS_FORMATS)
@pytest.mark.parametrize("mistake", vfi.GAP_MISTAKES)
def test_global_average_mistakes_are_noticed(fmt, mistake):
    n, hw, c = vfi.NOTICED_BY[mistake]
    assert (n, hw, c) in vfi.gap_shapes(fmt)
    case = vfi.gap_case(fmt, n, hw, c)
    ok, err, e32, bound = vfi.compare(vfi.gap_restatement(case, mistake), vfi.gap_reference(case), vfi.gap_restatement(case))
    assert not ok, (case.label, mistake, err, bound)


# --------------------------------------------------------------------------- the references are the oracle's / torch's
def test_batchnorm_reference_equals_the_oracle_in_float64():
    for fmt, c, regime in (("f32", 12, "normal"), ("f32", 64, "mean40"), ("bf16", 64, "const")):
        case, (scale, shift), _ = vfi.stats_bundle(fmt, c, regime)
        for g, (r0, r1) in enumerate(zip(case.group_rows[:-1], case.group_rows[1:])):
            if r1 == r0:
                continue
            xg = case.x[r0:r1].double()
            want = ocnn.bn_batch(xg.t().reshape(1, c, r1 - r0, 1), case.gamma.double(), case.beta.double(),
                                 eps=float(vfi.eps32().double()))
            got = xg * scale[g] + shift[g]
            scale_of_terms = max(1.0, (xg.abs() * scale[g].abs() + shift[g].abs()).max().item())
            assert (got - want.reshape(c, r1 - r0).t()).abs().max().item() <= 64 * 2.0 ** -53 * scale_of_terms


def test_pool_references_equal_torch_in_float64():
    compared = 0
    for case in _pool_cases("f32", None):
        if not vfi.torch_defines(case.h, case.w, case.k, case.p):
            continue            # (torch refuses a padded map smaller than the window; the kernel pools what is there)
        plain = vfi.pool_case("f32", None, case.c, case.mode, "plain" if case.flavour == "bias_relu" else case.flavour,
                              (case.k, case.s, case.p), (case.h, case.w))
        x = plain.x.double().permute(0, 3, 1, 2)
        want = F.max_pool2d(x, case.k, case.s, case.p) if case.mode == "max" else F.avg_pool2d(x, case.k, case.s, case.p)
        got = vfi.pool_eval(plain, torch.float64).permute(0, 3, 1, 2)
        assert got.shape == want.shape, plain.label
        if case.mode == "max":
            assert torch.equal(got, want), plain.label
        else:
            assert (got - want).abs().max().item() <= 32 * 2.0 ** -53 * max(1.0, x.abs().max().item()) * 4, plain.label
        compared += 1
    assert compared >= 2 * 4 * 17
    case = vfi.gap_case("f32", 3, 49, 4)
    want = F.adaptive_avg_pool2d(case.x.double().reshape(3, 7, 7, 4).permute(0, 3, 1, 2), 1).reshape(3, 4)
    assert (vfi.gap_reference(case) - want).abs().max().item() <= 64 * 2.0 ** -53 * 8


# --------------------------------------------------------------------------- every kernel instance is reached
def test_the_case_list_reaches_every_kernel_instance():
    # statistics: tc = 1 (256 row-threads), a second block in y whose last channel-threads are idle, groups on both sides
    # of tr, and ldx > c
    launches = {(fmt, c): vfi.stats_launch(fmt, c) for fmt in vfi.STATS_FORMATS for c in vfi.STATS_C[fmt]}
    assert launches[("f32", 4)] == (1, 256, 1) and launches[("f32", 8)] == (2, 128, 1) and launches[("f32", 12)] == (4, 64, 1)
    assert launches[("bf16", 64)] == (16, 16, 1) and launches[("bf16", 260)] == (64, 4, 2)
    assert launches[("f16x2", 8)] == (1, 256, 1) and launches[("f16x2", 64)] == (8, 32, 1) and launches[("f16x2", 520)] == (64, 4, 2)
    assert 260 - 64 * 4 == 4 and 520 - 64 * 8 == 8      # one live channel-thread in the second block
    for fmt in vfi.STATS_FORMATS:
        for c, regime in vfi.stats_cases(fmt):
            case = vfi.stats_case(fmt, c, regime)
            sizes = [b - a for a, b in zip(case.group_rows[:-1], case.group_rows[1:])]
            assert sizes == [1, 0, 3, 1, case.tr - 1, case.tr + 1, 777] and case.ldx > c and 3 < case.tr
            assert vfi.operand_alignment(fmt, case.ldx, 0) >= (32 if fmt == "f16x2" else 16 if fmt == "f32" else 8)

    hit = set()
    for fmt, narrow in INSTANCES:
        for base_c in vfi.APPLY_BASE_C:
            for variant in vfi.APPLY_VARIANTS:
                case = vfi.apply_case(fmt, narrow, base_c, variant)
                opers = [o for o in (case.ox, case.oy, case.ores) if o is not None]
                t, v, _ = vfi.vector_instance(fmt, case.c, opers)
                assert (t, v) == {"f32": ("float", 4), "f16x2": ("h2", 8)}.get(fmt, ("bf16", 4 if narrow else 8)), case.label
                hit.add(("apply", t, v))
                for ld, off in opers:
                    assert vfi.operand_alignment(fmt, ld, off) >= vfi.documented_alignment(fmt, narrow), case.label
                    assert ld >= off + case.c
                if variant == "res_relu":
                    assert len({case.ox[0], case.oy[0], case.ores[0]}) == 3
        cases = _pool_cases(fmt, narrow)
        assert {c.c for c in cases} == ({12, 4} if fmt == "f32" or narrow == "c" else {24})
        for pool2d, case in [(True, c) for c in cases] + [(False, c) for c in _bmp_cases(fmt, narrow)]:
            t, v, k3 = vfi.vector_instance(fmt, case.c, [case.ox, case.oy], case.k if pool2d else None)
            assert (t, v) == {"f32": ("float", 4), "f16x2": ("h2", 8)}.get(fmt, ("bf16", 4 if narrow else 8)), case.label
            hit.add(("pool2d" if pool2d else "bn_maxpool", t, v, k3))
            for ld, off in (case.ox, case.oy):
                assert vfi.operand_alignment(fmt, ld, off) >= vfi.documented_alignment(fmt, narrow), case.label
                assert ld >= off + case.c and case.ox[0] > case.c
            assert (case.ho - 1) * case.s - case.p < case.h and (case.wo - 1) * case.s - case.p < case.w
    insts = (("float", 4), ("bf16", 4), ("bf16", 8), ("h2", 8))
    assert {h[1:] for h in hit if h[0] == "apply"} == set(insts)
    assert {h[1:] for h in hit if h[0] == "bn_maxpool"} == {i + (False,) for i in insts}
    # pool2d: the K3 instances exist for <bf16, 8> and <h2, 8> only; every instance the launcher can pick is hit
    assert {h[1:] for h in hit if h[0] == "pool2d"} == {i + (False,) for i in insts} | {("bf16", 8, True), ("h2", 8, True)}
    # the narrow bf16 instance is reached each of the three ways
    c = vfi.channels("bf16", "c", 24)
    assert c % 8 and vfi.vector_instance("bf16", c, [vfi.operand("bf16", "c", c, 0)])[1] == 4
    assert vfi.operand("bf16", "stride", 24, 0)[0] % 8 == 4 and vfi.operand("bf16", "view", 24, 0)[1] * 2 % 16 == 8
    # the big apply case is one trip and a bit of the capped grid
    rows, c = vfi.APPLY_BIG
    assert 8192 * 256 < rows * c // 4 <= 8192 * 256 + 256
    # global average: a single pixel, c = 4, and more images than one block of 256 threads covers
    assert {s[0] for s in vfi.GAP_SHAPES} == {1, 3, 600} and {s[1] for s in vfi.GAP_SHAPES} == {1, 49, 64}
    assert {s[2] for s in vfi.GAP_SHAPES} == {4, 8, 2048} and any(n * c // 4 > 256 for n, _, c in vfi.GAP_SHAPES)
    assert all(n * hw * c <= 400_000 for n, hw, c in vfi.GAP_SHAPES)


def test_image_groups_is_the_kernels_binary_search():
    gr = [i * 60 for i in vfi.BMP_GROUP_IMAGES]
    want = vfi.image_groups(gr, vfi.BMP_IMAGES, 60).tolist()
    assert want == [0, 1, 3, 3, 3, 4, 5, 5, 5]          # the empty group 2 owns no image
    for img in range(vfi.BMP_IMAGES):                    # bn_maxpool_kernel's loop
        lo, hi = 0, len(gr) - 2
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            lo, hi = (mid, hi) if gr[mid] <= img * 60 else (lo, mid - 1)
        assert lo == want[img]


# --------------------------------------------------------------------------- refusals: nothing is launched
F32, BF16, H2 = 0, 1, 4
A = 1 << 20         # a 256-byte aligned non-null address; never read: every call below returns before any HIP call


def _lib():
    from avsum_amd import _abi
    assert (_abi.AVS_F32, _abi.AVS_BF16, _abi.AVS_F16X2) == (F32, BF16, H2)
    return _abi.lib()


def test_statistics_and_segment_mean_refusals():
    lib = _lib()
    st = lib.avs_bn_batch_stats
    assert st(7, A, 8, 8, 8, A, 1, A, A, 1e-5, A, A, None) == ARG                 # dtype
    assert st(F32, A, 8, 6, 8, A, 1, A, A, 1e-5, A, A, None) == SHAPE             # c % 4
    assert st(F32, A, 8, 8, 4, A, 1, A, A, 1e-5, A, A, None) == SHAPE             # ldx < c
    assert st(F32, A, 8, 8, 10, A, 1, A, A, 1e-5, A, A, None) == SHAPE            # ldx % 4
    assert st(F32, A, -1, 8, 8, A, 1, A, A, 1e-5, A, A, None) == SHAPE
    assert st(F32, A, 8, 8, 8, A, -1, A, A, 1e-5, A, A, None) == SHAPE
    assert st(F32, A, 8, 8, 8, None, 1, A, A, 1e-5, A, A, None) == ARG            # null
    assert st(F32, A + 8, 8, 8, 8, A, 1, A, A, 1e-5, A, A, None) == ALIGN
    assert st(BF16, A + 8, 8, 8, 8, A, 1, A, A, 1e-5, A, A, None) == ALIGN        # (the statistics ask 16 bytes of bf16 too)
    assert st(H2, A, 8, 12, 16, A, 1, A, A, 1e-5, A, A, None) == ALIGN            # c % 8
    assert st(H2, A, 8, 8, 12, A, 1, A, A, 1e-5, A, A, None) == ALIGN             # ldx % 8
    assert st(H2, A + 16, 8, 8, 8, A, 1, A, A, 1e-5, A, A, None) == ALIGN         # 32 bytes
    assert st(F32, None, 8, 8, 8, None, 0, None, None, 1e-5, None, None, None) == 0      # no groups: nothing to do
    sm = lib.avs_segment_mean_f32
    assert sm(A, 4, 0, A, 1, A, 4, None) == SHAPE
    assert sm(A, 3, 4, A, 1, A, 4, None) == SHAPE                                 # ldx < d
    assert sm(A, 4, 4, A, 1, A, 3, None) == SHAPE                                 # ldo < d
    assert sm(A, 4, 4, A, -1, A, 4, None) == SHAPE
    assert sm(A, 4, 4, None, 1, A, 4, None) == ARG
    assert sm(None, 4, 4, None, 0, None, 4, None) == 0


def test_apply_refusals():
    lib = _lib()

    def ap(dtype=F32, x=A, rows=8, c=8, ldx=8, gr=A, groups=1, mgr=8, sc=A, sf=A, res=None, ldr=0, act=0, y=A, ldy=8):
        return lib.avs_bn_apply(dtype, x, rows, c, ldx, gr, groups, mgr, sc, sf, res, ldr, act, y, ldy, None)

    assert ap(dtype=9) == ARG
    assert ap(c=6) == SHAPE and ap(ldx=4) == SHAPE and ap(ldy=10) == SHAPE and ap(rows=-1) == SHAPE
    assert ap(res=A, ldr=4) == SHAPE and ap(res=A, ldr=10) == SHAPE
    assert ap(gr=None, groups=1) == ARG and ap(gr=A, groups=0) == ARG
    assert ap(x=None) == ARG and ap(sc=None) == ARG and ap(y=None) == ARG
    assert ap(mgr=0) == SHAPE and ap(groups=70000) == SHAPE
    assert ap(rows=0, x=None, y=None, sc=None, sf=None) == 0
    assert ap(dtype=H2, c=12, ldx=16, ldy=16) == ALIGN and ap(dtype=H2, ldx=12, ldy=16) == ALIGN
    assert ap(dtype=H2, y=A + 16) == ALIGN and ap(dtype=H2, res=A + 16, ldr=8) == ALIGN
    # the vector accesses: 16 bytes in fp32, 8 bytes in (narrow) bf16, on x, y and the residual; 16 on scale / shift
    for kw in (dict(x=A + 8), dict(y=A + 8), dict(res=A + 8, ldr=8), dict(x=A + 4), dict(sc=A + 8), dict(sf=A + 4)):
        assert ap(**kw) == ALIGN, kw
        assert b"aligned" in lib.avs_last_error()
    for kw in (dict(x=A + 4), dict(y=A + 2), dict(res=A + 12, ldr=8), dict(sc=A + 8), dict(sf=A + 8)):
        assert ap(dtype=BF16, **kw) == ALIGN, kw


def test_pooling_refusals():
    lib = _lib()

    def pool(dtype=F32, mode=0, x=A, n=1, h=5, w=5, c=8, xps=8, k=3, s=2, p=1, bias=None, act=0, y=A, ho=3, wo=3, yps=8):
        return lib.avs_pool2d_nhwc(dtype, mode, x, n, h, w, c, xps, k, s, p, bias, act, y, ho, wo, yps, None)

    def bmp(dtype=F32, x=A, n=1, h=5, w=5, c=8, xps=8, gr=None, groups=0, sc=A, sf=A, relu=1, k=3, s=2, p=1, y=A, ho=3,
            wo=3, yps=8):
        return lib.avs_bn_maxpool_nhwc(dtype, x, n, h, w, c, xps, gr, groups, sc, sf, relu, k, s, p, y, ho, wo, yps, None)

    for fn in (pool, bmp):
        assert fn(dtype=2) == ARG
        assert fn(c=6) == SHAPE and fn(xps=4) == SHAPE and fn(yps=10) == SHAPE and fn(p=3) == SHAPE and fn(s=0) == SHAPE
        assert fn(ho=4) == SHAPE and fn(wo=5) == SHAPE and fn(h=0) == SHAPE and fn(n=-1) == SHAPE     # output extent too large
        assert fn(x=None) == ARG and fn(y=None) == ARG
        assert fn(n=0, x=None, y=None) == 0
        assert fn(dtype=H2, c=12, xps=16, yps=16) == ALIGN and fn(dtype=H2, yps=12) == ALIGN and fn(dtype=H2, x=A + 16) == ALIGN
        for kw in (dict(x=A + 8), dict(y=A + 8), dict(y=A + 4)):
            assert fn(**kw) == ALIGN, (fn.__name__, kw)
            assert b"aligned" in lib.avs_last_error()
        for kw in (dict(x=A + 4), dict(y=A + 2), dict(x=A + 12)):
            assert fn(dtype=BF16, **kw) == ALIGN, (fn.__name__, kw)
    assert pool(mode=2) == ARG and pool(act=5) == ARG
    assert pool(mode=1, bias=A + 2) == ALIGN
    assert bmp(gr=A, groups=0) == ARG and bmp(gr=None, groups=2) == ARG and bmp(sc=None) == ARG
    assert bmp(sc=A + 8) == ALIGN and bmp(sf=A + 4) == ALIGN

    def gap(dtype=F32, x=A, n=2, hw=4, c=8, y=A, ldy=8):
        return lib.avs_global_avgpool_nhwc(dtype, x, n, hw, c, y, ldy, None)

    assert gap(dtype=3) == ARG and gap(c=6) == SHAPE and gap(ldy=4) == SHAPE and gap(ldy=10) == SHAPE and gap(hw=0) == SHAPE
    assert gap(x=None) == ARG and gap(n=0, x=None, y=None) == 0
    assert gap(y=A + 8) == ALIGN and gap(dtype=H2, c=12, ldy=16) == ALIGN and gap(dtype=H2, x=A + 16) == ALIGN
    assert gap(x=A + 8) == ALIGN and gap(x=A + 4) == ALIGN and gap(dtype=BF16, x=A + 4) == ALIGN and gap(dtype=BF16, x=A + 2) == ALIGN
