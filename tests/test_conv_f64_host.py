"""The case table of the float64 tests of avs_conv2d_nhwc and avs_conv2d_nhwc_split, checked on the host (no GPU): the
restated plan pinned on the library's recorded answers, the instances of igemm_kernel the cases reach against REACHABLE,
the float64 reference against an explicit loop over taps, the restatements and planted mistakes against the bound, the
measured constants, the exactness of the integer operand set, and the entry points' refusals (conv_f64_inputs; the
device side is test_gpu_conv_f64.py)."""
import ctypes
import json
import os
import re

import pytest
import torch

import conv_f64_inputs as cfi
import gemm_f64_inputs as gfi

LIVE = [c for c in cfi.CASES if c.n > 0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_plan_host.json")
# second_dest_offset and relu_cols_ignored belong to avs_conv2d_nhwc_split, which takes AVS_F16X2 only
ONE_DTYPE = {"second_dest_offset", "relu_cols_ignored"}


# --------------------------------------------------------------------------- the plan
def test_the_restated_tile_rule_answers_as_the_library_did():
    """tile_choice(stats=True) against the first recorded answer (avs_conv2d_bnstats_workspace_bytes) of every dtype /
    shape entry of the corpus that the library did not refuse: round256(tiles_m * ((tile_rows + rpg - 2) // rpg + 1) *
    2 * N * 4).  Left out by predicate: the AVS_F16P8 input format (its own BatchNorm-only requirements decide whether
    the library answers at all; the tile rule is not restated for it)."""
    with open(GOLDEN) as f:
        corpus = json.load(f)
    i, checked, kinds = 0, 0, set()
    for shape in corpus["shapes"]:
        h, w, cin, kh, kw, s, pad, cout = shape
        ph, pw = pad if isinstance(pad, list) else (pad, pad)
        ho, wo = cfi.out_extent(h, w, kh, kw, s, s, ph, pw)
        for gf in corpus["group_frames"]:
            for dtype in corpus["dtypes"]:
                for variant in corpus["variants"]:
                    for formats in corpus["formats"]:
                        answer = corpus["answers"][i][0]
                        i += 1
                        if answer < 0 or formats != 0:
                            continue
                        m, k, rpg = corpus["n"] * ho * wo, kh * kw * cin, gf * ho * wo
                        bn, tiles_n, tall = cfi.tile_choice(dtype, m, cout, k, True, False, variant & 3, stats=True)
                        rows = 256 if tall else 128
                        want = (-(-m // rows) * ((rows + rpg - 2) // rpg + 1) * 2 * cout * 4 + 255) // 256 * 256
                        assert answer == want, (shape, gf, dtype, variant, answer, want)
                        checked += 1
                        kinds.add((dtype, rows))
    assert i == len(corpus["answers"]) and checked >= 1000
    assert kinds == {(cfi.F32, 128), (cfi.BF16, 128), (cfi.BF16, 256), (cfi.SPLIT, 128), (cfi.SPLIT, 256), (cfi.F16X2, 128),
                     (cfi.F16X2, 256)}


def _assert_edges(rules):
    """The edges the rules name, each shape on the side of its threshold that the case table puts it."""
    g = lambda cin, cout=40, k=(3, 3), p=(1, 1), n=3: (n, 9, 7, cin, k[0], k[1], 1, 1, p[0], p[1], cout)
    plain, brelu = cfi.EPILOGUES["plain"], cfi.EPILOGUES["brelu"]
    rowb = lambda dtype, geo, **kw: cfi.plan(dtype, geo, plain, rules=rules, **kw)[5]
    # rowb_threshold_bytes: 3x3 at cin 56 (2016 bytes) and 64 (2304 bytes); fast64_only keeps cin 80 (2880 bytes) on 64
    assert rowb(cfi.F32, g(56)) == 64 and rowb(cfi.F32, g(64)) == 128 and rowb(cfi.F32, g(80)) == 64
    assert rowb(cfi.F32, g(80), variant=cfi.GENERIC) == 128 and rowb(cfi.BF16, g(112)) == 64 and rowb(cfi.BF16, g(128)) == 128
    tall = [c for c in cfi.CASES if c.period]
    assert tall
    for c in tall:          # one frame fewer than two past the rule's count leaves the 256-row tiles
        assert cfi.case_plan(c, rules)[8] == 4, c.name
        fewer = c._replace(n=c.n - 3 * (256 // 63 + 1))
        assert cfi.case_plan(fewer, rules)[8] == 2, c.name
    # tall_min_k_bytes: the wide tiles need it, the narrow do not
    n = tall[0].n
    wide = lambda cin, dtype=cfi.F16X2: cfi.plan(dtype, g(cin, cout=104, n=2 * n), brelu, rules=rules)
    assert wide(32)[7] == 4 and wide(16)[7] == 2 and wide(32)[10] and not wide(16)[10]
    assert cfi.plan(cfi.F16X2, g(32, cout=96, n=n), brelu, rules=rules)[2] == 96
    assert cfi.plan(cfi.F16X2, g(16, cout=96, n=n), brelu, rules=rules)[2] == 128


def test_the_thresholds_are_read_from_the_source(tmp_path):
    src = open(gfi._source()).read()
    _assert_edges(None)
    for name in ("rowb_threshold_bytes", "tall_min_tiles", "tall_min_k_bytes"):
        for factor in (0.5, 2):
            edited = tmp_path / f"{name}_{factor}.hip"
            edited.write_text(re.sub(rf"(g_{name} = )\d+", lambda m: m.group(1) + str(int(cfi.RULES[name] * factor)), src))
            rules = cfi.read_rules(str(edited))
            assert rules[name] == int(cfi.RULES[name] * factor)
            with pytest.raises(AssertionError):
                _assert_edges(rules)
            # ... and where it moves cases onto other instances, the reach assertion fails too (a halved tall rule moves
            # none: the tall cases sit just past the rule they were built from and stay tall under a laxer one)
            moved = [c.name for c in cfi.CASES if cfi.instance(c, rules) != cfi.instance(c)]
            assert moved or (name != "rowb_threshold_bytes" and factor == 0.5), (name, factor)
            assert not moved or {cfi.instance(c, rules) for c in cfi.CASES} != cfi.REACHABLE - set(cfi.LEFT_OUT), (name, factor)


def test_the_cases_reach_every_instance_the_plain_entry_points_can():
    reached = {cfi.instance(c) for c in cfi.CASES}
    want = cfi.REACHABLE - set(cfi.LEFT_OUT)
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in cfi.LEFT_OUT.values())
    assert len(cfi.REACHABLE) == 495 and len(cfi.LEFT_OUT) == 53
    # every field's every value is reached, the shifted-row form on each tile width
    for f, values in enumerate(cfi.FIELDS):
        assert {t[f] for t in reached} == set(values), f
    assert {t[1] for t in reached if t[9]} == {64, 96, 128}
    # the plan tuple's element size and split follow the dtype
    for c in cfi.CASES:
        p = cfi.case_plan(c)
        assert p[1:3] == (cfi.es_of(c.dtype), {cfi.SPLIT: 1, cfi.F16X2: 2}.get(c.dtype, 0))


def test_the_table_has_the_issues_families():
    by = lambda **kw: [c for c in LIVE if all(getattr(c, k) == v for k, v in kw.items())]
    geo = lambda c: (c.kh, c.kw, c.sh, c.sw, c.ph, c.pw)
    assert all(c.h != c.w for c in cfi.CASES)
    for dtype in cfi.DTYPES:
        mine = by(dtype=dtype)
        assert {geo(c) for c in mine} >= {(1, 1, 1, 1, 0, 0), (1, 1, 2, 1, 0, 0), (3, 3, 1, 1, 1, 1), (3, 3, 2, 2, 1, 1),
                                          (3, 3, 1, 2, 1, 0), (3, 3, 1, 1, 0, 0), (3, 3, 1, 1, 2, 2), (3, 3, 1, 1, 3, 3), (1, 7, 1, 1, 0, 3),
                                          (7, 1, 1, 1, 3, 0), (5, 5, 2, 2, 2, 2), (2, 2, 2, 2, 0, 0), (7, 7, 2, 2, 3, 3)}
        assert [c for c in mine if c.xwide > c.cin and c.kh == 1] and [c for c in mine if c.crop and c.kh == 1]
        assert [c for c in mine if c.xwide > c.cin and c.crop and c.kh == 3]
        e = 4 // cfi.es_of(dtype)
        assert {c.cin for c in mine if c.kh == 3} >= {cf * e for cf in (8, 16, 24, 32, 48, 96)}
        assert {c.cout for c in mine} >= {8, 64, 72, 128, 136}
        extent = lambda c: c.n * cfi.extent(c)[0] * cfi.extent(c)[1]
        assert {extent(c) for c in mine} >= {127, 128, 129, 255, 256, 257}
        assert {c.variant & 3 for c in mine} == {0, 1, 2} and [c for c in mine if c.variant & cfi.GENERIC]
        kbytes = lambda c: c.kh * c.kw * c.cin * cfi.es_of(dtype)
        for walk in (0, cfi.GENERIC):       # each reduction class with the tap walk's alignment / flag and with STAGING_GENERIC
            on = {kbytes(c) for c in mine if (c.variant & cfi.GENERIC) == walk}
            assert [b for b in on if b < 64] and [b for b in on if 64 <= b <= 128], (dtype, walk)
            assert [b for b in on if 128 < b <= cfi.RULES["rowb_threshold_bytes"]] and [b for b in on if b > cfi.RULES["rowb_threshold_bytes"]]
        assert {c.w_layout for c in mine} == ({0} if dtype == cfi.ACC64 else {0, 1})
        assert {c.epi for c in mine} == ({"plain", "brelu"} if dtype == cfi.F16X2 else set(cfi.EPILOGUES))
        assert [c for c in mine if c.ypad and c.yc0] and [c for c in mine if c.ypad == 8 and not c.yc0]
        assert len(by(dtype=dtype, n=3)) > len(mine) // 2
        assert [c for c in cfi.CASES if c.dtype == dtype and c.n == 0]
    bf = by(dtype=cfi.BF16)
    for bn in (64, 128):
        on = [c for c in bf if cfi.case_plan(c)[3] == bn]
        ldc = lambda c: c.cout + c.ypad
        assert [c for c in on if ldc(c) % 8] and [c for c in on if ldc(c) % 8 == 0 and c.yc0 % 8]          # the scalar store
        assert [c for c in on if ldc(c) % 8 == 0 and c.yc0 % 8 == 0 and c.cout % 8 == 0]                   # 16-byte vectors
    assert cfi.case_plan(cfi.CASE_BY_NAME["f32-wide-m2048-n2048-brelu"])[3] == 128
    tall = [c for c in cfi.CASES if c.period]
    shifted = [c for c in tall if cfi.case_plan(c)[11]]
    assert {(c.kh, c.kw, cfi.case_plan(c)[3]) for c in shifted} == {(k[0], k[1], bn) for k in ((3, 3), (1, 7), (7, 1))
                                                                    for bn in (64, 96, 128)}
    assert {c.cout for c in shifted} >= {8, 96, 136} and [c for c in shifted if c.xwide > c.cin]
    assert {c.dtype for c in tall if not cfi.case_plan(c)[11]} == {cfi.BF16, cfi.SPLIT, cfi.F16X2}
    for c in tall:
        ho, wo = cfi.extent(c)
        assert c.period == cfi.TALL_PERIOD and c.variant == 0 and 256 % (ho * wo) and cfi.case_plan(c)[8] == 4
        assert -(-c.n * ho * wo // 256) >= cfi.RULES["tall_min_tiles"] // -(-c.cout // cfi.case_plan(c)[3])
    splits = [c for c in cfi.CASES if c.split]
    bn = lambda c: cfi.case_plan(c)[3]
    assert [c for c in splits if c.split[0] < bn(c) < c.cout] and [c for c in splits if c.split[0] % bn(c) == 0]
    assert [c for c in splits if c.split[0] > (c.cout - 1) // bn(c) * bn(c)]
    for c in splits:
        assert c.dtype == cfi.F16X2 and (c.kh, c.kw, c.sh, c.sw, c.ph, c.pw) == (1, 1, 1, 1, 0, 0)
    assert {(r == 0, r == c.split[0], 0 < r != c.split[0]) for c in splits if c.epi == "brelu" for r in (c.split[1],)} == \
        {(True, False, False), (False, True, False), (False, False, True)}


# --------------------------------------------------------------------------- reference, restatements, mistakes, exactness
def test_the_reference_is_the_explicit_loop_over_taps():
    for name in ("f32-3x3-s12-p10-brelu", "bf16-5x5-s2-p2-scaled", "f16x2-3x3-p1-chslice-crop-brelu", "split-epilogue-3x3-s12-scaled"):
        case = cfi.CASE_BY_NAME[name]
        assert (case.sh, case.ph) != (case.sw, case.pw) or case.crop or case.ph == 2
        for which in "ab":
            ref, loop = cfi.reference(case, which), cfi.explicit_reference(case, which)
            assert ref.shape == loop.shape
            assert bool(((ref - loop).abs() <= 2.0 ** -45 * cfi.magnitude(case, which)).all()), (name, which)
    # windows that lie wholly in the padding give the epilogue of 0
    for name in ("bf16-3x3-p3-brelu", "f16x2-3x3-p3-brelu"):
        case = cfi.CASE_BY_NAME[name]
        ref = cfi.reference(case, "a").reshape(case.n, 13, 11, case.cout)
        want = cfi.operands(case, "a").bias.double().clamp_min(0).expand(case.n, -1)
        assert torch.equal(ref[:, 0, 0], want) and torch.equal(ref[:, 12, 10], want) and not torch.equal(ref[:, 1, 1], want)


def _outside(case, which, v):
    ref, target, bound, e32, s = cfi.bundle(case, which)
    return int(((v - target).abs() > bound).sum().item())


@pytest.mark.parametrize("dtype", cfi.DTYPES, ids=lambda d: cfi.DTYPE_NAMES[d])
def test_restatements_lie_within_the_bound_and_mistakes_outside(dtype):
    worst = 0.0
    for case in (c for c in LIVE if c.dtype == dtype):
        ho, wo = cfi.extent(case)
        for which in "ab":
            ref, target, bound, e32, s = cfi.bundle(case, which)
            rs = cfi.restatement(case, which)
            assert rs.shape == ref.shape == (cfi.frames(case) * ho * wo, case.cout)
            assert _outside(case, which, rs) == 0, (case.name, which)
            assert _outside(case, which, cfi.fp32_yardstick(case, which)) == 0 or dtype in (cfi.SPLIT, cfi.F16X2), (case.name, which)
            if dtype in (cfi.SPLIT, cfi.F16X2):
                # (their target is the restatement; the fp32 evaluation is held to the reference + the restatement's distance)
                const = cfi.SPLIT_C if dtype == cfi.SPLIT else cfi.F16X2_C
                unit = cfi.restatement_unit(case)
                worst = max(worst, cfi.restatement_ratio(case, which))
                assert bool(((rs - ref).abs() <= const * unit * s).all()), (case.name, which)
                assert bool(((cfi.fp32_yardstick(case, which) - ref).abs() <= gfi.fp32_term(e32, s)).all()), (case.name, which)
            if which == "b":
                assert torch.equal(rs, cfi.exact_result(case)), case.name
        hit = 0
        for mistake in cfi.MISTAKES:
            if not cfi.applies(case, mistake):
                continue
            hit += 1
            assert _outside(case, "a", cfi.restatement(case, "a", mistake)) > 0, (case.name, mistake)
            assert not torch.equal(cfi.restatement(case, "b", mistake), cfi.exact_result(case)), (case.name, mistake)
        x_img, x_row, x_px, off = cfi.strides(case)
        if case.kh * case.kw > 1 or x_px != case.cin or x_row != case.w * x_px:
            assert hit > 0, case.name
    if dtype in (cfi.SPLIT, cfi.F16X2):
        measured = cfi.SPLIT_C_MEASURED if dtype == cfi.SPLIT else cfi.F16X2_C_MEASURED
        print(f"{cfi.DTYPE_NAMES[dtype]} restatement: largest |restatement - ref| / (unit * S) = {worst:.4f}")
        assert 0.9 * measured <= worst <= 1.001 * measured


def test_every_mistake_has_cases_in_two_dtypes():
    for mistake in cfi.MISTAKES:
        on = [c for c in LIVE if cfi.applies(c, mistake)]
        assert len(on) >= 3, mistake
        assert len({c.dtype for c in on}) >= (1 if mistake in ONE_DTYPE else 2), mistake
        if mistake in ONE_DTYPE:
            assert all(c.split for c in on)


def test_integer_operands_are_exact():
    for case in LIVE:
        partial, top = cfi.exact_headroom(case)
        assert partial < 2 ** 24 and top < 2 ** 8, case.name
        if case.dtype == cfi.F16X2:
            assert partial < 65504, case.name
        o = cfi.operands(case, "b")
        for t in (o.xv, o.wv) + ((o.bias,) if o.bias is not None else ()):
            assert torch.equal(t, t.round()) and t.abs().max().item() <= (2 * top if t is o.bias else top)
        if case.dtype == cfi.F16X2:       # no lo halves: the packed image holds the integers in its hi halves
            assert torch.equal(cfi.emu_unpack(o.x_buf), o.xv) and not o.x_buf.view(torch.float16).reshape(-1, 2, 8)[:, 1].any()


def test_operand_set_a_has_three_frame_magnitudes():
    for name, scales in (("f32-3x3-p1-n64-brelu", cfi.FRAME_SCALES[False]), ("f16x2-3x3-p1-n64-brelu", cfi.FRAME_SCALES[True])):
        case = cfi.CASE_BY_NAME[name]
        o = cfi.operands(case, "a")
        rms = o.x.pow(2).mean((1, 2, 3)).sqrt()
        assert all(0.8 * s < r < 1.25 * s for r, s in zip(rms.tolist(), scales))
        ref = cfi.reference(case, "a").reshape(case.n, -1)
        assert all(0.2 < (ref[f] == 0).double().mean().item() < 0.8 for f in range(2))      # the ReLU clips about half
        if case.dtype == cfi.F16X2:
            assert o.xv.abs().max().item() < 65504 / 4 and ref.abs().max().item() < 65504 / 4
            assert (o.x.abs() >= 2.0 ** -14).double().mean().item() > 0.99                   # fp16's normal range
    bf = cfi.operands(cfi.CASE_BY_NAME["bf16-3x3-p1-n64-brelu"], "a")
    assert torch.equal(bf.xv.bfloat16().float(), bf.xv) and torch.equal(bf.wv.bfloat16().float(), bf.wv)


# --------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("label,status,has_bias,changes", cfi.refusals(), ids=[r[0] for r in cfi.refusals()])
def test_refusals_launch_nothing(label, status, has_bias, changes):
    """With null operands nothing can be launched whatever the library answers.  conv_geometry's refusals come before
    every check of the operands, and so does the plan's refusal of AVS_F16X2's other epilogues (its first check), so
    the status is the same as with operands given (test_gpu_conv_f64.py makes these calls with device buffers)."""
    from avsum_amd import _abi
    lib = _abi.lib()
    d = _abi.ConvDesc(*cfi.desc_fields(**changes))
    bias = (ctypes.c_float * 64)() if has_bias else None
    got = lib.avs_conv2d_nhwc(ctypes.byref(d), None, None, bias, None, None)
    assert got == status, lib.avs_last_error()
    assert b"avs_conv2d_nhwc" in lib.avs_last_error()
    if changes.get("dtype") == cfi.F16X2:
        got = lib.avs_conv2d_nhwc_split(ctypes.byref(d), None, None, bias, None, 8, None, 32, 0, None)
        assert got < 0 and b"avs_conv2d_nhwc_split" in lib.avs_last_error()


def test_n_0_is_ok_with_null_operands():
    from avsum_amd import _abi
    for dtype in cfi.DTYPES:
        d = _abi.ConvDesc(*cfi.desc_fields(dtype=dtype, n=0))
        assert _abi.lib().avs_conv2d_nhwc(ctypes.byref(d), None, None, None, None, None) == 0
