"""The case table of the avs_gemm_nt float64 tests, checked on the host (no GPU): the instances of igemm_kernel it
reaches, its restatements and planted mistakes against the bound, the exactness of the integer operand set, and the
entry point's refusals (gemm_f64_inputs; the device side is test_gpu_gemm_f64.py)."""
import ctypes
import itertools
import re

import pytest
import torch

import gemm_f64_inputs as gfi

SMALL = [c for c in gfi.CASES if gfi.rows(c) * c.n <= 2 ** 20]      # everything but the unbatched 2048 x 2048 case


# --------------------------------------------------------------------------- reach
def _impossible(dtype, es, bn, rowb, pipe, wr, fastk, epi):
    """Why avs_gemm_nt cannot produce this plan, or None if the rules allow it."""
    if es != (2 if dtype == gfi.BF16 else 4):
        return "the element size is the dtype's"
    if dtype == gfi.ACC64 and bn != 64:
        return "AVS_F32_ACC64 is narrow by rule"
    if dtype == gfi.ACC64 and (pipe or fastk or wr != 2):
        return "the fp64 slice accumulation runs on the classic 128-row walk with the generic staging"
    if pipe and rowb != 64:
        return "the 3-buffer pipeline exists on 64-byte steps only"
    if wr == 4 and not pipe:
        return "the 256-row tiles are built on the pipeline"
    if wr == 4 and dtype not in (gfi.BF16, gfi.SPLIT):
        return "256-row tiles: bf16 and fp32-split only"
    if wr == 4 and epi == "any":
        return "256-row tiles: the compile-time epilogues only"
    return None


def _assert_edges(rules):
    """The edges the rules name, each case on the side of its threshold the issue puts it."""
    f32 = lambda k, **kw: gfi.plan(gfi.F32, 37, 40, k, rules=rules, **kw)[2:6]
    assert f32(32) == (64, False, 2, True) and f32(36) == (64, True, 2, False) and f32(48) == (64, True, 2, True)
    assert f32(512) == (64, True, 2, True) and f32(516) == (128, False, 2, False) and f32(544) == (128, False, 2, True)
    assert f32(528) == (64, True, 2, True)
    bf = lambda k: gfi.plan(gfi.BF16, 37, 40, k, rules=rules)[2:6]
    assert [bf(2 * k) for k in (32, 36, 48, 512, 516, 544, 528)] == [f32(k) for k in (32, 36, 48, 512, 516, 544, 528)]
    assert gfi.plan(gfi.F32, 257, 200, 52, rules=rules)[1] == 64 and gfi.plan(gfi.F32, 130, 129, 24, batch=2, rules=rules)[1] == 128
    assert gfi.plan(gfi.F32, 2048, 2048, 16, rules=rules)[1] == 128 and gfi.plan(gfi.F32, 2048, 2047 - 127, 16, rules=rules)[1] == 64
    assert gfi.plan(gfi.BF16, 2047 * 256 + 1, 8, 80, rules=rules)[4] == 4 and gfi.plan(gfi.BF16, 2047 * 256, 8, 80, rules=rules)[4] == 2
    assert gfi.plan(gfi.SPLIT, 2047 * 256 + 1, 8, 48, rules=rules)[4:6] == (4, True) and gfi.plan(gfi.SPLIT, 2047 * 256 + 1, 8, 32, rules=rules)[4] == 2
    assert gfi.plan(gfi.BF16, 1023 * 256 + 1, 129, 512, rules=rules)[4] == 4 and gfi.plan(gfi.BF16, 1023 * 256 + 1, 129, 504, rules=rules)[4] == 2
    # a window past 2 GiB turns the tap walk off
    assert gfi.plan(gfi.F32, 8, 8, 16, lda=2 ** 21, rules=rules)[5] is False and gfi.plan(gfi.F32, 8, 8, 16, lda=2 ** 20, rules=rules)[5] is True


def test_the_thresholds_are_read_from_the_source(tmp_path):
    assert {"rowb_threshold_bytes", "tall_min_tiles", "tall_min_k_bytes", "pipe3"} <= set(gfi.RULES)
    src = open(gfi._source()).read()
    for name in ("rowb_threshold_bytes", "tall_min_tiles", "tall_min_k_bytes"):
        assert re.search(rf"^AVS_RULE g_{name} = {gfi.RULES[name]};", src, re.M), name
    # a retuned rule moves shapes onto other instances: the edge assertions of the reach test then fail, in either direction
    for name in ("rowb_threshold_bytes", "tall_min_tiles", "tall_min_k_bytes"):
        for factor in (0.5, 2):
            edited = tmp_path / f"{name}_{factor}.hip"
            edited.write_text(re.sub(rf"(g_{name} = )\d+", lambda m: m.group(1) + str(int(gfi.RULES[name] * factor)), src))
            rules = gfi.read_rules(str(edited))
            assert rules[name] == int(gfi.RULES[name] * factor)
            with pytest.raises(AssertionError):
                _assert_edges(rules)


def test_the_cases_reach_every_instance_a_plain_gemm_can():
    every = itertools.product(gfi.DTYPES, (2, 4), (64, 128), (64, 128), (False, True), (2, 4), (False, True),
                              ("plain", "brelu", "any"))
    possible = {t for t in every if _impossible(*t) is None}
    reached = {gfi.case_plan(c) for c in gfi.CASES}
    assert reached == possible, (sorted(possible - reached), sorted(reached - possible))
    assert len(possible) == 130
    _assert_edges(None)


def test_the_table_has_the_issues_edges():
    by = lambda **kw: [c for c in gfi.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for dtype in gfi.DTYPES:
        scale = 2 if dtype == gfi.BF16 else 1
        assert {c.k for c in by(dtype=dtype)} >= {k * scale for k in (4, 12, 16, 32, 36, 48, 52, 512, 516, 544, 528)}
        assert {c.m for c in by(dtype=dtype)} >= {0, 1, 127, 128, 129, 257}
        assert {c.n for c in by(dtype=dtype)} >= {1, 63, 64, 65, 127, 128, 129, 200}
        assert {(c.bias_mode, c.act, c.alpha) for c in by(dtype=dtype)} == set(gfi.EPILOGUES.values())
        assert {c.batch for c in by(dtype=dtype)} >= {1, 3, 5}
        assert by(dtype=dtype, lda=0) and by(dtype=dtype, col0=16, m=33) and by(dtype=dtype, col0=8, m=1) and by(dtype=dtype, sb=0, batch=3)
        assert bool(by(dtype=dtype, via_linear=True)) == (dtype in (gfi.F32, gfi.BF16))      # ops.linear's dtypes
        assert [c for c in by(dtype=dtype) if c.batch > 1 and c.sc > c.m * c.ldc]          # a gap between batch entries
        assert [c for c in by(dtype=dtype) if c.batch > 1 and c.bias_mode and c.sbias == 0]
        assert [c for c in by(dtype=dtype) if c.batch > 1 and c.bias_mode and c.sbias != 0]
    assert all({(c.m, c.n) for c in by(dtype=d)} >= set(itertools.product((1, 127, 128, 129, 257), (1, 63, 64, 65, 127, 128, 129, 200)))
               for d in gfi.DTYPES)
    bf = by(dtype=gfi.BF16)
    for bn in (64, 128):
        on = [c for c in bf if gfi.case_plan(c)[2] == bn and c.m]
        assert [c for c in on if (c.ldc * 2) % 16 != 0]                                                    # scalar: row stride
        assert [c for c in on if (c.ldc * 2) % 16 == 0 and ((c.ldc + c.col0) * 2) % 16 != 0]               # scalar: C pointer
        assert [c for c in on if (c.ldc * 2) % 16 == 0 and ((c.ldc + c.col0) * 2) % 16 == 0 and c.n % 8 and c.n > 8]   # col + 8 > N
        assert [c for c in on if (c.ldc * 2) % 16 == 0 and c.col0 == 0 and c.m % 128 == 0 and c.n % bn == 0]         # whole tiles
    tall = [c for c in gfi.CASES if gfi.case_plan(c)[5] == 4]
    assert {(c.dtype, c.n, c.k, c.bias_mode) for c in tall} >= {(d, 8, k, b) for d, k in ((gfi.BF16, 80), (gfi.SPLIT, 48))
                                                                for b in (gfi.NONE, gfi.COL)}
    assert all(c.m % 256 == 1 and c.period == gfi.TALL_PERIOD for c in tall)


# --------------------------------------------------------------------------- restatements, mistakes, exactness
def _outside(case, which, v):
    """Number of elements of ``v`` outside the bound of the case's target."""
    ref, target, bound, e32, s = gfi.bundle(case, which)
    return int(((v - target).abs() > bound).sum().item())


@pytest.mark.parametrize("dtype", gfi.DTYPES, ids=lambda d: gfi.DTYPE_NAMES[d])
def test_restatements_lie_within_the_bound_and_mistakes_outside(dtype):
    worst_split = 0.0
    seen = {m: 0 for m in gfi.MISTAKES}
    for case in (c for c in SMALL if c.dtype == dtype):
        for which in "ab":
            ref, target, bound, e32, s = gfi.bundle(case, which)
            rs = gfi.restatement(case, which)
            assert rs.shape == ref.shape == (case.batch, gfi.rows(case), case.n)
            assert _outside(case, which, rs) == 0, (case.name, which)
            if dtype == gfi.SPLIT:
                worst_split = max(worst_split, gfi.split_ratio(case, which))
                assert bool(((rs - ref).abs() <= gfi.SPLIT_C * 2.0 ** -15 * s).all()), (case.name, which)
            if which == "b":
                assert torch.equal(rs, gfi.exact_result(case)), case.name
        for mistake in gfi.MISTAKES:
            if not gfi.applies(case, mistake):
                continue
            seen[mistake] += 1
            assert _outside(case, "a", gfi.restatement(case, "a", mistake)) > 0, (case.name, mistake)
            if mistake not in ("bf16_twice", "split_drop_al_bh"):      # (exact operands round once and have no lo halves)
                assert not torch.equal(gfi.restatement(case, "b", mistake), gfi.exact_result(case)), (case.name, mistake)
    for mistake, count in seen.items():
        expected = {"bf16_twice": dtype == gfi.BF16, "split_drop_al_bh": dtype == gfi.SPLIT}.get(mistake, True)
        assert (count > 0) == expected, (mistake, count)
    if dtype == gfi.SPLIT:
        # SPLIT_C is twice what the restatement needs, measured here against the float64 reference
        print(f"SPLIT restatement: largest |restatement - ref| / (2^-15 S) = {worst_split:.4f}")
        assert 0.9 * gfi.SPLIT_C_MEASURED <= worst_split <= 1.001 * gfi.SPLIT_C_MEASURED


def test_the_large_fp32_case_restates_within_its_bound():
    case = gfi.CASE_BY_NAME["f32-m2048-n2048-k16-brelu"]
    assert gfi.case_plan(case) == (gfi.F32, 4, 128, 64, False, 2, True, "brelu")
    assert _outside(case, "a", gfi.restatement(case, "a")) == 0
    assert _outside(case, "a", gfi.restatement(case, "a", "tile_seam")) > 0
    assert torch.equal(gfi.restatement(case, "b"), gfi.exact_result(case))


def test_integer_operands_are_exact_in_fp32():
    for case in gfi.CASES:
        partial, top = gfi.exact_headroom(case)
        assert partial < 2 ** 24 and top < 2 ** 8, case.name
        o = gfi.operands(case, "b")
        for t in (o.A, o.B) + ((o.bias,) if o.bias is not None else ()):
            assert torch.equal(t, t.round()) and (not t.numel() or t.abs().max().item() <= (2 * top if t is o.bias else top))
        if gfi.rows(case) * case.n <= 2 ** 20 and case.m:
            s = gfi.magnitude(case, "b")
            assert s.max().item() / min(1.0, abs(case.alpha)) < 2 ** 24
            assert not torch.equal(o.A[0], o.B[0, :o.A.shape[1]]) or case.m == 1 or case.n == 1      # asymmetric


def test_operand_set_a_has_three_row_magnitudes():
    case = gfi.CASE_BY_NAME["f32-epilogue-m70-n90-brelu"]
    o = gfi.operands(case, "a")
    rms = o.A[0].pow(2).mean(-1).sqrt()
    assert (rms[1::3] < 3e-3).all() and ((rms[0::3] > 0.5) & (rms[0::3] < 2)).all() and (rms[2::3] > 500).all()
    ref = gfi.reference(case, "a")
    assert 0.3 < (ref == 0).double().mean().item() < 0.7          # the ReLU clips about half
    bf = gfi.operands(gfi.CASE_BY_NAME["bf16-epilogue-m70-n90-brelu"], "a")
    assert torch.equal(bf.A.bfloat16().float(), bf.A) and torch.equal(bf.B.bfloat16().float(), bf.B)


# --------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("label,status,status_null,changes", gfi.refusals(), ids=[r[0] for r in gfi.refusals()])
def test_refusals_launch_nothing(label, status, status_null, changes):
    """With null operands nothing can be launched whatever the library answers; the order of checks then reports the
    null operand first for the checks that come after it.  The status of each check itself needs operands: where no
    device exists (no launch possible either) 16-byte-aligned host addresses stand in for them, which no refused call
    reads; on a device test_gpu_gemm_f64.py makes the same calls with device buffers."""
    from avsum_amd import _abi
    lib = _abi.lib()
    assert lib.avs_gemm_nt(*gfi.refusal_args(changes)) == status_null, lib.avs_last_error()
    assert lib.avs_last_error()
    if torch.cuda.is_available():
        return
    host = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(host) + 255) // 256 * 256
    ptrs = [ctypes.c_void_p(base + 1024 * i) for i in range(3)]
    assert lib.avs_gemm_nt(*gfi.refusal_args(changes, *ptrs)) == status, lib.avs_last_error()
    assert b"avs_gemm_nt" in lib.avs_last_error()


def test_m_0_is_ok_with_null_operands():
    from avsum_amd import _abi
    assert _abi.lib().avs_gemm_nt(*gfi.refusal_args(dict(m=0))) == 0
