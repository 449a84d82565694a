"""CPU-side checks of the fused AdamW step (libavsum_optim.so, avsum_amd/optim.py): the second header and the binding
derived from it, the library's exports, validation before any launch, the host restatement against float64 within the
project's bound, four planted mistakes caught by that bound, the constructor's refusals, the launch plan of 70 tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import optim_inputs as oi
from avsum_amd import _header, _optim_abi, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(_optim_abi.LIB_PATH))

PINNED = {
    "avso_abi_version": ("int", []),
    "avso_last_error": ("char*", []),
    "avso_workspace_bytes": ("size_t", ["int64_t"]),
    "avso_grad_sumsq_f32": ("int", ["int64_t*", "int", "double*", "int64_t", "int64_t", "avso_stream_t"]),
    "avso_adamw_prepare": ("int", ["double*", "int64_t", "double", "double", "double", "double", "double", "int",
                                   "double*", "float*", "avso_stream_t"]),
    "avso_adamw_apply_f32": ("int", ["int64_t*", "int", "float*", "double", "double", "double", "avso_stream_t"]),
}


# --------------------------------------------------------------------------- header, binding, library
def test_optim_header_parses_and_signatures_are_pinned():
    header = _optim_abi.load_header()
    assert header.prototypes == PINNED
    assert _optim_abi.declared_symbols() == sorted(PINNED)
    c = header.constants
    assert (c["AVSO_ABI_VERSION"], c["AVSO_MAX_TENSORS"], c["AVSO_CHUNK"], c["AVSO_TABLE_COLS"]) == (1, 32, 4096, 5)
    assert (c["AVSO_OK"], c["AVSO_E_ARG"], c["AVSO_E_SHAPE"], c["AVSO_E_ALIGN"], c["AVSO_E_HIP"],
            c["AVSO_E_WORKSPACE"]) == (0, -1, -2, -3, -4, -5)
    sig = header.signatures()
    assert sig["avso_last_error"] == (ctypes.c_char_p, [])
    assert sig["avso_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64])
    assert sig["avso_adamw_apply_f32"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    # the main header's reader keeps its behaviour: load() still reads include/avsum_hip.h, which knows no avso_ name
    main = _header.load()
    assert _header.HEADER_PATH.endswith(os.path.join("include", "avsum_hip.h"))
    assert not [n for n in list(main.prototypes) + list(main.constants) if n.lower().startswith("avso_")]


def test_optim_library_exports_exactly_the_headers_functions():
    lib = _optim_abi.lib()
    assert lib.avso_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _optim_abi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(avso_[a-z0-9_]+)\b", out))
    assert exported == set(PINNED), exported
    # and nothing of the main library: the two share no symbol
    assert not re.findall(r"\b(avs_[a-z0-9_]+)\b", out)
    for name, (res, args) in _optim_abi._SIGNATURES.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name


def test_optim_source_is_outside_srcs_and_built_with_the_same_flags():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "optim.hip" not in srcs and len(srcs) == 21
    assert re.search(r"^all: \$\(LIB\) \$\(OPTIM_LIB\)$", make, flags=re.M)
    rule = re.search(r"^\.\./build/optim\.o:.*\n(?:\t.*\n)*", make, flags=re.M).group(0)
    assert "$(HIPCC) $(CXXFLAGS) -c" in rule
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS = (.*)$", make, flags=re.M).group(1)
    text = open(os.path.join(PKG, "csrc", "optim.hip")).read()
    assert "avs_internal.h" not in text and "avsum_hip.h" not in text
    assert re.search(r"^static thread_local char g_err\[", text, flags=re.M)


def test_main_header_and_library_sources_are_the_parents():
    """This feature adds a second library and leaves the first alone: include/avsum_hip.h, every source of
    libavsum_hip.so, and the SRCS and CXXFLAGS lines of the Makefile are byte for byte what they were in the commit
    before include/avsum_optim.h appeared (before it is committed: in HEAD)."""
    if not os.path.exists(os.path.join(ROOT, ".git")):
        pytest.skip("not a git work tree")

    def git(*args):
        return subprocess.run(["git", "-C", ROOT, *args], capture_output=True, text=True)

    added = git("log", "--diff-filter=A", "--format=%H", "--", "include/avsum_optim.h").stdout.split()
    if added:
        old, new = [added[-1] + "~"], [added[-1]]
        if git("rev-parse", "--verify", "--quiet", old[0] + "^{commit}").returncode != 0:
            pytest.skip("the parent of the commit that added include/avsum_optim.h is not in this clone")
    else:
        old, new = ["HEAD"], []                     # not committed yet: HEAD against the work tree
    csrc = os.path.relpath(os.path.join(PKG, "csrc"), ROOT)
    make = open(os.path.join(PKG, "csrc", "Makefile")).read() if not new else git(
        "show", f"{new[0]}:{csrc}/Makefile").stdout
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    paths = ["include/avsum_hip.h"] + [f"{csrc}/{s}" for s in srcs] + [
        f"{csrc}/{h}" for h in ("avs_internal.h", "igemm_params.h", "lstm_h256.h")]
    diff = git("diff", "--quiet", *old, *new, "--", *paths)
    assert diff.returncode == 0, git("diff", "--stat", *old, *new, "--", *paths).stdout
    before = git("show", f"{old[0]}:{csrc}/Makefile").stdout
    for line in ("SRCS", "CXXFLAGS", "OBJS", "LIB"):
        pattern = rf"^{line} = .*$"
        assert re.search(pattern, make, flags=re.M).group(0) == re.search(pattern, before, flags=re.M).group(0), line


def test_optim_validation_before_launch_needs_no_gpu():
    lib = _optim_abi.lib()
    E_ARG, E_ALIGN, E_WORKSPACE = -1, -3, -5
    row = (ctypes.c_int64 * 5)(64, 64, 64, 64, 8)
    assert lib.avso_workspace_bytes(0) == 64 and lib.avso_workspace_bytes(10) == 64 + 80
    assert lib.avso_workspace_bytes(-1) == 0
    # null table, row counts outside 1..32, a negative element count, null and misaligned pointers
    assert lib.avso_grad_sumsq_f32(None, 1, 64, 0, 1, None) == E_ARG and b"h_table" in lib.avso_last_error()
    for n in (0, -1, 33):
        assert lib.avso_adamw_apply_f32(row, n, 64, 0.9, 0.999, 1e-8, None) == E_ARG
        assert b"ntensors" in lib.avso_last_error()
        assert lib.avso_grad_sumsq_f32(row, n, 64, 0, 1, None) == E_ARG
    bad = (ctypes.c_int64 * 5)(64, 64, 64, 64, -8)
    assert lib.avso_adamw_apply_f32(bad, 1, 64, 0.9, 0.999, 1e-8, None) == E_ARG and b"numel" in lib.avso_last_error()
    assert lib.avso_grad_sumsq_f32(bad, 1, 64, 0, 1, None) == E_ARG
    for col in range(4):
        null = (ctypes.c_int64 * 5)(64, 64, 64, 64, 8)
        null[col] = 0
        assert lib.avso_adamw_apply_f32(null, 1, 64, 0.9, 0.999, 1e-8, None) == E_ARG
        assert b"null" in lib.avso_last_error()
        odd = (ctypes.c_int64 * 5)(64, 64, 64, 64, 8)
        odd[col] = 66
        assert lib.avso_adamw_apply_f32(odd, 1, 64, 0.9, 0.999, 1e-8, None) == E_ALIGN
    assert lib.avso_adamw_apply_f32(row, 1, None, 0.9, 0.999, 1e-8, None) == E_ARG and b"d_coef" in lib.avso_last_error()
    assert lib.avso_adamw_apply_f32(row, 1, 64, 1.0, 0.999, 1e-8, None) == E_ARG and b"betas" in lib.avso_last_error()
    assert lib.avso_adamw_apply_f32(row, 1, 64, 0.9, 0.999, -1e-8, None) == E_ARG and b"eps" in lib.avso_last_error()
    assert lib.avso_grad_sumsq_f32(row, 1, None, 0, 1, None) == E_ARG and b"d_partials" in lib.avso_last_error()
    assert lib.avso_grad_sumsq_f32(row, 1, 64, -1, 1, None) == E_ARG
    # one chunk at first_chunk 3 does not fit 3 partials
    assert lib.avso_grad_sumsq_f32(row, 1, 64, 3, 3, None) == E_WORKSPACE and b"partials" in lib.avso_last_error()
    assert lib.avso_adamw_prepare(None, 1, 1e-3, 0.9, 0.999, 0.01, 0.0, 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(64, -1, 1e-3, 0.9, 0.999, 0.01, 0.0, 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 0.999, 0.01, 0.0, 0, None, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 0.999, 0.01, 0.0, 0, 64, None, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, -1e-3, 0.9, 0.999, 0.01, 0.0, 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 1.0, 0.01, 0.0, 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 0.999, -0.01, 0.0, 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 0.999, 0.01, float("nan"), 0, 64, 64, None) == E_ARG
    assert lib.avso_adamw_prepare(None, 0, 1e-3, 0.9, 0.999, 0.01, 0.0, 0, 68, 64, None) == E_ALIGN
    with pytest.raises(_optim_abi.AvsoError, match="status -1.*ntensors"):
        _optim_abi.check(lib.avso_adamw_apply_f32(row, 40, 64, 0.9, 0.999, 1e-8, None), "avso_adamw_apply_f32")


# --------------------------------------------------------------------------- the launch plan
def test_launch_plan_of_the_unit_table():
    table = oi.UnitTable()
    assert len(table.layout) == 70 and [n for _, n in table.layout[:10]] == list(oi.COUNTS)
    assert all(lo % 4 == k % 4 for k, (lo, _) in enumerate(table.layout))
    numels = [n for _, n in table.layout if n > 0]
    assert len(numels) == 63                                   # seven tensors of 0 elements are dropped
    plan, total = optim.launch_plan(numels)
    assert [launch["rows"] for launch in plan] == [(0, 32), (32, 63)]
    # with the empty tensors kept out, 63 rows need two launches; the full 70 would need three
    assert len(optim.launch_plan([max(n, 1) for _, n in table.layout])[0]) == 3
    chunks = [-(-n // 4096) for n in numels]
    assert total == sum(chunks) == 7 * (1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3)
    first = 0
    for launch in plan:
        lo, hi = launch["rows"]
        assert launch["first_chunk"] == first
        assert launch["starts"] == [sum(chunks[lo:lo + j]) for j in range(hi - lo + 1)]
        first += launch["starts"][-1]
    assert plan[0]["starts"][:10] == [0, 1, 2, 3, 4, 5, 6, 7, 9, 12]      # 1 3 4 5 64 4095 4096 | 4097: 2 | 8193: 3
    with pytest.raises(ValueError, match="empty tensors"):
        optim.launch_plan([4, 0])
    rows = [(16 * (i + 1), 16 * (i + 2), 16 * (i + 3), 16 * (i + 4), n) for i, n in enumerate(numels[:32])]
    packed = optim.pack_table(rows)
    assert list(packed)[:5 * 32] == [x for row in rows for x in row]
    assert optim.pack_table(rows[:2], packed) is packed
    for bad in ([], rows + rows[:1], [(1, 2, 3, 4)]):
        with pytest.raises(ValueError):
            optim.pack_table(bad)


# --------------------------------------------------------------------------- the restatement and the bound
@pytest.fixture(scope="module")
def table():
    return oi.UnitTable()


def _case_histories(table, lr, weight_decay, betas, max_grad_norm):
    params = table.views(table.params)
    grads = [table.views(g) for g in table.grads]
    kw = dict(lr=lr, betas=betas, eps=oi.EPS, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    ref64 = optim.adamw_reference(params, grads, dtype=torch.float64, **kw)
    cpu32 = oi.torch_adamw_fp32(params, grads, **kw)
    return params, grads, kw, ref64, cpu32


@pytest.mark.parametrize("case", oi.CASES, ids=[c[0] for c in oi.CASES])
def test_reference_fp32_within_the_bound(table, case):
    _, weight_decay, betas, max_grad_norm = case
    params, grads, kw, ref64, cpu32 = _case_histories(table, oi.LR, weight_decay, betas, max_grad_norm)
    got = optim.adamw_reference(params, grads, dtype=torch.float32, **kw)
    for step in range(oi.STEPS):
        assert all(x.dtype == torch.float32 for x in got[step]["params"])
        worst, misses = oi.check_step(got[step], ref64[step], cpu32[step])
        print(f"adamw_reference fp32, case {case[0]}, step {step + 1}: worst err / bound = {worst:.3f}")
        assert not misses, misses[:5]
        assert got[step]["applied"] == ref64[step]["applied"] == step + 1
    if max_grad_norm is not None:
        want, norm2 = oi.clip_coefficient([g for g in grads[-1] if g.numel()], max_grad_norm)
        assert want < 0.1                                        # the case does clip
        assert abs(ref64[-1]["norm2"] - norm2) <= 70 * 2.0 ** -52 * norm2
        assert abs(ref64[-1]["clip"] - want) <= 1e-15 and abs(got[-1]["clip"] - want) <= oi.ulp32(want)


@pytest.mark.parametrize("lr", [1e-2, 1e-4])
def test_a_reordered_evaluation_passes_and_planted_mistakes_are_caught(table, lr):
    """The bound separates a correct fp32 AdamW written in another order from four wrong ones, on the parameters."""
    params, grads, kw, ref64, cpu32 = _case_histories(table, lr, 0.01, (0.9, 0.999), None)
    kw.pop("max_grad_norm")
    good = oi.variant_fp32(params, grads, **kw)
    worst, misses = oi.check_step(good[-1], ref64[-1], cpu32[-1])
    print(f"reordered fp32 AdamW at lr {lr}: worst err / bound = {worst:.3f}")
    assert not misses, misses[:5]
    for mistake in ("coupled", "step_off_by_one", "no_bias_correction", "eps_in_sqrt"):
        wrong = oi.variant_fp32(params, grads, mistake=mistake, **kw)
        worst, misses = oi.check_step(wrong[-1], ref64[-1], cpu32[-1], kinds=("params",))
        print(f"  {mistake}: worst err / bound on the parameters = {worst:.1f}")
        assert misses, mistake


def test_reference_skips_a_nonfinite_step_and_leaves_out_missing_gradients():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(7, generator=gen), torch.randn(3, generator=gen)]
    g1 = [torch.randn(7, generator=gen), torch.randn(3, generator=gen)]
    bad = [g1[0].clone(), g1[1].clone()]
    bad[1][2] = float("inf")
    g3 = [torch.randn(7, generator=gen), None]
    h = optim.adamw_reference(params, [g1, bad, g3], lr=1e-2, skip_nonfinite=True)
    assert [s["applied"] for s in h] == [1, 1, 2] and [s["skipped"] for s in h] == [0, 1, 1]
    assert h[1]["skip"] and all(torch.equal(a, b) for k in oi.KINDS for a, b in zip(h[0][k], h[1][k]))
    assert torch.equal(h[2]["params"][1], h[1]["params"][1]) and not torch.equal(h[2]["params"][0], h[1]["params"][0])
    # the same two applied steps without the bad one in between
    plain = optim.adamw_reference(params, [g1, g3], lr=1e-2)
    assert all(torch.equal(a, b) for k in oi.KINDS for a, b in zip(h[2][k], plain[1][k]))
    assert plain[0]["norm2"] is None and plain[0]["clip"] == 1.0
    nan = [g1[0].clone(), g1[1].clone()]
    nan[0][0] = float("nan")
    assert optim.adamw_reference(params, [nan], skip_nonfinite=True)[0]["skip"]
    assert not optim.adamw_reference(params, [nan], skip_nonfinite=False)[0]["skip"]


# --------------------------------------------------------------------------- the constructor's refusals
def test_constructor_refusals():
    def p(*shape, dtype=torch.float32, device="cpu"):
        return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype, device=device))

    F = optim.FusedAdamW
    with pytest.raises(ValueError, match="parameter groups"):
        F([{"params": [p(3)]}, {"params": [p(4)]}])
    with pytest.raises(ValueError, match="fp32 only"):
        F([p(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="fp32 only"):
        F([p(3), p(3, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="contiguous"):
        F([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="one device only"):
        F([p(3), p(3, device="meta")])
    with pytest.raises(ValueError, match="GPU only"):
        F([p(3)])
    for kw in ({"amsgrad": True}, {"maximize": True}):
        with pytest.raises(ValueError, match="amsgrad and maximize"):
            F([p(3)], **kw)
        with pytest.raises(ValueError, match="amsgrad and maximize"):
            F([dict(params=[p(3)], **kw)])
    for kw in ({"lr": -1e-3}, {"eps": -1e-8}, {"weight_decay": -0.01}, {"betas": (1.0, 0.999)}, {"betas": (0.9, 1.0)},
               {"betas": (-0.1, 0.999)}, {"betas": (0.9,)}, {"lr": float("nan")}, {"max_grad_norm": 0.0},
               {"max_grad_norm": -1.0}, {"max_grad_norm": float("inf")}):
        with pytest.raises(ValueError, match="FusedAdamW"):
            F([p(3)], **kw)
    with pytest.raises(ValueError):
        F([])                                            # torch's own refusal of an empty parameter list
