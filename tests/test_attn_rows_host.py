"""CPU-side checks of the ragged-batch attention (libavsum_attn.so, avsum_amd/attn.py, ops.AttnTable): the fourth header
and the binding derived from it, the library's exports, every refusal before any launch, AttnTable against hand-built
tables, the tiled fp32 restatement of the backward against float64 on every case of attn_rows_inputs, and the planted
mistakes at their NOTICED_BY cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attn_rows_inputs as ari
from avsum_amd import _attn_abi, _header, attn, ops, ragged

PKG = os.path.dirname(os.path.dirname(_attn_abi.LIB_PATH))

_QKV = ["float*", "float*", "float*", "int64_t"]                                     # d_q, d_k, d_v, ld
_BATCH = ["int64_t*", "int64_t*", "int", "int32_t*", "int64_t", "int", "int"]       # h_offsets .. head_dim
_GRAD = _QKV + ["float*", "int64_t", "float*", "float*"] + _BATCH                    # + d_dctx, lddo, d_lse, d_delta
PINNED = {
    "avsa_abi_version": ("int", []),
    "avsa_last_error": ("char*", []),
    "avsa_mhsa_rows_fwd_f32": ("int", _QKV + _BATCH + ["float*", "int64_t", "float*", "avsa_stream_t"]),
    "avsa_mhsa_rows_delta_f32": ("int", ["float*", "int64_t", "float*", "int64_t", "int64_t*", "int", "int", "int", "float*",
                                         "avsa_stream_t"]),
    "avsa_mhsa_rows_dkv_f32": ("int", _GRAD + ["float*", "float*", "int64_t", "avsa_stream_t"]),
    "avsa_mhsa_rows_dq_f32": ("int", _GRAD + ["float*", "int64_t", "avsa_stream_t"]),
}
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


# --------------------------------------------------------------------------- header, binding, library
def test_attn_header_parses_and_signatures_are_pinned():
    header = _attn_abi.load_header()
    assert header.prototypes == PINNED
    assert _attn_abi.declared_symbols() == sorted(PINNED)
    c = header.constants
    assert (c["AVSA_ABI_VERSION"], c["AVSA_FWD_TILE"], c["AVSA_BWD_TILE"], c["AVSA_TILE_COLS"]) == (1, 128, 32, 2)
    assert (c["AVSA_MAX_HEADS"], c["AVSA_MAX_ROWS"], c["AVSA_DELTA_GROUPS"]) == (65535, (1 << 31) - 1, 16384)
    assert (c["AVSA_OK"], c["AVSA_E_ARG"], c["AVSA_E_SHAPE"], c["AVSA_E_ALIGN"], c["AVSA_E_HIP"]) == (0, -1, -2, -3, -4)
    # the binding is derived, not typed: it is the header's reader applied to the header
    assert _attn_abi._SIGNATURES == header.signatures()
    assert _attn_abi._SIGNATURES["avsa_last_error"] == (ctypes.c_char_p, [])
    assert _attn_abi._SIGNATURES["avsa_mhsa_rows_dq_f32"] == (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    source = open(os.path.join(PKG, "_attn_abi.py")).read()
    assert not re.search(r"c_int|c_void_p|c_float|argtypes\s*=\s*\[", source)
    # the python side takes its sizes from the header
    assert (_attn_abi.FWD_TILE, _attn_abi.BWD_TILE, attn.FWD_TILE, attn.BWD_TILE) == (128, 32, 128, 32)
    assert (ragged.ATTN_FWD_TILE, ragged.ATTN_BWD_TILE, ops.ATTN_FWD_TILE, ops.ATTN_BWD_TILE) == (128, 32, 128, 32)
    assert ops.AttnTable is ragged.AttnTable and "AttnTable" in ops.__all__
    # the main header is untouched: no avsa_ name in it, no AVS_ name defined again in the new one
    main = _header.load()
    assert len(main.prototypes) == 96 and main.constants["AVS_ABI_VERSION"] == 5
    assert not [n for n in list(main.prototypes) + list(main.constants) if n.lower().startswith("avsa_")]
    assert not set(c) & set(main.constants)
    for path in (_attn_abi.HEADER_PATH, os.path.join(PKG, "csrc", "attn_train.hip")):
        assert not re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AVS_\w+)", open(path).read(), flags=re.M), path


def test_attn_library_exports_exactly_the_headers_functions():
    lib = _attn_abi.lib()
    assert lib.avsa_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _attn_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(avsa_[a-z0-9_]+)\b", out)) == set(PINNED)
    assert not re.findall(r"\b(avs[io]?_[a-z0-9_]+)\b", out)            # nothing of the other three libraries is defined ...
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _attn_abi.LIB_PATH], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined
    assert not re.findall(r"\b(avs[aio]?_[a-z0-9_]+)\b", undefined)     # ... and nothing of them is wanted
    for name, (res, args) in _attn_abi._SIGNATURES.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name


def test_attn_source_is_outside_srcs_and_shares_the_forward_body():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "attn_train.hip" not in srcs and "attention.hip" in srcs
    assert re.search(r"^all: \$\(ATTN_LIB\)$", make, flags=re.M)
    rule = re.search(r"^\.\./build/attn_train\.o:.*\n(?:\t.*\n)*", make, flags=re.M).group(0)
    assert "$(HIPCC) $(CXXFLAGS) -c" in rule and "mhsa_flash_body.h" in rule.splitlines()[0]
    assert "$(ATTN_LIB)" in re.search(r"^clean:\n\t(.*)$", make, flags=re.M).group(1)
    text = open(os.path.join(PKG, "csrc", "attn_train.hip")).read()
    assert re.search(r"^static thread_local char g_err\[", text, flags=re.M)
    assert not re.search(r"\bavs_set_error\b|\bAVS_REQUIRE\b|\bAVS_CHECK_LAUNCH\b|avs_internal\.h", text)
    assert not re.search(r"\batomic(Add|Exch|CAS|Max|Min)\b|__hip_atomic|__atomic_fetch", text)
    assert not re.search(r"\bhipMalloc|\bhipFree|hipDeviceSynchronize|hipStreamSynchronize|hipMemcpy", text)
    # one text of the fp32 forward: both kernels call the shared body, neither holds a copy of it
    body = open(os.path.join(PKG, "csrc", "mhsa_flash_body.h")).read()
    dense = open(os.path.join(PKG, "csrc", "attention.hip")).read()
    assert len(re.findall(r"void flash_mhsa_body\(", body)) == 1
    for src in (text, dense):
        assert '#include "mhsa_flash_body.h"' in src and len(re.findall(r"flash_mhsa_body<", src)) == 1
        assert "m_run" not in src.split("flash_mhsa_h2q16_kernel")[0]
    ignored = subprocess.run(["git", "-C", os.path.dirname(PKG), "check-ignore", "-q", _attn_abi.LIB_PATH], capture_output=True)
    assert ignored.returncode in (0, 128)                            # ignored (128: not a git work tree)


# --------------------------------------------------------------------------- validation before any launch
P = 4096          # a well-aligned address that is never dereferenced: every call below is refused first


def _off(*values):
    return (ctypes.c_int64 * len(values))(*values)


def _calls(lib, off=None, nseq=2, heads=2, d=64, ld=128, ldo=128, lddo=128, ldg=128, nfwd=2, nbwd=3, ptr=P, out=P,
           small=P, d_off=P, tiles=P):
    """The four entry points on one batch description (default: sequences of 33 and 17 rows, every argument fine)."""
    off = _off(0, 33, 50) if off is None else off
    return [
        ("fwd", lambda: lib.avsa_mhsa_rows_fwd_f32(ptr, ptr, ptr, ld, off, d_off, nseq, tiles, nfwd, heads, d, out, ldo,
                                                   small, None)),
        ("delta", lambda: lib.avsa_mhsa_rows_delta_f32(ptr, lddo, ptr, ldo, off, nseq, heads, d, small, None)),
        ("dkv", lambda: lib.avsa_mhsa_rows_dkv_f32(ptr, ptr, ptr, ld, ptr, lddo, small, small, off, d_off, nseq, tiles,
                                                   nbwd, heads, d, out, out, ldg, None)),
        ("dq", lambda: lib.avsa_mhsa_rows_dq_f32(ptr, ptr, ptr, ld, ptr, lddo, small, small, off, d_off, nseq, tiles, nbwd,
                                                 heads, d, out, ldg, None)),
    ]


def test_attn_validation_before_launch_needs_no_gpu():
    """Every refusal of include/avsum_attn.h comes with its status and a message before any HIP call (no call here could
    launch: each has a fault the checks find first)."""
    lib = _attn_abi.lib()

    def refused(code, word, only=None, **kw):
        for name, call in _calls(lib, **kw):
            if only is None or name in only:
                assert call() == code, (name, kw, lib.avsa_last_error())
                assert word in lib.avsa_last_error(), (name, lib.avsa_last_error())

    tiled = ("fwd", "dkv", "dq")
    refused(E_ARG, b"at least one sequence", nseq=0)                               # V >= 1
    refused(E_ARG, b"h_offsets is null", off=ctypes.POINTER(ctypes.c_int64)())
    refused(E_SHAPE, b"is empty", off=_off(0, 33, 33))                             # every T_v >= 1
    refused(E_SHAPE, b"is empty", off=_off(0, 33, 20))                             # (decreasing)
    refused(E_SHAPE, b"negative row offset", off=_off(-1, 33, 50))
    refused(E_SHAPE, b"fewer than 2^31 rows", off=_off(0, 33, 1 << 31))            # R < 2^31
    refused(E_SHAPE, b"fewer than 2^31 rows", off=_off((1 << 31) - 1, 1 << 31), nseq=1)
    for d in (0, 32, 96, 512, -64):
        refused(E_SHAPE, b"head_dim", d=d)
    for heads in (0, -1, 65536):
        refused(E_SHAPE, b"heads =", heads=heads)
    refused(E_SHAPE, b"row stride ld ", only=tiled, ld=127)                        # below heads * head_dim
    refused(E_SHAPE, b"row stride ld ", only=tiled, ld=130)                        # no multiple of 4 floats
    refused(E_SHAPE, b"row stride ldo", only=("fwd", "delta"), ldo=124)
    refused(E_SHAPE, b"row stride ldo", only=("fwd", "delta"), ldo=134)
    refused(E_SHAPE, b"row stride lddo", only=("delta", "dkv", "dq"), lddo=64)
    refused(E_SHAPE, b"row stride ldg", only=("dkv", "dq"), ldg=126)
    refused(E_SHAPE, b"the offsets give 2 tiles", only=("fwd",), nfwd=3)           # tables of another batch
    refused(E_SHAPE, b"the offsets give 3 tiles", only=("dkv", "dq"), nbwd=2)
    refused(E_ARG, b"null pointer", only=tiled, tiles=None)
    refused(E_ARG, b"null pointer", ptr=None)                                      # q, k, v, dctx, ctx
    refused(E_ARG, b"null pointer", only=tiled, out=None)                          # ctx, dk, dv, dq
    refused(E_ARG, b"null pointer", small=None)                                    # lse, delta
    refused(E_ARG, b"null pointer", only=tiled, d_off=None)
    refused(E_ALIGN, b"16-byte aligned", ptr=P + 4)
    refused(E_ALIGN, b"16-byte aligned", only=tiled, out=P + 8)
    refused(E_ALIGN, b"aligned", small=P + 2)
    refused(E_ALIGN, b"aligned", only=tiled, d_off=P + 4)
    refused(E_ALIGN, b"4-byte aligned", only=tiled, tiles=P + 2)
    # the limits themselves pass the batch checks: the next check (a null pointer) is what refuses
    refused(E_ARG, b"null pointer", off=_off((1 << 31) - 2, (1 << 31) - 1), nseq=1, nfwd=1, nbwd=1, heads=65535, d=256,
            ld=65535 * 256, ldo=65535 * 256, lddo=65535 * 256, ldg=65535 * 256, ptr=None)
    with pytest.raises(_attn_abi.AvsaError, match="status -2.*head_dim = 96"):
        _attn_abi.check(_calls(lib, d=96)[0][1](), "avsa_mhsa_rows_fwd_f32")


def test_attn_wrappers_refuse_host_tensors_and_host_tables():
    table = ops.AttnTable([0, 33, 50], device="cpu")
    x = torch.zeros(50, 128)
    for call in (lambda: attn.mhsa_rows_fwd(x, x, x, table, 2), lambda: attn.mhsa_rows_delta(x, x, table, 2),
                 lambda: attn.mhsa_rows_dq(x, x, x, x, x, x, table, 2), lambda: attn.mhsa_rows_dkv(x, x, x, x, x, x, table, 2)):
        with pytest.raises(ValueError, match="mhsa_rows_.*device tensor"):
            call()
    from avsum_amd.models.attention import MultiHeadSelfAttention
    m = MultiHeadSelfAttention(128, 2)
    assert m.fused_backward is False
    with pytest.raises(RuntimeError, match="HIP path only"):
        m.forward_rows(x, [0, 33, 50])


# --------------------------------------------------------------------------- AttnTable
def test_attn_table_against_hand_built_tables():
    t = ops.AttnTable([3, 4, 37, 54, 118, 247, 504], device="cpu")                 # lengths 1, 33, 17, 64, 129, 257
    assert (t.nseq, t.first_row, t.rows, t.max_t) == (6, 3, 504, 257) and t.lengths.tolist() == [1, 33, 17, 64, 129, 257]
    assert t.fwd_tiles.dtype == np.int32 and t.bwd_tiles.dtype == np.int32
    assert t.fwd_tiles.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [4, 1], [5, 0], [5, 1], [5, 2]]
    want = [[0, 0], [1, 0], [1, 1], [2, 0], [3, 0], [3, 1]] + [[4, k] for k in range(5)] + [[5, k] for k in range(9)]
    assert t.bwd_tiles.tolist() == want and (t.n_fwd, t.n_bwd) == (9, 20)
    assert t.offsets_t.dtype == torch.int64 and t.offsets_t.tolist() == [3, 4, 37, 54, 118, 247, 504]
    assert t.fwd_tiles_t.device.type == "cpu" and t.fwd_tiles_t.tolist() == t.fwd_tiles.tolist()
    assert t.bwd_tiles_t.tolist() == want and t.offsets.flags["C_CONTIGUOUS"] and t.offsets.dtype == np.int64
    one = ops.AttnTable([0, 1031], device="cpu")
    assert one.fwd_tiles.tolist() == [[0, k] for k in range(9)] and one.bwd_tiles.tolist() == [[0, k] for k in range(33)]
    exact = ops.AttnTable([0, 128, 160], device="cpu")                             # whole tiles: no empty tail tile
    assert exact.fwd_tiles.tolist() == [[0, 0], [1, 0]] and exact.n_bwd == 5
    u = ops.AttnTable.uniform(3, 40, device="cpu")
    assert u.offsets.tolist() == [0, 40, 80, 120] and u.n_fwd == 3 and u.n_bwd == 6
    for bad, word in (([0], "batch is empty"), ([], "batch is empty"), ([0, 5, 5], "at least 1"), ([0, 5, 3], "decrease"),
                      ([-1, 4], "negative"), ([0, 1 << 31], "at most 2147483647")):
        with pytest.raises(ValueError, match=f"AttnTable.*{word}"):
            ops.AttnTable(bad, device="cpu")


# --------------------------------------------------------------------------- restatement and planted mistakes
ALL_SPECS = [spec for d in ari.HEAD_DIMS for spec in ari.specs(d)]


@pytest.mark.parametrize("spec", ALL_SPECS, ids=ari.label)
def test_tiled_restatement_within_the_bound_of_float64(spec):
    """The backward in the kernels' tiled form, in fp32 on the CPU: inside 4 e32 + 8 eps32 scale of float64 at every
    case - the bound accepts a correct kernel of this shape.  The yardsticks themselves are checked too: the handed-value
    references equal the plain ones to rounding, twins are twins."""
    b = ari.bundle(spec)
    case = b.case
    got = ari.restate(case, b.lse32, b.delta32)
    for name, (ok, err, e32, bound) in ari.check_grads(b, *got).items():
        print(f"{case.label} {name}: err {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
        assert ok, (case.label, name, err, bound)
    for name in ("dq", "dk", "dv"):        # handing over rounded lse / delta moves the reference by rounding only
        r, rg = getattr(b.ref, name), getattr(b.refg, name)
        assert (r - rg).abs().max().item() <= 64 * ari.EPS32 * max(1.0, r.abs().max().item(), b.ref.lse.abs().max().item()) \
            * max(1.0, r.abs().max().item())
    assert torch.equal(b.refg.ctx, b.ref.ctx) and torch.equal(b.refg.lse, b.ref.lse)
    o = case.offsets0
    for i, j in case.twin_seqs:
        for x in (b.ref.ctx, b.ref.dq, b.ref.dk, b.ref.dv, got[0], got[1], got[2]):
            assert torch.equal(x[o[i]:o[i + 1]], x[o[j]:o[j + 1]])
    assert (case.regime == "twins") == bool(case.twin_seqs) == bool(case.twin_rows)


def test_planted_mistakes_fall_outside_the_bound_at_their_cases():
    assert set(ari.NOTICED_BY) | set(ari.INERT) == set(ari.MISTAKES) and not set(ari.NOTICED_BY) & set(ari.INERT)
    for mistake, spec in ari.NOTICED_BY.items():
        b = ari.bundle(spec)
        checks = ari.check_grads(b, *ari.restate(b.case, b.lse32, b.delta32, mistake))
        print(mistake, {n: f"err {c[1]:.2e} bound {c[3]:.2e}" for n, c in checks.items()})
        assert not all(c[0] for c in checks.values()), mistake
    # which gradient shows which mistake
    b = ari.bundle(ari.NOTICED_BY["phantom_keys_counted"])
    outside = lambda m: {n for n, c in ari.check_grads(b, *ari.restate(b.case, b.lse32, b.delta32, m)).items() if not c[0]}
    assert outside("phantom_keys_counted") == {"dq"} and outside("phantom_queries_counted") == {"dk", "dv"}
    assert outside("ds_not_transposed") == {"dk"} and outside("boundary_ignored") == {"dq", "dk", "dv"}
    assert outside("delta_dropped") == outside("alpha_missing_in_ds") == outside("wrong_head_v") == {"dq", "dk"}
    assert outside("max_for_lse") == {"dq", "dk", "dv"}


def test_the_order_of_the_partial_sums_is_not_visible_to_a_bound_on_values():
    """The ninth planted mistake, the waves' partial S and dP tiles added in an order that depends on the wave: it moves
    roundings of a sum of 2 or 4 terms and nothing else, so it stays inside the bound at every case - no tolerance can
    see it.  It IS other bits (shown here), which is what the kernels' fixed order is for: the bit-for-bit tests of
    test_gpu_attn_rows.py (batch invariance, twins, a second run) are where an order that is not fixed would show."""
    assert list(ari.INERT) == ["wave_dependent_order"]
    differs = False
    for d in ari.HEAD_DIMS:
        b = ari.bundle((d, ari.LENGTHS, "flat"))
        plain = ari.restate(b.case, b.lse32, b.delta32)
        wrong = ari.restate(b.case, b.lse32, b.delta32, "wave_dependent_order")
        assert all(c[0] for c in ari.check_grads(b, *wrong).values())
        differs |= any(not torch.equal(x, y) for x, y in zip(plain, wrong))
    assert differs
