"""Inputs, float64 reference, fp32 yardstick, the tiled restatement and the planted mistakes of the tests of the
ragged-batch attention of csrc/attn_train.hip (test_attn_rows_host.py on the host, test_gpu_attn_rows.py on the
device).  torch-CPU only: both tests build the same seeded cases from here.  Shaped like mhsa_f64_inputs.py, whose value
regimes (its ``_draw``), sentinel and bound are reused; nothing here defines a tolerance of its own.

The operation (avsum_amd.attn): per sequence v (rows offsets[v] .. offsets[v + 1]) and head h, alpha = 1 / sqrt(D),

    S = alpha Q K^T   L = logsumexp_k S   P = exp(S - L)   O = P V   delta = rowsum(dO o O)
    dV = P^T dO   dP = dO V^T   dS = alpha P o (dP - delta)   dQ = dS K   dK = dS^T Q

Cases (``specs``): heads = 2, D in 64 / 128 / 256; the ragged batch LENGTHS = (1, 33, 17, 64, 129, 257) in every regime of
mhsa_f64_inputs but tiny_v (an f16x2 regime) - ``twins`` on TWIN_LENGTHS, where sequence 2 is a copy of sequence 0 and
sequence 4 a copy of sequence 1 (q, k, v and dctx), and query rows i and i + 16 of every sequence are copies too - and
one sequence of 1031 rows (33 tiles of 32, the last partial; 9 forward tiles of 128) for the regimes whose behaviour
changes with the number of tiles.

Layout of a case (``buffers``).  GUARD_FRONT guard rows in front of the first sequence, GUARD_BACK behind the last; the
offsets start at GUARD_FRONT.  Q, K, V live in buffers of their own [rows, E + 12], the heads from column 4; dctx, ctx,
dq, dk, dv in [rows, E + 8] from column 4; lse and delta are [rows, heads].  Every other entry - pad columns, guard rows,
and the whole of every output buffer before the launch - holds SENTINEL.

References and bound.  ``bundle(spec)``: ``ref`` = attn.mhsa_rows_reference in float64 on the fp32 inputs, ``yard`` the
same in float32 (the e32 of scorer_f64_inputs.compare: bound = 4 e32 + 8 eps32 max(1, max|ref|)).  The two gradient
kernels are handed lse and delta: ``lse32`` / ``delta32`` are the float64 values rounded to fp32, and ``refg`` / ``yardg``
are float64 / float32 evaluations of the gradient formulas ON those handed values, so that neither a forward error nor
the rounding of the handed values is charged to the kernel under test.  The delta kernel is handed ``ctx32`` (the float64
ctx rounded); its reference ``delta_ref`` / ``delta_yard`` is rowsum(dctx o ctx32) in float64 / float32.

``restate(case, handed, mistake)`` is the backward in the kernels' tiled form in fp32: tiles of 32 queries x 32 keys, S
and dP as the sum over the waves' head-dim slices in the fixed order w = 0, 1, .., P and dS masked for phantom rows and
columns, dK / dV accumulated over the query tiles in order, dQ over the key tiles.  The planted mistakes (MISTAKES) are
made in that form; NOTICED_BY names, per mistake, the case at which the host test shows it to lie outside the bound.
INERT names the one the bound cannot see (see test_attn_rows_host.py)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import mhsa_f64_inputs as mfi
from scorer_f64_inputs import EPS32, SENTINEL, compare  # noqa: F401  (one definition of the bound, shared)

HEADS = 2
HEAD_DIMS = mfi.HEAD_DIMS
LENGTHS = (1, 33, 17, 64, 129, 257)
TWIN_LENGTHS = (33, 17, 33, 64, 17)
TWIN_SEQS = ((0, 2), (1, 4))
LONG = (1031,)
REGIMES = tuple(r for r in mfi.REGIMES if r != "tiny_v")
LONG_REGIMES = ("flat", "peaked", "ramp_up", "ramp_down")
GUARD_FRONT, GUARD_BACK = 3, 2
COL0, PAD_IN, PAD_OUT = 4, 12, 8
TILE = 32

MISTAKES = ("delta_dropped", "alpha_missing_in_ds", "max_for_lse", "phantom_queries_counted", "phantom_keys_counted",
            "boundary_ignored", "wrong_head_v", "ds_not_transposed", "wave_dependent_order")
# mistake -> spec.  All are looked for on the flat ragged batch: its first sequence is ONE row (31 phantom rows of the
# neighbour in its only tile), its softmax is flat (so the row sum l, which max_for_lse leaves out, is about T) and
# neighbouring sequences weigh alike (so a neighbour's keys are not drowned by a peak).
_FLAT64 = (64, LENGTHS, "flat")
NOTICED_BY = {m: _FLAT64 for m in MISTAKES if m != "wave_dependent_order"}
# adding the waves' partial tiles in another order moves roundings, nothing else: no bound on the VALUES can see it
INERT = {"wave_dependent_order": _FLAT64}


def waves_of(d):
    """Waves of a gradient workgroup = head-dim slices of a tile product: avsa_bwd_shape of csrc/attn_train.hip."""
    return 2 if d == 64 else 4


def specs(d):
    """[(d, lengths, regime)] of one head dim."""
    out = [(d, TWIN_LENGTHS if regime == "twins" else LENGTHS, regime) for regime in REGIMES]
    return out + [(d, LONG, regime) for regime in LONG_REGIMES]


def label(spec):
    d, lengths, regime = spec
    return f"D={d} lengths={','.join(map(str, lengths))} {regime}"


def make_case(spec):
    """The seeded case of a spec: q, k, v, dctx fp32 [R, E] (the sequences one after another, no guard rows) and the
    layout numbers; ``offsets0`` start at 0, ``offsets`` at GUARD_FRONT."""
    d, lengths, regime = spec
    assert d in HEAD_DIMS and regime in REGIMES
    e = HEADS * d
    parts = []
    for i, t in enumerate(lengths):
        seed = 77000 + 100003 * REGIMES.index(regime) + 7919 * d + 31 * t + 7 * i
        g = torch.Generator().manual_seed(seed)
        q, k, v = (x.reshape(t, e) for x in mfi._draw("flat" if regime == "twins" else regime, d, t, 1, HEADS, g))
        parts.append([q, k, v, torch.randn(t, e, generator=g)])
    twin_rows = []
    if regime == "twins":
        for a, b in TWIN_SEQS:
            parts[b] = [x.clone() for x in parts[a]]
        for i, t in enumerate(lengths):
            for r in range(min(16, t - 16)):
                for x in parts[i]:
                    x[r + 16] = x[r]
                twin_rows.append((i, r, r + 16))
    q, k, v, dctx = (torch.cat([p[j] for p in parts]).contiguous() for j in range(4))
    offsets0 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = int(offsets0[-1])
    return SimpleNamespace(spec=spec, d=d, e=e, heads=HEADS, lengths=tuple(lengths), regime=regime, q=q, k=k, v=v,
                           dctx=dctx, rows=rows, offsets0=offsets0, offsets=offsets0 + GUARD_FRONT,
                           total_rows=GUARD_FRONT + rows + GUARD_BACK, ld=e + PAD_IN, ldo=e + PAD_OUT, col0=COL0,
                           twin_seqs=TWIN_SEQS if regime == "twins" else (), twin_rows=twin_rows, label=label(spec))


# --------------------------------------------------------------------------- buffers
def wide(case, x=None, pad=PAD_OUT):
    """A [total_rows, E + pad] buffer of SENTINEL with ``x`` [R, E] (bits, not values) in rows GUARD_FRONT .. and columns
    COL0 .. ; without ``x``: all SENTINEL (an output buffer before the launch)."""
    buf = torch.full((case.total_rows, case.e + pad), SENTINEL)
    if x is not None:
        buf.view(torch.int32)[GUARD_FRONT:GUARD_FRONT + case.rows, COL0:COL0 + case.e] = x.contiguous().view(torch.int32)
    return buf


def narrow(case, x=None):
    """A [total_rows, heads] buffer of SENTINEL with ``x`` [R, heads] in rows GUARD_FRONT .. (lse, delta)."""
    buf = torch.full((case.total_rows, case.heads), SENTINEL)
    if x is not None:
        buf[GUARD_FRONT:GUARD_FRONT + case.rows] = x
    return buf


def inner(case, buf):
    """The [R, E] (or [R, heads]) block of a wide (narrow) buffer that the kernels own."""
    rows = buf[GUARD_FRONT:GUARD_FRONT + case.rows]
    return rows if buf.shape[1] == case.heads else rows[:, COL0:COL0 + case.e]


def untouched(case, buf):
    """True when everything of a wide / narrow buffer outside inner() still holds SENTINEL."""
    mask = torch.ones(buf.shape, dtype=torch.bool)
    if buf.shape[1] == case.heads:
        mask[GUARD_FRONT:GUARD_FRONT + case.rows] = False
    else:
        mask[GUARD_FRONT:GUARD_FRONT + case.rows, COL0:COL0 + case.e] = False
    return bool((buf[mask] == SENTINEL).all()) and bool(mask.any())


# --------------------------------------------------------------------------- references
def _reference(case, dtype, **handed):
    from avsum_amd import attn
    return attn.mhsa_rows_reference(case.q, case.k, case.v, case.offsets0, case.heads, dctx=case.dctx, dtype=dtype, **handed)


def _delta_of(case, ctx32, dtype):
    prod = (case.dctx.to(dtype) * ctx32.to(dtype)).reshape(case.rows, case.heads, case.d)
    return prod.sum(-1)


@functools.lru_cache(maxsize=None)
def bundle(spec):
    """Everything the tests of a spec share, computed once per process; none of it is modified by a test."""
    case = make_case(spec)
    ref, yard = _reference(case, torch.float64), _reference(case, torch.float32)
    lse32, delta32, ctx32 = ref.lse.float(), ref.delta.float(), ref.ctx.float()
    handed = dict(lse=lse32, delta=delta32)
    return SimpleNamespace(case=case, ref=ref, yard=yard, lse32=lse32, delta32=delta32, ctx32=ctx32,
                           refg=_reference(case, torch.float64, **handed), yardg=_reference(case, torch.float32, **handed),
                           delta_ref=_delta_of(case, ctx32, torch.float64), delta_yard=_delta_of(case, ctx32, torch.float32))


def check_grads(b, dq, dk, dv):
    """{name: (ok, err, e32, bound)} of three gradients [R, E] against refg with yardg as yardstick."""
    return {n: compare(g, getattr(b.refg, n), getattr(b.yardg, n)) for n, g in (("dq", dq), ("dk", dk), ("dv", dv))}


# --------------------------------------------------------------------------- the tiled restatement
def _pad_rows(x, lo, n):
    """Rows lo .. lo + n of ``x``, zeros where they run past its end."""
    out = x.new_zeros((n,) + tuple(x.shape[1:]))
    have = max(0, min(n, x.shape[0] - lo))
    out[:have] = x[lo:lo + have]
    return out


def _tile_products(a, b, d, order):
    """[na, nb, 32, 32]: a_tile @ b_tile^T for every pair of 32-row tiles, as the sum over the waves' head-dim slices in
    ``order``."""
    nw = waves_of(d)
    ds = d // nw
    at, bt = a.reshape(-1, TILE, d), b.reshape(-1, TILE, d)
    total = None
    for w in order:
        part = torch.einsum("aid,bjd->abij", at[..., w * ds:(w + 1) * ds], bt[..., w * ds:(w + 1) * ds])
        total = part if total is None else total + part
    return total


def _backward_tiles(qs, ks, d, mistake, mask_q=True, mask_k=True, order=None):
    """One (sequence, head) in the tiled form.  qs = (q, do, lse, delta, valid rows) of the query side, ks = (k, v, valid
    rows) of the key side, each padded to a multiple of 32 rows.  -> (dq [Tq_pad, D], dk, dv [Tk_pad, D])."""
    q, do, lse, delta, nq = qs
    k, v, nk = ks
    sqrt_d = torch.tensor(math.sqrt(d), dtype=torch.float32)
    order = list(range(waves_of(d))) if order is None else order
    s = _tile_products(q, k, d, order) / sqrt_d                                    # [nqt, nkt, 32(q), 32(key)]
    dp = _tile_products(do, v, d, order)
    nqt, nkt = s.shape[:2]
    big = lse.reshape(nqt, 1, TILE, 1)
    if mistake == "max_for_lse":
        big = (s.permute(0, 2, 1, 3).reshape(nqt, TILE, -1).max(-1).values).reshape(nqt, 1, TILE, 1)
    p = torch.exp(s - big)
    ok = torch.ones(nqt, nkt, TILE, TILE, dtype=torch.bool)
    if mask_q:
        ok &= (torch.arange(nqt * TILE) < nq).reshape(nqt, 1, TILE, 1)
    if mask_k:
        ok &= (torch.arange(nkt * TILE) < nk).reshape(1, nkt, 1, TILE)
    p = torch.where(ok, p, torch.zeros(()))
    dl = torch.zeros(()) if mistake == "delta_dropped" else delta.reshape(nqt, 1, TILE, 1)
    ds = p * (dp - dl)
    if mistake != "alpha_missing_in_ds":
        ds = ds / sqrt_d
    qt, dot, kt = q.reshape(nqt, TILE, d), do.reshape(nqt, TILE, d), k.reshape(nkt, TILE, d)
    dk, dv, dq = torch.zeros(nkt, TILE, d), torch.zeros(nkt, TILE, d), torch.zeros(nqt, TILE, d)
    for i in range(nqt):                 # the dK/dV workgroups sweep the query tiles in order
        dv = dv + p[i].transpose(-1, -2) @ dot[i]
        dk = dk + (ds[i] if mistake == "ds_not_transposed" else ds[i].transpose(-1, -2)) @ qt[i]
    for j in range(nkt):                 # the dQ workgroups sweep the key tiles in order
        dq = dq + ds[:, j] @ kt[j]
    return dq.reshape(-1, d), dk.reshape(-1, d), dv.reshape(-1, d)


def restate(case, lse32, delta32, mistake=None):
    """(dq, dk, dv) fp32 [R, E]: the two gradient kernels' arithmetic in their tiled form on the CPU, on the handed lse
    and delta; ``mistake``: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    d, e = case.d, case.e
    out = [torch.zeros(case.rows, e) for _ in range(3)]
    for lo, hi in zip(case.offsets0[:-1], case.offsets0[1:]):
        lo, t = int(lo), int(hi - lo)
        tp = -(-t // TILE) * TILE
        for h in range(case.heads):
            c = slice(h * d, (h + 1) * d)
            vc = slice(0, d) if mistake == "wrong_head_v" else c
            # a tile's rows past the sequence's end: zeros, as the kernels stage them ...
            own = lambda x, n=tp: _pad_rows(x[lo:lo + t], 0, n)
            qs = (own(case.q[:, c]), own(case.dctx[:, c]), own(lse32[:, h]), own(delta32[:, h]), t)
            ks = (own(case.k[:, c]), own(case.v[:, vc]), t)
            if mistake == "wave_dependent_order":
                # every wave starts the sum at its own partial: wave 1's order stands for the slice it owns
                dq, dk, dv = _backward_tiles(qs, ks, d, None)
                nw, dsl = waves_of(d), d // waves_of(d)
                for w in range(1, nw):
                    alt = _backward_tiles(qs, ks, d, None, order=[(w + i) % nw for i in range(nw)])
                    for full, part in zip((dq, dk, dv), alt):
                        full[:, w * dsl:(w + 1) * dsl] = part[:, w * dsl:(w + 1) * dsl]
            else:
                dq, dk, dv = _backward_tiles(qs, ks, d, mistake)
            # ... the three boundary mistakes read what lies behind the end instead: the neighbour's rows
            nb = lambda x, n=tp: _pad_rows(x, lo, n)
            if mistake == "phantom_queries_counted":
                qs_nb = (nb(case.q[:, c]), nb(case.dctx[:, c]), nb(lse32[:, h]), nb(delta32[:, h]), tp)
                _, dk, dv = _backward_tiles(qs_nb, ks, d, None, mask_q=False)
            elif mistake == "phantom_keys_counted":
                dq, _, _ = _backward_tiles(qs, (nb(case.k[:, c]), nb(case.v[:, c]), tp), d, None, mask_k=False)
            elif mistake == "boundary_ignored":
                # the sweeps run over the whole batch's rows: every sequence's keys are attended
                rp = -(-case.rows // TILE) * TILE
                al = lambda x: _pad_rows(x, 0, rp)
                dq, _, _ = _backward_tiles(qs, (al(case.k[:, c]), al(case.v[:, c]), case.rows), d, None)
                qs_all = (al(case.q[:, c]), al(case.dctx[:, c]), al(lse32[:, h]), al(delta32[:, h]), case.rows)
                _, dk, dv = _backward_tiles(qs_all, ks, d, None)
            for full, part in zip(out, (dq, dk, dv)):
                full[lo:lo + t, c] = part[:t]
    return tuple(out)

