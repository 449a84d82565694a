"""Inputs, float64 references and the error bound of the per-kernel scorer tests (test_lstm_f64_host.py on the host,
test_gpu_lstm_f64.py and test_gpu_scorer_small_f64.py on the device).  torch-CPU only: the host and the device tests
build the same seeded cases from here.

The bound (``compare``): a kernel's result must lie within ``4 * e32 + 8 * eps32 * scale`` of the float64 reference, where
e32 is the largest error of the SAME operation evaluated in fp32 on the CPU on the same inputs, and scale is
max(1, max|ref|) - for LSTM gradients max|ref dxproj| of the case.  The factor 4 is what a different summation order
(slices of the reduction added in ascending order, fmaf chains) and the device's expf / tanhf may cost over the CPU's
fp32; the floor keeps tiny cases (hidden 1), where e32 can come out as 0 by accident, from demanding more than fp32 has.

The fp32 restatement of the LSTM is oracle.scorer.lstm_recurrence in fp32 followed by ``lstm_backward``, the backward
through time written out step by step as the kernels compute it; ``mistake`` plants one deliberate error in it
(MISTAKES), which the bound has to notice at every hidden size the device tests run."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import scorer as osc

EPS32 = float(torch.finfo(torch.float32).eps)      # 2^-23
SENTINEL = -777.25                                 # exact in fp32; no result of these kernels comes near it
OUT_COL0, OUT_PAD = 4, 9                           # the recurrence's h goes to columns [4, 4 + ndir*H) of rows ndir*H + 9 wide

GENERIC_HIDDEN = (1, 3, 20, 33, 90, 255, 257, 300, 600, 1024)
ALL_HIDDEN = tuple(sorted(GENERIC_HIDDEN + (256,)))
COMMON_LENS = (0, 1, 2, 9)
H256_LENS = (700, 1, 0, 333, 2)
MISTAKES = ("c_prev_zero", "swap_forget_cell", "walk_forward", "drop_dh_carry")


# --------------------------------------------------------------------------- the bound
def compare(got, ref, cpu32, scale=None):
    """(ok, err, e32, bound) of ``got`` against the float64 ``ref`` with the fp32 CPU evaluation ``cpu32`` as yardstick.
    A non-finite ``got`` is never ok."""
    ref = ref.double()
    err = (got.double() - ref).abs().max().item() if ref.numel() else 0.0
    e32 = (cpu32.double() - ref).abs().max().item() if ref.numel() else 0.0
    if scale is None:
        scale = max(1.0, ref.abs().max().item() if ref.numel() else 0.0)
    bound = 4.0 * e32 + 8.0 * EPS32 * float(scale)
    return bool(err <= bound), err, e32, bound


# --------------------------------------------------------------------------- LSTM cases
def lstm_case(hidden, ndir=3, reverse_mask=0b010, lens=COMMON_LENS, first_row=2, tail_rows=1, seed=None, saturate=False,
              twins=None):
    """One launch: ``lens`` sequences laid out back to back from ``first_row``; xproj [rows, ndir*4H] ~ N(0, 1), W_hh
    [ndir, 4H, H] uniform in +-1/sqrt(H) (as tests/test_gpu_kernels.py draws it), dL/dh ``dout`` [rows, ndir*H + 9] with h in
    columns [4, 4 + ndir*H).  saturate: every third xproj column times 30 (sigmoid = 0 or 1, tanh = +-1 in fp32).
    twins=(a, b): sequence b gets the rows of sequence a (same length), xproj and dout."""
    g = torch.Generator().manual_seed(7000 + 13 * hidden + ndir if seed is None else seed)
    rows = first_row + sum(lens) + tail_rows
    xproj = torch.randn(rows, ndir * 4 * hidden, generator=g)
    if saturate:
        xproj[:, ::3] *= 30.0
    whh = (torch.rand(ndir, 4 * hidden, hidden, generator=g) - 0.5) * 2 / math.sqrt(hidden)
    ldo = ndir * hidden + OUT_PAD
    dout = torch.randn(rows, ldo, generator=g)
    seq_rows = first_row + np.cumsum([0] + list(lens)).astype(np.int64)
    if twins is not None:
        a, b = twins
        assert lens[a] == lens[b]
        xproj[seq_rows[b]:seq_rows[b + 1]] = xproj[seq_rows[a]:seq_rows[a + 1]]
        dout[seq_rows[b]:seq_rows[b + 1]] = dout[seq_rows[a]:seq_rows[a + 1]]
    in_seq = torch.zeros(rows, dtype=torch.bool)
    in_seq[first_row:first_row + sum(lens)] = True
    return SimpleNamespace(hidden=hidden, ndir=ndir, reverse_mask=reverse_mask, lens=tuple(lens), rows=rows, ldo=ldo,
                           out_col0=OUT_COL0, seq_rows=seq_rows, xproj=xproj, whh=whh, dout=dout, in_seq=in_seq)


def recurrences(case):
    """[(dir, reversed, r0, r1)] of a case, empty sequences included."""
    return [(d, bool((case.reverse_mask >> d) & 1), int(r0), int(r1))
            for d in range(case.ndir) for r0, r1 in zip(case.seq_rows[:-1], case.seq_rows[1:])]


def _blocks(case, dtype):
    h, n = case.hidden, case.ndir
    z = lambda cols: torch.zeros(case.rows, cols, dtype=dtype)
    return SimpleNamespace(out=z(n * h), gates=z(4 * n * h), cell=z(n * h), dxproj=z(4 * n * h))


def lstm_reference(case, backward=True):
    """float64: oracle.scorer.lstm_recurrence per (sequence, direction) and torch.autograd.grad for dL/dxproj.  Tensors
    [rows, ndir * ...] in the kernels' layouts (without the pad columns of out); rows outside the sequences are zero."""
    h = case.hidden
    res = _blocks(case, torch.float64)
    for d, rev, r0, r1 in recurrences(case):
        if r1 == r0:
            continue
        xp = case.xproj[r0:r1, 4 * h * d:4 * h * (d + 1)].double().requires_grad_(backward)
        with torch.set_grad_enabled(backward):
            hs, gs, cs = osc.lstm_recurrence(xp, case.whh[d].double(), rev)
        if backward:
            c0 = case.out_col0 + d * h
            res.dxproj[r0:r1, 4 * h * d:4 * h * (d + 1)] = torch.autograd.grad(hs, xp, case.dout[r0:r1, c0:c0 + h].double())[0]
        res.out[r0:r1, h * d:h * (d + 1)] = hs.detach()
        res.gates[r0:r1, 4 * h * d:4 * h * (d + 1)] = gs.detach()
        res.cell[r0:r1, h * d:h * (d + 1)] = cs.detach()
    return res


def lstm_backward(dout, gates, cell, w_hh, reverse, mistake=None):
    """Backward through time of one recurrence from its saved post-activation gates [T, 4H] and cell states [T, H], in
    their dtype: dL/dxproj [T, 4H] for dL/dh = dout [T, H].  The formulae of the kernels (csrc/train.hip), step by step."""
    t_len, hid = cell.shape
    dx = torch.zeros_like(gates)
    order = list(range(t_len - 1, -1, -1)) if reverse else list(range(t_len))     # rows in processing order
    dc_next = cell.new_zeros(hid)
    dh_next = cell.new_zeros(hid)
    w_t = w_hh.t().contiguous()
    for s in range(t_len - 1, -1, -1):
        row = order[s]
        c_prev = cell[order[s - 1]] if s > 0 else cell.new_zeros(hid)
        if mistake == "c_prev_zero" and s == t_len // 2 and 0 < s < t_len - 1:
            c_prev = cell.new_zeros(hid)
        i, f, g, o = gates[row].view(4, hid)
        tc = torch.tanh(cell[row])
        dh = dout[row] + dh_next
        d_o = dh * tc
        dc = dh * o * (1 - tc * tc) + dc_next
        d_i, d_g, d_f = dc * g, dc * i, dc * c_prev
        dc_next = dc * f
        ai, af, ag, ao = d_i * i * (1 - i), d_f * f * (1 - f), d_g * (1 - g * g), d_o * o * (1 - o)
        da = torch.cat([ai, ag, af, ao] if mistake == "swap_forget_cell" else [ai, af, ag, ao])
        dx[row] = da
        dh_next = w_t @ da
        if mistake == "drop_dh_carry":
            dh_next[hid // 2] = 0
    return dx


def lstm_restatement(case, dtype=torch.float32, mistake=None, saved=None, backward=True):
    """The case evaluated on the CPU in ``dtype`` (fp32: the yardstick of the bound): lstm_recurrence, then lstm_backward
    on its saved tensors - or on ``saved`` = (gates, cell) [rows, ...] where given (the backward on its own).
    ``mistake``: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    h = case.hidden
    res = _blocks(case, dtype)
    with torch.no_grad():
        for d, rev, r0, r1 in recurrences(case):
            if r1 == r0:
                continue
            if mistake == "walk_forward":
                rev = False
            w = case.whh[d].to(dtype)
            hs, gs, cs = osc.lstm_recurrence(case.xproj[r0:r1, 4 * h * d:4 * h * (d + 1)].to(dtype), w, rev)
            res.out[r0:r1, h * d:h * (d + 1)] = hs
            res.gates[r0:r1, 4 * h * d:4 * h * (d + 1)] = gs
            res.cell[r0:r1, h * d:h * (d + 1)] = cs
            if not backward:
                continue
            if saved is not None:
                gs, cs = saved[0][r0:r1, 4 * h * d:4 * h * (d + 1)].to(dtype), saved[1][r0:r1, h * d:h * (d + 1)].to(dtype)
            c0 = case.out_col0 + d * h
            res.dxproj[r0:r1, 4 * h * d:4 * h * (d + 1)] = lstm_backward(case.dout[r0:r1, c0:c0 + h].to(dtype), gs, cs, w, rev,
                                                                          mistake)
    return res


@functools.lru_cache(maxsize=None)
def lstm_bundle(hidden, ndir=3, reverse_mask=0b010, lens=COMMON_LENS, saturate=False, twins=None, backward=True):
    """(case, float64 reference, fp32 restatement, fp32 backward fed the reference's saved tensors rounded to fp32 - or
    None), computed once per process and shared by the tests; none of them is modified by a test."""
    case = lstm_case(hidden, ndir, reverse_mask, lens, saturate=saturate, twins=twins)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)      # thousands of small matrix-vector products: a thread pool only adds its hand-over to each
    try:
        ref = lstm_reference(case, backward)
        cpu32 = lstm_restatement(case, backward=backward)
        iso32 = lstm_restatement(case, saved=(ref.gates.float(), ref.cell.float())) if backward else None
    finally:
        torch.set_num_threads(threads)
    return case, ref, cpu32, iso32


# --------------------------------------------------------------------------- the small scorer kernels
SOFTMAX_N = (1, 63, 64, 65, 255, 256, 257, 1003)
SOFTMAX_ROWS = 7
SCORE_D = (1, 63, 64, 65, 200)
SCORE_ROWS = (1, 5, 1027)
ELEMENTWISE_N = (1, 255, 256, 257, 70001, 8192 * 256 + 257)    # the last: a second trip of the grid-stride loop
TRANSPOSE_SHAPES = ((1, 1), (3, 5), (33, 65), (257, 40), (1800, 7))
MHA_E_HEADS = ((64, 4), (400, 4), (1024, 4), (2048, 4))
MHA_B, MHA_T = (1, 2, 5), (1, 7)


def softmax_case(n):
    """x [7, n + 3]: columns < n are 4 * N(0, 1), the pad columns SENTINEL; dp [7, n + 3] likewise with N(0, 1)."""
    g = torch.Generator().manual_seed(8100 + n)
    x = torch.full((SOFTMAX_ROWS, n + 3), SENTINEL)
    x[:, :n] = torch.randn(SOFTMAX_ROWS, n, generator=g) * 4
    dp = torch.full((SOFTMAX_ROWS, n + 3), SENTINEL)
    dp[:, :n] = torch.randn(SOFTMAX_ROWS, n, generator=g)
    return x, dp


def softmax_bwd_formula(p, dp, alpha):
    """alpha * p * (dp - sum(p * dp)) per row, in the dtype of p."""
    return alpha * p * (dp - (p * dp).sum(-1, keepdim=True))


def score_case(rows, d):
    """pre [rows, d + 3] ~ N(0, 1) (columns >= d: SENTINEL pads), w2 [d], b2 [1], dscores [rows]."""
    g = torch.Generator().manual_seed(8200 + 1000 * d + rows)
    pre = torch.full((rows, d + 3), SENTINEL)
    pre[:, :d] = torch.randn(rows, d, generator=g)
    return pre, torch.randn(d, generator=g), torch.randn(1, generator=g), torch.randn(rows, generator=g)


def elementwise_case(n):
    """dy, relu_out (about half zeros), keep (0 or 1/0.7) of n elements."""
    g = torch.Generator().manual_seed(8300 + n % 1000)
    dy = torch.randn(n, generator=g)
    relu_out = torch.relu(torch.randn(n, generator=g))
    keep = (torch.rand(n, generator=g) < 0.7).float() / 0.7
    return dy, relu_out, keep


def transpose_case(rows, cols, k=9):
    """dy [rows, cols] as a view of a [rows, cols + 3] buffer (row stride wider than cols), x [rows, k]."""
    g = torch.Generator().manual_seed(8400 + 10 * rows + cols)
    wide = torch.randn(rows, cols + 3, generator=g)
    return wide, torch.randn(rows, k, generator=g)


@functools.lru_cache(maxsize=None)
def _mha_perms(e):
    g = torch.Generator().manual_seed(8500 + e)
    return tuple(torch.randperm(e, generator=g) for _ in range(3))


def mha_case(e, b, t):
    """x [b, t, e] ~ N(0, 1) and qkv [b*t, 3e] = x under three column permutations scaled by 1, 2 and 0.5: an in_proj
    whose products are exact in fp32 and in float64, so the device (fed qkv) and oracle.scorer.mha_seq_first (fed x and
    the matrix of ``mha_in_proj``) see the same q, k, v to the bit."""
    g = torch.Generator().manual_seed(8600 + 100 * b + t + e)
    x = torch.randn(b, t, e, generator=g)
    pq, pk, pv = _mha_perms(e)
    qkv = torch.cat([x[..., pq], 2.0 * x[..., pk], 0.5 * x[..., pv]], -1).reshape(b * t, 3 * e).contiguous()
    return x, qkv


@functools.lru_cache(maxsize=None)
def mha_in_proj(e, dtype):
    """The [3e, e] in_proj matrix of ``mha_case`` (one non-zero per row) and its zero bias."""
    w = torch.zeros(3 * e, e, dtype=dtype)
    for blk, (perm, s) in enumerate(zip(_mha_perms(e), (1.0, 2.0, 0.5))):
        w[blk * e + torch.arange(e), perm] = s
    return w, torch.zeros(3 * e, dtype=dtype)


def mha_reference(x, e, heads, dtype):
    """oracle.scorer.mha_seq_first in ``dtype`` with identity output projection: [b*t, e]."""
    w, bias = mha_in_proj(e, dtype)
    out = osc.mha_seq_first(x.to(dtype), w, bias, torch.eye(e, dtype=dtype), torch.zeros(e, dtype=dtype), heads)
    return out.reshape(-1, e)
