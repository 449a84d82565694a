"""Multi-head self-attention over a ragged batch of sequences with a fused backward: the launch wrappers of
libavsum_attn.so (include/avsum_attn.h) and the host restatement the tests compare them against.

The batch is the layout of every ragged stage of this package: the sequences lie one after another in the rows of the
projections Q, K, V [rows, E], an ``ops.AttnTable`` holds the validated row offsets and the (sequence, tile) tables, and
nothing is padded.  Per sequence and head (D = E / heads, alpha = 1 / sqrt(D)):

    S = alpha Q K^T     L = logsumexp_k S     P = exp(S - L)     O = P V                              (mhsa_rows_fwd)
    delta = rowsum(dO o O)                                                                            (mhsa_rows_delta)
    dV = P^T dO     dP = dO V^T     dS = alpha P o (dP - delta)     dK = dS^T Q                       (mhsa_rows_dkv)
    dQ = dS K                                                                                         (mhsa_rows_dq)

No [T, T] matrix reaches memory in either direction: the forward saves L [rows, heads], the backward rebuilds P from
it tile by tile.  Every output element has one owner (no atomics), so a sequence's ctx, lse, dq, dk, dv are the same
bits alone and in any batch, run after run.  Host tensors are refused: there is no CPU fallback.
``mhsa_rows_reference`` is the definition in torch on the CPU, float64 or float32, for tests and studies.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from ._attn_abi import BWD_TILE, FWD_TILE, check, lib
from .ops import AttnTable, _device_arg, _p, _stream, _tables_arg

__all__ = ["HEAD_DIMS", "FWD_TILE", "BWD_TILE", "mhsa_rows_fwd", "mhsa_rows_delta", "mhsa_rows_dkv", "mhsa_rows_dq",
           "mhsa_rows_bwd", "mhsa_rows_reference"]

HEAD_DIMS = (64, 128, 256)


def _rows_arg(x, name, what, table, cols, device):
    """An fp32 device operand [at least table.rows, cols] with unit column stride (a column slice of a wider buffer is
    fine: the row stride travels with it).  Returns its row stride."""
    _device_arg(x, name, what, (torch.float32,), ndim=2, device=device, contiguous=False)
    if x.shape[1] != cols or x.stride(1) != 1 or x.shape[0] < table.rows:
        raise ValueError(f"{what}: {name} must be [at least {table.rows}, {cols}] with unit column stride, got shape "
                         f"{list(x.shape)} strides {list(x.stride())}")
    return x.stride(0)


def _head_dim(e, heads, what):
    heads = int(heads)
    if heads < 1 or e % heads or e // heads not in HEAD_DIMS:
        raise ValueError(f"{what}: head dim {e}/{heads} must be one of {HEAD_DIMS}")
    return e // heads


def _per_row(x, name, what, table, heads, device):
    """lse / delta: fp32 contiguous [at least table.rows, heads]."""
    _device_arg(x, name, what, (torch.float32,), ndim=2, device=device)
    if x.shape[1] != heads or x.shape[0] < table.rows:
        raise ValueError(f"{what}: {name} must be [at least {table.rows}, {heads}], got {list(x.shape)}")
    return x


def _shared_stride(what, names, *strides):
    if len(set(strides)) != 1:
        raise ValueError(f"{what}: {names} must share a row stride, got {list(strides)}")
    return strides[0]


def _batch_args(table):
    """(h_offsets, d_offsets, nseq) of the C entry points."""
    return table.offsets.ctypes.data, _p(table.offsets_t), table.nseq


def mhsa_rows_fwd(q, k, v, table, heads, ctx=None, lse=None):
    """q, k, v fp32 [rows, E] (projected; rows >= table.rows) -> (ctx [rows, E], lse [rows, heads]).  Sequence v of
    ``table`` (an ops.AttnTable) attends over its own rows only.  ``ctx`` / ``lse``: buffers to write into (allocated
    when None); rows outside the table's sequences are left as they were.  The ctx bits of a sequence are those of
    ops.mhsa_flash(q_v, k_v, v_v, 1, T_v, heads, split=False)."""
    what = "mhsa_rows_fwd"
    _device_arg(q, "q", what, (torch.float32,), ndim=2, contiguous=False)
    dev, e = q.device, q.shape[1]
    _tables_arg(table, AttnTable, what, device=dev)
    d = _head_dim(e, heads, what)
    ld = _shared_stride(what, "q, k, v", *(_rows_arg(x, n, what, table, e, dev) for n, x in (("q", q), ("k", k), ("v", v))))
    if ctx is None:
        ctx = torch.empty((q.shape[0], e), dtype=torch.float32, device=dev)
    if lse is None:
        lse = torch.empty((q.shape[0], int(heads)), dtype=torch.float32, device=dev)
    ldo = _rows_arg(ctx, "ctx", what, table, e, dev)
    _per_row(lse, "lse", what, table, int(heads), dev)
    check(lib().avsa_mhsa_rows_fwd_f32(_p(q), _p(k), _p(v), ld, *_batch_args(table), _p(table.fwd_tiles_t), table.n_fwd,
                                       int(heads), d, _p(ctx), ldo, _p(lse), _stream()), "avsa_mhsa_rows_fwd_f32")
    return ctx, lse


def mhsa_rows_delta(dctx, ctx, table, heads, delta=None):
    """delta fp32 [rows, heads] = rowsum over a head's columns of dctx * ctx, for the rows of the table's sequences."""
    what = "mhsa_rows_delta"
    _device_arg(dctx, "dctx", what, (torch.float32,), ndim=2, contiguous=False)
    dev, e = dctx.device, dctx.shape[1]
    _tables_arg(table, AttnTable, what, device=dev)
    d = _head_dim(e, heads, what)
    lddo, ldo = _rows_arg(dctx, "dctx", what, table, e, dev), _rows_arg(ctx, "ctx", what, table, e, dev)
    if delta is None:
        delta = torch.empty((dctx.shape[0], int(heads)), dtype=torch.float32, device=dev)
    _per_row(delta, "delta", what, table, int(heads), dev)
    check(lib().avsa_mhsa_rows_delta_f32(_p(dctx), lddo, _p(ctx), ldo, table.offsets.ctypes.data, table.nseq, int(heads), d,
                                         _p(delta), _stream()), "avsa_mhsa_rows_delta_f32")
    return delta


def _grad_args(what, dctx, q, k, v, lse, delta, table, heads):
    _device_arg(q, "q", what, (torch.float32,), ndim=2, contiguous=False)
    dev, e = q.device, q.shape[1]
    _tables_arg(table, AttnTable, what, device=dev)
    d = _head_dim(e, heads, what)
    ld = _shared_stride(what, "q, k, v", *(_rows_arg(x, n, what, table, e, dev) for n, x in (("q", q), ("k", k), ("v", v))))
    lddo = _rows_arg(dctx, "dctx", what, table, e, dev)
    _per_row(lse, "lse", what, table, int(heads), dev)
    _per_row(delta, "delta", what, table, int(heads), dev)
    return dev, e, d, ld, lddo


def mhsa_rows_dkv(dctx, q, k, v, lse, delta, table, heads, dk=None, dv=None):
    """(dk, dv) fp32 [rows, E]: a workgroup per 32 keys of a (sequence, head) sweeps that sequence's queries."""
    what = "mhsa_rows_dkv"
    dev, e, d, ld, lddo = _grad_args(what, dctx, q, k, v, lse, delta, table, heads)
    if dk is None:
        dk = torch.empty((q.shape[0], e), dtype=torch.float32, device=dev)
    if dv is None:
        dv = torch.empty((q.shape[0], e), dtype=torch.float32, device=dev)
    ldg = _shared_stride(what, "dk, dv", _rows_arg(dk, "dk", what, table, e, dev), _rows_arg(dv, "dv", what, table, e, dev))
    check(lib().avsa_mhsa_rows_dkv_f32(_p(q), _p(k), _p(v), ld, _p(dctx), lddo, _p(lse), _p(delta), *_batch_args(table),
                                       _p(table.bwd_tiles_t), table.n_bwd, int(heads), d, _p(dk), _p(dv), ldg, _stream()),
          "avsa_mhsa_rows_dkv_f32")
    return dk, dv


def mhsa_rows_dq(dctx, q, k, v, lse, delta, table, heads, dq=None):
    """dq fp32 [rows, E]: a workgroup per 32 queries of a (sequence, head) sweeps that sequence's keys."""
    what = "mhsa_rows_dq"
    dev, e, d, ld, lddo = _grad_args(what, dctx, q, k, v, lse, delta, table, heads)
    if dq is None:
        dq = torch.empty((q.shape[0], e), dtype=torch.float32, device=dev)
    ldg = _rows_arg(dq, "dq", what, table, e, dev)
    check(lib().avsa_mhsa_rows_dq_f32(_p(q), _p(k), _p(v), ld, _p(dctx), lddo, _p(lse), _p(delta), *_batch_args(table),
                                      _p(table.bwd_tiles_t), table.n_bwd, int(heads), d, _p(dq), ldg, _stream()),
          "avsa_mhsa_rows_dq_f32")
    return dq


def mhsa_rows_bwd(dctx, q, k, v, ctx, lse, table, heads):
    """(dq, dk, dv) fp32 [rows, E] from dctx and what mhsa_rows_fwd was given and returned: three launches (delta, dK/dV,
    dQ) and one [rows, heads] + three [rows, E] allocations, whatever the sequences' lengths."""
    delta = mhsa_rows_delta(dctx, ctx, table, heads)
    dk, dv = mhsa_rows_dkv(dctx, q, k, v, lse, delta, table, heads)
    return mhsa_rows_dq(dctx, q, k, v, lse, delta, table, heads), dk, dv


# --------------------------------------------------------------------------- the definition, on the host
def mhsa_rows_reference(q, k, v, offsets, heads, dctx=None, dtype=torch.float64, lse=None, delta=None):
    """The operation of the module docstring in torch on the CPU, in ``dtype`` (float64: the reference; float32: the
    yardstick of the tests' bound - plain products, S divided by sqrt(D) as the kernels do).  q, k, v (and dctx) are
    host tensors [rows, E]; ``offsets`` the host row offsets [V + 1].  Returns a namespace of [rows, E] ``ctx`` and
    [rows, heads] ``lse`` and, with ``dctx``, ``delta``, ``dq``, ``dk``, ``dv``; rows outside the sequences are zero.
    ``lse`` / ``delta`` [rows, heads]: values to rebuild P and dS from INSTEAD of the ones computed here - what a
    gradient kernel is handed - so that their rounding is not charged to the kernel under test."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    rows, e = q.shape
    heads = int(heads)
    d = e // heads
    sqrt_d = torch.tensor(math.sqrt(d), dtype=dtype)
    cast = lambda x: None if x is None else x.to(dtype)
    q, k, v, dctx, lse_in, delta_in = (cast(x) for x in (q, k, v, dctx, lse, delta))
    out = SimpleNamespace(ctx=torch.zeros(rows, e, dtype=dtype), lse=torch.zeros(rows, heads, dtype=dtype))
    if dctx is not None:
        out.delta = torch.zeros(rows, heads, dtype=dtype)
        out.dq, out.dk, out.dv = (torch.zeros(rows, e, dtype=dtype) for _ in range(3))
    for lo, hi in zip(off[:-1], off[1:]):
        for h in range(heads):
            r, c = slice(int(lo), int(hi)), slice(h * d, (h + 1) * d)
            s = q[r, c] @ k[r, c].T / sqrt_d
            big = torch.logsumexp(s, dim=1)
            out.lse[r, h] = big
            o = torch.exp(s - big[:, None]) @ v[r, c]
            out.ctx[r, c] = o
            if dctx is None:
                continue
            do = dctx[r, c]
            out.delta[r, h] = (do * o).sum(1)
            p = torch.exp(s - (big if lse_in is None else lse_in[r, h])[:, None])
            dl = out.delta[r, h] if delta_in is None else delta_in[r, h]
            ds = p * (do @ v[r, c].T - dl[:, None]) / sqrt_d
            out.dv[r, c] = p.T @ do
            out.dq[r, c] = ds @ k[r, c]
            out.dk[r, c] = ds.T @ q[r, c]
    return out
