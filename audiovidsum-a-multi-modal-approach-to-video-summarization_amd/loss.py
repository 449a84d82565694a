"""Per-shot training targets and a pairwise ranking loss for a ragged batch of videos: the launch wrappers of
libavsum_loss.so (include/avsum_loss.h - its comment is the definition), the autograd function, and the same
definitions restated on the host in numpy / float64.

    shot_targets(...)   the reference's utils/alignments.py per shot, on the device     (avsl_shot_targets_f32)
    rank_loss(...)      per-video pairwise ranking loss, differentiable in the scores   (avsl_rank_loss_f32, one forward
                        pass that also leaves the gradient; the backward is one elementwise launch)
    rank_loss_fwd(...)  (losses, g, P): what that pass leaves, for tests and studies

The per-shot target of shot (start, end) of video v: a = floor((start / fps_v) / bin_seconds), b = floor((end / fps_v) /
bin_seconds) + 1 in float64, both clipped to [0, A_v]; the target is the float64 sum of annotations_v[a:b] in index
order over b - a, rounded once to fp32; an empty slice gives NaN and sets flags[v].

The ranking loss of video v over the pairs (i, j) with y_i > y_j (ties form no pair), P_v of them, d_ij = s_i - s_j:

    logistic   L_v = (1 / P_v) * sum softplus(-scale * d_ij)
    hinge      L_v = (1 / P_v) * sum max(0, margin - d_ij)

P_v = 0 gives loss 0 and gradient 0.  Every sum on the device has one order that depends on the video's length alone:
a video's targets, loss and gradient are the same bits alone and in any batch.  Memory is O(R): no [T, T] matrix.

Host tensors are refused by the launch wrappers: there is no CPU fallback.  math, numpy and torch are all this module
imports; the library is loaded at the first launch.
"""
import math

import numpy as np
import torch

__all__ = ["KINDS", "shot_targets_host", "rank_loss_host", "shot_targets", "rank_loss_fwd", "rank_loss", "rank_loss_bwd"]

KINDS = ("logistic", "hinge")


# --------------------------------------------------------------------------- the definitions, on the host
def _fps_vector(fps, nvideos, what):
    f = np.asarray(fps, dtype=np.float64)
    f = np.full(nvideos, float(f), dtype=np.float64) if f.ndim == 0 else f.reshape(-1).copy()
    if f.size != nvideos:
        raise ValueError(f"{what}: {f.size} frame rates for {nvideos} videos")
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError(f"{what}: a frame rate must be finite and > 0, got {f.tolist()}")
    return f


def _bin_seconds(bin_seconds, what):
    b = float(bin_seconds)
    if not (math.isfinite(b) and b > 0):
        raise ValueError(f"{what}: bin_seconds must be finite and > 0, got {bin_seconds!r}")
    return b


def _host_segments(offsets, what, rows=None, min_length=0):
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if off.size < 2 or off[0] != 0 or (np.diff(off) < min_length).any():
        raise ValueError(f"{what}: offsets must hold V + 1 >= 2 entries, start at 0 and "
                         f"{'increase strictly' if min_length else 'not decrease'}")
    if rows is not None and int(off[-1]) != rows:
        raise ValueError(f"{what}: the offsets end at {int(off[-1])}, the rows are {rows}")
    return off


def _host_shots(shots, what):
    table = np.asarray(shots, dtype=np.int64).reshape(-1, 2)
    if (table < 0).any():
        raise ValueError(f"{what}: a shot bound is negative")
    return table


def shot_targets_host(annotations, ann_offsets, shots, shot_offsets, fps, bin_seconds=2.0, planted=None):
    """The definition in numpy: (targets fp32 [S], flags uint8 [V]).  ``annotations``: the videos' annotation vectors
    concatenated (cast to fp32, what the device reads); ``ann_offsets`` [V + 1]; ``shots`` int64 [S, 2] video-relative
    frame bounds, ``shot_offsets`` [V + 1]; ``fps`` a scalar or [V].  The sum is a sequential float64 loop in index
    order (np.sum adds pairwise: another order).  ``planted`` exists for the tests: "end_without_plus_one" leaves the
    ``+ 1`` of the end bin out, and the cases are expected to notice."""
    what = "shot_targets_host"
    ann = np.asarray(annotations, dtype=np.float32).reshape(-1)
    aoff = _host_segments(ann_offsets, what + ": ann_offsets", ann.size)
    table = _host_shots(shots, what)
    soff = _host_segments(shot_offsets, what + ": shot_offsets", table.shape[0])
    if soff.size != aoff.size:
        raise ValueError(f"{what}: {aoff.size - 1} annotation vectors for {soff.size - 1} shot lists")
    nv = aoff.size - 1
    f, bin_s = _fps_vector(fps, nv, what), np.float64(_bin_seconds(bin_seconds, what))
    targets, flags = np.empty(table.shape[0], dtype=np.float32), np.zeros(nv, dtype=np.uint8)
    plus = 0 if planted == "end_without_plus_one" else 1
    for v in range(nv):
        seg = ann[aoff[v]:aoff[v + 1]].astype(np.float64)
        for s in range(soff[v], soff[v + 1]):
            a = int(np.floor((np.float64(table[s, 0]) / f[v]) / bin_s))
            b = int(np.floor((np.float64(table[s, 1]) / f[v]) / bin_s)) + plus
            a, b = min(max(a, 0), seg.size), min(max(b, 0), seg.size)
            if b <= a:
                targets[s], flags[v] = np.nan, 1
                continue
            total = np.float64(0.0)
            for x in seg[a:b]:
                total = total + x
            targets[s] = np.float32(total / np.float64(b - a))
    return targets, flags


def _kind(kind, what):
    if kind not in KINDS:
        raise ValueError(f"{what}: kind must be one of {KINDS}, got {kind!r}")
    return kind


def _scale_margin(scale, margin, what):
    scale, margin = float(scale), float(margin)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"{what}: scale must be finite and > 0, got {scale}")
    if not math.isfinite(margin):
        raise ValueError(f"{what}: margin must be finite, got {margin}")
    return scale, margin


def rank_loss_host(scores, targets, offsets, kind="logistic", scale=1.0, margin=0.1, planted=None):
    """The float64 definition, O(T^2) numpy with math.fsum for every sum: (losses float64 [V], dscores float64 [R] for
    dlosses = 1, P int64 [V]).  ``scores`` and ``targets`` are cast to fp32 first (what the device reads); ``offsets``
    host [V + 1].  ``planted`` exists for the tests, which expect their cases to notice each: "ge" forms pairs with
    ``>=`` (ties pair up), "t_squared" divides by T^2 instead of P, "sign" flips the sign of one gradient half."""
    what = "rank_loss_host"
    _kind(kind, what)
    scale, margin = _scale_margin(scale, margin, what)
    s_all = np.asarray(scores, dtype=np.float32).reshape(-1).astype(np.float64)
    y_all = np.asarray(targets, dtype=np.float32).reshape(-1)
    if s_all.size != y_all.size:
        raise ValueError(f"{what}: {s_all.size} scores and {y_all.size} targets")
    off = _host_segments(offsets, what, s_all.size, min_length=1)
    nv = off.size - 1
    losses, grads, pairs = np.zeros(nv), np.zeros(s_all.size), np.zeros(nv, dtype=np.int64)
    flip = -1.0 if planted == "sign" else 1.0
    for v in range(nv):
        s, y = s_all[off[v]:off[v + 1]], y_all[off[v]:off[v + 1]]
        t = s.size
        terms, bracket, count = [], np.zeros(t), 0
        for r0 in range(0, t, 512):                              # row blocks: [512, T] at a time, never [T, T]
            rows = slice(r0, min(r0 + 512, t))
            d = s[rows, None] - s[None, :]                       # d_ij, exact in float64
            above = (y[rows, None] >= y[None, :]) if planted == "ge" else (y[rows, None] > y[None, :])
            below = (y[None, :] >= y[rows, None]) if planted == "ge" else (y[None, :] > y[rows, None])
            count += int(above.sum())
            if kind == "logistic":
                x = -scale * d                                   # the pair (i, j): x_ij; the pair (j, i): -x_ij
                e = np.exp(-np.abs(x))
                terms.append((np.maximum(x, 0.0) + np.log1p(e))[above])
                sig_ij = np.where(x >= 0.0, 1.0, e) / (1.0 + e)              # sigma(-scale * d_ij)
                sig_ji = np.where(-x >= 0.0, 1.0, e) / (1.0 + e)             # sigma(-scale * d_ji)
                for k in range(d.shape[0]):
                    bracket[r0 + k] = flip * math.fsum(sig_ji[k][below[k]].tolist()) - \
                        math.fsum(sig_ij[k][above[k]].tolist())
            else:
                up, down = margin - d, margin + d                # margin - d_ij, margin - d_ji
                terms.append(up[above & (up > 0.0)])
                bracket[rows] = flip * (below & (down > 0.0)).sum(1) - (above & (up > 0.0)).sum(1)
        pairs[v] = count
        if count == 0:
            continue
        denom = float(t) * float(t) if planted == "t_squared" else float(count)
        losses[v] = math.fsum(np.concatenate(terms).tolist()) / denom
        grads[off[v]:off[v + 1]] = (scale * bracket if kind == "logistic" else bracket) / denom
    return losses, grads, pairs


# --------------------------------------------------------------------------- launches
def _abi():
    from . import _loss_abi
    return _loss_abi


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _vector(x, name, what, dtype=torch.float32, numel=None, device=None):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what}: {name} must be a device tensor (there is no CPU fallback)")
    if x.dtype != dtype or x.dim() != 1 or not x.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} vector, got {x.dtype} {list(x.shape)}")
    if (numel is not None and x.numel() != numel) or (device is not None and x.device != device):
        raise ValueError(f"{what}: {name} must hold {numel} entries on {device}, got {x.numel()} on {x.device}")
    return x


def _device_table(t, name, what, shape, device):
    if t.dtype != torch.int64 or not t.is_contiguous() or t.device != device or t.dim() != len(shape) or \
            any(want is not None and got != want for got, want in zip(t.shape, shape)):
        raise ValueError(f"{what}: a device {name} must be contiguous int64 {list(shape)} on {device}, got {t.dtype} "
                         f"{list(t.shape)} on {t.device}")
    return t


def shot_targets(annotations, ann_offsets, shots, shot_offsets, fps, bin_seconds=2.0, out=None, flags_out=None):
    """(targets fp32 [S], flags uint8 [V]) on the device, nothing read back.  ``annotations``: fp32 device vector, the
    videos' annotation vectors concatenated; ``ann_offsets``: host [V + 1].  ``shots`` int64 [S, 2] and ``shot_offsets``
    int64 [V + 1], video-relative frame bounds in the layout evaluation.keyshots.keyshot_summaries_device consumes:
    device tensors are used where they lie (the tables of a ShotBatchResult or KtsResult; S is then the table's
    capacity, and the targets of rows no video owns are not written), host arrays are validated (non-negative, offsets
    from 0 that do not decrease and end at S) and uploaded with the other host tables in ONE copy.  ``fps``: a scalar
    or a host [V].  flags[v] = 1 where a shot of video v has an empty annotation slice (its target is NaN).  ``out`` /
    ``flags_out``: the buffers to write into (contiguous fp32 [S] / uint8 [V] on the device, e.g. slices of larger
    ones; what lies outside them is left alone)."""
    what = "shot_targets"
    ann = _vector(annotations, "annotations", what)
    dev = ann.device
    aoff = _host_segments(ann_offsets, what + ": ann_offsets", ann.numel())
    nv = aoff.size - 1
    f, bin_s = _fps_vector(fps, nv, what), _bin_seconds(bin_seconds, what)
    host = [aoff, f.view(np.int64)]                              # (the fp64 frame rates travel as their bit patterns)
    if isinstance(shots, torch.Tensor) and shots.is_cuda:
        shots_t = _device_table(shots, "shots", what, (None, 2), dev)
    else:
        shots_t = None
        table = _host_shots(shots.numpy() if isinstance(shots, torch.Tensor) else shots, what)
        host.append(table.reshape(-1))
    nshots = shots_t.shape[0] if shots_t is not None else table.shape[0]
    if isinstance(shot_offsets, torch.Tensor) and shot_offsets.is_cuda:
        soff_t = _device_table(shot_offsets, "shot_offsets", what, (nv + 1,), dev)
    else:
        soff_t = None
        soff = _host_segments(shot_offsets.numpy() if isinstance(shot_offsets, torch.Tensor) else shot_offsets,
                              what + ": shot_offsets", nshots if shots_t is None else None)
        if soff.size != nv + 1 or soff[-1] > nshots:
            raise ValueError(f"{what}: {soff.size - 1} shot lists ending at {int(soff[-1])} for {nv} videos and "
                             f"{nshots} shots")
        host.append(soff)
    parts = list(torch.split(torch.from_numpy(np.concatenate(host)).to(dev), [h.size for h in host]))
    aoff_t, fps_t = parts[0], parts[1].view(torch.float64)
    if soff_t is None:
        soff_t = parts.pop()
    if shots_t is None:
        shots_t = parts.pop().view(-1, 2)
    targets = torch.empty(nshots, dtype=torch.float32, device=dev) if out is None else \
        _vector(out, "out", what, numel=nshots, device=dev)
    flags = torch.empty(nv, dtype=torch.uint8, device=dev) if flags_out is None else \
        _vector(flags_out, "flags_out", what, torch.uint8, nv, dev)
    abi = _abi()
    abi.check(abi.lib().avsl_shot_targets_f32(_ptr(ann), ann.numel(), _ptr(aoff_t), _ptr(shots_t), nshots, _ptr(soff_t),
                                              _ptr(fps_t), nv, bin_s, _ptr(targets), _ptr(flags), _stream(dev)),
              "avsl_shot_targets_f32")
    return targets, flags


def _rank_table(offsets, rows, device, what):
    from .ragged import RankTables
    if isinstance(offsets, RankTables):
        if offsets.device.type != "cuda" or offsets.device != device:
            raise ValueError(f"{what}: the RankTables are on {offsets.device}, the scores on {device}")
        if offsets.rows != rows:
            raise ValueError(f"{what}: the offsets end at {offsets.rows}, the scores have {rows} rows")
        return offsets
    return RankTables(offsets, rows, device)


def rank_loss_fwd(scores, targets, offsets, kind="logistic", scale=1.0, margin=0.1):
    """The one pass of the ranking loss: (losses fp32 [V], g fp32 [R] = dlosses-free gradient dL_v/ds_r, P int64 [V]),
    all on the device.  Arguments as rank_loss; nothing is recorded for autograd."""
    what = "rank_loss"
    _kind(kind, what)
    scale, margin = _scale_margin(scale, margin, what)
    s = _vector(scores, "scores", what)
    y = _vector(targets, "targets", what, numel=s.numel(), device=s.device)
    table = _rank_table(offsets, s.numel(), s.device, what)
    abi = _abi()
    lib, dev = abi.lib(), s.device
    nbytes = lib.avsl_rank_workspace_bytes(table.rows)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    losses = torch.empty(table.nseq, dtype=torch.float32, device=dev)
    g = torch.empty(table.rows, dtype=torch.float32, device=dev)
    pairs = torch.empty(table.nseq, dtype=torch.int64, device=dev)
    abi.check(lib.avsl_rank_loss_f32(_ptr(s), _ptr(y), table.rows, _ptr(table.offsets_t), table.nseq, _ptr(table.tiles_t),
                                     table.ntiles, table.max_t, abi.KINDS[kind], scale, margin, _ptr(workspace), nbytes,
                                     _ptr(losses), _ptr(g), _ptr(pairs), _stream(dev)), "avsl_rank_loss_f32")
    return losses, g, pairs


def rank_loss_bwd(dlosses, g, offsets):
    """dscores[r] = dlosses[v] * g[r] in fp32: the backward of rank_loss, one elementwise launch.  ``offsets``: a
    RankTables on the device of ``g``."""
    what = "rank_loss_bwd"
    g = _vector(g, "g", what)
    table = _rank_table(offsets, g.numel(), g.device, what)
    dlosses = _vector(dlosses, "dlosses", what, numel=table.nseq, device=g.device)
    dscores = torch.empty_like(g)
    abi = _abi()
    abi.check(abi.lib().avsl_rank_loss_bwd_f32(_ptr(dlosses), _ptr(g), table.rows, _ptr(table.offsets_t), table.nseq,
                                               _ptr(dscores), _stream(g.device)), "avsl_rank_loss_bwd_f32")
    return dscores


class _RankLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, targets, table, kind, scale, margin):
        losses, g, _ = rank_loss_fwd(scores, targets, table, kind, scale, margin)
        ctx.table = table
        ctx.save_for_backward(g)                                 # the gradient is all the backward needs
        return losses

    @staticmethod
    def backward(ctx, dlosses):
        g, = ctx.saved_tensors
        return rank_loss_bwd(dlosses.contiguous().float(), g, ctx.table), None, None, None, None, None


def rank_loss(scores, targets, offsets, kind="logistic", scale=1.0, margin=0.1):
    """Per-video pairwise ranking loss of a ragged batch: fp32 [V], differentiable with respect to ``scores``.
    ``scores`` fp32 [R] and ``targets`` fp32 [R] on the device; ``offsets``: a host array [V + 1] or an
    ops.RankTables; ``kind``: "logistic" (softplus(-scale * d_ij)) or "hinge" (max(0, margin - d_ij)).  The forward
    pass computes the gradient with the loss and keeps only it; the backward is dscores[r] = dlosses[v] * g[r]."""
    what = "rank_loss"
    _kind(kind, what)
    scale, margin = _scale_margin(scale, margin, what)
    s = _vector(scores, "scores", what)
    table = _rank_table(offsets, s.numel(), s.device, what)
    return _RankLoss.apply(s, targets, table, kind, scale, margin)
