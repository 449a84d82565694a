"""Drop-in for the reference's features/fusion.py on the MI355X.

  compute_dtw(visual, audio)            fusion.py:7-12   Tensor[Tv,D], Tensor[Ta,D] -> np.float64 [Tv,Ta]
  compute_optimal_path(dtw_matrix)      fusion.py:15-18  -> np.int64 [L,2]
  interpolate_features(feats, path, n)  fusion.py:21-32  -> Tensor [min(U,n), D] float32

and the batched form of the three together, for many (visual, audio) pairs at once (no counterpart in the reference):

  fuse_batch_device(visual, audio, v_offsets, a_offsets, n)  device rows + offsets -> (fused rows, their offsets)
  fuse_batch(visuals, audios, n)                             lists of host tensors -> list of host tensors

``compute_optimal_path`` cannot run as written in the reference (fastdtw is called without its
second series); this build implements the evident intent — the exact DTW path over
the cost matrix with fastdtw's tie order — and says so.  Inputs are host tensors/arrays as in
the reference; they are moved to the HIP device, computed there, and returned on the host.
"""
import numpy as np
import torch

from .. import ops
from ..ragged import exclusive_offsets


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("avsum_amd needs an MI355X (HIP device); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def compute_dtw_device(visual, audio):
    """Device tensors in, device float64 [Tv,Ta] out."""
    return ops.cdist(visual.float(), audio.float())


def compute_dtw(visual, audio):
    """Compute DTW cost matrix (Euclidean, float64)."""
    dev = _dev()
    v = torch.as_tensor(visual)
    a = torch.as_tensor(audio)
    if v.dim() != 2 or a.dim() != 2:
        raise ValueError("XA must be a 2-dimensional array.")
    return compute_dtw_device(v.to(dev), a.to(dev)).cpu().numpy()


def compute_optimal_path(dtw_matrix):
    """Optimal warping path through the cost matrix, start -> end, as int64 [L,2]."""
    dev = _dev()
    cost = torch.as_tensor(np.ascontiguousarray(dtw_matrix, dtype=np.float64)).to(dev)
    path, plen, _ = ops.dtw_path(cost)
    n = int(plen.item())
    return path[:n].cpu().numpy()


def interpolate_features(features, path, target_length):
    """features[idx] * (count/sum(count)) for the unique first-column indices of path, first target_length rows."""
    dev = _dev()
    aligned_indices = np.asarray(path)[:, 0]
    unique_indices, counts = np.unique(aligned_indices, return_counts=True)  # host: a few thousand ints
    weights = counts / counts.sum()
    feats = torch.as_tensor(features).float()
    out = ops.gather_scale(feats.to(dev).contiguous(), torch.from_numpy(unique_indices.astype(np.int64)).to(dev),
                           torch.from_numpy(weights.astype(np.float64)).to(dev))
    return out[:target_length].cpu()


def _ranges(offsets):
    off = [int(x) for x in (offsets.tolist() if hasattr(offsets, "tolist") else offsets)]
    if len(off) < 1 or any(b < a for a, b in zip(off[:-1], off[1:])):
        raise ValueError("offsets must be a non-decreasing list of P + 1 row offsets")
    return off


def fuse_batch_device(visual, audio, v_offsets, a_offsets=None, target_length=None, tables=None):
    """interpolate_features(v, compute_optimal_path(compute_dtw(v, a)), target_length) for every pair of a batch in one
    fixed set of launches (ops.fusion_batch), device in, device out.  visual [Rv, D] / audio [Ra, D] hold the pairs' rows
    one after another; pair p is visual[v_offsets[p]:v_offsets[p+1]] against audio[a_offsets[p]:a_offsets[p+1]] (host
    lists of P + 1 offsets; a_offsets=None: the same ranges as v_offsets).  Returns (fused [sum min(n_p,
    target_length), D] fp32, out_offsets int64 [P + 1]), both on the device.  A caller that fuses the same layout again
    passes ``tables`` (the ops.FusionTables of an earlier call, see fusion_tables) and pays no table upload."""
    if tables is None:
        tables = fusion_tables(v_offsets, a_offsets, visual.device if isinstance(visual, torch.Tensor) else None)
    res = ops.fusion_batch(tables, visual, audio, target_length)
    return res["fused"], res["out_offsets"]


def fusion_tables(v_offsets, a_offsets=None, device=None):
    """The ops.FusionTables of a batch given as row offsets (see fuse_batch_device)."""
    vo = _ranges(v_offsets)
    ao = vo if a_offsets is None else _ranges(a_offsets)
    if len(ao) != len(vo):
        raise ValueError("v_offsets and a_offsets must describe the same number of pairs")
    if device is not None and torch.device(device).type != "cuda":
        raise ValueError("avsum HIP ops need device tensors (there is no CPU fallback)")
    return ops.FusionTables([(vo[p], vo[p + 1] - vo[p], ao[p], ao[p + 1] - ao[p]) for p in range(len(vo) - 1)], device)


def fuse_batch(visuals, audios, target_length):
    """The fused rows of every (visuals[p], audios[p]) pair - what interpolate_features(v, compute_optimal_path(
    compute_dtw(v, a)), target_length) returns for each - with one upload and one download for the whole batch."""
    dev = _dev()
    if len(visuals) != len(audios):
        raise ValueError("visuals and audios must have the same length")
    if not len(visuals):
        return []
    vs = [torch.as_tensor(x).float() for x in visuals]
    aus = [torch.as_tensor(x).float() for x in audios]
    if any(x.dim() != 2 for x in vs + aus):
        raise ValueError("XA must be a 2-dimensional array.")
    vo = exclusive_offsets([x.shape[0] for x in vs]).tolist()
    ao = exclusive_offsets([x.shape[0] for x in aus]).tolist()
    tables = fusion_tables(vo, ao, dev)
    fused, _ = fuse_batch_device(torch.cat(vs).contiguous().to(dev), torch.cat(aus).contiguous().to(dev), vo, ao,
                                 target_length, tables=tables)
    host = fused.cpu()
    return list(host.split(tables.out_rows(target_length).tolist()))
