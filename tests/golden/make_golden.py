#!/usr/bin/env python3
"""Generates the golden fixtures under tests/golden/ by IMPORTING the reference's own Python
(<reference>/models, features/fusion.py with a stub `fastdtw` module, utils, evaluation,
scripts/evaluate.py) and recording inputs + outputs.  Only data is written: no reference source text or bytecode.
Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py <reference checkout> [--only reference_classes]
"""
import argparse
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = None   # the reference checkout, from the command line
sys.dont_write_bytecode = True


def ref_modules():
    sys.path.insert(0, REF)
    sys.modules.setdefault("fastdtw", types.SimpleNamespace(fastdtw=None))  # fusion.py imports it at module level
    from models.av_model import AVBiLSTMModel
    from models.attention import MultiHeadSelfAttention
    from features import fusion
    from utils.alignments import align_shots_to_annotations
    from evaluation.metrics import compute_temporal_f1
    sys.path.pop(0)
    return AVBiLSTMModel, MultiHeadSelfAttention, fusion, align_shots_to_annotations, compute_temporal_f1


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().numpy().tobytes())
    return h.hexdigest()


def reference_classes():
    """reference_classes.npz: what tests/test_oracle_pins.py::test_against_reference_classes_directly compares the oracle
    with - the reference classes' forward (three shapes) and parameter gradients of AVBiLSTMModel(32, 12, 16),
    MultiHeadSelfAttention(48, 6), compute_dtw / interpolate_features, and both temporal-F1 functions."""
    AVBiLSTMModel, MHSA, fusion, _, tf1 = ref_modules()
    sys.path.insert(0, REF)
    from utils.shot_metrics import compute_f1
    sys.path.pop(0)
    from oracle import fusion as ofu
    out = {}
    g = torch.Generator().manual_seed(77)
    torch.manual_seed(3)
    m = AVBiLSTMModel(32, 12, 16).eval()
    out.update({"sd_" + k: v.numpy() for k, v in m.state_dict().items()})
    for b, t in ((1, 50), (4, 9), (2, 1)):
        v, a = torch.randn(b, t, 32, generator=g), torch.randn(b, t, 12, generator=g)
        with torch.no_grad():
            y = m(v, a)
        out[f"fwd_{b}x{t}_visual"], out[f"fwd_{b}x{t}_audio"], out[f"fwd_{b}x{t}_out"] = v.numpy(), a.numpy(), y.numpy()
    m.zero_grad()
    vg, ag = torch.randn(1, 13, 32, generator=g), torch.randn(1, 13, 12, generator=g)
    m(vg, ag).sum().backward()
    out["bwd_visual"], out["bwd_audio"] = vg.numpy(), ag.numpy()
    for k, p in m.named_parameters():
        out["grad_" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    at = MHSA(48, 6).eval()
    x = torch.randn(3, 21, 48, generator=g)
    with torch.no_grad():
        out["mhsa_out"] = at(x).numpy()
    out.update({"mhsa_sd_" + k: v.numpy() for k, v in at.state_dict().items()})
    out["mhsa_x"] = x.numpy()
    vv, aa = torch.randn(15, 8, generator=g), torch.randn(11, 8, generator=g)
    cost = fusion.compute_dtw(vv, aa)
    _, path = ofu.dtw_path(cost)
    out.update(dtw_v=vv.numpy(), dtw_a=aa.numpy(), dtw_cost=cost, dtw_path=path,
               interp=fusion.interpolate_features(vv, path, 9).numpy())
    segs = ([(0, 10), (20, 30)], [(5, 15), (20, 25)])
    out["temporal_f1"], out["shot_f1"] = tf1(*segs, 30), compute_f1(*segs, 30)
    np.savez_compressed(os.path.join(HERE, "reference_classes.npz"), **out)


def main():
    global REF
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference (the directory holding models/, features/, utils/)")
    ap.add_argument("--only", choices=["reference_classes"], default=None, help="write this one fixture only")
    args = ap.parse_args()
    REF = os.path.abspath(args.reference)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root (oracle/)
    if args.only == "reference_classes":
        reference_classes()
        print("golden fixture written to", HERE)
        return
    AVBiLSTMModel, MHSA, fusion, align, tf1 = ref_modules()
    torch.manual_seed(1234)
    m = AVBiLSTMModel(64, 24, 32).eval()
    g = torch.Generator().manual_seed(5)
    out = {"sd_" + k: v.numpy() for k, v in m.state_dict().items()}
    for name, (b, t) in {"b1": (1, 37), "b3": (3, 11), "t1": (1, 1)}.items():
        v, a = torch.randn(b, t, 64, generator=g), torch.randn(b, t, 24, generator=g)
        with torch.no_grad():
            y = m(v, a)
        out[f"{name}_visual"], out[f"{name}_audio"], out[f"{name}_out"] = v.numpy(), a.numpy(), y.numpy()
    np.savez_compressed(os.path.join(HERE, "scorer_small.npz"), **out)

    # full dims: parameters are NOT stored; they are reproduced from the seed by constructing the model in the
    # reference's order (that the mirror class does so is part of the drop-in contract) and checked by hash.
    torch.manual_seed(7)
    mf = AVBiLSTMModel().eval()
    gv = torch.Generator().manual_seed(1007)
    v = torch.randn(1, 300, 4096, generator=gv)
    a = torch.zeros(1, 300, 296)
    with torch.no_grad():
        y = mf(v, a)
    np.savez_compressed(os.path.join(HERE, "scorer_full.npz"), seed=7, input_seed=1007,
                        sd_sha256=sd_hash(mf.state_dict()), keys=np.array(sorted(mf.state_dict().keys())),
                        out=y.numpy(), n_params=sum(p.numel() for p in mf.parameters()))

    # configs[1] / configs[3] sequence lengths: the same seeded full-size reference class on
    # T = 1800 and T = 5000 steps; inputs are regenerated from their seeds, only the scores are stored
    long_out = {"seed": 7, "sd_sha256": sd_hash(mf.state_dict())}
    for t_len, in_seed in ((1800, 11800), (5000, 15000)):
        v = torch.randn(1, t_len, 4096, generator=torch.Generator().manual_seed(in_seed))
        with torch.no_grad():
            y = mf(v, torch.zeros(1, t_len, 296))
        long_out[f"t{t_len}_input_seed"], long_out[f"t{t_len}_out"] = in_seed, y.numpy()
    np.savez_compressed(os.path.join(HERE, "scorer_long.npz"), **long_out)

    # MultiHeadSelfAttention(1024, 4) at T = 5000 (the reference materialises 4 x 5000 x 5000 scores): 64 output
    # rows at a fixed stride are stored, parameters and input come from their seeds
    torch.manual_seed(4242)
    atl = MHSA(1024, 4).eval()
    xl = torch.randn(1, 5000, 1024, generator=torch.Generator().manual_seed(4243))
    with torch.no_grad():
        yl = atl(xl)
    rows = np.arange(0, 5000, 79)[:64]
    np.savez_compressed(os.path.join(HERE, "mhsa_long.npz"), seed=4242, input_seed=4243, t=5000, rows=rows,
                        sd_sha256=sd_hash(atl.state_dict()), out_rows=yl[0, rows].numpy(),
                        out_abs_sum=float(yl.double().abs().sum()))

    torch.manual_seed(99)
    at = MHSA(64, 4).eval()
    x = torch.randn(2, 19, 64, generator=g)
    with torch.no_grad():
        ya = at(x)
    oa = {"sd_" + k: v.numpy() for k, v in at.state_dict().items()}
    oa.update(x=x.numpy(), out=ya.numpy())
    np.savez_compressed(os.path.join(HERE, "mhsa_small.npz"), **oa)

    vv, aa = torch.randn(23, 16, generator=g), torch.randn(31, 16, generator=g)
    cost = fusion.compute_dtw(vv, aa)
    path = np.array([[0, 0], [0, 1], [1, 2], [2, 2], [2, 3], [2, 4], [5, 5], [5, 6]])
    interp = fusion.interpolate_features(vv, path, 3)
    ann = np.arange(100, dtype=np.float64)
    al = align([(0, 50), (60, 200), (10, 11)], ann, 30)
    np.savez_compressed(os.path.join(HERE, "fusion_metrics.npz"), v=vv.numpy(), a=aa.numpy(), cost=cost, path=path,
                        interp=interp.numpy(), interp_dtype=str(interp.dtype), ann=ann, align=al.numpy(),
                        tf1=tf1([(0, 10), (20, 30)], [(5, 15), (20, 25)], 30))
    reference_classes()
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
