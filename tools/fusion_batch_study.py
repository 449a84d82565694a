#!/usr/bin/env python3
"""Study: the fusion step of the configs[2] leg, per-video loop against one batched call.

Layout: synthetic.config(2) (50 videos of U[2000, 10000] frames), one row per 30-frame shot of synthetic.uniform_shots
exactly as bench.py builds them, D = 512, seeded random rows (ReLU of Gaussians, as the embedded streams are ReLU
outputs).  After a warm-up of both, the two forms alternate within one process, --rounds times each:

  (a) the per-video loop as bench.py's configs[2] leg writes it: compute_dtw_device, ops.dtw_path, plen.item(),
      torch.unique, ops.gather_scale - five launches and one host round trip per video;
  (b) one ops.fusion_batch call on prebuilt ops.FusionTables - the same values in a fixed number of launches.

Also times (batched form only) a many-small-pairs case: --small-pairs pairs of 1-12 rows, D = 16.
Wall-clock ms per step around a device synchronise (the loop's cost IS its host round trips, which device events would
not see).  Prints one JSON line.  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/fusion_batch_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small-pairs", type=int, default=10000)
    args = ap.parse_args()
    from avsum_amd import ops, synthetic
    from avsum_amd.features import fusion
    dev = torch.device("cuda", 0)
    cfg = synthetic.config(2, videos=args.videos)
    shot_rows = [0]
    for ln in cfg["lengths"]:
        shot_rows.append(shot_rows[-1] + len(synthetic.uniform_shots(ln)))
    gen = torch.Generator().manual_seed(7)
    v512 = torch.relu(torch.randn((shot_rows[-1], 512), generator=gen)).to(dev)
    a512 = torch.relu(torch.randn((shot_rows[-1], 512), generator=gen)).to(dev)
    nvid = len(cfg["lengths"])

    def loop(keep=None):
        fused_rows = 0
        for v in range(nvid):
            rows = slice(shot_rows[v], shot_rows[v + 1])
            cost = fusion.compute_dtw_device(v512[rows], a512[rows])
            path, plen, _ = ops.dtw_path(cost)
            uniq, counts = torch.unique(path[:int(plen.item()), 0], return_counts=True)
            out = ops.gather_scale(v512[rows].contiguous(), uniq, counts.double() / counts.sum())
            fused_rows += out.shape[0]
            if keep is not None:
                keep.append(out)
        return fused_rows

    tables = fusion.fusion_tables(shot_rows, None, dev)

    def batch():
        return ops.fusion_batch(tables, v512, a512)["fused"].shape[0]

    assert loop() == batch() == shot_rows[-1]          # warm-up of both forms (and of the allocator)
    kept = []
    loop(kept)                                         # the two forms compute the same rows, bit for bit
    same = bool(torch.equal(torch.cat(kept), ops.fusion_batch(tables, v512, a512)["fused"]))
    del kept
    t_loop, t_batch = [], []
    for _ in range(args.rounds):
        t_loop.append(wall_ms(loop))
        t_batch.append(wall_ms(batch))

    rng = np.random.default_rng(7)
    ns, ms = rng.integers(1, 13, args.small_pairs), rng.integers(1, 13, args.small_pairs)
    vo, ao = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(ms)])
    vs = torch.randn((int(vo[-1]), 16), generator=gen).to(dev)
    au = torch.randn((int(ao[-1]), 16), generator=gen).to(dev)
    stables = fusion.fusion_tables(vo.tolist(), ao.tolist(), dev)
    small = lambda: ops.fusion_batch(stables, vs, au)["fused"].shape[0]
    small()
    t_small = [wall_ms(small) for _ in range(args.rounds)]

    out = {"layout": {"videos": nvid, "shots": shot_rows[-1], "rows_per_video": [min(np.diff(shot_rows).tolist()),
                                                                               max(np.diff(shot_rows).tolist())],
                      "d": 512, "classes": tables.class_count, "cells": tables.cells},
           "loop_per_video": spread(t_loop), "fusion_batch": spread(t_batch), "same_bits": same,
           "ratio_of_medians": round(statistics.median(t_loop) / statistics.median(t_batch), 2),
           "separated": min(t_loop) > max(t_batch),
           "small_pairs": {"pairs": args.small_pairs, "d": 16, "classes": stables.class_count, **spread(t_small)},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
