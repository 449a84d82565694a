#!/usr/bin/env python3
"""Study: evaluating a dataset, the per-video loop (scripts.evaluate.evaluate) against one ragged batch
(scripts.evaluate.evaluate_batch).

Dataset: --videos (50) seeded synthetic videos of T drawn uniformly from 300..5000 rows (the range configs[1] / [2] put
through the scorer), visual [T, 4096] and audio [T, 296] Gaussian rows, float32 targets quantised to 81 levels (ties, as
annotation scores have).  The model is AVBiLSTMModel seeded with torch.manual_seed(7).  After a warm-up of both, the two
forms alternate within one process, --rounds (5) times each:

  (a) evaluate: per video an upload, a B = 1 model call, .cpu(), numpy's mean-threshold F1 and two SciPy calls;
  (b) evaluate_batch: one upload, one score_rows call, four metric launches, one download of an int64 [V, 10] table.

Wall-clock ms per call, host work and transfers included (that IS the difference).  Also times the metric part alone on
scores already on the device (summarize_scores_device against summarize_scores on downloaded pairs).  Prints one JSON
line.  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/eval_batch_study.py"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs": len(xs)}


def make_dataset(videos, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(300, 5001, videos).tolist()
    gen = torch.Generator().manual_seed(seed)
    items = []
    for t in lengths:
        feats = {"visual": torch.randn(t, 4096, generator=gen), "audio": torch.randn(t, 296, generator=gen)}
        items.append((feats, torch.floor(torch.rand(t, generator=gen) * 81) / 81))
    return items, lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from avsum_amd import ops
    from avsum_amd.evaluation.metrics import summarize_scores, summarize_scores_device
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.evaluate import evaluate, evaluate_batch, predict_dataset
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    model = AVBiLSTMModel().eval().to(dev)
    data, lengths = make_dataset(args.videos, args.seed)

    want, got = evaluate(model, data), evaluate_batch(model, data)      # warm-up of both forms (and of the allocator)
    diff = {k: abs(float(got[k]) - float(want[k])) for k in want}
    t_loop, t_batch = [], []
    for _ in range(args.rounds):
        t_loop.append(wall_ms(lambda: evaluate(model, data))[0])
        t_batch.append(wall_ms(lambda: evaluate_batch(model, data))[0])

    # the metric part alone, the scores already computed
    pairs = predict_dataset(model, data)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    tables = ops.EvalTables(offsets, dev)
    pred = torch.from_numpy(np.concatenate([p for p, _ in pairs])).to(dev)
    target = torch.from_numpy(np.concatenate([t for _, t in pairs])).to(dev)
    summarize_scores_device(pred, target, tables)
    t_host, t_dev = [], []
    for _ in range(args.rounds):
        t_host.append(wall_ms(lambda: summarize_scores(pairs))[0])
        t_dev.append(wall_ms(lambda: summarize_scores_device(pred, target, tables))[0])

    out = {"layout": {"videos": len(lengths), "rows": int(offsets[-1]), "t_min": min(lengths), "t_max": max(lengths),
                      "pair_comparisons": int(sum(t * t for t in lengths)), "target_dtype": "float32"},
           "evaluate_loop": spread(t_loop), "evaluate_batch": spread(t_batch),
           "ratio_of_medians": round(statistics.median(t_loop) / statistics.median(t_batch), 2),
           "separated": min(t_loop) > max(t_batch),
           "metrics_only": {"summarize_scores": spread(t_host), "summarize_scores_device": spread(t_dev)},
           "f1_equal": bool(got["f1"] == want["f1"]), "abs_diff": diff,
           "values": {k: float(got[k]) for k in got}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
