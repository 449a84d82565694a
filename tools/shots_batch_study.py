#!/usr/bin/env python3
"""Study: shot detection and frame sampling of a ragged batch, the per-video loop against one batched pass.

Batch: BASELINE configs[1]'s layout (25 videos, lengths ~N(1800, 300), 224x224 frames resident in HBM: 6.8 GB) filled
with synthetic.make_frames_scenes (a new scene every 60 frames, so the detector has cuts to find); --videos /
--mean-frames shrink it.  After a warm-up of both, the two forms alternate within one process, --rounds (5) times each:

  (a) loop:  per video detect_shots (one download of the sums and the host threshold loop), then per video the sample
             list by sample_shot_indices per shot, its upload and torch's index_select;
  (b) batch: detect_shots_batch + sample_frames (five launches and a memset, one gather, ONE download).

Wall-clock ms per call, host work and transfers included (that IS the difference), and whether the two agree.  Then the
gather alone on the batch's sample index, device events over --gather-reps launches each, alternating: ops.gather_rows
against torch.index_select, as GB/s of bytes read + bytes written.  Prints one JSON line.  Run it under its own time
limit, e.g.
  timeout -k 10 600 python tools/shots_batch_study.py"""
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
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=None)
    ap.add_argument("--mean-frames", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gather-reps", type=int, default=5)
    args = ap.parse_args()
    from avsum_amd import ops, synthetic
    from avsum_amd.features.extractors import sample_shot_indices
    from avsum_amd.features.shots import detect_shots, detect_shots_batch, sample_frames
    dev = torch.device("cuda", 0)
    cfg = synthetic.config(1, videos=args.videos, mean_frames=args.mean_frames)
    lengths = cfg["lengths"]
    offsets = np.asarray(synthetic.offsets_of(lengths), dtype=np.int64)
    frames = synthetic.make_frames_scenes(lengths, dev, cfg["seed"])
    plan = ops.ShotTables(offsets, device=dev)

    def loop():
        shots, picked = [], []
        for a, b in zip(offsets[:-1], offsets[1:]):
            video = frames[a:b]
            found = detect_shots(video)
            idx = [i for s, e in found for i in sample_shot_indices(s, e)]
            picked.append(video.index_select(0, torch.tensor(idx, dtype=torch.int64).to(dev)))
            shots.append(found)
        return shots, torch.cat(picked)

    def batch():
        res = detect_shots_batch(frames, plan)
        dense, groups = sample_frames(frames, res)
        return res.host(), dense, groups, res

    (want_shots, want_dense), (got_shots, got_dense, groups, res) = loop(), batch()     # warm-up of both forms
    agree = {"shots_equal": got_shots == want_shots, "frames_equal": bool(torch.equal(got_dense, want_dense))}
    del want_dense, got_dense
    t_loop, t_batch = [], []
    for _ in range(args.rounds):
        t_loop.append(wall_ms(loop)[0])
        t_batch.append(wall_ms(batch)[0])

    # the gather alone: the same rows by the kernel (count read on the device) and by index_select
    f = int(res.host_tables()["counts"][1])
    index = res.sample_index[:f].contiguous()
    out = torch.empty((res.plan.sample_cap,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=dev)
    out_t = torch.empty((f,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=dev)
    run_k = lambda: ops.gather_rows(frames, res.sample_index, res.counts[1:2], out)
    run_t = lambda: torch.index_select(frames, 0, index, out=out_t)
    run_k(), run_t()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[:f], out_t))
    g_k, g_t = [], []
    for _ in range(args.rounds):
        g_k.append(event_ms(run_k, args.gather_reps))
        g_t.append(event_ms(run_t, args.gather_reps))
    moved = 2.0 * f * frames[0].numel()
    gbs = lambda xs: round(moved / (statistics.median(xs) * 1e-3) / 1e9, 1)

    out_line = {"layout": {"videos": len(lengths), "frames": int(offsets[-1]), "frame_bytes": int(frames[0].numel()),
                           "shots": sum(len(s) for s in got_shots), "sampled_frames": f, "groups": int(groups.numel() - 1)},
                "loop": spread(t_loop), "batch": spread(t_batch),
                "ratio_of_medians": round(statistics.median(t_loop) / statistics.median(t_batch), 2),
                "separated": min(t_loop) > max(t_batch), **agree,
                "gather": {"bytes_moved": int(moved), "gather_rows": spread(g_k), "index_select": spread(g_t),
                           "gather_rows_gbs": gbs(g_k), "index_select_gbs": gbs(g_t), "equal": same,
                           "gather_rows_beats_index_select": statistics.median(g_k) < statistics.median(g_t)},
                "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out_line))


if __name__ == "__main__":
    main()
