#!/usr/bin/env python3
"""Study: the keyshot-summary F1 of a dataset, one device batch (evaluation.keyshots.keyshot_f1_device) against the numpy
oracle looped over the same problems (keyshot_summary_host + compute_temporal_f1).

Dataset: --videos (50) seeded videos of 3000 .. 10 000 frames, detector-like shots (one per 15 .. 60 frames, tiling the
video), one prediction and --users (20) annotator score rows: (users + 1) x videos knapsacks, 1050 by default.

  (a) keyshot_f1_device with the shots as host lists: validation and one upload of the shot table, one concatenation of
      the score rows, three launches, one download of the int64 [V, U, 3] table, the host finish;
  (b) the same with every table resident (ops.SummaryTables and the shot table prepared once): three launches + the
      download + the finish - what a caller holding a ShotBatchResult pays;
  (c) the host oracle: keyshot_summary_host for every (row, video), then compute_temporal_f1 per (video, user), in this
      one process (numpy with the threads the environment grants).

Wall-clock ms per call behind a device synchronise, a warm-up first, (a) and (b) alternating --rounds (5) times, (c)
--host-rounds (2) times.  Also: device-event time of the knapsack launch alone for the batch, and for the longest video
alone with one score row (time per shot step = that / its shots).  Prints one JSON line.  Run it under its own time
limit, e.g.  timeout -k 10 600 python tools/keyshots_study.py"""
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


def event_ms(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / repeats


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs": len(xs)}


def make_dataset(videos, users, seed):
    rng = np.random.default_rng(seed)
    lengths = [int(n) for n in rng.integers(3000, 10001, videos)]
    shots = []
    for n in lengths:
        bounds, s = [0], 0
        while s < n:
            s = min(n, s + int(rng.integers(15, 61)))
            bounds.append(s)
        shots.append(list(zip(bounds[:-1], bounds[1:])))
    total = sum(lengths)
    t = np.arange(total, dtype=np.float64)
    rows = [np.clip(0.5 + 0.4 * np.sin(t / rng.uniform(20, 90) + rng.uniform(0, 6)) + 0.1 * rng.standard_normal(total), 0, 1)
            for _ in range(users + 1)]
    return lengths, shots, np.stack(rows).astype(np.float32)


def host_pipeline(rows, lengths, shots, off):
    from avsum_amd.evaluation.keyshots import keyshot_summary_host
    from avsum_amd.evaluation.metrics import compute_temporal_f1
    f1 = np.full((len(lengths), rows.shape[0] - 1), np.nan)
    for v, (n, sh) in enumerate(zip(lengths, shots)):
        segs = []
        for r in range(rows.shape[0]):
            picked = keyshot_summary_host(rows[r, off[v]:off[v + 1]], sh, n)[0]
            segs.append([s for s, p in zip(sh, picked) if p])
        for u in range(1, rows.shape[0]):
            if segs[0] and segs[u]:
                f1[v, u - 1] = compute_temporal_f1(segs[0], segs[u], n)
    return f1.mean(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--users", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from avsum_amd import ops
    from avsum_amd.evaluation.keyshots import _upload_shot_lists, f1_from_overlap, keyshot_f1_device
    dev = torch.device("cuda", 0)
    lengths, shots, rows = make_dataset(args.videos, args.users, args.seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    scores = torch.from_numpy(rows).to(dev)
    pred, users = scores[0], scores[1:]

    shot_offsets, shot_table, cap = _upload_shot_lists(shots, lengths, dev)
    plan = ops.SummaryTables(off, 0.15, cap, dev)

    def resident():
        sums = ops.shot_value_sums(plan, scores, shot_offsets, shot_table)
        out = ops.knapsack_batch(plan, sums, shot_offsets, shot_table)
        counts = ops.mask_overlap_counts(plan, out["mask"][0], out["mask"][1:]).cpu().numpy()
        return f1_from_overlap(counts).mean(axis=1)

    got = keyshot_f1_device(pred, users, off, shots)[0]                  # warm-up of both device forms
    got_resident = resident()
    t_lists, t_resident = [], []
    for _ in range(args.rounds):
        t_lists.append(wall_ms(lambda: keyshot_f1_device(pred, users, off, shots))[0])
        t_resident.append(wall_ms(resident)[0])
    t_host, want = [], None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        want = host_pipeline(rows, lengths, shots, off)
        t_host.append((time.perf_counter() - t0) * 1e3)

    sums = ops.shot_value_sums(plan, scores, shot_offsets, shot_table)
    sums_ms = event_ms(lambda: ops.shot_value_sums(plan, scores, shot_offsets, shot_table), 20)
    knap_ms = event_ms(lambda: ops.knapsack_batch(plan, sums, shot_offsets, shot_table), 20)
    longest = int(np.argmax([len(s) for s in shots]))
    one_off, one_table, one_cap = _upload_shot_lists([shots[longest]], [lengths[longest]], dev)
    one_plan = ops.SummaryTables([0, lengths[longest]], 0.15, one_cap, dev)
    one_scores = scores[0, off[longest]:off[longest + 1]].contiguous()
    one_sums = ops.shot_value_sums(one_plan, one_scores, one_off, one_table)
    one_ms = event_ms(lambda: ops.knapsack_batch(one_plan, one_sums, one_off, one_table), 50)

    out = {"layout": {"videos": len(lengths), "users": args.users, "problems": (args.users + 1) * len(lengths),
                      "frames": int(off[-1]), "n_min": min(lengths), "n_max": max(lengths), "shots": cap,
                      "max_capacity": plan.max_capacity, "words": plan.words},
           "device_host_lists": spread(t_lists), "device_resident_tables": spread(t_resident),
           "host_oracle": spread(t_host),
           "ratio_host_over_device_lists": round(statistics.median(t_host) / statistics.median(t_lists), 1),
           "ratio_host_over_device_resident": round(statistics.median(t_host) / statistics.median(t_resident), 1),
           "separated": min(t_host) > max(t_lists),
           "kernels_event_ms": {"shot_value_sums": round(sums_ms, 4), "knapsack_batch": round(knap_ms, 4)},
           "longest_video": {"frames": lengths[longest], "shots": len(shots[longest]),
                             "capacity": int(one_plan.capacity[0]), "knapsack_ms": round(one_ms, 4),
                             "us_per_shot_step": round(one_ms * 1e3 / len(shots[longest]), 4)},
           "f1_equal": bool(np.array_equal(got, want, equal_nan=True) and np.array_equal(got_resident, want, equal_nan=True)),
           "mean_f1": float(np.mean(got)), "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
