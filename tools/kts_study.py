#!/usr/bin/env python3
"""Study: kernel temporal segmentation of a dataset, one device batch (features.kts.kts_batch_device) against the numpy
oracle (features.kts.kts_host).

Dataset: --videos (50) seeded videos whose frame counts spread like TVSum's, 1800 .. 9700 frames, --dim (4096) wide
features with planted segments (a unit vector per segment plus noise, generated on the device), subsampled at stride 15:
120 .. 647 samples per video, ncp = n - 1 (full depth).

  device: wall-clock ms of kts_batch_device on the resident features behind a device synchronise, a warm-up first,
          --rounds (7) times; then, in rounds of their own, the device-event time of the three entry points: the Gram
          launch, the scatter tables (three launches) and the dynamic programme with its shot table (two launches);
  host:   the wall time of kts_host on the shortest, the median and the longest video; the batch figure is
          EXTRAPOLATED from those three by a power law t = a n^p fitted to them (least squares in log-log).
          --host-all also runs the oracle on the subsampled rows of every video and reports the measured sum.

Prints one JSON line.  Run it under its own time limit, e.g.  timeout -k 10 600 python tools/kts_study.py"""
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


def make_dataset(videos, dim, seed, dev):
    rng = np.random.default_rng(seed)
    lengths = sorted(int(n) for n in np.linspace(1800, 9700, videos) + rng.integers(-40, 41, videos))
    lengths[0], lengths[-1] = 1800, 9700
    rng.shuffle(lengths)
    gen = torch.Generator(device=dev).manual_seed(seed)
    feats = torch.empty((sum(lengths), dim), dtype=torch.float32, device=dev)
    row, planted = 0, []
    for n in lengths:
        cuts, s = [], 0
        while n - s > 1100:
            s += int(rng.integers(300, 901))
            cuts.append(s)
        planted.append(cuts)
        for a, b in zip([0] + cuts, cuts + [n]):
            c = torch.randn(dim, generator=gen, device=dev)
            feats[row + a:row + b] = c / c.norm() + 0.002 * torch.randn((b - a, dim), generator=gen, device=dev)
        row += n
    return lengths, planted, feats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--stride", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host-all", action="store_true", help="also time the host oracle on every video")
    args = ap.parse_args()
    from avsum_amd import _abi, ops
    from avsum_amd.features.kts import kts_batch_device, kts_host
    dev = torch.device("cuda", 0)
    lengths, planted, feats = make_dataset(args.videos, args.dim, args.seed, dev)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    plan = ops.KtsTables(off, args.stride, device=dev)

    result = kts_batch_device(feats, plan)                                  # warm-up
    torch.cuda.synchronize()
    t_device = [wall_ms(lambda: kts_batch_device(feats, plan))[0] for _ in range(args.rounds)]
    t_with_download = [wall_ms(lambda: kts_batch_device(feats, plan).host())[0] for _ in range(args.rounds)]

    gram = result.gram
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    flags = torch.empty(plan.nvideos, dtype=torch.int64, device=dev)
    entries = (plan.k1_entries, plan.k_entries, plan.jt_entries, plan.p_entries)

    def scatters():
        _abi.check(_abi.lib().avs_kts_scatters_f64(ops._p(gram), ops._p(plan.videos_t), plan.nvideos, plan.max_n, ops._p(ws),
                                                   plan.workspace_bytes, *entries, ops._p(flags), ops._stream()),
                   "avs_kts_scatters_f64")

    gram_ms = event_ms(lambda: ops.kts_gram(plan, feats), 5)
    scatter_ms = event_ms(scatters, 5)
    segment_ms = event_ms(lambda: ops.kts_segment(plan, gram), 5)

    # the host oracle on three videos, the batch extrapolated
    order = np.argsort(plan.n)
    picks = [int(order[0]), int(order[len(order) // 2]), int(order[-1])]
    dev_host, host_rows, equal = result.host(), [], True
    for v in picks:
        x = feats[int(off[v]):int(off[v + 1])].cpu().numpy()
        t0 = time.perf_counter()
        cps, shots, costs, flag = kts_host(x, args.stride)
        host_rows.append({"video": v, "n": int(plan.n[v]), "ms": round((time.perf_counter() - t0) * 1e3, 1),
                          "change_points": int(cps.size)})
        equal = equal and shots == dev_host[v]["shots"] and \
            cps.tolist() == [-(-c // args.stride) for c in planted[v]]     # the first sample past a planted cut
    power, log_a = np.polyfit(np.log([r["n"] for r in host_rows]), np.log([r["ms"] for r in host_rows]), 1)
    host_batch_ms = float(np.exp(log_a + power * np.log(plan.n.astype(np.float64))).sum())
    host_all = None
    if args.host_all:                                  # the whole host loop on the subsampled rows (K, tables, programme)
        t_all, same = 0.0, True
        for v in range(plan.nvideos):
            x = feats[int(off[v]):int(off[v + 1]):args.stride].cpu().numpy()
            t0 = time.perf_counter()
            cps = kts_host(x, 1)[0]
            t_all += (time.perf_counter() - t0) * 1e3
            same = same and cps.tolist() == dev_host[v]["change_points"].tolist()
        host_all = {"ms": round(t_all, 1), "change_points_equal_device": bool(same),
                    "ratio_over_device": round(t_all / statistics.median(t_device), 1)}

    out = {"layout": {"videos": plan.nvideos, "dim": args.dim, "stride": args.stride, "frames": int(off[-1]),
                      "n_min": int(plan.n.min()), "n_max": int(plan.n.max()), "samples": int(plan.n.sum()),
                      "ncp": "n - 1", "gram_tiles": plan.ntiles, "workspace_mib": round(plan.workspace_bytes / 2 ** 20, 1),
                      "gram_mib": round(plan.k_entries * 8 / 2 ** 20, 1)},
           "dp_form": "one 1024-thread workgroup per video, stages separated by workgroup barriers",
           "launches": 6, "device_batch": spread(t_device), "device_batch_with_download": spread(t_with_download),
           "entry_points_event_ms": {"gram": round(gram_ms, 3), "scatters": round(scatter_ms, 3),
                                     "dp_and_shot_table": round(segment_ms - scatter_ms, 3),
                                     "segment_total": round(segment_ms, 3)},
           "host_oracle_three_videos": host_rows, "host_fit_power_of_n": round(float(power), 2),
           "host_batch_ms_extrapolated": round(host_batch_ms, 1), "host_all_videos": host_all,
           "ratio_host_extrapolated_over_device": round(host_batch_ms / statistics.median(t_device), 1),
           "three_videos_equal_host_and_planted": bool(equal),
           "change_points_found": int(result.totals[:, 0].sum().item()), "flags": int(result.totals[:, 3].sum().item()),
           "cpu_threads": torch.get_num_threads(), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
