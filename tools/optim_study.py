#!/usr/bin/env python3
"""Study: the optimiser step of the scorer's training loop, torch.optim.AdamW against optim.FusedAdamW.

Part 1, the step alone, on the real scorer's 28 parameters (9.67 M elements) with resident gradients:
  (a) torch.optim.AdamW.step() (its default foreach path - what the training script runs by default),
  (b) FusedAdamW.step() without the norm pass: 28 bytes per element (p, g, m, v read; p, m, v written),
  (c) FusedAdamW.step() with the norm pass (max_grad_norm set): 32 bytes per element.
Each variant owns a copy of the parameters, gradients and moments (155 MB).  Device events around every step();
--warmup (5) steps of each, then --steps (60) timed steps of each, once ALTERNATING a, b, c, a, b, c, ... (every step
finds the caches filled by the other two variants' 310 MB) and once BACK TO BACK (a variant's 155 MB working set may
stay in the 256 MiB Infinity Cache from one step to the next).  Medians and spreads in microseconds; achieved bytes/s
of (b) and (c) = their bytes per element * elements / median.

Part 2, the whole training step (scripts.train_av_model.train_step, full dimensions, Dropout active) at T = 300 and
T = 1800 rows, two models from the same initialisation, one stepping with torch.optim.AdamW and one with FusedAdamW:
--rounds (7) regions of --region (10) steps each, alternating, wall clock between device synchronisations.

Device events around a step() measure what the stream saw between them: where the host needs longer to enqueue a step
than the device to run it, that is the host's time ("host_us_per_step_call" says what the host spends).  The kernels' own
durations come from a kernel trace of part 1 in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/optim_study.py --skip-train-step

Prints one JSON line (and writes it to --out).  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/optim_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3


def spread_us(ms):
    us = [x * 1e3 for x in ms]
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "p10_us": round(sorted(us)[len(us) // 10], 2), "p90_us": round(sorted(us)[(9 * len(us)) // 10], 2),
            "runs": len(us)}


def timed_step(opt):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    opt.step()
    e.record()
    return s, e


def part1(dev, args):
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.optim import FusedAdamW
    torch.manual_seed(7)
    shapes = [tuple(p.shape) for p in AVBiLSTMModel().parameters()]
    elements = sum(int(torch.Size(s).numel()) for s in shapes)

    def copy():
        gen = torch.Generator(device=dev).manual_seed(11)
        params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        return params

    opts = {"a_torch_adamw": torch.optim.AdamW(copy(), lr=1e-4),
            "b_fused": FusedAdamW(copy(), lr=1e-4),
            "c_fused_with_norm": FusedAdamW(copy(), lr=1e-4, max_grad_norm=1.0)}
    for _ in range(args.warmup):
        for opt in opts.values():
            opt.step()
    torch.cuda.synchronize()
    pairs = {k: [] for k in opts}
    for _ in range(args.steps):
        for k, opt in opts.items():
            pairs[k].append(timed_step(opt))
    torch.cuda.synchronize()
    alternating = {k: [s.elapsed_time(e) for s, e in v] for k, v in pairs.items()}
    back_to_back = {}
    for k, opt in opts.items():
        for _ in range(args.warmup):
            opt.step()
        ev = [timed_step(opt) for _ in range(args.steps)]
        torch.cuda.synchronize()
        back_to_back[k] = [s.elapsed_time(e) for s, e in ev]
    # what the HOST spends in step() (launches only enqueue): where it exceeds the device time above, the events measure
    # the host, not the kernels - the kernels' own durations come from a kernel trace of this tool (--skip-train-step)
    host = {}
    for k, opt in opts.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            opt.step()
        host[k] = round((time.perf_counter() - t0) * 1e6 / args.steps, 2)
        torch.cuda.synchronize()
    out = {"tensors": len(shapes), "elements": elements, "host_us_per_step_call": host, "working_set_mb_per_variant": round(16 * elements / 1e6, 1),
           "warmup": args.warmup, "steps": args.steps, "alternating": {}, "back_to_back": {}}
    bytes_per_element = {"b_fused": 28, "c_fused_with_norm": 32}
    for name, runs in (("alternating", alternating), ("back_to_back", back_to_back)):
        for k, ms in runs.items():
            res = spread_us(ms)
            if k in bytes_per_element:
                tbs = bytes_per_element[k] * elements / (res["median_us"] * 1e-6) / 1e12
                res.update(bytes_per_element=bytes_per_element[k], achieved_tb_per_s=round(tbs, 3),
                           share_of_achievable_hbm=round(tbs / HBM_ACHIEVABLE_TBS, 3))
            out[name][k] = res
        med = {k: out[name][k]["median_us"] for k in runs}
        out[name]["a_over_b"] = round(med["a_torch_adamw"] / med["b_fused"], 3)
        out[name]["a_over_c"] = round(med["a_torch_adamw"] / med["c_fused_with_norm"], 3)
        out[name]["c_not_slower_than_a"] = med["c_fused_with_norm"] <= med["a_torch_adamw"]
    out["stats_c"] = opts["c_fused_with_norm"].stats()
    return out


def part2(dev, args):
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.optim import FusedAdamW
    from avsum_amd.scripts.train_av_model import train_step
    out = {}
    for t in args.lengths:
        torch.manual_seed(7)
        a = AVBiLSTMModel()
        b = AVBiLSTMModel()
        b.load_state_dict(a.state_dict())
        a, b = a.to(dev).train(), b.to(dev).train()
        runs = {"torch_adamw": (a, torch.optim.AdamW(a.parameters(), lr=1e-4)),
                "fused_adamw": (b, FusedAdamW(b.parameters(), lr=1e-4))}
        gen = torch.Generator().manual_seed(100 + t)
        feats = {"visual": torch.randn(t, 4096, generator=gen), "audio": torch.randn(t, 296, generator=gen)}
        scores = torch.rand(t * 30, generator=gen) * 4 + 1

        def region(model, opt):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.region):
                train_step(model, opt, feats, scores, dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.region

        for model, opt in runs.values():
            for _ in range(3):
                train_step(model, opt, feats, scores, dev)
        ms = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, (model, opt) in runs.items():
                ms[k].append(region(model, opt))
        res = {k: {"median_ms_per_step": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                   "max_ms": round(max(v), 4), "regions": len(v), "steps_per_region": args.region}
               for k, v in ms.items()}
        res["torch_over_fused"] = round(res["torch_adamw"]["median_ms_per_step"] /
                                        res["fused_adamw"]["median_ms_per_step"], 4)
        res["separated"] = (min(ms["torch_adamw"]) > max(ms["fused_adamw"])
                            or min(ms["fused_adamw"]) > max(ms["torch_adamw"]))
        out[str(t)] = res
    out["lstm_split_errors"] = ops.lstm_split_errors(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 1800])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--region", type=int, default=10)
    ap.add_argument("--skip-train-step", action="store_true", help="part 1 only (for a run under a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.steps < 50:
        raise SystemExit("optim_study: at least 5 warm-up steps and 50 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("optim_study needs an MI355X: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "step_alone": part1(dev, args),
           "train_step": None if args.skip_train_step else part2(dev, args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
