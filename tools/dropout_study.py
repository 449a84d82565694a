#!/usr/bin/env python3
"""Study: what counter-based Dropout (dropout.py, libavsum_dropout.so) costs the scorer's training step, against the
masks torch draws (models/_scorer_train.py::dropout_keep, the default).

Part 1, the two kernels alone, at the [R, 512] sizes of the training step (R = 300, 1800 and a batch of 8 videos) and at
one size that cannot stay in a cache (R = 131072: 256 MiB per tensor), beside the mask-tensor kernels they replace:
  apply     avsd_dropout_fwd_f32       reads x, writes out: 8 bytes per element          | ops.mul: 12 (x, mask, out)
  relu_bwd  avsd_relu_dropout_bwd_f32  reads dy, relu_out, writes out: 12 bytes          | ops.relu_dropout_bwd: 16
Device events around --inner (20) launches in a row, --warmup (5) such groups first, then --steps (50) timed groups of
each kernel, the four kernels ALTERNATING; time per launch = group time / inner.  Achieved bytes/s = the bytes above
over the median, and its share of the 8 TB/s HBM peak.  At the small sizes the operands stay in the caches and a launch
is a few microseconds: those rows measure the launch, the large size measures the kernel.  Per 32 bytes of traffic the
kernel does 40 32-bit integer multiplies (20 products of 32 x 32 -> 64 bits): the large size says whether the memory
or the vector ALU bounds it - if `apply` reaches the bytes/s of ops.mul's class, the memory does.

Part 2, the whole training step (scripts.train_av_model.train_step at T = 300 and T = 1800 rows, train_step_batch on 8
videos of 150 .. 450 rows, full dimensions, Dropout active): two models from the same initialisation, one drawing with
torch, one after seed_dropout(seed); --rounds (7) regions of --region (10) steps each, the two ALTERNATING, wall clock
between device synchronisations.  `separated` says whether the two variants' region times do not overlap at all;
otherwise the difference lies inside the run-to-run spread.  Launches per step are counted with torch.profiler around
ONE step per variant, after the timed regions (profiling slows the host: never inside them).

--root DIR imports avsum_amd from another checkout of this project (built), e.g. the parent commit's: a tree without
dropout.py gets part 2's torch variant only, which is that tree's default path.  Run the two trees one after the other
in one job, twice, and compare the same variant across processes for the spread between processes.

The memory the counter path saves is derived, not measured: 2 * R * hidden * 4 bytes per step, the two masks that are
no longer held for the backward.

Prints one JSON line (and writes it to --out).  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/dropout_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

HBM_PEAK_TBS = 8.0
HIDDEN = 512
SEED = 2024


def spread(values, unit, digits=3):
    values = sorted(values)
    return {f"median_{unit}": round(statistics.median(values), digits), f"min_{unit}": round(values[0], digits),
            f"max_{unit}": round(values[-1], digits), "runs": len(values)}


def part1(torch, dev, args):
    from avsum_amd import dropout, ops
    out = {}
    for rows in args.kernel_rows:
        table = ops.SeqTable([0, rows], rows, dev)
        gen = torch.Generator(device=dev).manual_seed(rows)
        x = torch.randn(rows, HIDDEN, device=dev, generator=gen)
        y = torch.randn(rows, HIDDEN, device=dev, generator=gen)
        mask = dropout.keep_mask(SEED, 0.3, 0, 0, table, HIDDEN)
        buf = torch.empty_like(x)
        off = table.offsets_t
        kernels = {
            "apply": (8, lambda: dropout.apply(x, SEED, 0.3, 0, 0, off, out=buf)),
            "ops_mul": (12, lambda: ops.mul(x, mask)),
            "relu_bwd": (12, lambda: dropout.relu_bwd(x, y, SEED, 0.3, 0, 0, off, out=buf)),
            "ops_relu_dropout_bwd": (16, lambda: ops.relu_dropout_bwd(x, y, mask)),
        }
        assert torch.equal(kernels["apply"][1](), kernels["ops_mul"][1]())
        assert torch.equal(kernels["relu_bwd"][1](), kernels["ops_relu_dropout_bwd"][1]())

        def group(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.inner):
                fn()
            e.record()
            return s, e

        for _ in range(args.warmup):
            for _, fn in kernels.values():
                group(fn)
        torch.cuda.synchronize()
        pairs = {k: [] for k in kernels}
        for _ in range(args.steps):
            for k, (_, fn) in kernels.items():
                pairs[k].append(group(fn))
        torch.cuda.synchronize()
        res = {"elements": rows * HIDDEN, "inner": args.inner}
        for k, (bytes_per_element, _) in kernels.items():
            r = spread([s.elapsed_time(e) * 1e3 / args.inner for s, e in pairs[k]], "us")
            tbs = bytes_per_element * rows * HIDDEN / (r["median_us"] * 1e-6) / 1e12
            r.update(bytes_per_element=bytes_per_element, achieved_tb_per_s=round(tbs, 3),
                     share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 3))
            res[k] = r
        out[str(rows)] = res
    return out


def count_launches(torch, step):
    """Device kernels and copies of ONE call of step(), from torch.profiler; None where it cannot tell."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        device = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [e for e in device if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
        if not device:
            return None
        return {"kernels": len(device) - len(copies), "copies_and_memsets": len(copies)}
    except Exception as exc:  # noqa: BLE001 - the count is an extra: the timings above stand without it
        return {"error": repr(exc)}


def part2(torch, dev, args, counter_available):
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import train_step, train_step_batch
    variants = ["torch_masks"] + (["counter_masks"] if counter_available else [])
    gen = torch.Generator().manual_seed(100)

    def video(t):
        return ({"visual": torch.randn(t, 4096, generator=gen), "audio": torch.randn(t, 296, generator=gen)},
                torch.rand(t * 30, generator=gen) * 4 + 1)

    batch_lengths = [150, 450, 300, 210, 390, 270, 330, 300]             # 2400 rows
    workloads = {f"train_step_T{t}": ("one", video(t), t) for t in args.lengths}
    workloads["train_step_batch_8_videos"] = ("batch", [video(t) for t in batch_lengths], sum(batch_lengths))
    out = {}
    for name, (kind, data, rows) in workloads.items():
        torch.manual_seed(7)
        first = AVBiLSTMModel()
        runs = {}
        for v in variants:
            model = AVBiLSTMModel()
            model.load_state_dict(first.state_dict())
            model = model.to(dev).train()
            if v == "counter_masks":
                model.seed_dropout(SEED)
            runs[v] = (model, torch.optim.AdamW(model.parameters(), lr=1e-4))

        def step(model, opt):
            if kind == "one":
                return train_step(model, opt, data[0], data[1], dev)
            return train_step_batch(model, opt, data, dev)

        def region(model, opt):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.region):
                step(model, opt)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.region

        for model, opt in runs.values():
            for _ in range(3):
                step(model, opt)
        ms = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, (model, opt) in runs.items():
                ms[v].append(region(model, opt))
        res = {v: dict(spread(ms[v], "ms_per_step", 4), steps_per_region=args.region) for v in variants}
        for v, (model, opt) in runs.items():
            res[v]["launches_per_step"] = count_launches(torch, lambda: step(model, opt))
        if counter_available:
            a, b = ms["torch_masks"], ms["counter_masks"]
            res["counter_over_torch"] = round(statistics.median(b) / statistics.median(a), 4)
            res["separated"] = min(a) > max(b) or min(b) > max(a)
            res["mask_bytes_not_held_derived"] = 2 * rows * HIDDEN * 4
        out[name] = res
    out["lstm_split_errors"] = ops.lstm_split_errors(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose avsum_amd is measured (default: this one)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--kernel-rows", type=int, nargs="+", default=[300, 1800, 2400, 131072])
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 1800])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--region", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.steps < 50 or args.rounds < 5:
        raise SystemExit("dropout_study: at least 5 warm-up groups, 50 timed groups and 5 rounds")
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dropout_study needs an MI355X: a timing taken anywhere else says nothing about it")
    import avsum_amd
    counter_available = os.path.exists(os.path.join(avsum_amd.__path__[0], "dropout.py"))
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "root": os.path.abspath(args.root),
           "counter_available": counter_available,
           "kernels_alone": part1(torch, dev, args) if counter_available else None,
           "training_step": part2(torch, dev, args, counter_available)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
