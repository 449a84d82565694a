#!/usr/bin/env python3
"""Study: what the pairwise ranking loss (loss.py, libavsum_loss.so) costs, alone and inside the batched training step.

Part 1, forward plus backward of loss.rank_loss for 8 videos of T rows each (T = 300, 1800, 5000), both kinds, beside
two baselines on the same rows:
  seq_mse   ops.seq_mse with one target per row, forward plus backward: the O(R) loss the step already has
  dense     the [T, T] torch formulation a user would otherwise write (softplus(-scale * d) or clamp(margin - d) under a
            y_i > y_j mask, per video, fp32, autograd): its time and its peak device memory above what was held before
Device events around --inner (10) forward + backward pairs in a row, --warmup (5) such groups first, then --steps (30)
timed groups, the variants ALTERNATING.  The pair kernel evaluates exp, log1p and a division in fp64 per ordered pair:
pairs_per_second = 8 * T * T / time says what that costs.  The memory of rank_loss is derived, not measured: the
workspace of 20 bytes per row, g and the outputs - O(R).

Part 2, the whole training step (scripts.train_av_model.train_step_batch, 8 videos, full dimensions, Dropout seeded) at
--step-lengths (8 x 300 and 8 x 1800 rows; 8 x 5000 with --long): loss="mse" with targets="video" - the default, bit for
bit the step of the parent commit (tests/test_gpu_rank_loss.py holds it to that) - against targets="shots" with "mse" and
with "mse+rank" of both kinds; --rounds (7) regions of --region (5) steps each, the variants ALTERNATING, wall clock
between device synchronisations.  Launches per step are counted with torch.profiler around ONE step per variant, after
the timed regions.

--root DIR imports avsum_amd from another built checkout, e.g. the parent commit's: a tree without loss.py gets part 2's
default variant only.

Prints one JSON line (and writes it to --out).  Run it under its own time limit, e.g.
  timeout -k 10 900 python tools/rank_loss_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

SEED = 2024
VIDEOS = 8


def spread(values, unit, digits=3):
    values = sorted(values)
    return {f"median_{unit}": round(statistics.median(values), digits), f"min_{unit}": round(values[0], digits),
            f"max_{unit}": round(values[-1], digits), "runs": len(values)}


def dense_loss(torch, s, y, offsets, kind, scale, margin):
    losses = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        d = s[a:b, None] - s[None, a:b]
        pair = y[a:b, None] > y[None, a:b]
        term = torch.nn.functional.softplus(-scale * d) if kind == "logistic" else torch.clamp(margin - d, min=0.0)
        losses.append((term * pair).sum() / pair.sum().clamp(min=1))
    return torch.stack(losses)


def part1(torch, dev, args):
    from avsum_amd import loss as avloss, ops
    out = {}
    for t in args.lengths:
        rows = VIDEOS * t
        offsets = [v * t for v in range(VIDEOS + 1)]
        gen = torch.Generator(device=dev).manual_seed(t)
        s = torch.rand(rows, device=dev, generator=gen).requires_grad_(True)
        y = torch.rand(rows, device=dev, generator=gen) * 4 + 1
        dl = torch.full((VIDEOS,), 1.0 / VIDEOS, device=dev)
        rank_table, seq_table = ops.RankTables(offsets, rows, dev), ops.SeqTable(offsets, rows, dev)

        def run(make):
            s.grad = None
            make().backward(dl)

        variants = {"seq_mse": lambda: ops.seq_mse(s, y, seq_table)}
        for kind in avloss.KINDS:
            variants[f"rank_{kind}"] = lambda kind=kind: avloss.rank_loss(s, y, rank_table, kind, 1.0, 0.1)
            variants[f"dense_{kind}"] = lambda kind=kind: dense_loss(torch, s, y, offsets, kind, 1.0, 0.1)
        res = {"rows": rows, "ordered_pairs": VIDEOS * t * t, "inner": args.inner,
               "rank_workspace_bytes_derived": 20 * rows, "rank_saved_for_backward_bytes_derived": 4 * rows}
        for kind in avloss.KINDS:                                 # the two formulations agree before anything is timed
            a, b = variants[f"rank_{kind}"]().detach(), variants[f"dense_{kind}"]().detach()
            res[f"max_abs_diff_dense_{kind}"] = float((a - b).abs().max())

        def group(make):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(args.inner):
                run(make)
            en.record()
            return st, en

        for _ in range(args.warmup):
            for make in variants.values():
                group(make)
        torch.cuda.synchronize()
        events = {k: [] for k in variants}
        for _ in range(args.steps):
            for k, make in variants.items():
                events[k].append(group(make))
        torch.cuda.synchronize()
        for k in variants:
            r = spread([st.elapsed_time(en) * 1e3 / args.inner for st, en in events[k]], "us")
            if k.startswith("rank_"):
                r["ordered_pairs_per_second"] = round(VIDEOS * t * t / (r["median_us"] * 1e-6))
            res[k] = r
        for kind in avloss.KINDS:                                 # peak memory of one forward + backward, each alone
            for name in (f"rank_{kind}", f"dense_{kind}"):
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                run(variants[name])
                torch.cuda.synchronize()
                res[name]["peak_bytes_above_held"] = torch.cuda.max_memory_allocated(dev) - held
        out[str(t)] = res
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


def part2(torch, dev, args, loss_available):
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import train_step_batch
    settings = {"mse_video_targets": {}}
    if loss_available:
        settings["mse_shot_targets"] = dict(targets="shots", loss="mse")
        settings["mse+rank_logistic"] = dict(targets="shots", loss="mse+rank", rank_kind="logistic")
        settings["mse+rank_hinge"] = dict(targets="shots", loss="mse+rank", rank_kind="hinge")
    out = {}
    for t in args.step_lengths:
        gen = torch.Generator().manual_seed(100 + t)
        items = []
        for _ in range(VIDEOS):
            cuts = torch.sort(torch.randperm(30 * t - 1, generator=gen)[:t - 1] + 1).values
            bounds = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([30 * t])])
            feats = {"visual": torch.randn(t, 4096, generator=gen), "audio": torch.randn(t, 296, generator=gen),
                     "shots": torch.stack([bounds[:-1], bounds[1:]], 1)}
            items.append((feats, torch.rand(t * 30, generator=gen) * 4 + 1))
        torch.manual_seed(7)
        first = AVBiLSTMModel()
        runs = {}
        for name in settings:
            model = AVBiLSTMModel()
            model.load_state_dict(first.state_dict())
            model = model.to(dev).train().seed_dropout(SEED)
            runs[name] = (model, torch.optim.AdamW(model.parameters(), lr=1e-4))

        def step(name):
            model, opt = runs[name]
            return train_step_batch(model, opt, items, dev, **settings[name])

        def region(name):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.region):
                step(name)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.region

        for name in settings:
            for _ in range(3):
                step(name)
        ms = {name: [] for name in settings}
        for _ in range(args.rounds):
            for name in settings:
                ms[name].append(region(name))
        res = {name: dict(spread(ms[name], "ms_per_step", 4), steps_per_region=args.region) for name in settings}
        for name in settings:
            res[name]["launches_per_step"] = count_launches(torch, lambda: step(name))
        base = ms["mse_video_targets"]
        for name in settings:
            if name != "mse_video_targets":
                res[name]["over_default"] = round(statistics.median(ms[name]) / statistics.median(base), 4)
                res[name]["separated_from_default"] = min(base) > max(ms[name]) or min(ms[name]) > max(base)
        out[f"8x{t}"] = res
    out["lstm_split_errors"] = ops.lstm_split_errors(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose avsum_amd is measured (default: this one)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 1800, 5000])
    ap.add_argument("--step-lengths", type=int, nargs="+", default=[300, 1800])
    ap.add_argument("--long", action="store_true", help="add 8 x 5000 rows to part 2")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--region", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.warmup < 3 or args.steps < 10 or args.rounds < 5:
        raise SystemExit("rank_loss_study: at least 3 warm-up groups, 10 timed groups and 5 rounds")
    if args.long:
        args.step_lengths = list(args.step_lengths) + [5000]
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_loss_study needs an MI355X: a timing taken anywhere else says nothing about it")
    import avsum_amd
    loss_available = os.path.exists(os.path.join(avsum_amd.__path__[0], "loss.py"))
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "root": os.path.abspath(args.root), "loss_available": loss_available,
           "loss_alone": part1(torch, dev, args) if loss_available else None,
           "training_step": None if args.skip_steps else part2(torch, dev, args, loss_available)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
