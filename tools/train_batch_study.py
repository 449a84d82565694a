#!/usr/bin/env python3
"""Study: a training step on eight videos, the loop as it stands (eight scripts.train_av_model.train_step calls, one video
each) against one ragged batch (scripts.train_av_model.train_step_batch on the same eight videos).

Full dimensions (visual 4096, audio 296, hidden 512), eight seeded synthetic videos of T rows each, for T = 300 and
T = 1800 (--lengths).  Dropout is active, AdamW steps are real.  After a warm-up of both forms at that length the two
alternate within one process, --rounds (7) timed regions each:

  (a) eight consecutive train_step calls: per video an upload, forward, F.mse_loss, backward, AdamW step, loss.item();
  (b) one train_step_batch call: one upload, train_rows, ops.seq_mse(...).mean(), backward, ONE AdamW step, one download.

Wall-clock ms per region between device synchronisations, host work and uploads included (both forms upload the same
bytes); videos/s = 8 / region.  Note what is compared: (a) takes eight optimiser steps, (b) one step on the averaged
gradient - the figure is videos through forward + backward per second, not steps.  In further rounds of their own (events
are barriers between kernels, so not in the timed regions above) the LSTM forward and backward launches of both forms are
bracketed with device events: their share of a region.  Prints one JSON line.  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/train_batch_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

VIDEOS = 8


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs": len(xs)}


def make_items(t, seed):
    gen = torch.Generator().manual_seed(seed)
    return [({"visual": torch.randn(t, 4096, generator=gen), "audio": torch.randn(t, 296, generator=gen)},
             torch.rand(t * 30, generator=gen) * 4 + 1) for _ in range(VIDEOS)]


class LstmEvents:
    """Brackets ops.lstm_train_fwd / ops.lstm_bwd with device events while installed."""

    def __init__(self, ops):
        self.ops, self.pairs = ops, {"fwd": [], "bwd": []}
        self.real = (ops.lstm_train_fwd, ops.lstm_bwd)

    def _wrap(self, kind, fn):
        def timed(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **kw)
            e.record()
            self.pairs[kind].append((s, e))
            return r
        return timed

    def __enter__(self):
        self.ops.lstm_train_fwd = self._wrap("fwd", self.real[0])
        self.ops.lstm_bwd = self._wrap("bwd", self.real[1])
        return self

    def __exit__(self, *exc):
        self.ops.lstm_train_fwd, self.ops.lstm_bwd = self.real

    def take(self):
        """(forward ms, backward ms, launches of each) since the last take."""
        torch.cuda.synchronize()
        out = tuple(sum(s.elapsed_time(e) for s, e in self.pairs[k]) for k in ("fwd", "bwd"))
        n = (len(self.pairs["fwd"]), len(self.pairs["bwd"]))
        self.pairs = {"fwd": [], "bwd": []}
        return out + n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 1800])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import train_step, train_step_batch
    if not torch.cuda.is_available():
        raise SystemExit("train_batch_study needs an MI355X: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    model = AVBiLSTMModel().to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)

    def loop(items):
        return [train_step(model, opt, feats, labels, dev) for feats, labels in items]

    def batch(items):
        return train_step_batch(model, opt, items, dev)

    out = {"videos_per_region": VIDEOS, "rounds": args.rounds, "warmup": args.warmup, "lengths": {}}
    for t in args.lengths:
        items = make_items(t, args.seed + t)
        for _ in range(args.warmup):
            loop(items)
            batch(items)
        t_loop, t_batch = [], []
        for _ in range(args.rounds):
            t_loop.append(wall_ms(lambda: loop(items))[0])
            t_batch.append(wall_ms(lambda: batch(items))[0])
        ev = {"loop": [], "batch": []}
        with LstmEvents(ops) as rec:
            for _ in range(args.rounds):
                ms = wall_ms(lambda: loop(items))[0]
                ev["loop"].append((ms,) + rec.take())
                ms = wall_ms(lambda: batch(items))[0]
                ev["batch"].append((ms,) + rec.take())
        med_a, med_b = statistics.median(t_loop), statistics.median(t_batch)
        res = {"rows_per_video": t,
               "a_eight_train_step": dict(spread(t_loop), videos_per_s=round(VIDEOS / med_a * 1e3, 1)),
               "b_one_train_step_batch": dict(spread(t_batch), videos_per_s=round(VIDEOS / med_b * 1e3, 1)),
               "ratio_b_over_a_videos_per_s": round(med_a / med_b, 3),
               "separated": min(t_loop) > max(t_batch) or min(t_batch) > max(t_loop)}
        for k, name in (("loop", "a_with_lstm_events"), ("batch", "b_with_lstm_events")):
            res[name] = {"region": spread([x[0] for x in ev[k]]),
                         "lstm_fwd": spread([x[1] for x in ev[k]]), "lstm_bwd": spread([x[2] for x in ev[k]]),
                         "lstm_fwd_launches": ev[k][0][3], "lstm_bwd_launches": ev[k][0][4]}
        out["lengths"][str(t)] = res
    out["lstm_split_errors"] = ops.lstm_split_errors(dev)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
