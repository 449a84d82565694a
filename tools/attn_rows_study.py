#!/usr/bin/env python3
"""Study: training through MultiHeadSelfAttention, the unfused backward (_MHSAFunction: batched GEMMs over materialised
[H, T, tp] score buffers, a Python loop over the batch) against the fused ragged-batch path (forward_rows:
libavsum_attn.so, nothing of size [T, T] in memory).  E = 1024, H = 4 (D = 256) unless told otherwise.

Part 1, one sequence of T = 300 / 1800 / 5000 rows, forward + backward of ``module(x).sum()``-like work (a fixed random
upstream gradient), three variants ALTERNATING step by step after --warmup steps of each:
  unfused        module.forward, fused_backward = False, use_flash = "auto": what the parent commit trains with
                 (f16x2 fused forward, unfused backward)
  unfused_f32    the same with use_flash = "f32" (the exact-fp32 fused forward; the backward is the same)
  fused          module.forward_rows on the same rows (exact-fp32 fused forward with lse, fused backward)
Device events around forward + backward; medians with min / max / p10 / p90; and the rise of
torch.cuda.max_memory_allocated across one forward + backward of each variant.

Part 2, a ragged batch of 8 videos with lengths between 300 and 1800 (RAGGED_LENGTHS):
  fused_batch    one forward_rows over the concatenated rows
  fused_loop     forward_rows per video (8 calls)
  unfused_loop   module.forward per video, [1, T_v, E] (what one has to do without this path, short of padding)

Part 3, the four kernels of the fused path on their own at the same sizes: device events around ONE launch each
(fwd, delta, dkv, dq), and the achieved share of the 157.3 TFLOP/s fp32-MFMA peak from the products each kernel runs:
fwd 2, dkv 4, dq 3 products of 2 T^2 D flops per (sequence, head).  The kernels' own durations come from a kernel
trace in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attn_rows_study.py --trace-only

Prints one JSON line (and writes it to --out).  Run it under its own time limit, e.g.
  timeout -k 10 600 python tools/attn_rows_study.py"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3
RAGGED_LENGTHS = (300, 520, 760, 1010, 1240, 1460, 1650, 1800)


def spread_ms(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "runs": len(s)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def compare(variants, warmup, steps):
    """{name: spread} of the callables, alternating step by step; each is warmed up first."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in variants}
    for _ in range(steps):
        for name, fn in variants.items():
            events[name].append(timed(fn))
    torch.cuda.synchronize()
    return {name: spread_ms([s.elapsed_time(e) for s, e in ev]) for name, ev in events.items()}


def peak_rise(fn):
    """Bytes by which the allocator's peak rises across one call (after the call has run once before)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def make_module(dev, e, h):
    from avsum_amd.models.attention import MultiHeadSelfAttention
    torch.manual_seed(11)
    return MultiHeadSelfAttention(e, h).to(dev)


def train_call(m, forward, x, gout):
    """forward + backward with every parameter and the input taking a gradient."""
    def call():
        for prm in m.parameters():
            prm.grad = None
        x.grad = None
        forward(x).backward(gout)
    return call


def part1(dev, args, m):
    out = {}
    for t in args.lengths:
        g = torch.Generator().manual_seed(t)
        x = torch.randn(t, args.embed, generator=g).to(dev).requires_grad_(True)
        x3 = x.detach().reshape(1, t, args.embed).clone().requires_grad_(True)
        gout = torch.randn(t, args.embed, generator=g).to(dev)
        offsets = [0, t]

        def unfused(flash):
            def forward(xin):
                m.use_flash, m.fused_backward = flash, False
                return m(xin)
            return train_call(m, forward, x3, gout.reshape(1, t, args.embed))

        variants = {"unfused": unfused("auto"), "unfused_f32": unfused("f32"),
                    "fused": train_call(m, lambda xin: m.forward_rows(xin, offsets), x, gout)}
        steps = max(3, args.steps // (1 + t // 1500))
        row = compare(variants, args.warmup, steps)
        for name, fn in variants.items():
            row[name]["peak_rise_bytes"] = peak_rise(fn)
        row["score_buffer_bytes"] = args.heads * t * ((t + 3) // 4 * 4) * 4
        out[str(t)] = row
    return out


def part2(dev, args, m):
    from avsum_amd import ops
    lengths = RAGGED_LENGTHS
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    rows = int(offsets[-1])
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, args.embed, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(rows, args.embed, generator=g).to(dev)
    table = ops.AttnTable(offsets, device=dev)
    tables = [ops.AttnTable([0, n], device=dev) for n in lengths]
    spans = list(zip(offsets[:-1].tolist(), offsets[1:].tolist()))

    def fused_loop(xin):
        m.fused_backward = False
        return torch.cat([m.forward_rows(xin[lo:hi], tb) for (lo, hi), tb in zip(spans, tables)])

    def unfused_loop(xin):
        m.use_flash, m.fused_backward = "auto", False
        return torch.cat([m(xin[lo:hi][None])[0] for lo, hi in spans])

    variants = {"fused_batch": train_call(m, lambda xin: m.forward_rows(xin, table), x, gout),
                "fused_loop": train_call(m, fused_loop, x, gout), "unfused_loop": train_call(m, unfused_loop, x, gout)}
    row = compare(variants, args.warmup, max(3, args.steps // 2))
    for name, fn in variants.items():
        row[name]["peak_rise_bytes"] = peak_rise(fn)
    row["lengths"], row["rows"] = list(lengths), rows
    return row


def kernel_calls(dev, args, lengths):
    """{name: (callable, products)} of the four launches on projected random rows of the sequences ``lengths``."""
    from avsum_amd import attn, ops
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    rows = int(offsets[-1])
    g = torch.Generator().manual_seed(rows + 1)
    q, k, v, dctx = (0.6 * torch.randn(rows, args.embed, generator=g).to(dev) for _ in range(4))
    table = ops.AttnTable(offsets, device=dev)
    ctx, lse = attn.mhsa_rows_fwd(q, k, v, table, args.heads)
    delta = attn.mhsa_rows_delta(dctx, ctx, table, args.heads)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    return {
        "fwd": (lambda: attn.mhsa_rows_fwd(q, k, v, table, args.heads, ctx=ctx, lse=lse), 2),
        "delta": (lambda: attn.mhsa_rows_delta(dctx, ctx, table, args.heads, delta=delta), 0),
        "dkv": (lambda: attn.mhsa_rows_dkv(dctx, q, k, v, lse, delta, table, args.heads, dk=dk, dv=dv), 4),
        "dq": (lambda: attn.mhsa_rows_dq(dctx, q, k, v, lse, delta, table, args.heads, dq=dq), 3),
    }


def part3(dev, args):
    out = {}
    for label, lengths in [(str(t), (t,)) for t in args.lengths] + [("ragged", RAGGED_LENGTHS)]:
        calls = kernel_calls(dev, args, lengths)
        row = compare({name: fn for name, (fn, _) in calls.items()}, args.warmup, args.steps)
        for name, (_, products) in calls.items():
            flops = products * 2.0 * sum(n * n for n in lengths) * args.embed
            row[name]["flops"] = flops
            if products:
                row[name]["share_of_f32_mfma_peak"] = round(flops / (row[name]["median_ms"] * 1e-3) / (PEAK_F32_MFMA_TFLOPS * 1e12), 4)
        out[label] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--embed", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 1800, 5000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--trace-only", action="store_true", help="a few launches of the four kernels at every size, for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_rows_study needs an MI355X: there is no CPU fallback and no timing without the device")
    dev = torch.device("cuda", 0)
    if args.trace_only:
        for lengths in [(t,) for t in args.lengths] + [RAGGED_LENGTHS]:
            for fn, _ in kernel_calls(dev, args, lengths).values():
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        return
    m = make_module(dev, args.embed, args.heads)
    result = {"study": "attn_rows", "embed": args.embed, "heads": args.heads, "head_dim": args.embed // args.heads,
              "one_sequence": part1(dev, args, m), "ragged_batch": part2(dev, args, m), "kernels": part3(dev, args),
              "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
