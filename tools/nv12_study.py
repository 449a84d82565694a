#!/usr/bin/env python3
"""Study: what reading NV12 surfaces where they lie saves against converting them to BGR first.

Batch: --videos (8) seeded synthetic videos of 640x360 NV12 surfaces (pitch 640, chroma at row 360), 150-300 frames
each, a new smooth scene in Y, U and V every 40-70 frames plus luma noise, so the detector has cuts to find.  Three
steps, each a fresh process under its own time limit (run without --step to run them in turn; a step that fails ends
the study):

  stage1   after a warm-up of all three, alternating --rounds (7) times, device-synchronised wall clock per call of
           detect_shots_batch + StageOneTables.from_result + embed_shots ("f16x2" trunks):
             (a) on BGR frames already resident (converted before the clock starts): the parent's path;
             (b) nv12_to_bgr of every frame, then (a): what a user with NV12 surfaces has to do without this library;
             (c) on the Nv12Frames themselves: the fused path.
           Also the resident bytes of the two forms and whether (c)'s rows equal (b)'s.
  kernels  device events over --reps launches, alternating --rounds times: nv12_to_bgr of every frame; the shot scan on
           BGR and on NV12; the two-size resize of the batch's sampled frames from BGR and from NV12.  With the bytes
           each must move, as GB/s.
  pull     ops.pull_copy of the first --pull-frames (512) frames from pinned host memory, as BGR and as NV12.

Prints one JSON line per step.  e.g.  timeout -k 10 900 python tools/nv12_study.py"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 360, 640
STEP_LIMITS = {"stage1": 420, "kernels": 240, "pull": 180}      # seconds


def make_surfaces(lengths, device, seed):
    """uint8 [sum(lengths), 540, 640] on the device: per video a new smooth random (Y, U, V) image every 40-70 frames,
    chroma at half resolution, with luma noise of +-6 per frame."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    gh = torch.Generator().manual_seed(seed)
    out = torch.empty((int(sum(lengths)), H + H // 2, W), dtype=torch.uint8, device=device)
    row = 0
    for n in lengths:
        f = 0
        while f < n:
            run = min(n - f, int(torch.randint(40, 71, (1,), generator=gh)))
            field = torch.rand((1, 3, 6, 10), device=device, generator=g) * torch.tensor(
                [219.0, 160.0, 160.0], device=device).view(1, 3, 1, 1) + torch.tensor(
                [16.0, 48.0, 48.0], device=device).view(1, 3, 1, 1)
            luma = torch.nn.functional.interpolate(field[:, :1], size=(H, W), mode="bilinear", align_corners=False)[0, 0]
            chroma = torch.nn.functional.interpolate(field[:, 1:], size=(H // 2, W // 2), mode="bilinear",
                                                     align_corners=False)[0]
            noise = torch.randint(-6, 7, (run, H, W), device=device, generator=g, dtype=torch.int16)
            out[row:row + run, :H] = (luma.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
            out[row:row + run, H:] = chroma.permute(1, 2, 0).reshape(H // 2, W).to(torch.uint8)
            f, row = f + run, row + run
    return out


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def event_ms(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def spread(xs, nbytes=None):
    out = {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
           "runs": len(xs)}
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["gb_per_s_at_median"] = round(nbytes / statistics.median(xs) / 1e6, 1)
    return out


def batch_of(args):
    import numpy as np
    import torch
    from avsum_amd.ingest import Nv12Frames
    dev = torch.device("cuda", 0)
    lengths = [int(v) for v in torch.randint(150, 301, (args.videos,), generator=torch.Generator().manual_seed(args.seed))]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return dev, offsets, Nv12Frames(make_surfaces(lengths, dev, args.seed), H, W)


def step_stage1(args):
    import torch
    from avsum_amd import ops
    from avsum_amd.features.extractors import VisualFeatureExtractor
    from avsum_amd.features.shots import detect_shots_batch
    from avsum_amd.ingest import nv12_to_bgr
    dev, offsets, nv12 = batch_of(args)
    torch.manual_seed(7)
    vis = VisualFeatureExtractor(arith="f16x2").to(dev)

    def stage1(frames):
        result = detect_shots_batch(frames, offsets)
        plan = ops.StageOneTables.from_result(result, 4096)
        return vis.embed_shots(frames, plan), plan

    bgr = nv12_to_bgr(nv12)
    forms = {"a_resident_bgr": lambda: stage1(bgr), "b_convert_then_bgr": lambda: stage1(nv12_to_bgr(nv12)),
             "c_fused_nv12": lambda: stage1(nv12)}
    warm = {k: f() for k, f in forms.items()}
    plan = warm["c_fused_nv12"][1]
    equal = bool(torch.equal(warm["c_fused_nv12"][0], warm["b_convert_then_bgr"][0]))
    del warm
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            times[k].append(wall_ms(f)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"layout": {"videos": int(len(offsets) - 1), "frames": int(offsets[-1]), "frame": [H, W], "shots": plan.nshots,
                       "sampled_frames": plan.nsamples, "arith": "f16x2"},
            "resident_bytes": {"bgr": bgr.numel(), "nv12": nv12.nbytes},
            **{k: spread(v) for k, v in times.items()},
            "c_rows_equal_b_rows": equal,
            "b_over_c": round(med["b_convert_then_bgr"] / med["c_fused_nv12"], 3),
            "a_over_c": round(med["a_resident_bgr"] / med["c_fused_nv12"], 3),
            "b_separated_from_c": min(times["b_convert_then_bgr"]) > max(times["c_fused_nv12"])}


def step_kernels(args):
    import torch
    from avsum_amd import ops
    from avsum_amd.features.shots import detect_shots_batch, downscale_factor
    from avsum_amd.ingest import nv12_hsv_frame_diff_batch, nv12_resize_gather, nv12_to_bgr
    dev, offsets, nv12 = batch_of(args)
    n = nv12.frames
    bgr = nv12_to_bgr(nv12)
    result = detect_shots_batch(nv12, offsets)
    plan = ops.StageOneTables.from_result(result, 1 << 20)
    index, count = plan.pass_frame_index_t, plan.nsamples
    sizes = [(224, 224), (299, 299)]
    outs = [torch.empty((count, s, s, 3), dtype=torch.uint8, device=dev) for s, _ in sizes]
    step = downscale_factor(W)
    px = len(range(0, H, step)) * len(range(0, W, step))
    out_bytes = count * sum(3 * a * b for a, b in sizes)
    forms = {
        "nv12_to_bgr": (lambda: nv12_to_bgr(nv12, out=bgr), n * H * W * (1.5 + 3)),
        # the scan reads `px` strided pixels of two frames per frame: bytes actually used (the lines fetched are more)
        "scan_bgr": (lambda: ops.hsv_frame_diff_batch(bgr, result.plan, step, raw=True), n * px * 2 * 3),
        "scan_nv12": (lambda: nv12_hsv_frame_diff_batch(nv12, result.plan, step, raw=True), n * px * 2 * 3),
        "resize_gather_bgr": (lambda: ops.resize_gather(bgr, index, count, sizes, outs), count * H * W * 3 + out_bytes),
        "resize_gather_nv12": (lambda: nv12_resize_gather(nv12, index, count, sizes, outs=outs),
                               count * H * W * 1.5 + out_bytes),
    }
    for f, _ in forms.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, (f, _) in forms.items():
            times[k].append(event_ms(f, args.reps))
    return {"layout": {"frames": n, "sampled_frames": int(count), "scan_step": step},
            **{k: spread(times[k], forms[k][1]) for k in forms}}


def step_pull(args):
    import torch
    from avsum_amd import ops
    from avsum_amd.ingest import Nv12Frames, nv12_to_bgr
    dev, offsets, nv12 = batch_of(args)
    k = min(args.pull_frames, nv12.frames)
    part = Nv12Frames(nv12.data[:k].clone(), H, W)
    bgr = nv12_to_bgr(part)
    pin_nv12, pin_bgr = part.pinned_like(), torch.empty(bgr.shape, dtype=torch.uint8, pin_memory=True)
    pin_nv12.copy_(part.data)
    pin_bgr.copy_(bgr)
    torch.cuda.synchronize()
    forms = {"pull_bgr": (lambda: ops.pull_copy(pin_bgr, bgr), bgr.numel()),
             "pull_nv12": (lambda: ops.pull_copy(pin_nv12, part.data), part.nbytes)}
    for f, _ in forms.values():
        f()
    torch.cuda.synchronize()
    same = bool(torch.equal(nv12_to_bgr(part), bgr))
    times = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, (f, _) in forms.items():
            times[name].append(event_ms(f, 3))
    return {"frames": k, "equal_after_upload": same, **{name: spread(times[name], forms[name][1]) for name in forms}}


STEPS = {"stage1": step_stage1, "kernels": step_kernels, "pull": step_pull}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pull-frames", type=int, default=512)
    ap.add_argument("--seed", type=int, default=4104)
    args = ap.parse_args()
    if args.step:
        import torch
        line = {"step": args.step, **STEPS[args.step](args), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        return 0
    passed = [a for a in sys.argv[1:]]
    for name in ("stage1", "kernels", "pull"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name] + passed
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"nv12_study: step {name} ended with status {rc}; the later steps are not started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
