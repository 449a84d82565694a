#!/usr/bin/env python3
"""Study: the three YUV 4:2:0 ingest kernels of libavsum_yuv.so per layout, beside the NV12 library in the same run.

Batch: tools/nv12_study.py's - --videos (8) seeded synthetic videos of 640x360 surfaces, 1 587 frames at the default
seed.  The NV12 surfaces are built as there (libavsum_ingest.so reads them, unchanged: the yardstick); the same picture is
repacked on the device as I420 (three planes, tight), P010 (16-bit words, the 8-bit sample << 2 in the top ten bits) and
planar 10-bit (the same value in the low ten bits), so every layout converts to the same BGR bytes and the study can say
so.  Steps, each a fresh process under its own time limit (run without --step to run them in turn; a step that fails
ends the study):

  kernels  device events over --reps launches, alternating --rounds times after a warm-up of every form: per layout the
           dense conversion of every frame, the shot scan, and the two-size resize of the batch's sampled frames; the BGR
           scan and resize once, as what a converted batch costs.  With the bytes each must read and write, as GB/s.
  stage1   device-synchronised wall clock per call of detect_shots_batch + StageOneTables.from_result + embed_shots
           ("f16x2" trunks) on each layout's surfaces, alternating, and whether the rows equal those of the converted frames.
  trace    per layout one `rocprofv3 --kernel-trace --stats` run of its own over --step launches (the three kernels,
           --reps launches each, nothing else on the device), read back from the profiler's kernel statistics.

Prints one JSON line per step.  e.g.  timeout -k 10 1100 python tools/yuv_study.py"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nv12_study import H, W, event_ms, make_surfaces, spread, wall_ms  # noqa: E402  (the same batch, the same clocks)

LAYOUTS = ("nv12", "i420", "p010", "i010")
SAMPLE_BYTES = {"nv12": 1, "i420": 1, "p010": 2, "i010": 2}
STEP_LIMITS = {"kernels": 300, "stage1": 420, "trace": 420}      # seconds
SIZES = [(224, 224), (299, 299)]


def repack(nv12, layout):
    """The picture of the NV12 tensor [N, 540, 640] in ``layout``: (frames object, tensor).  8-bit samples s become the
    ten-bit samples 4 * s."""
    import torch
    from avsum_amd.ingest import Nv12Frames
    from avsum_amd.yuv import YuvFrames
    if layout == "nv12":
        return Nv12Frames(nv12, H, W)
    n = nv12.shape[0]
    if layout == "p010":        # the word s << 8: a zero byte, then s
        data = torch.zeros((n, H + H // 2, W, 2), dtype=torch.uint8, device=nv12.device)
        data[..., 1] = nv12
        return YuvFrames.p010(data.view(n, H + H // 2, 2 * W), H, W)
    planes = torch.cat([nv12[:, :H].reshape(n, -1), nv12[:, H:, 0::2].reshape(n, -1), nv12[:, H:, 1::2].reshape(n, -1)], dim=1)
    if layout == "i420":
        return YuvFrames.i420(planes.contiguous(), H, W)
    words = torch.stack([planes << 2, planes >> 6], dim=-1)     # s << 2, little-endian (the uint8 shift wraps)
    return YuvFrames.i010(words.view(n, -1).contiguous(), H, W)


def batch_of(args, layouts):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    lengths = [int(v) for v in torch.randint(150, 301, (args.videos,), generator=torch.Generator().manual_seed(args.seed))]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nv12 = make_surfaces(lengths, dev, args.seed)
    return dev, offsets, {name: repack(nv12, name) for name in layouts}


def calls_of(name):
    """(to_bgr, scan, resize) of a layout: the NV12 library's for "nv12", this library's for the others."""
    from avsum_amd import ingest, yuv
    if name == "nv12":
        return ingest.nv12_to_bgr, ingest.nv12_hsv_frame_diff_batch, ingest.nv12_resize_gather
    return yuv.yuv_to_bgr, yuv.yuv_hsv_frame_diff_batch, yuv.yuv_resize_gather


def kernel_forms(args, layouts):
    """{form: (callable, bytes it must read and write)} over the batch, and the batch's layout line."""
    import torch
    from avsum_amd import ops
    from avsum_amd.features.shots import detect_shots_batch, downscale_factor
    dev, offsets, frames = batch_of(args, layouts)
    first = frames[layouts[0]]
    n = first.frames
    bgr = calls_of(layouts[0])[0](first)
    result = detect_shots_batch(first, offsets)
    plan = ops.StageOneTables.from_result(result, 1 << 20)
    index, count = plan.pass_frame_index_t, plan.nsamples
    outs = [torch.empty((count, s, s, 3), dtype=torch.uint8, device=dev) for s, _ in SIZES]
    step = downscale_factor(W)
    px = len(range(0, H, step)) * len(range(0, W, step))
    out_bytes = count * sum(3 * a * b for a, b in SIZES)
    forms, same = {}, {}
    for name in layouts:
        to_bgr, scan, resize = calls_of(name)
        f, sb = frames[name], SAMPLE_BYTES[name]
        same[name] = bool(torch.equal(to_bgr(f), bgr))
        forms[f"to_bgr_{name}"] = (lambda to_bgr=to_bgr, f=f: to_bgr(f, out=bgr), n * H * W * (1.5 * sb + 3))
        # the scan uses `px` strided pixels of two frames per frame, a Y, a U and a V sample each (the lines fetched are more)
        forms[f"scan_{name}"] = (lambda scan=scan, f=f: scan(f, result.plan, step, raw=True), n * px * 2 * 3 * sb)
        forms[f"resize_gather_{name}"] = (lambda resize=resize, f=f: resize(f, index, count, SIZES, outs=outs),
                                          count * H * W * 1.5 * sb + out_bytes)
    forms["scan_bgr"] = (lambda: ops.hsv_frame_diff_batch(bgr, result.plan, step, raw=True), n * px * 2 * 3)
    forms["resize_gather_bgr"] = (lambda: ops.resize_gather(bgr, index, count, SIZES, outs), count * H * W * 3 + out_bytes)
    return forms, {"frames": n, "sampled_frames": int(count), "scan_step": step, "frame": [H, W],
                   "converted_equal_to_first_layout": same}


def step_kernels(args):
    import torch
    forms, layout = kernel_forms(args, args.layouts)
    for f, _ in forms.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, (f, _) in forms.items():
            times[k].append(event_ms(f, args.reps))
    return {"layout": layout, **{k: spread(times[k], forms[k][1]) for k in forms}}


def step_launches(args):
    """What the profiler traces: every form of the given layouts, --reps launches each, after one warm-up launch."""
    import torch
    forms, layout = kernel_forms(args, args.layouts)
    for f, _ in forms.values():
        f()
    torch.cuda.synchronize()
    for f, _ in forms.values():
        for _ in range(args.reps):
            f()
    torch.cuda.synchronize()
    return {"layout": layout, "launches_per_form": args.reps + 1, "bytes": {k: int(b) for k, (_, b) in forms.items()}}


def step_stage1(args):
    import torch
    from avsum_amd import ops
    from avsum_amd.features.extractors import VisualFeatureExtractor
    from avsum_amd.features.shots import detect_shots_batch
    dev, offsets, frames = batch_of(args, args.layouts)
    torch.manual_seed(7)
    vis = VisualFeatureExtractor(arith="f16x2").to(dev)

    def stage1(f):
        result = detect_shots_batch(f, offsets)
        plan = ops.StageOneTables.from_result(result, 4096)
        return vis.embed_shots(f, plan), plan

    bgr = calls_of(args.layouts[0])[0](frames[args.layouts[0]])
    forms = {"resident_bgr": lambda: stage1(bgr), **{name: (lambda f=frames[name]: stage1(f)) for name in args.layouts}}
    warm = {k: f() for k, f in forms.items()}
    plan = warm[args.layouts[0]][1]
    equal = {k: bool(torch.equal(warm[k][0], warm["resident_bgr"][0])) for k in args.layouts}
    del warm
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            times[k].append(wall_ms(f)[0])
    return {"layout": {"videos": int(len(offsets) - 1), "frames": int(offsets[-1]), "frame": [H, W], "shots": plan.nshots,
                       "sampled_frames": plan.nsamples, "arith": "f16x2"},
            "resident_bytes": {"bgr": bgr.numel(), **{k: frames[k].nbytes for k in args.layouts}},
            **{k: spread(v) for k, v in times.items()},
            "rows_equal_resident_bgr": equal}


def form_of(kernel, layout):
    """The study's form a traced kernel belongs to, None for every other kernel of the run."""
    own = "nv12_" if layout == "nv12" else "yuv_"
    for start, form in ((own + "to_bgr", f"to_bgr_{layout}"), (own + "resize_gather2", f"resize_gather_{layout}"),
                        (own + "hsv_diff", f"scan_{layout}"), ("hsv_frame_diff_batch", "scan_bgr"),
                        ("resize_gather2", "resize_gather_bgr")):
        if kernel.startswith(start):
            return form
    return None


def step_trace(args):
    """One profiler run per layout, the program after `--`; the kernels' own durations from its statistics."""
    report = {}
    for name in args.layouts:
        work = tempfile.mkdtemp(prefix=f"yuv_trace_{name}_")
        cmd = ["timeout", "-k", "10", "150", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--",
               sys.executable, os.path.abspath(__file__), "--step", "launches", "--layouts", name, "--videos", str(args.videos),
               "--reps", str(args.reps), "--seed", str(args.seed)]
        run = subprocess.run(cmd, capture_output=True, text=True)
        if run.returncode != 0:
            print(run.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"yuv_study: the profiler run of {name} ended with status {run.returncode}")
        launched = json.loads([line for line in run.stdout.splitlines() if line.startswith("{")][-1])
        stats = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit(f"yuv_study: the profiler wrote no kernel statistics for {name}")
        rows = {}
        for r in csv.DictReader(open(stats[0])):
            kernel = r["Name"].split("(")[0].replace("void ", "")
            form = form_of(kernel, name)
            if form is None:
                continue
            avg_us = float(r["AverageNs"]) / 1e3
            rows[form] = {"kernel": kernel, "calls": int(r["Calls"]), "average_us": round(avg_us, 2),
                          "gb_per_s_at_average": round(launched["bytes"][form] / avg_us / 1e3, 1)}
        report[name] = rows
        shutil.rmtree(work, ignore_errors=True)
    return {"profiler": "rocprofv3 --kernel-trace --stats", **report}


STEPS = {"kernels": step_kernels, "stage1": step_stage1, "trace": step_trace, "launches": step_launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--layouts", default=",".join(LAYOUTS), help="comma-separated, of " + ", ".join(LAYOUTS))
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=4104)
    args = ap.parse_args()
    args.layouts = tuple(args.layouts.split(","))
    if not args.layouts or any(name not in LAYOUTS for name in args.layouts):
        ap.error(f"--layouts takes names of {LAYOUTS}")
    if args.step:
        line = {"step": args.step, **STEPS[args.step](args)}
        if args.step != "trace":           # (the trace step opens no device of its own: its children do)
            import torch
            line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)
        return 0
    passed = [a for a in sys.argv[1:]]
    for name in ("kernels", "stage1", "trace"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name] + passed
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"yuv_study: step {name} ended with status {rc}; the later steps are not started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
