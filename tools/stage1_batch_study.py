#!/usr/bin/env python3
"""Study: stage-1 extraction of a ragged batch, the per-video process_decoded loop against one process_decoded_batch call.

Batch: --videos (8) seeded synthetic videos of 640x360 frames, 150-300 frames each, a new smooth scene every 40-70
frames plus sensor-like noise, so the detector has cuts to find; the shots are detected once (detect_shots_batch) and
both forms are given the same host lists.  Per arithmetic ("f16x2", "f32"), after a warm-up of both, the two forms
alternate within one process, --rounds (5) times each:

  (a) loop:  per video AVProcessor.process_decoded(host frames, ..., batch_audio=True): per shot a host stack, an
             upload, both trunks on at most 100 frames in non-uniform BatchNorm groups, one download;
  (b) batch: AVProcessor.process_decoded_batch on the device-resident frames: passes of uniform groups, one download.

Device-synchronised wall-clock ms per call, host work and transfers included (that IS the difference), as videos/s and
sampled frames/s, and the largest difference between the two forms' rows.  Then the glue alone on the batch's sample
index, device events over --glue-reps launches each, alternating: ops.gather_rows + two ops.resize_bilinear calls (the
dense full-resolution copy and one thread per output pixel) against one ops.resize_gather launch.  Prints one JSON line.
Run it under its own time limit, e.g.
  timeout -k 10 900 python tools/stage1_batch_study.py"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 360, 640


def make_videos(lengths, device, seed):
    """uint8 [sum(lengths), 360, 640, 3] on the device: per video a new smooth random image (a 6x10x3 field upsampled)
    every 40-70 frames, with noise of +-6 per frame."""
    g = torch.Generator(device=device).manual_seed(seed)
    gh = torch.Generator().manual_seed(seed)
    out = torch.empty((int(sum(lengths)), H, W, 3), dtype=torch.uint8, device=device)
    row = 0
    for n in lengths:
        f = 0
        while f < n:
            run = min(n - f, int(torch.randint(40, 71, (1,), generator=gh)))
            field = torch.rand((1, 3, 6, 10), device=device, generator=g) * 255.0
            scene = torch.nn.functional.interpolate(field, size=(H, W), mode="bilinear", align_corners=False)[0]
            noise = torch.randint(-6, 7, (run, H, W, 3), device=device, generator=g, dtype=torch.int16)
            out[row:row + run] = (scene.permute(1, 2, 0).to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
            f, row = f + run, row + run
    return out


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
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--glue-reps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=4104)
    args = ap.parse_args()
    from avsum_amd import ops
    from avsum_amd.features.extractors import AVProcessor
    from avsum_amd.features.shots import detect_shots_batch
    dev = torch.device("cuda", 0)
    lengths = [int(v) for v in torch.randint(150, 301, (args.videos,), generator=torch.Generator().manual_seed(args.seed))]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    frames = make_videos(lengths, dev, args.seed)
    host = frames.cpu().numpy()
    fps = 30.0
    waves = [np.zeros(int(n / fps * 16000), dtype=np.float32) for n in lengths]
    shots = detect_shots_batch(frames, offsets).host()
    plan = ops.StageOneTables(offsets, shots, device=dev)
    nframes = plan.nsamples
    line = {"layout": {"videos": len(lengths), "frames": int(offsets[-1]), "frame": [H, W], "shots": plan.nshots,
                       "sampled_frames": nframes, "passes": [[g, hi - lo] for g, lo, hi in plan.passes]}}

    for arith in ("f16x2", "f32"):
        torch.manual_seed(7)
        proc = AVProcessor(arith=arith)
        proc.visual_extractor.to(dev)
        loop = lambda: [proc.process_decoded(host[a:b], w, fps, s, batch_audio=True)
                        for a, b, w, s in zip(offsets[:-1], offsets[1:], waves, shots)]
        batch = lambda: proc.process_decoded_batch(frames, offsets, waves, fps, shots)
        want, got = loop(), batch()                                   # warm-up of both forms
        diff = max((float(np.abs(g[0] - w[0]).max()) for g, w in zip(got, want) if w[0].size), default=0.0)
        scale = max((float(np.abs(w[0]).max()) for w in want if w[0].size), default=0.0)
        t_loop, t_batch = [], []
        for _ in range(args.rounds):
            t_loop.append(wall_ms(loop)[0])
            t_batch.append(wall_ms(batch)[0])
        ml, mb = statistics.median(t_loop), statistics.median(t_batch)
        line[arith] = {"loop": spread(t_loop), "batch": spread(t_batch), "ratio_of_medians": round(ml / mb, 2),
                       "separated": min(t_loop) > max(t_batch),
                       "loop_videos_per_s": round(len(lengths) / ml * 1e3, 2), "batch_videos_per_s": round(len(lengths) / mb * 1e3, 2),
                       "loop_frames_per_s": round(nframes / ml * 1e3, 1), "batch_frames_per_s": round(nframes / mb * 1e3, 1),
                       "max_abs_diff": diff, "max_abs_ref": scale}
        del proc

    # the glue alone: the sampled frames of the whole batch at both trunk sizes
    index = torch.from_numpy(plan.sample_index).to(dev)
    count = torch.tensor([nframes], dtype=torch.int64, device=dev)
    dense = torch.empty((nframes, H, W, 3), dtype=torch.uint8, device=dev)
    outs = [torch.empty((nframes, s, s, 3), dtype=torch.uint8, device=dev) for s in (224, 299)]

    def parent():
        ops.gather_rows(frames, index, count, dense)
        return ops.resize_bilinear(dense, 224, 224), ops.resize_bilinear(dense, 299, 299)

    fused = lambda: ops.resize_gather(frames, index, nframes, [(224, 224), (299, 299)], outs)
    a, b = parent()
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, outs[0]) and torch.equal(b, outs[1]))
    del a, b
    g_p, g_f = [], []
    for _ in range(args.rounds):
        g_p.append(event_ms(parent, args.glue_reps))
        g_f.append(event_ms(fused, args.glue_reps))
    line["glue"] = {"gather_rows_and_two_resize_bilinear": spread(g_p), "resize_gather": spread(g_f), "equal": same,
                    "ratio_of_medians": round(statistics.median(g_p) / statistics.median(g_f), 2),
                    "separated": min(g_p) > max(g_f), "dense_copy_bytes_avoided": int(nframes) * H * W * 3}
    line["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
