#!/usr/bin/env python3
"""Study: rendering a keyshot summary on the device (libavsum_render.so) beside the mirror kernel and the host route it
replaces, in one run.

Batch: tools/yuv_study.py's - --videos (8) seeded synthetic videos of 640x360, 1 587 frames at the default seed - as BGR
frames, as NV12 and as I420 surfaces of the same picture; shots of 30 frames and seeded scores give a 15 % keyshot summary
(evaluation.keyshots.keyshot_summaries_device); one 16 kHz track per video, 25 fps.  Timed, device events over --reps
launches, alternating --rounds times after a warm-up of every form (the median and the spread are reported):

  index            render.summary_index: the three launches (count, scan, scatter)
  bgr_to_nv12      render.bgr_to_yuv gathered by the summary's frame list (the new forward kernel)
  i420_to_nv12     render.repack gathered (the new repack kernel)
  gather_bgr       the same-format route: ops.gather_rows of the BGR rows
  audio_cut        render.summary_audio: bounds + copy, fade 160
  mirror_nv12_to_bgr   yuv.yuv_to_bgr gathered over the same frame list: the same bytes in the other direction
and, wall clock with a device synchronisation, ``host_route``: what a user did before - KeyshotResult.host(), a Python
loop over videos and shots, index_select, a torch-expressed BGR -> NV12 conversion, the waveform sliced by hand.

For the two new pixel kernels the report gives the bytes moved (what must be read and written for the frames really
picked) over the median time, as a fraction of --hbm-gb-s (6 290: the measured copy rate of the chip, the memory side of
its roofline), and the ratio to the mirror kernel.  Prints one JSON line.
e.g.  timeout -k 10 300 python tools/render_study.py"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nv12_study import H, W, event_ms, make_surfaces, spread, wall_ms  # noqa: E402  (the same batch, the same clocks)
from yuv_study import repack  # noqa: E402

FPS, SR, SHOT = 25, 16000, 30


def host_route(result, bgr, wave, offsets, wave_offsets, forward):
    """The route the device rendering replaces, with what exists without it: one download of the picks, a loop, a gather,
    a conversion written in torch (float32 matrix, 2x2 mean, rounding - close to, not equal to, the integer definition),
    slices of the waveform."""
    import torch
    picks = result.host()[0]
    rows, pieces = [], []
    for v, shots in enumerate(picks):
        for s, e in shots:
            rows.append(torch.arange(offsets[v] + s, offsets[v] + e, device=bgr.device))
            a, b = int(s / FPS * SR), int(e / FPS * SR)
            pieces.append(wave[wave_offsets[v] + a:wave_offsets[v] + b])
    frames = bgr.index_select(0, torch.cat(rows)).to(torch.float32)
    yuv = frames @ forward[:, 1:].t() + forward[:, 0]
    luma = yuv[..., 0].round().clamp(0, 255).to(torch.uint8)
    chroma = torch.nn.functional.avg_pool2d(yuv[..., 1:].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    chroma = chroma.round().clamp(0, 255).to(torch.uint8).reshape(-1, H // 2, W)
    return torch.cat([luma, chroma], dim=1), torch.cat(pieces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=4104)
    ap.add_argument("--hbm-gb-s", type=float, default=6290.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from avsum_amd import ingest, ops, render, yuv
    from avsum_amd.evaluation.keyshots import keyshot_summaries_device
    dev = torch.device("cuda", 0)
    lengths = [int(v) for v in torch.randint(150, 301, (args.videos,), generator=torch.Generator().manual_seed(args.seed))]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1])
    surfaces = make_surfaces(lengths, dev, args.seed)
    nv12 = yuv.YuvFrames.from_nv12(repack(surfaces, "nv12"))
    i420 = repack(surfaces, "i420")
    bgr = ingest.nv12_to_bgr(repack(surfaces, "nv12"))
    shots = [[(s, min(s + SHOT, m)) for s in range(0, m, SHOT)] for m in lengths]
    scores = torch.rand(n, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    result = keyshot_summaries_device(scores, offsets, shots, 0.15)
    wave_offsets = np.concatenate([[0], np.cumsum([m * SR // FPS for m in lengths])]).astype(np.int64)
    wave = torch.randn(int(wave_offsets[-1]), generator=torch.Generator().manual_seed(args.seed + 2)).to(dev)
    tables = ops.RenderTables.from_keyshots(result, wave_offsets=wave_offsets, fps=FPS, sr=SR)
    index = render.summary_index(result, tables)
    cap = tables.frame_cap
    picked = int(index.count.item())
    out_nv12 = yuv.YuvFrames.nv12(torch.zeros((cap, H + H // 2, W), dtype=torch.uint8, device=dev), H, W)
    out_bgr = torch.zeros((cap, H, W, 3), dtype=torch.uint8, device=dev)
    audio = torch.zeros(tables.sample_cap, dtype=torch.float32, device=dev)
    samples = int(render._audio_cut(wave, index, tables, 160, audio)[1][-1].item())
    px = picked * H * W
    forms = {
        "index": (lambda: render.summary_index(result, tables), None),
        "bgr_to_nv12": (lambda: render.bgr_to_yuv(bgr, out_nv12, index, cap), px * (3 + 1.5)),
        "i420_to_nv12": (lambda: render.repack(i420, out_nv12, index, cap), px * (1.5 + 1.5)),
        "gather_bgr": (lambda: ops.gather_rows(bgr, index.frame_index, index.count, out_bgr), px * (3 + 3)),
        "audio_cut": (lambda: render._audio_cut(wave, index, tables, 160, audio), samples * 8),
        "mirror_nv12_to_bgr": (lambda: yuv.yuv_to_bgr(nv12, index.frame_index, cap, out=out_bgr), px * (1.5 + 3)),
    }
    forward = torch.tensor(render.FORWARD_MATRICES_F64["bt601"], dtype=torch.float32, device=dev)
    forward = torch.stack([torch.cat([torch.tensor([o], device=dev), forward[1 + 3 * r:4 + 3 * r]])
                           for r, o in enumerate((16.0, 128.0, 128.0))])

    def host():
        result._host = None       # (the download is part of the route)
        return host_route(result, bgr, wave, offsets, wave_offsets, forward)

    for f, _ in forms.values():
        f()
    host_frames, host_audio = host()
    torch.cuda.synchronize()
    # what the routes agree on: the audio exactly (fade 0), the torch-expressed pixels within rounding of the definition
    render.bgr_to_yuv(bgr, out_nv12, index, cap)
    worst = int((out_nv12.data[:picked].to(torch.int16) - host_frames.to(torch.int16)).abs().max().item())
    plain = render._audio_cut(wave, index, tables, 0, torch.zeros_like(audio))[0]
    times = {k: [] for k in forms}
    times["host_route"] = []
    for _ in range(args.rounds):
        for k, (f, _) in forms.items():
            times[k].append(event_ms(f, args.reps))
        times["host_route"].append(wall_ms(host)[0])
    report = {k: spread(times[k], forms[k][1]) if k in forms else spread(times[k]) for k in times}
    for k in ("bgr_to_nv12", "i420_to_nv12"):
        report[k]["fraction_of_hbm_roof"] = round(report[k]["gb_per_s_at_median"] / args.hbm_gb_s, 3)
        report[k]["time_over_mirror"] = round(report[k]["median_ms"] / report["mirror_nv12_to_bgr"]["median_ms"], 2)
    device_ms = sum(report[k]["median_ms"] for k in ("index", "bgr_to_nv12", "audio_cut"))
    print(json.dumps({
        "layout": {"videos": args.videos, "frames": n, "frame": [H, W], "summary_frames": picked, "frame_cap": cap,
                   "runs": int(index.run_offsets[-1].item()), "run_cap": tables.run_cap, "summary_samples": samples,
                   "sample_cap": tables.sample_cap, "index_tiles": tables.ntiles, "reps": args.reps, "rounds": args.rounds},
        **report,
        "device_route_ms_at_medians": round(device_ms, 3),
        "host_route_over_device_route": round(report["host_route"]["median_ms"] / device_ms, 1),
        "host_route_audio_equals_fade0_cut": bool(torch.equal(plain[:host_audio.numel()], host_audio)),
        "host_route_pixels_max_abs_difference": worst,
        "hbm_roof_gb_s": args.hbm_gb_s, "device": torch.cuda.get_device_name(0)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
