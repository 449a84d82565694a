#!/usr/bin/env python3
"""Study: per-shot audio features on the configs[2] shape (synthetic.config(2): 50 tracks of U[2000, 10000] frames at
30 fps, 16 kHz audio, 30-frame shots from synthetic.uniform_shots), timed with device events after a warm-up, the three
forms alternating within one run:

  (a) the per-shot AudioFeatureExtractor.forward loop (intent mode), on the first --loop-shots shots (it costs ~ms per
      shot); reported per shot and scaled to the batch's shot count;
  (b) AudioFeatureExtractor.forward_shots_batch over all tracks (end to end: tables, launches, copy back), and its parts
      on prebuilt tables: the mel / MFCC means (MelPlan.shot_means_batch + the DCT) and VGGish (VGGish.embed_shots);
  (c) MelPlan.segment_means_batch on the same tracks (the whole-track variant, prebuilt tables): the cost floor of the
      mel / MFCC part.

Prints one JSON line.  Run it under its own time limit, e.g.  timeout -k 10 900 python tools/audio_shots_study.py"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--loop-shots", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from avsum_amd import ops, synthetic
    from avsum_amd.audio import HOP, MelPlan
    from avsum_amd.features.extractors import AudioFeatureExtractor
    dev = torch.device("cuda", 0)
    cfg = synthetic.config(2, videos=args.videos)
    sr = synthetic.SAMPLE_RATE
    waves = [synthetic.make_waveform(int(ln / synthetic.FPS * sr), cfg["seed"] + i).to(dev) for i, ln in enumerate(cfg["lengths"])]
    shots = [synthetic.uniform_shots(ln) for ln in cfg["lengths"]]
    bounds = [[(int(s / synthetic.FPS * sr), int(e / synthetic.FPS * sr)) for s, e in sv] for sv in shots]
    nshot = sum(len(b) for b in bounds)
    torch.manual_seed(0)
    ext = AudioFeatureExtractor(strict_reference=False)
    plan = MelPlan.get(sr, 128, 40, dev)
    tables = plan.shot_tables(waves, bounds, dev)
    nf = [1 + w.numel() // HOP for w in waves]
    segs = [[min(n, int(s / synthetic.FPS * sr) // HOP) for s, _ in sv] + [n] for sv, n in zip(shots, nf)]
    btables = plan.batch_tables(waves, segs, dev)
    out_log2, out_db = (torch.empty((nshot, 128), device=dev) for _ in range(2))
    out_vg = torch.empty((nshot, 128), device=dev)
    host0 = waves[0].cpu().numpy()
    loop_bounds = bounds[0][:args.loop_shots]
    if len(loop_bounds) < args.loop_shots:
        raise SystemExit(f"track 0 has only {len(loop_bounds)} shots")

    def run_a():
        for a, b in loop_bounds:
            ext(host0[a:b])

    def run_b():
        ext.forward_shots_batch(waves, bounds)

    def run_b_mel():
        plan.shot_means_batch(tables, out_log2, out_db)
        ops.linear(out_db, plan.dct)

    def run_b_vggish():
        ext.vggish.embed_shots(tables, out_vg)

    def run_c():
        plan.segment_means_batch(btables, out_log2, out_db)
        ops.linear(out_db, plan.dct)

    forms = {"a_loop": run_a, "b_batch": run_b, "b_mel": run_b_mel, "b_vggish": run_b_vggish, "c_whole_track": run_c}
    with torch.no_grad():
        for fn in forms.values():   # warm-up: workspaces, constants, code objects
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    a_per_shot = med["a_loop"] / len(loop_bounds)
    res = {"tool": "audio_shots_study", "tracks": len(waves), "shots": nshot, "samples": int(sum(w.numel() for w in waves)),
           "vggish_examples": int(tables.ex_start.numel()), "rounds": args.rounds, "loop_shots": len(loop_bounds),
           "a_ms_per_shot": round(a_per_shot, 4), "a_ms_scaled_to_batch": round(a_per_shot * nshot, 1),
           "b_ms": round(med["b_batch"], 2), "b_mel_mfcc_ms": round(med["b_mel"], 3), "b_vggish_ms": round(med["b_vggish"], 2),
           "c_ms": round(med["c_whole_track"], 3),
           "a_over_b": round(a_per_shot * nshot / med["b_batch"], 1),
           "b_mel_over_c": round(med["b_mel"] / med["c_whole_track"], 3),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
