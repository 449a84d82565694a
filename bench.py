#!/usr/bin/env python3
"""bench.py — frames/sec end-to-end (extract + fuse + score) on synthetic 224x224x3 frames + 16 kHz audio.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Headline workload at N=1 = BASELINE.json configs[1]: SumMe-shape batch, 25 videos x ~1.8k frames (lengths
~N(1800,300) clipped to [900,2700], seed 2002), visual-only (audio = the literal zeros(296)), ResNet-50
extractor in the reference's batch-statistics BatchNorm mode over micro-batches of 4 consecutive frames of a video
(features/extractors.py:48-56; `--frames-per-group 1` = every frame its own one-frame shot, sub_results.frames_per_group_1),
per-frame embeddings, then the AVBiLSTMModel scorer (fp32) and the mean-threshold selection.
The headline arithmetic is the FASTEST MODE THAT CARRIES PARITY (accuracy.bars_met true): f16x2 - activations and
weights stored as fp16 hi | lo runs (22 significant bits), every product three v_mfma_f32_32x32x16_f16, centred
BatchNorm statistics; the bf16 throughput mode (configs[1]'s "bf16", which does NOT meet the accuracy bars) is
sub_results.bf16_throughput_mode with its accuracy beside it.  One step = one pass of that path over the whole batch, uint8 frames already resident in HBM.  For N>1
every rank runs its own batch of the same shape (weak scaling; videos are independent, the data path has no
collective) and the per-video scores are all-gathered (C2) inside the timed region.  `--config 3` runs one rank's
share of configs[3] instead (50 videos x 5000 frames per rank).

ONE JSON line on rank 0 (contract in the task description).  A plain run sets up, warms up, times the K steps, writes
the last timed step's outputs if --dump-outputs is given, and prints the line: the headline only, its roofline,
cpu_baseline, accuracy and sub_results null.  --full adds, beside the headline:
  roofline      the dominant kernel (implicit-GEMM conv, MFMA-bound): algorithmic FLOPs of all its launches in the
                timed region / their summed HIP-event durations (events on the launch stream);
  cpu_baseline  the oracle (CPU restatement of the same path) on bounded samples, median of --cpu-runs runs;
  accuracy      the benchmarked arithmetic mode against the fp32 oracle on those same samples: score error,
                selection agreement, F1 drift, and whether north_star's bars (1e-4 / 0.001) are met by THIS mode;
  sub_results   (N=1, with the default headline) the other claimed configurations, each timed the same way with fewer steps:
                the bf16 throughput mode, the reference's 4-frame micro-batches, both trunks, the exact-fp32 and
                fp32-split modes (each with its own roofline block), a PCIe-inclusive pass (pinned host frames,
                upload overlapped with compute), the configs[2] audio+visual+fusion leg with the audio kernels' HBM
                roofline, one rank's configs[3] share, the configs[4] training leg.

--dump-outputs DIR writes what the timed path computed in its last timed step (rank 0's share), as float32 .npy files:
scores.npy (the per-frame importance scores, [frames]) and selected_mask.npy (1.0 where the selection rule keeps the
frame); --config 2: the same per shot; --config 4: loss_t<T>.npy, the last step's loss per sequence length (float64).
Inputs and weights are seeded, so two runs with the same arguments see the same inputs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0
PMC_TRAFFIC_FILES = {"bf16": ("r02_pmc_traffic.json", "r01_e_pmc_traffic.json"),   # newest first, under profiles/
                     "f16x2+inception3": ("r04_g_both_pmc_traffic.json",),   # the both-trunks configuration's own passes
                     "f16x2": ("r04_j_pmc_traffic.json", "r04_h_pmc_traffic.json", "r04_g_pmc_traffic.json", "r04_f_pmc_traffic.json", "r04_e_pmc_traffic.json", "r03_e_pmc_traffic.json", "r03_c_pmc_traffic.json", "r03_b_pmc_traffic.json", "r03_a_pmc_traffic.json")}

T_START = time.perf_counter()


def log(msg):
    """Progress on stderr (stdout carries exactly one JSON line)."""
    print(f"[bench {time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------------ CPU leg
def cpu_runs(trunk_sd, scorer_sd, sample_frames, runs, use_inception, inception_sd, fpg):
    """Oracle leg: the CPU restatement (oracle/) of the same path on `runs` bounded samples (one video of
    `sample_frames` frames each).  Returns (frames of every run, oracle scores of every run, seconds of every run)."""
    from avsum_amd import synthetic
    from oracle import cnn as ocnn, scorer as osc
    frames_all, scores_all, secs = [], [], []
    for r in range(runs):
        frames = synthetic.host_frames_uniform(sample_frames, 7 + r)
        t0 = time.perf_counter()
        with torch.no_grad():
            feats = []
            for g in range(0, sample_frames, fpg):  # micro-batches of fpg frames (train-mode BN over the micro-batch)
                x = torch.cat([ocnn.preprocess_frame(f) for f in frames[g:g + fpg]])
                rfeat = ocnn.resnet50_trunk_forward(trunk_sd, x)
                if use_inception:
                    ifeat = ocnn.inception_v3_forward(inception_sd,
                                                      torch.cat([ocnn.preprocess_inception(f) for f in frames[g:g + fpg]]))
                else:
                    ifeat = torch.zeros(rfeat.shape[0], 2048)
                feats.append(torch.cat([rfeat, ifeat], 1))
            visual = torch.cat(feats).unsqueeze(0)
            scores = osc.av_bilstm_forward(scorer_sd, visual, torch.zeros(1, sample_frames, 296)).reshape(-1).numpy()
            _ = np.flatnonzero(scores > scores.mean())
        secs.append(time.perf_counter() - t0)
        frames_all.append(frames)
        scores_all.append(scores)
    return frames_all, scores_all, secs


def cpu_cores():
    # the GPU box grants a CPU share of 16 cores per GPU; asking torch for every visible core (256 on the host)
    # oversubscribes that share and is ~1000x slower
    visible = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return min(16, visible)


# ------------------------------------------------------------------------------------------------ GPU timing
def timed_steps(step, steps, warmup, barrier, profile=None):
    """`warmup` untimed steps, then exactly `steps` steps bracketed by barrier + synchronize.  profile: None, or n =
    bracket every n-th launch of each kernel kind of the timed steps with HIP events.
    Returns (seconds, last result, profiler | None)."""
    from avsum_amd import ops
    counter = ops.LaunchProfiler(count_only=True)
    per_step, last = 0, None
    for _ in range(warmup):
        counter.count = 0
        ops.set_profiler(counter)
        last = step()
        ops.set_profiler(None)
        per_step = counter.count
        torch.cuda.synchronize()
    prof = None
    if profile is not None:
        if per_step == 0:   # no warm-up step was asked for: count one pass now (untimed)
            ops.set_profiler(counter)
            last = step()
            ops.set_profiler(None)
            per_step = counter.count
            torch.cuda.synchronize()
        # the HIP events of the timed launches are created here, outside the timed region (creation is the costly
        # part); inside it they are only recorded, on the stream the kernels are launched on
        prof = ops.LaunchProfiler(prealloc=per_step * steps // profile + 64, sample_every=profile)
        ops.set_profiler(prof)
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    barrier()
    elapsed = time.perf_counter() - t0
    ops.set_profiler(None)
    return elapsed, last, prof


def roofline_from(prof, dtype, elapsed, traffic, split=False):
    """split: False | True (AVS_F32_SPLIT) | "f16x2" (AVS_F16X2)."""
    from avsum_amd import ops
    summ = prof.summary()
    code = ops.dtype_code(dtype, split)
    conv = summ.get(("conv", code))
    if not conv or conv["ms"] <= 0:
        return None
    achieved = conv["flops"] / (conv["ms"] * 1e-3) / 1e12
    # f32split / f16x2 run three 16-bit MFMAs per algorithmic product: against the dense 16-bit peak (2.5 PF for
    # bf16 and fp16 alike) the ALGORITHMIC rate can reach a third of it
    peak = MFMA_BF16_PEAK_TFLOPS if dtype == torch.bfloat16 else (MFMA_BF16_PEAK_TFLOPS / 3.0 if split
                                                                   else MFMA_F32_PEAK_TFLOPS)
    seen = prof.seen.get(("conv", code), conv["launches"])
    roofline = {"bound": "mfma", "kernel": "igemm_kernel + igemm_h2_local224_kernel (avs_conv2d_nhwc[_bnstats|_bnlocal|_affine])",
                "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                "traffic": traffic[0], "traffic_source": traffic[1],
                "launches": seen, "timed_launches": conv["launches"],
                "avg_launch_us": round(conv["ms"] * 1e3 / conv["launches"], 2),
                "algorithmic_flop_per_launch": round(conv["flops"] / conv["launches"], 1),
                "algorithmic_bytes_per_launch": round(conv["bytes"] / conv["launches"], 1),
                "share_of_step": round(conv["ms"] * 1e-3 / elapsed * seen / conv["launches"], 3)}
    # the other reading, side by side: the ALGORITHMIC rate against the nominal dense 16-bit peak (fp32: its own peak)
    nominal = MFMA_F32_PEAK_TFLOPS if (dtype == torch.float32 and not split) else MFMA_BF16_PEAK_TFLOPS
    roofline["frac_of_nominal_peak"] = round(achieved / nominal, 4)
    roofline["nominal_peak"] = nominal
    if split:
        roofline["mfma_rate_tflops"] = round(3.0 * achieved, 1)
        roofline["note"] = ("three 16-bit MFMAs per algorithmic product (hi*hi + hi*lo + lo*hi): peak = 2500 / 3; "
                            "mfma_rate_tflops = the matrix-core rate behind the algorithmic figure; "
                            "frac_of_nominal_peak = algorithmic rate / 2500")
    # where the step goes, by form of the contraction kernel (epilogue form x filter size): share of the step,
    # algorithmic TFLOP/s and algorithmic TB/s of each (matrix-pipe busy per form: profiles/*_sq_counters.json)
    frm = prof.forms("conv", code)
    scale_up = seen / conv["launches"]
    rows = []
    for name, rec in sorted(frm.items(), key=lambda kv: -kv[1]["ms"]):
        if rec["ms"] <= 0:
            continue
        rows.append({"form": name, "timed_launches": rec["launches"],
                     "share_of_step": round(rec["ms"] * 1e-3 * scale_up / elapsed, 4),
                     "tflops": round(rec["flops"] / (rec["ms"] * 1e-3) / 1e12, 1),
                     "frac_of_peak": round(rec["flops"] / (rec["ms"] * 1e-3) / 1e12 / peak, 4),
                     "tb_per_s": round(rec["bytes"] / (rec["ms"] * 1e-3) / 1e12, 3),
                     "frac_of_hbm_peak": round(rec["bytes"] / (rec["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
    roofline["forms"] = rows
    others = []
    for kind, label in (("convbn", "conv1x1_bn_kernel (avs_conv1x1_bn[_in]_bf16)"),
                        ("bn_apply", "bn_apply_kernel / bn_maxpool_kernel (avs_bn_apply, avs_bn_maxpool_nhwc)")):
        rec = summ.get((kind, code)) or summ.get((kind, ops.dtype_code(dtype)))
        if rec and rec["ms"] > 0:
            gbs = rec["flops"] / (rec["ms"] * 1e-3) / 1e9
            n = prof.seen.get((kind, code), rec["launches"])
            others.append({"bound": "hbm", "kernel": label, "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4), "launches": n,
                           "timed_launches": rec["launches"],
                           "avg_launch_us": round(rec["ms"] * 1e3 / rec["launches"], 2),
                           "algorithmic_bytes_per_launch": round(rec["flops"] / rec["launches"], 1),
                           "share_of_step": round(rec["ms"] * 1e-3 / elapsed * n / rec["launches"], 3)})
    if others:
        roofline["other_kernels"] = others
    return roofline


def pmc_traffic(mode):
    """HBM bytes per launch of the contraction kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE x2 on
    gfx950 + WRITE_SIZE, KiB -> bytes; profiles/summarize_pmc.py).  NOT measured in this run: the source file is
    named beside the number; (None, None) when no summary of this arithmetic mode is committed."""
    for name in PMC_TRAFFIC_FILES.get(mode, ()):
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        for key in ("igemm_kernel<4,split2>", "igemm_kernel<2>", "igemm_kernel"):
            if key in d:
                return d[key].get("hbm_bytes_per_launch"), f"profiles/{name} [{key}] (separate rocprofv3 --pmc run)"
    return None, None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """Write each array of `arrays` ({name: 1-D float32 / float64 numpy array}, all of one length) as out_dir/<name>.npy.
    Past `limit` bytes in all, the same fixed, seeded sample of positions is taken from every array and its positions
    are written beside them (sample_index.npy, float64).  Returns the names written."""
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        if v.dtype not in (np.float32, np.float64) or v.ndim != 1:
            raise ValueError(f"--dump-outputs: {k} is {v.dtype} {v.shape}, not a 1-D float32 / float64 array")
    n = {v.shape[0] for v in arrays.values()}
    if len(n) != 1:
        raise ValueError(f"--dump-outputs: arrays of different lengths {sorted(n)}")
    n = n.pop()
    total = sum(v.nbytes for v in arrays.values())
    if total > limit:
        keep = limit * n // (total + 8 * n)   # bytes per kept position: the arrays' + 8 for its float64 position
        idx = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["sample_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    log(f"outputs of the last timed step written to {out_dir}: {', '.join(sorted(arrays))}")
    return sorted(arrays)


def selection_mask(selected, offsets):
    """The per-video selected indices (FrameScoringPipeline.select) as one float32 0 / 1 mask over the frames."""
    mask = np.zeros(offsets[-1], dtype=np.float32)
    for a, sel in zip(offsets[:-1], selected):
        mask[a + np.asarray(sel, dtype=np.int64)] = 1.0
    return mask


# ------------------------------------------------------------------------------------------------ configs[2] leg
def config2_leg(extractor, scorer, dev, steps, videos, outputs=None):
    """configs[2] (TVSum shape): per video the whole-track log2-mel and MFCC (+ mfcc_proj) kernels
    (features/extractors.py:236-246), CNN embeddings of the frames the reference's sampling rule keeps (30-frame
    shots, absolute index % 3 == 0, mean over a shot, :395-413, :97-110), an audio vector per shot pooled from the
    track's frames, features/fusion.py (cost matrix float64, warping path, path-weighted gather, fusion.py:7-32) on
    the two 512-d embedded streams, then the scorer and the selection.  outputs (a dict): receives the last step's
    per-shot scores and selection mask (--dump-outputs)."""
    from avsum_amd import ops, synthetic
    from avsum_amd.audio import HOP, MelPlan
    from avsum_amd.features import fusion
    from avsum_amd.features.extractors import sample_shot_indices
    cfg = synthetic.config(2, videos=videos)
    lengths = cfg["lengths"]
    offsets = synthetic.offsets_of(lengths)
    total = offsets[-1]
    log(f"configs[2] leg: {len(lengths)} videos, {total} frames ({total * 150528 / 1e9:.1f} GB), generating")
    frames = synthetic.make_frames_uniform(total, dev, cfg["seed"])
    waves = [synthetic.make_waveform(int(ln / synthetic.FPS * synthetic.SAMPLE_RATE), cfg["seed"] + i).to(dev)
             for i, ln in enumerate(lengths)]
    samples = sum(w.numel() for w in waves)
    plan = MelPlan.get(synthetic.SAMPLE_RATE, 128, 40, dev)
    torch.manual_seed(11)
    proj = torch.nn.Linear(40, 128).to(dev)   # mfcc_proj: random, never trained (extractors.py:193)
    pw, pb = proj.weight.detach().float().contiguous(), proj.bias.detach().float().contiguous()
    # host plan: sampled frame indices, shot boundaries in frames / STFT frames
    pick, shot_of_pick, shot_rows, segs = [], [0], [0], []
    for v, ln in enumerate(lengths):
        shots_v = synthetic.uniform_shots(ln)
        for s, e in shots_v:
            idx = sample_shot_indices(s, e)
            pick.extend(offsets[v] + i for i in idx)
            shot_of_pick.append(shot_of_pick[-1] + len(idx))
        shot_rows.append(len(shot_of_pick) - 1)
        nf = 1 + waves[v].numel() // HOP
        bounds = [min(nf, int(s / synthetic.FPS * synthetic.SAMPLE_RATE) // HOP) for s, _ in shots_v] + [nf]
        segs.append(bounds)
    audio_tables = plan.batch_tables(waves, segs, dev)   # the batch's tracks in one buffer + block / segment tables
    pick_t = torch.tensor(pick, dtype=torch.int64, device=dev)
    seg_pick = torch.tensor(shot_of_pick, dtype=torch.int64, device=dev)
    shots = len(shot_of_pick) - 1
    runner = extractor._resnet_runner
    vfc, afc = scorer.visual_fc[0], scorer.audio_fc[0]
    audio_ms = [0.0]
    last_host = [None]

    def step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # audio front end, per track: the per-shot time means of the log2-mel rows and of the clamped dB-mel rows straight
        # from the waveform (no [frames, 128] matrix reaches HBM); the MFCC rows' mean is the DCT of the mean dB row and
        # mfcc_proj of that (both linear): two small GEMMs over all shots
        e0.record()
        audio296 = torch.zeros((shots, 296), dtype=torch.float32, device=dev)
        mean_db = torch.empty((shots, 128), dtype=torch.float32, device=dev)
        plan.segment_means_batch(audio_tables, audio296[:, 128:256], mean_db)   # all 50 tracks: four launches
        audio296[:, :128] = ops.linear(ops.linear(mean_db, plan.dct), pw, pb)   # per-shot mean of the projected MFCC
        e1.record()
        # visual: CNN embedding of the sampled frames (passes of 12288), mean over each shot
        feats = torch.empty((len(pick), 2048), dtype=torch.float32, device=dev)
        for a in range(0, len(pick), 12288):
            b = min(a + 12288, len(pick))
            runner.forward(frames.index_select(0, pick_t[a:b]), out=feats[a:b])
        visual = torch.zeros((shots, 4096), dtype=torch.float32, device=dev)
        ops.segment_mean(feats, seg_pick, visual[:, :2048])
        # fusion on the two 512-d embedded streams, per video
        v512 = ops.linear(visual, vfc.weight, vfc.bias, ops.ACT_RELU)
        a512 = ops.linear(audio296, afc.weight, afc.bias, ops.ACT_RELU)
        fused_rows = 0
        for v in range(len(lengths)):
            rows = slice(shot_rows[v], shot_rows[v + 1])
            cost = fusion.compute_dtw_device(v512[rows], a512[rows])
            path, plen, _ = ops.dtw_path(cost)
            # interpolate_features (fusion.py:21-32): unique() of the path's first column, here on the device
            uniq, counts = torch.unique(path[:int(plen.item()), 0], return_counts=True)
            fused_rows += ops.gather_scale(v512[rows].contiguous(), uniq, counts.double() / counts.sum()).shape[0]
        seq = torch.tensor(shot_rows, dtype=torch.int64, device=dev)
        scores = scorer.score_rows(visual, audio296, seq, attn_batch=1)
        host = scores.cpu().numpy()
        last_host[0] = host
        sel = sum(int((host[a:b] > host[a:b].mean()).sum()) for a, b in zip(shot_rows[:-1], shot_rows[1:]))
        audio_ms[0] += e0.elapsed_time(e1)
        return sel, fused_rows

    with torch.no_grad():
        step()
        torch.cuda.synchronize()
        audio_ms[0] = 0.0
        t0 = time.perf_counter()
        for _ in range(steps):
            sel, fused_rows = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if outputs is not None:
        host = last_host[0]
        outputs["scores"] = host.astype(np.float32)
        outputs["selected_mask"] = np.concatenate([(host[a:b] > host[a:b].mean()).astype(np.float32)
                                                   for a, b in zip(shot_rows[:-1], shot_rows[1:])])
    stft_frames = sum(1 + w.numel() // HOP for w in waves)
    # 4 B per sample read; "if time-mean pooled on-chip, output ~ 0": the two per-shot [shots, 128] means
    algo_bytes = 4.0 * samples + 2 * 512.0 * shots
    a_s = audio_ms[0] * 1e-3 / steps
    del frames
    torch.cuda.empty_cache()
    return {"workload": cfg["name"] + f": {total} frames, {len(pick)} sampled frames through the CNN, {shots} shots, "
                        f"{samples / 16000:.0f} s of 16 kHz audio (whole-track log2-mel + MFCC-proj, pooled per shot), "
                        "cdist + DTW path + gather on the 512-d streams, scorer + selection",
            "value": round(total * steps / dt, 1), "unit": "frames/s", "steps": steps,
            "ms_per_step": round(dt * 1e3 / steps, 2), "cnn_frames_per_s": round(len(pick) * steps / dt, 1),
            "selected_shots": sel, "fused_rows": fused_rows,
            "audio_roofline": {"bound": "hbm", "kernels": "avs_stft_mel_segmean_batch_f32 (all tracks in one set of launches: span in LDS, folded fp64-MFMA DFT, mel + log on chip, ONE pass - the unclamped dB rows through a workspace, the track maxima in the same pass, then a bandwidth-bound clamp + sum) + DCT, mfcc_proj on the means",
                               "achieved": round(algo_bytes / a_s / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(algo_bytes / a_s / 1e9 / HBM_PEAK_GBS, 4),
                               "samples_per_s": round(samples / a_s, 0), "ms_per_step": round(a_s * 1e3, 3),
                               "algorithmic_bytes": algo_bytes,
                               "stft_frames": stft_frames,
                               "fp64_mfma_tflops": round(stft_frames * 0.16e6 / a_s / 1e12, 2),
                               "fp64_mfma_frac": round(stft_frames * 0.16e6 / a_s / 1e12 / 78.6, 4),
                               "note": "4 B/sample read + the per-shot means written (SURVEY 8 D3, pooled on chip); bound by the exact fp64 DFT (0.16 MFLOP per STFT frame against the 78.6 TFLOP/s fp64-MFMA peak: fp64_mfma_frac), DESIGN section 3"}}


# ------------------------------------------------------------------------------------------------ configs[4] leg
def config4_leg(dev, steps=20, lengths=(300, 1800), oracle_steps=6, rank=0, world=1, outputs=None):
    """configs[4] (scripts/train_av_model.py:70-96 on synthetic labels) at world size 1: the reference's training step -
    Dropout active, forward, MSE against the one broadcast target, loss.backward(), AdamW(lr 1e-4).step() - for `steps`
    steps per sequence length, every step through avsum_amd.scripts.train_av_model.train_step (forward and backward are
    libavsum_hip.so calls; loss / optimiser are the caller's torch, as in the reference).  Features resident on the
    device.  Also: the LSTM sweeps alone (us per time step, forward with saved gates and backward through time, all four
    recurrences in one launch: split over four CUs each as the step runs them, and one CU per recurrence beside it), and the first `oracle_steps` losses against the CPU restatement under the same Dropout
    masks (<= 1e-4 relative).
    world > 1 (launched with torch.distributed.run, one rank per GPU): plain data parallelism as SURVEY 8 E1 states it - every
    rank takes its own video per step, train_step averages the gradients over the ranks (dist.allreduce_gradients: one RCCL
    all-reduce of the 38.7 MB bucket) before AdamW; videos per second = world x steps per second.  The loss trajectory against
    the oracle is a world-1 statement (the effective batch differs) and is skipped.  outputs (a dict): receives the loss of
    the last timed step of every length (--dump-outputs)."""
    from avsum_amd import _abi, ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import train_step
    from oracle import scorer as osc
    out = {"workload": "configs[4]: scripts/train_av_model.py:70-96 on synthetic labels ~U[1,5], one video per step "
                       f"(B = 1), fp32, world size 1, {steps} timed steps per length (2 warm-up); visual randn "
                       "[T,4096], audio = zeros [T,296] (SURVEY Q5), features resident in HBM", "lengths": {}}
    for t_len in lengths:
        torch.manual_seed(7)
        model = AVBiLSTMModel().to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        g = torch.Generator().manual_seed(5005 + t_len + 7919 * rank)      # every rank its own video
        feats = {"visual": torch.randn(t_len, 4096, generator=g).to(dev), "audio": torch.zeros(t_len, 296, device=dev)}
        labels = torch.rand(t_len * 30, generator=g) * 4 + 1
        for _ in range(2):
            train_step(model, opt, feats, labels, dev)
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = train_step(model, opt, feats, labels, dev)
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        dt = time.perf_counter() - t0
        if outputs is not None:
            outputs[f"loss_t{t_len}"] = np.array([loss], dtype=np.float64)
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
            dt = float(tmax.item())
        # forward-only (inference kernel path) for the ratio
        model.eval()
        with torch.no_grad():
            model(feats["visual"].unsqueeze(0), feats["audio"].unsqueeze(0))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(steps):
                model(feats["visual"].unsqueeze(0), feats["audio"].unsqueeze(0))
            torch.cuda.synchronize()
            dt_inf = time.perf_counter() - t1
        # the two LSTM sweeps alone, four recurrences per launch
        hid = 256
        xproj = torch.randn(t_len, 16 * hid, generator=g).to(dev)
        whh = torch.stack([model.visual_bilstm.weight_hh_l0, model.visual_bilstm.weight_hh_l0_reverse,
                           model.audio_bilstm.weight_hh_l0, model.audio_bilstm.weight_hh_l0_reverse]).detach().contiguous()
        whh_t = whh.transpose(1, 2).contiguous()
        seq = torch.tensor([0, t_len], dtype=torch.int64, device=dev)
        fused = torch.empty(t_len, 4 * hid, device=dev)
        dfused = torch.randn(t_len, 4 * hid, generator=g).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def sweeps(variant):
            f_ms, b_ms = [], []
            for _ in range(6):
                ev[0].record()
                gates, cell = ops.lstm_train_fwd(xproj, whh_t, hid, 4, 0b1010, seq, fused, 0, variant=variant)
                ev[1].record()
                ops.lstm_bwd(dfused, 0, gates, cell, whh, hid, 4, 0b1010, seq, variant=variant)
                ev[2].record()
                torch.cuda.synchronize()
                f_ms.append(ev[0].elapsed_time(ev[1]))
                b_ms.append(ev[1].elapsed_time(ev[2]))
            return statistics.median(f_ms[1:]) * 1e3 / t_len, statistics.median(b_ms[1:]) * 1e3 / t_len
        f_us, b_us = sweeps(_abi.LSTM_AUTO)                 # what the step runs: one recurrence split over four CUs
        f1_us, b1_us = sweeps(_abi.LSTM_RESIDENT_20_8)      # beside it: one recurrence per CU (rounds 3-4's kernels)
        if ops.lstm_split_errors(dev):
            raise RuntimeError("split LSTM recurrence: a bounded wait ran out")
        out["lengths"][str(t_len)] = {
            "steps_per_s": round(steps / dt, 2), "ms_per_step": round(dt * 1e3 / steps, 3),
            "videos_per_s": round(world * steps / dt, 2), "frames_per_s": round(world * steps * t_len / dt, 1),
            "last_loss": round(loss, 6),
            "inference_forward_ms": round(dt_inf * 1e3 / steps, 3),
            "lstm_forward_us_per_time_step": round(f_us, 3), "lstm_backward_us_per_time_step": round(b_us, 3),
            "lstm_backward_over_forward": round(b_us / f_us, 3),
            "lstm_one_cu_per_recurrence_us_per_time_step": {"forward": round(f1_us, 3), "backward": round(b1_us, 3)}}
        log(f"configs[4] T={t_len}: {steps / dt:.1f} steps/s, LSTM {f_us:.2f} / {b_us:.2f} us per time step (fwd / bwd)")
    if world > 1:
        return out
    # loss trajectory against the oracle (CPU autograd through the restatement), same Dropout masks, T = lengths[0]
    t_len = lengths[0]
    torch.manual_seed(7)
    model = AVBiLSTMModel()
    ref_params = {k: p.detach().clone().requires_grad_(True) for k, p in model.named_parameters()}
    opt_ref = torch.optim.AdamW(list(ref_params.values()), lr=1e-4)
    model = model.to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(99)
    got, ref = [], []
    for _ in range(oracle_steps):
        v, a = torch.randn(1, t_len, 4096, generator=g), torch.zeros(1, t_len, 296)
        kv = (torch.rand(t_len, 512, generator=g) >= 0.3).float() / 0.7
        ka = (torch.rand(t_len, 512, generator=g) >= 0.3).float() / 0.7
        target = torch.rand(1, generator=g) * 4 + 1
        o_ref = osc.av_bilstm_forward_train(ref_params, v, a, kv, ka)
        l_ref = torch.nn.functional.mse_loss(o_ref, target.expand_as(o_ref))
        opt_ref.zero_grad()
        l_ref.backward()
        opt_ref.step()
        model._dropout_keep = (kv.to(dev), ka.to(dev))
        o = model(v.to(dev), a.to(dev))
        l_ = torch.nn.functional.mse_loss(o, target.to(dev).expand_as(o))
        opt.zero_grad()
        l_.backward()
        opt.step()
        got.append(float(l_.item()))
        ref.append(float(l_ref.item()))
    rel = max(abs(x - y) / abs(y) for x, y in zip(got, ref))
    out["loss_trajectory"] = {"steps": oracle_steps, "t": t_len, "hip": [round(x, 7) for x in got],
                              "oracle": [round(x, 7) for x in ref], "max_rel_err": rel, "bar": 1e-4,
                              "within_bar": bool(rel <= 1e-4)}
    return out


# ------------------------------------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 5; --config 4: 20 per sequence length)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3, 4],
                    help="BASELINE config of the headline: 1 = SumMe-shape batch per rank; 2 = the TVSum-shape "
                         "audio + visual + fusion leg alone (one GPU); 3 = one rank's share of the 400 x 5000-frame "
                         "sharded inference; 4 = the training loop leg alone (one GPU; sub_results.config4_training)")
    ap.add_argument("--videos", type=int, default=None)
    ap.add_argument("--mean-frames", type=int, default=None)
    ap.add_argument("--dtype", default="f16x2", choices=["f16x2", "bf16", "f32", "f32split"],
                    help="arithmetic of the CNN: f16x2 (default: the fastest mode that meets the accuracy bars - values "
                         "stored as fp16 hi | lo runs, three fp16 MFMAs per product), bf16 (throughput, misses the "
                         "bars), f32 (exact fp32 MFMA), f32split (fp32 storage, products on the bf16 matrix cores as "
                         "hi*hi + hi*lo + lo*hi)")
    ap.add_argument("--extractor", default="resnet50", choices=["resnet50", "resnet50+inception3"])
    ap.add_argument("--chunk", type=int, default=None,
                    help="most frames per pass of the trunk (passes are made equal).  Default: 24576 for bf16 (45 143 "
                         "frames = 2 x 22 572, ~160 GB of activations), 12288 for the 4-byte modes")
    ap.add_argument("--streams", type=int, default=1, choices=[1, 2],
                    help="2: consecutive passes of the trunk on two HIP streams, staggered by half a pass (the HBM-bound "
                         "layers 1-2 of one pass under the matrix-core-bound layers 3-4 of the other)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline as well: the live roofline (HIP events on the timed "
                         "launches), the CPU baseline and the accuracy of the timed mode, and (default headline, N=1) the "
                         "sub-results.  Off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--cpu-sample", type=int, default=None,
                    help="frames per CPU-baseline run (0 = skip; default: 128 with --full, 0 without)")
    ap.add_argument("--cpu-runs", type=int, default=5, help="CPU-baseline runs (the median is reported)")
    ap.add_argument("--frames-per-group", type=int, default=4,
                    help="BatchNorm micro-batch inside a video: 4 (default) = frames normalised in the reference's "
                         "micro-batches of 4 consecutive frames (extractors.py:48-56; a video's last group is shorter), "
                         "per-frame scores; 1 = every frame its own one-frame shot (= its own micro-batch)")
    ap.add_argument("--sub", default=None, choices=["auto", "all", "none"],
                    help="sub-results (other configurations): auto = all of them at N=1 with the default headline "
                         "(default: auto with --full, none without)")
    ap.add_argument("--no-profile", action="store_true", help="--full without the live roofline's HIP events")
    ap.add_argument("--profile-every", type=int, default=1,
                    help="bracket every n-th launch of each kernel kind with HIP events (1 = all: ~3%% slower at "
                         "small passes, nothing at 12288 frames)")
    ap.add_argument("--bn-local", default="on", choices=["on", "off"],
                    help="tuning: one-launch tile-local convolution + BatchNorm on the layers that take it")
    ap.add_argument("--p8", default="on", choices=["on", "off"],
                    help="tuning (f16x2): the inner block outputs of ResNet layers 1-2 stored as AVS_F16P8 (3 bytes per value)")
    ap.add_argument("--fuse", default=None, help="tuning: min_rows,ratio_num,ratio_den of the one-kernel conv+BN")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 20 if args.config == 4 else 5
    if args.cpu_sample is None:
        args.cpu_sample = 128 if args.full else 0
    if args.sub is None:
        args.sub = "auto" if args.full else "none"
    dumped = {} if args.dump_outputs else None

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the documented launcher as a CHILD process (this
        # process has not touched the GPU: nothing is re-exec'ed) and pass its exit code and its one JSON line through
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        log("no RANK / WORLD_SIZE in the environment: launching " + " ".join(cmd))
        raise SystemExit(subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")).returncode)
    from avsum_amd import _abi, dist as avd, synthetic
    from avsum_amd.evaluation.accuracy import accuracy_report
    from avsum_amd.features.extractors import VisualFeatureExtractor
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.pipeline import FrameScoringPipeline

    if args.chunk is None:
        # frames per pass of the trunk.  4-byte modes, ResNet-50 only: 16 384 (three passes of 15 048 for configs[1]; measured on
        # one box, back to back: 12 288 -> 26 624, 16 384 -> 26 750, 24 576 -> 26 779 frames/s; layer 1's 72 GB tensors at
        # 24 576 leave too little of the 288 GB); with Inception-v3 (its 147 x 147 maps are 5.5 MB per frame) 12 288
        args.chunk = 24576 if args.dtype == "bf16" else (16384 if args.extractor == "resnet50" else 12288)
    rank, world, local = avd.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    split = {"f32split": True, "f16x2": "f16x2"}.get(args.dtype, False)
    use_inception = args.extractor != "resnet50"
    fpg = args.frames_per_group

    # seeded random-init weights of the reference architectures (no pretrained files offline)
    torch.manual_seed(7)
    extractor = VisualFeatureExtractor(dtype, "batch", f32_split=split)
    scorer = AVBiLSTMModel().eval()
    with torch.no_grad():
        # seeded RE-SCALED init of the scoring head (tests/test_gpu_accuracy.py uses the same): with the
        # default init the sigmoid outputs span ~1.7e-3, so the 1e-4 score bar would be 6 % of the range and say
        # little; with this the scores span ~0.05 and 1e-4 is 0.2 % of it.  Random weights either way, same speed.
        scorer.scorer[0].weight.mul_(6.0)
        scorer.scorer[2].weight.mul_(6.0)
    sd_cpu = None
    if rank == 0 and args.cpu_sample > 0 and world == 1:
        sd_cpu = ({k: v.clone() for k, v in extractor.resnet.state_dict().items()},
                  {k: v.clone() for k, v in scorer.state_dict().items()},
                  {k: v.clone() for k, v in extractor.inception.state_dict().items()})
    runner = extractor._resnet_runner
    runner.bn_local = args.bn_local == "on"
    if os.environ.get("AVS_DIST_REHEARSAL") == "1" and world > 1:
        # several ranks on ONE GPU (tests only): the kernels whose workgroups wait for each other (clustered BatchNorm, split
        # LSTM recurrences) assume the device's CUs are fed by their own queue - processes time-sharing a GPU can each hold
        # partial groups that keep the other's partners out until the bounded waits give up (seen with 4 ranks on one GPU:
        # the launch ends, the error counters are raised as RuntimeError).  The rehearsal is about the multi-rank program
        # flow: it runs the forms without cross-workgroup waits
        from avsum_amd import ops as _ops_mod
        runner.bn_cluster = False
        _ops_mod.LSTM_SPLIT_MAX_RECURRENCES = 0
    if args.p8 == "off":
        runner.p8_blocks = ()
    if args.fuse is not None:
        runner.fuse_min_rows, runner.fuse_ratio_num, runner.fuse_ratio_den = [int(v) for v in args.fuse.split(",")]
    extractor = extractor.to(dev)
    scorer = scorer.to(dev)
    avd.broadcast_module(extractor, 0)  # C1
    avd.broadcast_module(scorer, 0)

    if args.config == 4:
        # the configs[4] training leg on its own (what sub_results.config4_training runs at N = 1); N > 1: data-parallel
        c4_steps = args.steps
        leg = config4_leg(dev, steps=c4_steps, rank=rank, world=world, outputs=dumped)
        if rank == 0:
            if dumped is not None:
                dump_outputs(args.dump_outputs, dumped)
            best = leg["lengths"]["1800"]
            print(json.dumps({"metric": "training videos/sec (scripts/train_av_model.py loop, T = 1800, data-parallel over the ranks)",
                              "value": best["videos_per_s"], "unit": "videos/s", "n_gpus": world, "steps": c4_steps, "warmup": 2,
                              "ms_per_step": best["ms_per_step"], "higher_is_better": True, "scaling": "weak",
                              "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                              "config": {"workload": leg["workload"], "parallelism": f"data-parallel x{world}: one video per rank "
                                         "per step, gradients averaged by one RCCL all-reduce (38.7 MB) before AdamW"},
                              "roofline": None, "cpu_baseline": None, "detail": leg}))
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return
    if args.config == 2:
        # the configs[2] leg on its own (what sub_results.config2_audio_visual_fusion runs), for profiling it alone
        if world != 1:
            raise SystemExit("--config 2 is the one-GPU audio + visual + fusion leg")
        leg = config2_leg(extractor, scorer, dev, args.steps, args.videos or 50, outputs=dumped)
        if dumped is not None:
            dump_outputs(args.dump_outputs, dumped)
        print(json.dumps({"metric": "frames/sec end-to-end (extract+fuse+score), 224x224 + 16kHz", "value": leg["value"],
                          "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": 1,
                          "ms_per_step": leg["ms_per_step"], "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
                          "config": {"workload": leg["workload"]}, "roofline": leg["audio_roofline"],
                          "cpu_baseline": None, "detail": leg}))
        return

    cfg = synthetic.config(args.config, rank, world, args.videos, args.mean_frames)
    lengths, video_ids = cfg["lengths"], cfg["video_ids"]
    offsets = synthetic.offsets_of(lengths)
    total = offsets[-1]
    log(f"rank {rank}: {cfg['name']}: {len(lengths)} videos, {total} frames ({total * 150528 / 1e9:.1f} GB); "
        "generating in HBM")
    frames = synthetic.make_frames_uniform(total, dev, cfg["seed"])
    torch.cuda.synchronize()
    log("frames ready")
    pipe = FrameScoringPipeline(extractor, scorer, use_inception=use_inception, chunk_frames=args.chunk,
                                frames_per_group=fpg, streams=args.streams)

    last_scores = [None]

    def step():
        scores = pipe.score(frames, offsets)
        last_scores[0] = scores
        if world > 1:
            gathered = avd.gather_video_scores(scores, video_ids, lengths, cfg["num_videos"])   # C2, global ids
            assert all(g is not None for g in gathered), "score gather is incomplete"
        return pipe.select(scores, offsets)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    elapsed, selected, prof = timed_steps(step, args.steps, args.warmup, barrier,
                                          args.profile_every if args.full and not args.no_profile else None)
    log(f"headline timed region {elapsed:.2f}s")
    if dumped is not None and rank == 0:
        dump_outputs(args.dump_outputs, {"scores": last_scores[0].float().cpu().numpy(),
                                         "selected_mask": selection_mask(selected, offsets)})

    t_all = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    n_all = torch.tensor([float(total)], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(t_all, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(n_all, op=torch.distributed.ReduceOp.SUM)
    t_max = float(t_all.item())
    frames_all = float(n_all.item())

    if rank == 0:
        roofline = roofline_from(prof, dtype, elapsed, pmc_traffic(args.dtype + ("+inception3" if use_inception else "")),
                                 split) if prof is not None else None
        group_txt = "per-frame shots" if fpg == 1 else f"the reference's {fpg}-frame BatchNorm micro-batches inside each video"

        # ---- CPU baseline + accuracy of the benchmarked mode on the same samples (outside every timed region)
        cpu, accuracy, s_frames, s_off, ref = None, None, None, None, None
        if sd_cpu is not None:
            cores = cpu_cores()
            torch.set_num_threads(cores)
            log(f"CPU baseline: {args.cpu_runs} runs of {args.cpu_sample} frames on {cores} cores")
            s_frames, s_ref, secs = cpu_runs(sd_cpu[0], sd_cpu[1], args.cpu_sample, args.cpu_runs, use_inception,
                                             sd_cpu[2] if use_inception else None, fpg)
            rates = [args.cpu_sample / s for s in secs]
            cpu = {"value": round(statistics.median(rates), 2), "unit": "frames/s", "cores": cores, "kind": "port",
                   "runs": len(rates), "min": round(min(rates), 2), "max": round(max(rates), 2),
                   "sample": f"median of {len(rates)} runs, each one {args.cpu_sample}-frame video of the same "
                             f"workload ({group_txt}) through oracle/ (torch-CPU fp32), {sum(secs):.1f} s in all"}
            s_off = synthetic.offsets_of([args.cpu_sample] * len(s_frames))
            dev_frames = torch.from_numpy(np.concatenate(s_frames)).to(dev)
            ref = np.concatenate(s_ref)
            got = pipe.score(dev_frames, s_off).cpu().numpy()
            again = pipe.score(dev_frames, s_off).cpu().numpy()
            rep = accuracy_report(got, ref, s_off)   # guard-banded bars: ONE definition, shared with the tests
            accuracy = {k: (round(v, 8) if isinstance(v, float) else v) for k, v in rep.items()}
            accuracy.update({"mode": args.dtype, "against": "oracle/ fp32 (CPU) on the cpu_baseline samples",
                             "deterministic": bool(np.array_equal(got, again))})
            del dev_frames

        # ---- sub-results: the other claimed configurations (N = 1)
        subs = None
        default_headline = (args.config == 1 and fpg == 4 and not use_inception and args.dtype == "f16x2"
                            and args.videos is None and args.mean_frames is None)
        if world == 1 and (args.sub == "all" or (args.sub == "auto" and default_headline)):
            subs = {}
            dev_samples = torch.from_numpy(np.concatenate(s_frames)).to(dev) if s_frames is not None else None

            def run_sub(name, pipe_, frames_, offsets_, note, steps_=2, roof=None, acc=False, stream_of_batches=False,
                        traffic_mode=None):
                """roof = (torch dtype, split): also bracket the contraction launches with HIP events -> own roofline
                block; acc: this mode's accuracy against the oracle on the cpu_baseline samples."""
                def s_step():
                    # stream_of_batches: the next batch (synthetic: the same pinned tensor) is announced to the call, which
                    # uploads its first pass under its own last pass - steady state of a stream of host-resident batches
                    sc = pipe_.score(frames_, offsets_, next_batch=(frames_, offsets_) if stream_of_batches else None)
                    return pipe_.select(sc, offsets_)
                dt, sel, prof_ = timed_steps(s_step, steps_, 1, torch.cuda.synchronize, 1 if roof else None)
                n = offsets_[-1]
                subs[name] = {"workload": note, "value": round(n * steps_ / dt, 1), "unit": "frames/s",
                              "steps": steps_, "ms_per_step": round(dt * 1e3 / steps_, 2),
                              "selected_frames": int(sum(len(s) for s in sel))}
                if roof:
                    subs[name]["roofline"] = roofline_from(prof_, roof[0], dt,
                                                           pmc_traffic(traffic_mode) if traffic_mode else (None, None), roof[1])
                if acc and dev_samples is not None:
                    a_ = accuracy_report(pipe_.score(dev_samples, s_off).cpu().numpy(), ref, s_off)
                    subs[name]["accuracy"] = {k: (round(v, 8) if isinstance(v, float) else v) for k, v in a_.items()}
                log(f"sub-result {name}: {subs[name]['value']} frames/s")

            base = cfg["name"] + f" ({total} frames), "

            def other_mode(dt_, split_):
                e = VisualFeatureExtractor(dt_, "batch", f32_split=split_)
                e.load_state_dict(extractor.state_dict())
                return e.to(dev)

            # bf16 throughput mode: what configs[1] names ("bf16"); fast, and NOT parity-grade - its accuracy is beside it
            ext16 = other_mode(torch.bfloat16, False)
            pipe16 = FrameScoringPipeline(ext16, scorer, use_inception=False, chunk_frames=24576, frames_per_group=fpg)
            run_sub("bf16_throughput_mode", pipe16, frames, offsets, base + "bf16 storage and MFMA (8 significant bits "
                    "per stored activation): the throughput mode; misses north_star's accuracy bars (accuracy beside it)",
                    roof=(torch.bfloat16, False), acc=True)
            run_sub("bf16_resnet50+inception3", FrameScoringPipeline(ext16, scorer, use_inception=True,
                                                                     chunk_frames=min(args.chunk, 12288),
                                                                     frames_per_group=fpg),
                    frames, offsets, base + "bf16, both trunks of VisualFeatureExtractor.forward (Inception-v3: eval "
                    "BatchNorm folded, 299x299 bilinear resize on the GPU)")
            del ext16, pipe16
            pipe_both = FrameScoringPipeline(extractor, scorer, use_inception=True, chunk_frames=min(args.chunk, 8192),
                                             frames_per_group=fpg)
            run_sub("resnet50+inception3", pipe_both, frames, offsets, base + args.dtype + ", both trunks of "
                    "VisualFeatureExtractor.forward in the headline arithmetic (Inception-v3: eval BatchNorm folded, bias + ReLU "
                    "epilogue, the 1x1 heads of a block as one contraction, 299x299 bilinear resize on the GPU): the 4096-d "
                    "embedding with both halves live", roof=(dtype, split),
                    traffic_mode=(args.dtype + "+inception3"))
            if sd_cpu is not None and args.cpu_sample > 0:
                # its accuracy against the oracle with BOTH trunks on the CPU: two of the cpu_baseline's sample videos
                log("both trunks: oracle scores of 2 sample videos (ResNet-50 + Inception-v3 on the CPU)")
                b_frames, b_ref, _ = cpu_runs(sd_cpu[0], sd_cpu[1], args.cpu_sample, 2, True, sd_cpu[2], fpg)
                b_off = synthetic.offsets_of([args.cpu_sample] * 2)
                b_dev = torch.from_numpy(np.concatenate(b_frames)).to(dev)
                a_ = accuracy_report(pipe_both.score(b_dev, b_off).cpu().numpy(), np.concatenate(b_ref), b_off)
                subs["resnet50+inception3"]["accuracy"] = {k: (round(v, 8) if isinstance(v, float) else v) for k, v in a_.items()}
                del b_dev
            del pipe_both
            run_sub("frames_per_group_1", FrameScoringPipeline(extractor, scorer, use_inception=False,
                                                               chunk_frames=args.chunk, frames_per_group=1),
                    frames, offsets, base + args.dtype + ", every frame its own one-frame shot = its own BatchNorm "
                    "micro-batch (the per-frame-shot reading of extractors.py:48-56; rounds 1-3's headline grouping)")
            # PCIe-inclusive: the same headline step with the frames in pinned host memory, each pass uploaded by a
            # copy stream while the previous pass computes
            host_frames = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
            host_frames.copy_(frames)
            torch.cuda.synchronize()
            run_sub("h2d_inclusive", pipe, host_frames, offsets, base + args.dtype + " headline step with the uint8 "
                    "frames in PINNED HOST memory: every pass pulled over PCIe by a 16-workgroup kernel on a copy "
                    "stream into one of two staging buffers while the previous pass computes; a stream of batches: the next "
                    "batch's first pass is pulled under this batch's last pass (the warm-up step pays the one exposed upload)",
                    steps_=3, stream_of_batches=True)
            subs["h2d_inclusive"]["fraction_of_resident"] = round(subs["h2d_inclusive"]["value"] * t_max / (frames_all * args.steps), 4)
            del host_frames
            # exact fp32 MFMA
            ext32 = other_mode(torch.float32, False)
            pipe32 = FrameScoringPipeline(ext32, scorer, use_inception=False, chunk_frames=4096, frames_per_group=fpg)
            run_sub("fp32_exact_mode", pipe32, frames, offsets, base + "exact fp32 MFMA (v_mfma_f32_32x32x2_f32, "
                    "157 TFLOP/s peak), fp32 storage", roof=(torch.float32, False), acc=True)
            if accuracy is not None and last_scores[0] is not None:
                # the headline arithmetic on ALL the frames it times, against the exact-fp32 HIP path (GPU vs GPU: the CPU
                # oracle at 35 frames/s cannot cover 45 k frames): score difference, per-video selection agreement
                s32 = pipe32.score(frames, offsets).cpu().numpy()
                sh = last_scores[0].cpu().numpy()
                xr = accuracy_report(sh, s32, offsets)
                per_video = [float(np.mean((sh[a:b] > sh[a:b].mean()) == (s32[a:b] > s32[a:b].mean())))
                             for a, b in zip(offsets[:-1], offsets[1:])]
                accuracy["full_batch_cross_mode"] = {
                    "what": f"{args.dtype} scores vs exact-fp32 HIP scores on all {total} frames of the timed batch "
                            f"({len(lengths)} videos, T = {min(lengths)}..{max(lengths)})",
                    "score_max_abs_diff": round(float(np.abs(sh - s32).max()), 9),
                    "selection_agreement_unguarded_min_over_videos": round(min(per_video), 6),
                    "selection_agreement_unguarded_mean": round(float(np.mean(per_video)), 6),
                    **{k: (round(v, 8) if isinstance(v, float) else v) for k, v in xr.items()}}
                log(f"cross-mode on the full batch: max |{args.dtype} - fp32| = {np.abs(sh - s32).max():.3e}")
            del ext32, pipe32
            # fp32 storage, convolution products on the bf16 matrix cores as hi*hi + hi*lo + lo*hi (AVS_F32_SPLIT)
            exts = other_mode(torch.float32, True)
            pipes = FrameScoringPipeline(exts, scorer, use_inception=False, chunk_frames=4096, frames_per_group=fpg)
            run_sub("fp32_split_mode", pipes, frames, offsets, base + "fp32 activations and weights split into bf16 hi + "
                    "lo inside the contraction loop (~2^-15 relative per product)", roof=(torch.float32, True), acc=True)
            del exts, pipes, dev_samples
            frames = None
            torch.cuda.empty_cache()
            subs["config2_audio_visual_fusion"] = config2_leg(extractor, scorer, dev, 3, 50)
            log(f"sub-result config2: {subs['config2_audio_visual_fusion']['value']} frames/s")
            c3 = synthetic.config(3, 0, 1)
            off3 = synthetic.offsets_of(c3["lengths"])
            log(f"configs[3] share: {off3[-1]} frames ({off3[-1] * 150528 / 1e9:.1f} GB), generating")
            frames3 = synthetic.make_frames_uniform(off3[-1], dev, c3["seed"])
            run_sub("config3_one_rank_share", pipe, frames3, off3, "configs[3]: one rank's share of the 400 x "
                    "5000-frame sharded inference (50 videos x 5000 frames, 37.6 GB of frames in HBM), " + args.dtype +
                    ", " + group_txt + "; N > 1 is not measured here (one GPU per box)", steps_=3)
            del frames3
            torch.cuda.empty_cache()
            subs["config4_training"] = config4_leg(dev)

        out = {
            "metric": "frames/sec end-to-end (extract+fuse+score), 224x224 + 16kHz",
            "value": round(frames_all * args.steps / t_max, 2),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_max * 1e3 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic (uniform uint8 frames resident in HBM, seeded random-init weights; audio = literal "
                    "zeros(296) in the headline, SURVEY Q5; the 16 kHz mel/MFCC + fusion leg is sub_results.config2)",
            "config": {"workload": f"{cfg['name']} ({total} frames/GPU), visual-only {args.extractor} extractor "
                                   f"(batch-stat BN, {group_txt}) + AVBiLSTM attention scorer + mean-threshold selection",
                       "frames_per_gpu": total, "videos_per_gpu": len(lengths), "extractor": args.extractor,
                       "frames_per_group": fpg, "chunk_frames": args.chunk,
                       "parallelism": f"videos sharded x{world}, no data-path collective",
                       "selected_frames_rank0": int(sum(len(s) for s in selected))},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "accuracy": accuracy,
            "sub_results": subs,
        }
        print(json.dumps(out))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
