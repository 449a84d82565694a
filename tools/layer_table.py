#!/usr/bin/env python3
"""Per-layer accounting of the production ResNet-50 forward (bf16, batch-statistics BatchNorm, per-frame groups unless
--gf): every step of the runner's plan (convolution + BatchNorm + residual + ReLU in the step's form; the first block's
shared Gram step as its Gram matrix + one row per convolution) and the stem are bracketed with events IN PLACE, so the table
is the real pass, not isolated kernels.

Per layer: time per pass, matrix rate (algorithmic FLOP / time), stream rate (bf16 input + output + residual bytes /
time) and the time an ideal kernel would take: max(FLOP / 1.2 PFLOP/s, bytes / 5.5 TB/s) - 1.2 PF is what the LDS-DMA
intake allows a 128x128-tile contraction here, 5.5 TB/s what a streaming kernel reaches on this chip.

Usage: python tools/layer_table.py [--n 8192] [--gf 1] [--dtype bf16|f32split|f16x2] [--pack on|off|ab] [--mfma 16|32|ab]
       [--lookups ab]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if any(a.startswith("--mfma") or a.startswith("--lookups") for a in sys.argv[1:]):
    os.environ["AVS_STUDY_LIB"] = "1"  # the shape switch of the 224-row kernel lives in the study build only (make -C <pkg>/csrc study)
import torch
from avsum_amd import cnn, ops
from avsum_amd.features.extractors import VisualFeatureExtractor

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--gf", type=int, default=1)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32split", "f32", "f16x2"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--set", action="append", default=[], help="runner attribute override, e.g. --set gram_finish_min_k=64")
ap.add_argument("--p8", default="on", choices=["on", "off"], help="f16x2: AVS_F16P8 storage of the inner block outputs of layers 1-2")
ap.add_argument("--pack", default="on", choices=["on", "off", "ab"],
                help="f16x2, --gf 4: the packed clustered BatchNorm on / off, or ab: off, on, off in one run and a comparison of the cluster rows")
ap.add_argument("--mfma", default="", choices=["", "16", "32", "ab"],
                help="f16x2, study build: the 224-row kernel's matrix instruction forced to 16x16x32 / 32x32x16 (AVS_LOCAL224_MFMA), "
                     "or ab: 32, 16, 32 in one run and a comparison of its rows per instance (3x3 / 1x1)")
ap.add_argument("--lookups", default="", choices=["", "ab"],
                help="f16x2, study build: the per-value group lookups of layers 1-2 (AVS_GROUP_LOOKUPS: bit 0 the given-affine "
                     "epilogue's selects, bit 1 the nine-tap input transform's per-row lookups) - ab: kept, removed, kept again "
                     "in one run and a comparison per piece")
ap.add_argument("--short", type=int, default=0,
                help="study build (AVS_STUDY_LIB=1): reductions of at most this many bytes per row take 64-byte steps (rule: 2048)")
args = ap.parse_args()
if args.short:
    from avsum_amd import _abi
    _abi.lib().avs_tune_short_reduction_bytes(args.short)
dev = torch.device("cuda", 0)
dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
es = 2 if dt == torch.bfloat16 else 4
torch.manual_seed(0)
SPLIT = {"f32split": True, "f16x2": "f16x2"}.get(args.dtype, False)
MFMA_IDEAL = 1.2e15 / (3.0 if SPLIT else 1.0)   # three 16-bit MFMAs per product in the split modes
ext = VisualFeatureExtractor(dt, "batch", f32_split=SPLIT).to(dev)
runner = ext._resnet_runner if hasattr(ext, "_resnet_runner") else None
if runner is None:
    runner = next(v for v in vars(ext).values() if isinstance(v, cnn.ResNet50Runner))
for kv in args.set:
    k, v = kv.split("=")
    setattr(runner, k, type(getattr(runner, k))(int(v)))
if args.p8 == "off":
    runner.p8_blocks = ()
frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device=dev)
gf = torch.arange(0, args.n + 1, args.gf, dtype=torch.int64)

records = []
orig_conv = cnn.ResNet50Runner._conv
orig_stem = ops.stem_conv_bn_pool


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_conv(self, st, w, x, x_aff, groups, residual=None, res_aff=None):
    e0, e1 = ev(), ev()
    e0.record()
    out = orig_conv(self, st, w, x, x_aff, groups, residual, res_aff)
    e1.record()
    geom = st.geom[0]
    n, h, cin, kh, sh, ho, cout = geom[0], geom[1], geom[3], geom[4], geom[6], geom[10], geom[12]
    kk = (147 if st.block < 0 else kh * geom[5] * cin)
    rows = n * ho * geom[11]
    flops = 2.0 * rows * kk * cout
    in_elems = n * h * h * cin if sh == 1 or kh > 1 else rows * cin
    byts = (in_elems + rows * cout * (2 if residual is not None else 1)) * es
    form = st.form + ("+defer" if st.out == "deferred" else "")
    records.append((f"{h}x{h} {kh}x{kh}/{sh} {cin}->{cout}" + (" +res" if residual is not None else ""), form,
                    flops, byts, e0, e1))
    return out


def timed_stem(frames_u8, *a, **kw):
    e0, e1 = ev(), ev()
    e0.record()
    out = orig_stem(frames_u8, *a, **kw)
    e1.record()
    n = frames_u8.shape[0]
    records.append(("stem 7x7/2 3->64 + pool", "fused", 2.0 * n * 112 * 112 * 147 * 64,
                    n * (224 * 224 * 3 + 56 * 56 * 64 * es), e0, e1))
    return out


inside = [0]


def timed_conv_outer(self, *a, **kw):
    inside[0] += 1
    try:
        return timed_conv(self, *a, **kw)
    finally:
        inside[0] -= 1


def timed_op(fn, label):
    # the first block's shared Gram step (bf16): its Gram matrix and one streaming pass per convolution
    def wrapper(x2d, wt, rpg, *a, **kw):
        if inside[0]:
            return fn(x2d, wt, rpg, *a, **kw)
        e0, e1 = ev(), ev()
        e0.record()
        out = fn(x2d, wt, rpg, *a, **kw)
        e1.record()
        rows, k = x2d.shape
        nn = wt.shape[0]
        if label == "gram":
            records.append((f"56x56 gram {k} (for {nn} outputs)", "gram", 2.0 * rows * k * k, rows * k * es, e0, e1))
        else:
            records.append((f"56x56 1x1/1 {k}->{nn} (raw stem in)", "affine", 2.0 * rows * k * nn, rows * (k + nn) * es,
                            e0, e1))
        return out
    return wrapper


def timed_h2(fn, label):
    # AVS_F16X2: the first block's shared Gram step: its Gram matrix and one streaming pass per convolution
    def wrapper(*a, **kw):
        if inside[0]:
            return fn(*a, **kw)
        e0, e1 = ev(), ev()
        e0.record()
        out = fn(*a, **kw)
        e1.record()
        if label == "gram":
            rows, k = a[0].shape
            records.append((f"56x56 gram {k} (for {a[1].shape[0]} outputs)", "gram", 2.0 * rows * k * k, rows * k * es, e0, e1))
        else:
            n, h, cin, cout = a[1], a[2], a[4], a[9]
            rows = n * h * h
            records.append((f"56x56 1x1/1 {cin}->{cout} (one Gram)", "affine", 2.0 * rows * cin * cout,
                            rows * (cin + cout) * es, e0, e1))
        return out
    return wrapper


cnn.ResNet50Runner._conv = timed_conv_outer
ops.bn_gram_affine_h2 = timed_h2(ops.bn_gram_affine_h2, "gram")
ops.conv2d_affine = timed_h2(ops.conv2d_affine, "affine")
ops.stem_conv_bn_pool = timed_stem
orig_stem_h2 = ops.stem_conv_pool_h2


def timed_stem_h2(frames_u8, *a, **kw):
    e0, e1 = ev(), ev()
    e0.record()
    out = orig_stem_h2(frames_u8, *a, **kw)
    e1.record()
    n = frames_u8.shape[0]
    records.append(("stem 7x7/2 3->64 + pool", "fused h2", 2.0 * n * 112 * 112 * 147 * 64,
                    n * (224 * 224 * 3 + 56 * 56 * 64 * es), e0, e1))
    return out


ops.stem_conv_pool_h2 = timed_stem_h2
ops.bn_gram_affine = timed_op(ops.bn_gram_affine, "gram")
ops.conv1x1_affine = timed_op(ops.conv1x1_affine, "affine")


def measure(label):
    """One table of the pass as the runner's switches stand -> {(layer, form): ms}."""
    for _ in range(2):
        runner.forward(frames, gf)
    torch.cuda.synchronize()
    acc = None
    for _ in range(args.reps):
        records.clear()
        t0, t1 = ev(), ev()
        t0.record()
        runner.forward(frames, gf)
        t1.record()
        torch.cuda.synchronize()
        ms = [r[4].elapsed_time(r[5]) for r in records]
        acc = ms if acc is None else [min(a, b) for a, b in zip(acc, ms)]
        total = t0.elapsed_time(t1)
    print(f"{label}{args.n} frames, groups of {args.gf}, {args.dtype}: forward {total:.1f} ms = {args.n / total * 1e3:.0f} frames/s "
          f"(events between layers cost a few %)")
    print(f"{'layer':34s} {'form':11s} {'ms':>8s} {'TFLOP/s':>8s} {'TB/s':>6s} {'ideal ms':>8s} {'x ideal':>7s} {'excess ms':>9s}")
    tsum = isum = 0.0
    agg = {}
    for (name, form, flops, byts, _, _), ms in zip(records, acc):
        ideal = max(flops / MFMA_IDEAL, byts / 5.5e12) * 1e3
        tsum += ms
        isum += ideal
        k = (name, form)
        a = agg.setdefault(k, [0, 0.0, 0.0, flops, byts])
        a[0] += 1
        a[1] += ms
        a[2] += ideal
    for (name, form), (cnt, ms, ideal, flops, byts) in agg.items():
        print(f"{(str(cnt) + ' x ' + name):34s} {form:11s} {ms:8.2f} {flops * cnt / ms / 1e9:8.0f} {byts * cnt / ms / 1e9:6.2f} "
              f"{ideal:8.2f} {ms / ideal:7.2f} {ms - ideal:9.2f}")
    print(f"{'sum of layers':46s} {tsum:8.2f} {'':15s} {isum:8.2f} {tsum / isum:7.2f} {tsum - isum:9.2f}")
    print(f"{'sum of the cluster rows':46s} {sum(v[1] for k, v in agg.items() if k[1] == 'cluster'):8.2f}")
    return {k: (v[0], v[1]) for k, v in agg.items()}


if args.mfma == "ab":
    # shape 32, shape 16, shape 32 again in ONE process: the second shape-32 table gives the tool's repeatability per row.
    # The rows of the 224-row kernel: the cluster and local forms of the 14x14 and 7x7 maps, per instance (3x3: spatial)
    runner.pack_groups = args.pack != "off"
    tabs = []
    for label, shape in (("[mfma 32, 1st] ", "32"), ("[mfma 16] ", "16"), ("[mfma 32, 2nd] ", "32")):
        os.environ["AVS_LOCAL224_MFMA"] = shape
        tabs.append(measure(label))
        print()
    a1, s16, a2 = tabs
    for inst, spatial in (("3x3 rows (SPATIAL = true)", True), ("1x1 rows (SPATIAL = false)", False)):
        print(f"{inst:34s} {'shape 32':>9s} {'again':>9s} {'repeat':>7s} {'shape 16':>9s} {'change':>7s}  (ms; shape 32 = the faster of the two)")
        su = sp = rep = 0.0
        for k, (cnt, ms) in s16.items():
            if k[1] not in ("cluster", "local") or (" 3x3/" in k[0]) != spatial:
                continue
            a, b = a1[k][1], a2[k][1]
            base = min(a, b)
            su += base
            sp += ms
            rep += abs(a - b)
            print(f"{(str(cnt) + ' x ' + k[0]):34s} {a:9.2f} {b:9.2f} {abs(a - b) / base * 100:6.1f}% {ms:9.2f} {(ms - base) / base * 100:+6.1f}%")
        if su:
            print(f"{'sum':34s} {su:9.2f} {'':9s} {rep / su * 100:6.1f}% {sp:9.2f} {(sp - su) / su * 100:+6.1f}%")
        print()
elif args.lookups == "ab":
    # general paths, the group-aligned ones, general again in ONE process: the second general table gives the repeatability.
    # Piece A: the rows that hold a one-pass given-affine 1x1 (gram / affine forms of the 56 x 56 and 28 x 28 maps);
    # piece B: the 3x3 statistics rows of those maps (the nine-tap form with the input affine)
    tabs = []
    for label, bits in (("[lookups kept, 1st] ", "3"), ("[lookups removed] ", "0"), ("[lookups kept, 2nd] ", "3")):
        os.environ["AVS_GROUP_LOOKUPS"] = bits
        tabs.append(measure(label))
        print()
    a1, new, a2 = tabs
    maps = ("56x56 ", "28x28 ")
    for piece, pick in (("A: one-pass given-affine 1x1", lambda k: k[1] in ("gram", "affine") and " gram " not in k[0]),
                        ("B: nine-tap input transform", lambda k: k[1].startswith("stats") and " 3x3/1 " in k[0])):
        print(f"{piece:34s} {'kept':>9s} {'again':>9s} {'repeat':>7s} {'removed':>9s} {'change':>7s}  (ms; kept = the faster of the two)")
        su = sp = rep_ = 0.0
        for k, (cnt, ms) in new.items():
            if not k[0].startswith(maps) or not pick(k):
                continue
            a, b = a1[k][1], a2[k][1]
            base = min(a, b)
            su += base
            sp += ms
            rep_ += abs(a - b)
            verdict = "" if ms - base <= abs(a - b) else "  SLOWER than the repeatability"
            print(f"{(str(cnt) + ' x ' + k[0]):34s} {a:9.2f} {b:9.2f} {abs(a - b) / base * 100:6.1f}% {ms:9.2f} {(ms - base) / base * 100:+6.1f}%{verdict}")
        if su:
            print(f"{'sum':34s} {su:9.2f} {'':9s} {rep_ / su * 100:6.1f}% {sp:9.2f} {(sp - su) / su * 100:+6.1f}%"
                  f"  keep rule: {'met' if su - sp > rep_ else 'NOT met'}")
        print()
elif args.pack != "ab":
    if args.mfma:
        os.environ["AVS_LOCAL224_MFMA"] = args.mfma
    runner.pack_groups = args.pack == "on"
    measure("")
else:
    # unpacked, packed, unpacked again in ONE process: the second unpacked table gives the tool's repeatability per row
    tabs = []
    for label, pack in (("[unpacked, 1st] ", False), ("[packed] ", True), ("[unpacked, 2nd] ", False)):
        runner.pack_groups = pack
        tabs.append(measure(label))
        print()
    u1, pk, u2 = tabs
    print(f"{'cluster rows':34s} {'unpacked':>9s} {'again':>9s} {'repeat':>7s} {'packed':>9s} {'change':>7s}  (ms; unpacked = the faster of the two)")
    su = sp = 0.0
    for k, (cnt, ms) in pk.items():
        if k[1] != "cluster":
            continue
        a, b = u1[k][1], u2[k][1]
        base = min(a, b)
        su += base
        sp += ms
        print(f"{(str(cnt) + ' x ' + k[0]):34s} {a:9.2f} {b:9.2f} {abs(a - b) / base * 100:6.1f}% {ms:9.2f} {(ms - base) / base * 100:+6.1f}%")
    print(f"{'sum':34s} {su:9.2f} {'':9s} {'':7s} {sp:9.2f} {(sp - su) / su * 100:+6.1f}%")
