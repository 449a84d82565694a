#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/isa_compare.py parent.s new.s

Kernels are matched by demangled name.  Classes:
  identical text      the kernel's body is the same text, register names included
  identical mnemonics the same sequence of mnemonics (operands and register names aside)
  same resources      another sequence; VGPRs, AGPRs, SGPRs, scratch, LDS and occupancy as in the first file
  moved               some resource figure differs
Every kernel outside the first two classes is listed with its figures and its mnemonic counts, second minus first."""
import collections
import re
import subprocess
import sys

FIELDS = ("instructions", "vgprs", "agprs", "sgprs", "sgpr_spills", "vgpr_spills", "scratch", "lds", "occupancy")
INFO = {"NumVgprs": "vgprs", "NumAgprs": "agprs", "TotalNumSgprs": "sgprs", "ScratchSize": "scratch",
        "LDSByteSize": "lds", "Occupancy": "occupancy"}


def kernels(path):
    """{mangled name: (body lines, mnemonics, figures)} of every .amdhsa_kernel of an assembly file."""
    text = open(path).read()
    spills = {}
    for entry in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):]):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            spills[name.group(1)] = tuple(int(re.search(rf"\.{k}_spill_count:\s+(\d+)", entry).group(1)) for k in ("sgpr", "vgpr"))
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\t\.amdhsa_kernel \1\n.*?^; Kernel info:\n(.*?)^\t\.", text, flags=re.S | re.M):
        name, body, info = m.groups()
        lines = [ln.strip() for ln in body.splitlines()]
        lines = [ln for ln in lines if re.match(r"[a-z]+_\w+", ln)]
        fig = {"instructions": len(lines), "sgpr_spills": spills[name][0], "vgpr_spills": spills[name][1]}
        for key, val in re.findall(r"^; (\w+)\s*[:=]\s*(\d+)", info, flags=re.M):
            if key in INFO:
                fig[INFO[key]] = int(val)
        out[name] = (lines, [ln.split()[0] for ln in lines], fig)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    print(f"kernels: {len(a)} in {a_path}, {len(b)} in {b_path}")
    if set(a) != set(b):
        print("NOT THE SAME SET.  only in the first:", sorted(set(a) - set(b)), "only in the second:", sorted(set(b) - set(a)))
    names = demangle(sorted(set(a) & set(b)))
    classes = collections.defaultdict(list)
    for sym, name in names.items():
        (la, ma, fa), (lb, mb, fb) = a[sym], b[sym]
        if la == lb:
            cls = "identical text"
        elif ma == mb:
            cls = "identical mnemonics"
        elif all(fa[k] == fb[k] for k in FIELDS[1:]):
            cls = "same resources"
        else:
            cls = "moved"
        classes[cls].append(name)
    for cls in ("identical text", "identical mnemonics", "same resources", "moved"):
        print(f"{cls:20s} {len(classes[cls])}")
    for cls in ("same resources", "moved"):
        for name in sorted(classes[cls]):
            sym = next(s for s, n in names.items() if n == name)
            fa, fb = a[sym][2], b[sym][2]
            ca, cb = collections.Counter(a[sym][1]), collections.Counter(b[sym][1])
            diff = ", ".join(f"{k} {cb[k] - ca[k]:+d}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k])
            figs = "  ".join(f"{k} {fa[k]}" + (f" -> {fb[k]}" if fa[k] != fb[k] else "") for k in FIELDS)
            print(f"\n[{cls}] {name}\n  {figs}\n  mnemonics: {diff or 'the same counts, another order'}")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
