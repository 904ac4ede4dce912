#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of one translation unit (a refactor's proof that the device code did not move):
    hipcc --cuda-device-only -S -O3 -std=c++17 --offload-arch=gfx950 [-fno-slp-vectorize] <file>.hip -o <side>.s      (both sides)
    python tools/compare_device_asm.py parent.s change.s [--normalise-label-ordinals]
compares, per kernel, the text from its label to .end_amdhsa_kernel and its amdhsa.kernels metadata entry, ignoring only lines that
carry the __hip_cuid_ symbol (a hash of the source text). Prints a markdown table; exit status 1 if a kernel present in both differs
or one exists only in the change. --normalise-label-ordinals: local labels (.LBB<n>_<m>, .Lfunc_end<n>) carry the function's ordinal
in the module, which shifts for every later kernel when an instantiation is added or removed; the option replaces <n> (and the
padding between such a label and its comment, which follows the label's length)."""
import re, sys, subprocess

def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))

def kernels(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    if NORM:      # local labels carry the function's ordinal in the module, which shifts when an instantiation leaves
        lines = [re.sub(r"BB\d+_", "BBn_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_endn", l)) for l in lines]
        # ... and a label's trailing comment is aligned to a column, so the padding moves when the ordinal gains or loses a digit
        lines = [re.sub(r"^(\.LBBn_\d+:)\s+;", r"\1 ;", l) for l in lines]
    body, meta = {}, {}
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    idx = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(_Z\w+):", l))}
    for n in names:
        a = idx[n]
        b = next(i for i in range(a, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        body[n] = "\n".join(lines[a:b + 1])
    # metadata: yaml entries start with "  - .agpr_count:" (first key of an entry) inside amdhsa.kernels
    a = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith("amdhsa.target:"))
    ent = []
    for l in lines[a + 1:b]:
        if l.startswith("  - "): ent.append([l])
        else: ent[-1].append(l)
    for e in ent:
        n = next(l.split()[1] for l in e if l.startswith("    .name:"))
        meta[n] = "\n".join(e)
    return body, meta

NORM = "--normalise-label-ordinals" in sys.argv
pa, ca = sys.argv[1], sys.argv[2]
pb, pm = kernels(pa); cb, cm = kernels(ca)
dm = demangle(sorted(set(pb) | set(cb)))
bad = 0
print("| kernel | body lines | body | metadata |"); print("|---|---|---|---|")
for n in sorted(set(pb) | set(cb), key=lambda x: dm[x]):
    if n not in cb: print(f"| `{dm[n]}` | {pb[n].count(chr(10)) + 1} | absent from the change | absent |"); continue
    if n not in pb: print(f"| `{dm[n]}` | - | ONLY IN CHANGE | |"); bad += 1; continue
    b = pb[n] == cb[n]; m = pm[n] == cm[n]; bad += (not b) + (not m)
    print(f"| `{dm[n]}` | {pb[n].count(chr(10)) + 1} | {'identical' if b else 'DIFFERS'} | {'identical' if m else 'DIFFERS'} |")
print(f"\n{len(pb)} kernels in the parent, {len(cb)} in the change, {bad} differences")
sys.exit(1 if bad else 0)
