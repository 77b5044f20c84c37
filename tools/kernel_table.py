#!/usr/bin/env python3
"""Two builds of the kernel objects side by side (the table of profiles/ray_kernel_bodies.txt).
For every build/csrc/*.o of both builds: is the gfx950 .text byte-identical; and for the objects where it is not, per kernel, first build >
second build: VGPRs, SGPR spills, LDS and scratch bytes (the code object's kernel metadata), occupancy (the compiler's remarks next to
the object), the number of instructions, and whether the multiset of floating-point opcodes (every mnemonic containing f64 or f32) is the
same -- where it is not, the opcodes whose counts differ --, and whether the kernel's instructions with their operands are the same
text.  It counts opcodes and reads kernel descriptors, nothing else; no GPU.
usage: python tools/kernel_table.py <parent>/cuda-ray-tracer_amd/build/csrc <tree>/cuda-ray-tracer_amd/build/csrc"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"
TMP = tempfile.mkdtemp(prefix="kernel_table_")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tag):
    fat, co = os.path.join(TMP, tag + ".fat"), os.path.join(TMP, tag + ".co")
    run(LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    run(LLVM + "clang-offload-bundler", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle", "--output=" + co)
    return co


def text_bytes(co):
    out = co + ".text"
    run(LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.text", co, out)
    return open(out, "rb").read()


def kernels(obj, co):
    """name -> dict(vgpr, sspill, lds, scratch, occ, ops)"""
    notes = run(LLVM + "llvm-readelf", "--notes", co)
    k = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
        k[name] = dict(vgpr=get("vgpr_count"), sspill=get("sgpr_spill_count"), vspill=get("vgpr_spill_count"), lds=get("group_segment_fixed_size"),
                       scratch=get("private_segment_fixed_size"), occ=None, ops=collections.Counter(), text=[])
    remarks = open(obj + ".remarks").read()
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", remarks, re.S):
        if m.group(1) in k:
            k[m.group(1)]["occ"] = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", m.group(2)).group(1))
    cur = None
    for line in run(LLVM + "llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = k.get(m.group(1))
        elif cur is not None and line.startswith("\t"):
            cur["ops"][line.split()[0]] += 1
            cur["text"].append(line.split("//")[0].strip())
    return k


def fp(ops):
    return {o: n for o, n in ops.items() if "f64" in o or "f32" in o}


def demangled(name):
    """kernel<template arguments> of _ZN<len>rtk_<variant><len><kernel>I(Lb<0|1>E | Lj<n>E | Li<n>E)...E...; other names as they are"""
    m = re.match(r"_ZN\d+rtk_(?:strict|fast)(\d+)", name)
    if not m:
        return name[:48]
    rest = name[m.end():]
    kernel, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
    args = re.match(r"I((?:L[bji]\d+E)+)E", rest)
    if not args:
        return kernel
    return kernel + "<" + ", ".join(("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([bji])(\d+)E", args.group(1))) + ">"


def main(parent, tree):
    same, differ, rows, alone = [], [], [], []
    for obj in sorted(glob.glob(os.path.join(tree, "rt_*.o"))):
        base = os.path.basename(obj)
        if base == "rt_capi.o":
            continue
        a, b = code_object(os.path.join(parent, base), "a_" + base), code_object(obj, "b_" + base)
        if text_bytes(a) == text_bytes(b):
            same.append(base[:-2])
            continue
        differ.append(base[:-2])
        # paired by kernel name and template arguments, not by the mangled name: that one also spells the parameters' types
        ka = {demangled(name): k for name, k in kernels(os.path.join(parent, base), a).items()}
        kb = {demangled(name): k for name, k in kernels(obj, b).items()}
        alone += [(base[:-2], name, "first" if name in ka else "second") for name in sorted(set(ka) ^ set(kb))]      # (an instantiation that came or went)
        for name in kb:
            if name in ka:
                rows.append((base[:-2], name, ka[name], kb[name]))
    print(f"byte-identical .text ({len(same)}): {' '.join(same)}")
    print(f"differ ({len(differ)}): {' '.join(differ)}")
    print()
    print(f"{'object':<27}{'kernel<template args>':<50}{'VGPRs':>9}{'SGPRspill':>10}{'occ':>6}{'LDS':>13}{'scr':>5}{'instructions':>14}  same code  FP opcodes")
    bad = 0
    for obj, name, p, t in rows:
        fa, fb = fp(p["ops"]), fp(t["ops"])
        diff = "equal" if fa == fb else "DIFFER " + " ".join(f"{o} {fa.get(o, 0)}>{fb.get(o, 0)}" for o in sorted(set(fa) | set(fb)) if fa.get(o, 0) != fb.get(o, 0))
        ok = t["vspill"] == 0 and t["scratch"] == 0 and t["lds"] == p["lds"] and t["occ"] >= p["occ"]
        bad += not ok
        pair = lambda key: f"{p[key]}>{t[key]}"
        print(f"{obj:<27}{name:<50}{pair('vgpr'):>9}{pair('sspill'):>10}{pair('occ'):>6}{pair('lds'):>13}{t['scratch']:>5}"
              f"{sum(p['ops'].values()):>7}>{sum(t['ops'].values()):<6}  {'yes' if p['text'] == t['text'] else 'no':<9}  {diff}{'' if ok else '   <-- CONDITION MISSED'}")
    for obj, name, side in alone:
        print(f"{obj:<27}{name:<50}in the {side} build only")
    print()
    print(f"{len(rows)} kernels; conditions (no VGPR spill, no scratch, LDS equal, occupancy not lower) missed by {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
