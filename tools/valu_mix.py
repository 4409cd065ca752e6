#!/usr/bin/env python3
"""Static figures of the path B kernels: compiles raytracing_engine_amd/csrc/path_b.hip to gfx950 assembly with exactly the flags the
library's Makefile gives that file (asked of make itself, so the two cannot drift) and prints, per kernel, the registers
(.vgpr_count), spills (.vgpr_spill_count), scratch bytes (.private_segment_fixed_size), the instruction count and the vector-
instruction mix that bench.py's roofline.valu_issue prices: wave-level vector instructions of the fast issue class (v_fma / v_fmac /
v_mul / v_add / v_sub f32, v_mov_b32: 2.65-2.87 cycles per SIMD, profiles/r02_valu_issue_rates.txt) against all others (4.3-4.8
cycles).   python tools/valu_mix.py [--src other/path_b.hip] [kernel-substring ...]"""
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_engine_amd", "csrc")
FAST = re.compile(r"^v_(fma_f32|fmac_f32|mul_f32|add_f32|sub_f32|subrev_f32|mov_b32)(_e32|_e64)?$")


def library_command():
    """The compile command of _obj/path_b.hip.o as make would run it, without its -c / -o."""
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", "_obj/path_b.hip.o"], check=True, capture_output=True, text=True).stdout
    cmd = shlex.split(next(l for l in out.splitlines() if " -c path_b.hip" in l))
    o = cmd.index("-o")
    del cmd[o:o + 2]
    cmd.remove("-c")
    cmd.remove("path_b.hip")
    return cmd


args = sys.argv[1:]
src = os.path.join(CSRC, "path_b.hip")
if args[:1] == ["--src"]:
    src, args = os.path.abspath(args[1]), args[2:]
want = args or ["pt_trace"]
with tempfile.TemporaryDirectory() as d:
    asm = os.path.join(d, "path_b.s")
    subprocess.run(library_command() + ["-I", CSRC, "--cuda-device-only", "-S", src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()

cur, stats, meta = None, {}, {}
for line in text.splitlines():
    m = re.match(r"^(_ZN2rt\w+):", line)
    if m:
        cur = m.group(1)
        stats[cur] = [0, 0, 0]  # instructions, vector instructions, fast class
        continue
    t = line.split()
    if not cur or not t or not line.startswith("\t") or t[0][0] in ".;" or t[0].endswith(":"):
        continue
    stats[cur][0] += 1
    if t[0].startswith("v_"):
        stats[cur][1] += 1
        if FAST.match(t[0]):
            stats[cur][2] += 1
    if t[0] == "s_endpgm":
        cur = None
for block in re.split(r"(?m)^  - (?=\.)", text.split("amdhsa.kernels:")[-1]):
    name = re.search(r"(?m)^    \.name:\s+(\S+)", block)
    if name:
        meta[name.group(1)] = [int(re.search(r"(?m)^    \.%s:\s+(\d+)" % k, block).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")]

names = subprocess.run(["c++filt"] + list(stats), capture_output=True, text=True).stdout.splitlines()
print(f"{'kernel':64s} {'vgpr':>4s} {'spill':>5s} {'scratch':>7s} {'instr':>6s} {'vector':>6s} {'fast':>5s} {'cycles/vector instr':>19s}")
for sym, name in sorted(zip(stats, names), key=lambda p: p[1]):
    total, vec, fast = stats[sym]
    name = name.split("(")[0].replace("void rt::", "")
    if any(w in name for w in want) and vec:
        v, s, p = meta[sym]
        print(f"{name:64s} {v:4d} {s:5d} {p:7d} {total:6d} {vec:6d} {fast:5d} {fast / vec * 2.75 + (1 - fast / vec) * 4.7:19.2f}")
