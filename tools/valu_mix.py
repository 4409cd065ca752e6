#!/usr/bin/env python3
"""Static figures of the path B kernels: compiles the path B units of raytracing_engine_amd/csrc (the Makefile's PT_SRCS) to gfx950
assembly with exactly the flags the library's Makefile gives them (asked of make itself, so the two cannot drift) and prints, per
kernel, the registers (.vgpr_count), spills (.vgpr_spill_count), scratch bytes (.private_segment_fixed_size), the instruction count
and the vector-instruction mix that bench.py's roofline.valu_issue prices: wave-level vector instructions of the fast issue class
(v_fma / v_fmac / v_mul / v_add / v_sub f32, v_mov_b32: 2.65-2.87 cycles per SIMD, profiles/r02_valu_issue_rates.txt) against all
others (4.3-4.8 cycles).   python tools/valu_mix.py [--src other/pt_trace.hip] [kernel-substring ...]
--src: that file alone, with the flags of the unit of its name."""
import os
import re
import subprocess
import sys
import tempfile

import hip_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = re.compile(r"^v_(fma_f32|fmac_f32|mul_f32|add_f32|sub_f32|subrev_f32|mov_b32)(_e32|_e64)?$")

args = sys.argv[1:]
units = {u: None for u in hip_asm.make_var(ROOT, "PT_SRCS")}
if args[:1] == ["--src"]:
    units, args = {os.path.basename(args[1]): os.path.abspath(args[1])}, args[2:]
want = args or ["pt_trace"]
stats, meta = {}, {}
with tempfile.TemporaryDirectory() as d:
    for unit, src in units.items():
        text = hip_asm.assembly(ROOT, unit, d, src)
        for sym, (body, _) in hip_asm.functions(text).items():
            count = stats[sym] = [0, 0, 0]  # instructions, vector instructions, fast class
            for line in body:
                t = line.split()
                if not t or not line.startswith("\t") or t[0][0] in ".;" or t[0].endswith(":"):
                    continue
                count[0] += 1
                if t[0].startswith("v_"):
                    count[1] += 1
                    if FAST.match(t[0]):
                        count[2] += 1
                if t[0] == "s_endpgm":
                    break
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
