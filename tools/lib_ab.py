#!/usr/bin/env python3
"""bench.py with two builds of librt_amd.so alternated in one call (results of its first use: profiles/shade_chain.txt).

    python tools/lib_ab.py --parent-lib PATH/librt_amd.so [--runs 5] [-- bench.py arguments]

Every run is a fresh process that loads its library through RT_AMD_LIB (raytracing_engine_amd/_lib.py), so the two builds must
share the ABI.  Runs go parent, branch, parent, branch, ...; each has a time limit of its own and the first that fails ends the
call.  The gate it prints: the branch's ms_per_step below the parent's in every adjacent pair of runs, and the difference of the
medians at least twice the parent's own max - min spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="librt_amd.so built from the parent commit")
    ap.add_argument("--branch-lib", default=os.path.join(ROOT, "raytracing_engine_amd", "librt_amd.so"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one bench.py process may take")
    ap.add_argument("bench_args", nargs="*", help="passed on to bench.py (after --)")
    args = ap.parse_args()
    libs = [("parent", os.path.abspath(args.parent_lib)), ("branch", os.path.abspath(args.branch_lib))]
    cmd = [sys.executable, "bench.py"] + args.bench_args
    print(f"{' '.join(cmd[1:])}", flush=True)
    ms = {name: [] for name, _ in libs}
    for k in range(args.runs):
        for name, lib in libs:
            p = subprocess.run(cmd, env=dict(os.environ, RT_AMD_LIB=lib), capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
            if p.returncode != 0:
                sys.exit(f"run {k + 1} of the {name} build exited with {p.returncode}: nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            ms[name].append(res["ms_per_step"])
            print(f"  run {k + 1} {name:7s} ms_per_step {res['ms_per_step']:.4f}  value {res['value']:.1f} {res['unit']}  host BVH build {res['config'].get('bvh_build_ms_host')} ms", flush=True)
    pa, br = ms["parent"], ms["branch"]
    pm, bm, spread = statistics.median(pa), statistics.median(br), max(pa) - min(pa)
    pairs = all(b < p for p, b in zip(pa, br)) and all(b < p for p, b in zip(pa[1:], br[:-1]))
    print(f"  parent median {pm:.4f}  min {min(pa):.4f}  max {max(pa):.4f}  spread {spread:.4f}")
    print(f"  branch median {bm:.4f}  min {min(br):.4f}  max {max(br):.4f}")
    print(f"  gain {pm - bm:+.4f} ms ({(pm - bm) / pm * 100:+.2f} %); branch below parent in every adjacent pair: {pairs}; "
          f"gain at least twice the parent's spread: {pm - bm >= 2 * spread}")


if __name__ == "__main__":
    main()
