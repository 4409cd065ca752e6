#!/usr/bin/env python3
"""What sharing one device mesh among contexts changes (results: profiles/shared_mesh.txt).

    python tools/shared_mesh_ab.py bench  --parent-tree DIR [--workloads W,W] [--runs 5] [--lanes N]
        bench.py alternated in one call: the parent's checkout, this build, this build with RT_AMD_MESH_SHARING=0; per configuration the
        median and min - max of ms per step, the gate of profiles/shared_mesh.txt, and the wall time of the whole process
    python tools/shared_mesh_ab.py setup  --parent-tree DIR [--n-tris N]
        three contexts given the same soup: seconds per set_mesh (first and later contexts) and device memory in use afterwards
    python tools/shared_mesh_ab.py pmc    --parent-tree DIR [--workload W] [--lanes 3,1] [--fetch-only]
        rocprofv3 --kernel-trace --pmc passes (counters in runs of their own) over bench.py with the given lanes: L2 hit rate and
        fabric-side bytes per launch of the per-lane traversal kernels
Every GPU process runs under a time limit of its own, and the first one that fails ends the run."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"pt_trace_fused": "pt_trace_fused", "pt_trace<true, false": "pt_trace<any>", "pt_trace_packet": "pt_trace_packet"}


def configs(parent_tree):
    """(name, checkout whose bench.py and package run, environment)"""
    return [("parent", os.path.abspath(parent_tree), {}), ("branch", ROOT, {}), ("branch, sharing off", ROOT, {"RT_AMD_MESH_SHARING": "0"})]


def run(cmd, env, limit, cwd=ROOT):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit, cwd=cwd)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"{' '.join(cmd)} exited with {p.returncode}: nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout, dt


def bench(args):
    for w in args.workloads.split(","):
        cmd = [sys.executable, "bench.py", "--workload", w, "--steps", str(args.steps), "--warmup", "3"] + (["--frames-in-flight", str(args.lanes)] if args.lanes else [])
        print(f"{w}: {' '.join(cmd[1:])}", flush=True)
        ms, wall = {}, {}
        for k in range(args.runs):
            for name, tree, env in configs(args.parent_tree):
                out, dt = run(cmd, env, args.limit, cwd=tree)
                res = json.loads(out.strip().splitlines()[-1])
                ms.setdefault(name, []).append(res["ms_per_step"])
                wall.setdefault(name, []).append(dt)
                print(f"  run {k + 1} {name:20s} ms_per_step {res['ms_per_step']:8.4f}  value {res['value']:9.3f} Mrays/s  lanes {res['config']['frames_in_flight']}  process {dt:6.2f} s", flush=True)
        for name in ms:
            print(f"  {name:20s} ms_per_step median {statistics.median(ms[name]):.4f}  min {min(ms[name]):.4f}  max {max(ms[name]):.4f}   "
                  f"process wall median {statistics.median(wall[name]):.2f} s  min {min(wall[name]):.2f}  max {max(wall[name]):.2f}")
        spread = max(ms["parent"]) - min(ms["parent"])
        pm, bm, om = (statistics.median(ms[k]) for k in ("parent", "branch", "branch, sharing off"))
        print(f"  parent spread (max - min) {spread:.4f} ms; branch median - parent median = {bm - pm:+.4f} ms ({(bm - pm) / pm * 100:+.2f} %)")
        print(f"  gain gate (branch median < parent median - parent spread = {pm - spread:.4f}): {'MET' if bm < pm - spread else 'NOT MET'}")
        print(f"  no-loss check (branch median <= parent median + parent spread = {pm + spread:.4f}): {'ok' if bm <= pm + spread else 'SLOWER'}")
        print(f"  sharing off inside the parent's range [{min(ms['parent']):.4f}, {max(ms['parent']):.4f}]: median {om:.4f} "
              f"{'yes' if min(ms['parent']) <= om <= max(ms['parent']) else 'no'}", flush=True)


SETUP_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import raytracing_engine_amd as R
n = int(sys.argv[2])
mesh = [np.ascontiguousarray(x, np.float32) for x in R.scenes.soup_scene(n, seed=1, edge=0.08 if n <= 1000000 else 0.032)]
torch.cuda.init()
free0, total = torch.cuda.mem_get_info(0)
rs, secs, sharers = [], [], []
for k in range(3):
    r = R.Renderer(0)
    t0 = time.perf_counter()
    r.set_mesh(*mesh)
    secs.append(time.perf_counter() - t0)
    rs.append(r)
torch.cuda.synchronize()
free1, _ = torch.cuda.mem_get_info(0)
sharers = [r.mesh_sharers() for r in rs] if hasattr(rs[0], "mesh_sharers") else None
print(json.dumps({"set_mesh_s": secs, "mesh_bytes_in_use": free0 - free1, "build_ms": rs[0].pt_stats()["bvh_build_ms"], "sharers": sharers}))
for r in rs:
    r.close()
"""


def setup(args):
    print(f"three contexts, soup of {args.n_tris} triangles: seconds per set_mesh, device memory taken by the three meshes", flush=True)
    for name, tree, env in configs(args.parent_tree):
        out, _ = run([sys.executable, "-c", SETUP_CHILD, tree, str(args.n_tris)], env, args.limit, cwd=tree)
        res = json.loads(out.strip().splitlines()[-1])
        print(f"  {name:20s} set_mesh {' '.join('%.3f' % s for s in res['set_mesh_s'])} s  (host BVH build of the first {res['build_ms']:.0f} ms)  "
              f"device memory {res['mesh_bytes_in_use'] / 1e6:.1f} MB  sharers {res['sharers']}", flush=True)


def pmc(args):
    if shutil.which("rocprofv3") is None:
        sys.exit("rocprofv3 not found")
    passes = [["FETCH_SIZE"]] if args.fetch_only else [["TCC_HIT_sum", "TCC_MISS_sum"], ["FETCH_SIZE"], ["WRITE_SIZE"]]
    for lanes in [int(x) for x in args.lanes.split(",")]:
        for name, tree, env in configs(args.parent_tree)[:2] if lanes > 1 else configs(args.parent_tree)[:1]:
            per = {}
            for counters in passes:
                d = tempfile.mkdtemp(prefix="rt_pmc_", dir="/tmp")
                try:
                    run(["rocprofv3", "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", d, "--", sys.executable, os.path.join(tree, "bench.py"),
                         "--workload", args.workload, "--steps", "6", "--warmup", "0", "--frames-in-flight", str(lanes)], dict(env, TMPDIR="/tmp"), args.limit, cwd="/tmp")
                    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                        for row in csv.DictReader(open(f)):
                            for sub, label in KERNELS.items():
                                if sub in row["Kernel_Name"]:
                                    per.setdefault(label, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
                finally:
                    shutil.rmtree(d, ignore_errors=True)
            print(f"{args.workload}, {lanes} lane(s), {name}: per launch (mean over the launches of the run)", flush=True)
            for label, c in sorted(per.items()):
                mean = {k: sum(v) / len(v) for k, v in c.items()}
                line = f"  {label:16s} launches {len(c.get('FETCH_SIZE', []))}"
                if "TCC_HIT_sum" in mean:
                    hit = mean["TCC_HIT_sum"] / max(mean["TCC_HIT_sum"] + mean["TCC_MISS_sum"], 1.0)
                    line += f"  L2 hit rate {hit:.4f}  TCC_HIT {mean['TCC_HIT_sum']:.4g}  TCC_MISS {mean['TCC_MISS_sum']:.4g}"
                line += f"  FETCH_SIZE {mean.get('FETCH_SIZE', 0):.1f} KB raw (x2: {mean.get('FETCH_SIZE', 0) * 2.048e-3:.1f} MB)"
                if "WRITE_SIZE" in mean:
                    line += f"  WRITE_SIZE {mean['WRITE_SIZE'] * 1.024e-3:.1f} MB"
                print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bench", "setup", "pmc"])
    ap.add_argument("--parent-tree", required=True, help="a built checkout of the parent commit (its bench.py and package are run from there)")
    ap.add_argument("--workloads", default="tri1m_1080p_4spp,terrain1m_1080p_4spp")
    ap.add_argument("--workload", default="tri1m_1080p_4spp")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lanes", default="")
    ap.add_argument("--fetch-only", action="store_true", help="pmc: the FETCH_SIZE pass alone")
    ap.add_argument("--n-tris", type=int, default=1000000)
    ap.add_argument("--limit", type=int, default=240, help="seconds one GPU process may take")
    args = ap.parse_args()
    if args.what == "pmc" and not args.lanes:
        args.lanes = "3,1"
    {"bench": bench, "setup": setup, "pmc": pmc}[args.what](args)


if __name__ == "__main__":
    main()
