#!/usr/bin/env python3
"""Rate of the closest-point queries on device arrays (rt_query_points_device) on 1 M-triangle scenes.

    python tools/point_query.py [--points 8388608] [--repeats 20] [--warmup 3] [--attributes] [--out profiles/point_queries.txt]

Scenes: the 1 M-triangle soup and the 1 M-triangle terrain (raytracing_engine_amd/scenes.py).  Point distributions per scene, made
on the device from fixed seeds: UNIFORM in the mesh's bounding box; NEAR, within 1e-3 M of the surface (a uniform point of a uniformly
chosen triangle plus a uniform offset of that size; M = the largest |coordinate|); FAR, on cubes of half-width 8 .. 32 M about the
origin of the coordinates (log-uniform), where the first boxes of the walk all look alike.

Time = rt_point_query_stats.ms (HIP events around the launch of pt_query_points), median of --repeats after --warmup, with
tune_refill_min swept over 8, 24 and 48 (24 is the default).  Nodes and triangles per query come from one more run with
count_traversal = 1, outside the timed ones.  There is no bar and no parent to compare with: the capability is new.
--attributes: every batch once more through rt_query_points_attr_device (barycentrics and normals) at
refill_min 24, in the same process under the same protocol; its tri must be the plain query's."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402


def scene_list():
    return [("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08)), ("terrain 1M", lambda: scenes.terrain_scene(708, seed=1))]


def distributions(verts, n, dev):
    """[(label, (n, 3) float32 device tensor)]"""
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(11)
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev).reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(0).values, v.reshape(-1, 3).max(0).values
    M = max(1.0, float(v.abs().max()))
    rand = lambda *shape: torch.rand(*shape, generator=g, device=dev, dtype=torch.float32)  # noqa: E731
    uniform = lo + (hi - lo) * rand(n, 3)
    tri = torch.randint(0, len(v), (n,), generator=g, device=dev)
    a, b = rand(n), rand(n)
    flip = a + b > 1
    a, b = torch.where(flip, 1 - a, a), torch.where(flip, 1 - b, b)
    t = v[tri]
    near = t[:, 0] + (t[:, 1] - t[:, 0]) * a[:, None] + (t[:, 2] - t[:, 0]) * b[:, None] + (rand(n, 3) * 2 - 1) * (1e-3 * M)
    cube = rand(n, 3) * 2 - 1
    cube = cube / cube.abs().max(1, keepdim=True).values
    far = cube * (M * 8.0 * torch.exp(rand(n, 1) * float(np.log(4.0 * (1 - 2.0 ** -20)))))
    return [("uniform", uniform.contiguous()), ("near", near.contiguous()), ("far", far.contiguous())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--attributes", action="store_true", help="every batch with barycentrics and normals too")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="what to name as the commit (default: git rev-parse of this checkout)")
    a = ap.parse_args()
    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        if a.commit:
            raise OSError
        commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        if subprocess.run(["git", "-C", root, "status", "--porcelain", "-uno"], capture_output=True, text=True).stdout.strip():
            commit += " + uncommitted changes"
    except (OSError, subprocess.CalledProcessError):
        commit = a.commit or "unknown (not a git checkout)"
    lines = [f"# tools/point_query.py --points {a.points} --repeats {a.repeats} --warmup {a.warmup}{' --attributes' if a.attributes else ''}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# ms = rt_point_query_stats.ms (HIP events around the launch of pt_query_points), median of the repeats; Mpoints/s = points / that",
             "# nodes, tris = node records fetched and triangles tested per query (one run with count_traversal = 1, not timed)"]
    if a.attributes:
        lines.append("# '24 + attr' = the same batch through rt_query_points_attr_device (barycentrics and normals, DESIGN.md section 6.18), refill_min 24")
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    for name, make in scene_list():
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        lines.append(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {a.points} points per batch")
        lines.append(f"{'points':8} {'refill_min':>10} {'ms':>9} {'min':>9} {'max':>9} {'Mpoints/s':>10} {'nodes':>8} {'tris':>8}")
        for label, p in distributions(mesh[0], a.points, dev):
            r.query_points(p, want_points=False, count_traversal=True)
            c = r.point_query_stats()
            ref = None
            for refill, attr in [(v, False) for v in (8, 24, 48)] + ([(24, True)] if a.attributes else []):
                ms = []
                for k in range(a.warmup + a.repeats):
                    dist, tri = r.query_points(p, want_points=False, tune_refill_min=refill, attributes=attr)[:2]
                    st = r.point_query_stats()
                    if k >= a.warmup:
                        ms.append(st["ms"])
                if st["stack_overflow"] or st["invalid_points"]:
                    raise SystemExit(f"{name} {label}: {st}")
                if ref is None:
                    ref = tri.clone()
                elif not torch.equal(ref, tri):
                    raise SystemExit(f"{name} {label} refill_min {refill}: answers differ from the first setting's")
                med = statistics.median(ms)
                lines.append(f"{label:8} {str(refill) + (' + attr' if attr else ''):>10} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} {a.points / med * 1e-3:10.1f} "
                             f"{c['nodes_visited'] / a.points:8.2f} {c['tris_tested'] / a.points:8.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
