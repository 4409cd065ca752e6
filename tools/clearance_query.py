#!/usr/bin/env python3
"""Rate of the clearance queries on device arrays (rt_query_clearance_device) on 1 M-triangle scenes.

    python tools/clearance_query.py [--queries 1048576] [--repeats 10] [--warmup 2] [--out profiles/clearance_queries.txt]

Scenes: the 1 M-triangle soup and the 1 M-triangle terrain (raytracing_engine_amd/scenes.py).  Query triangles per scene, made on the
device from a fixed seed: uniformly chosen mesh triangles displaced by 0.05, 1 and 5 of their size (the longest edge) in a random
direction - touching or cutting the surface, a triangle's width off it, and well clear of it.

Time = rt_clearance_query_stats.ms (HIP events around the launch of pt_query_clearance), median of --repeats after --warmup, with
tune_refill_min swept over 8, 24 and 48 (24 is the default).  Nodes and records per query come from one more run with
count_traversal = 1, outside the timed ones.  THE YARDSTICK is what a caller could do before: three rt_query_points_device batches on
the vertices (an upper bound on the clearance, not the clearance), timed the same way as one batch of 3 n points; the share of the
queries whose vertex bound lies above the clearance is printed beside it.  There is no bar: the capability is new."""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from point_query import scene_list  # noqa: E402


def displaced(verts, n, share, dev, seed):
    """(n, 9) float32 device tensor: uniformly chosen mesh triangles moved by share x their longest edge in a random direction."""
    import numpy as np
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev).reshape(-1, 3, 3)
    t = v[torch.randint(0, len(v), (n,), generator=g, device=dev)]
    size = torch.stack([(t[:, 1] - t[:, 0]).norm(dim=1), (t[:, 2] - t[:, 1]).norm(dim=1), (t[:, 0] - t[:, 2]).norm(dim=1)]).max(0).values
    d = torch.randn(n, 3, generator=g, device=dev, dtype=torch.float32)
    d = d / d.norm(dim=1, keepdim=True)
    return (t + (d * (share * size)[:, None])[:, None, :]).reshape(n, 9).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    lines = [f"# tools/clearance_query.py --queries {a.queries} --repeats {a.repeats} --warmup {a.warmup}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# ms = rt_clearance_query_stats.ms (HIP events around the launch of pt_query_clearance), median of the repeats; Mqueries/s = queries / that",
             "# nodes, records = node records and triangle records fetched per query (one run with count_traversal = 1, not timed)",
             "# 'vertices' = the yardstick: rt_query_points_device on the 3 n vertices (an upper bound only), refill_min 24; above = share of the queries it overestimates"]
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    for name, make in scene_list():
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        lines.append(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {a.queries} query triangles per batch")
        lines.append(f"{'moved by':9} {'refill_min':>10} {'ms':>9} {'min':>9} {'max':>9} {'Mqueries/s':>10} {'nodes':>8} {'records':>8} {'above':>7}")
        for k, share in enumerate((0.05, 1.0, 5.0)):
            q = displaced(mesh[0], a.queries, share, dev, 21 + k)
            r.query_clearance(q, want_points=False, count_traversal=True)
            c = r.clearance_query_stats()
            ref = None
            for refill in (8, 24, 48):
                ms = []
                for i in range(a.warmup + a.repeats):
                    dist, tri = r.query_clearance(q, want_points=False, tune_refill_min=refill)[:2]
                    st = r.clearance_query_stats()
                    if i >= a.warmup:
                        ms.append(st["ms"])
                if st["stack_overflow"] or st["invalid_triangles"]:
                    raise SystemExit(f"{name} {share}: {st}")
                if ref is None:
                    ref = tri.clone()
                elif not torch.equal(ref, tri):
                    raise SystemExit(f"{name} {share} refill_min {refill}: answers differ from the first setting's")
                med = statistics.median(ms)
                lines.append(f"{share:<9g} {refill:>10} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} {a.queries / med * 1e-3:10.2f} "
                             f"{c['nodes_visited'] / a.queries:8.2f} {c['tris_tested'] / a.queries:8.2f}")
                print(lines[-1], flush=True)
            points = q.view(-1, 3)
            ms = []
            for i in range(a.warmup + a.repeats):
                by_vertex = r.query_points(points, want_points=False)[0]
                if i >= a.warmup:
                    ms.append(r.point_query_stats()["ms"])
            above = float((by_vertex.view(-1, 3).min(1).values > dist * (1 + 1e-5)).float().mean())
            med = statistics.median(ms)
            lines.append(f"{share:<9g} {'vertices':>10} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} {a.queries / med * 1e-3:10.2f} {'':8} {'':8} {above:7.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
