#!/usr/bin/env python3
"""Cost of the inside/outside queries on device arrays (rt_query_sides_device) on 1 M-triangle scenes.

    python tools/side_query.py [--points 8388608] [--repeats 20] [--warmup 3] [--scenes planet,soup] [--out profiles/side_queries.txt]

Scenes: the 1 M-triangle planet (closed: the answers mean inside / outside) and the 1 M-triangle soup (open: for cost only), both of
raytracing_engine_amd/scenes.py.  Point distributions per scene, made on the device from fixed seeds as tools/point_query.py makes
them: UNIFORM in the mesh's bounding box; NEAR, within 1e-3 M of the surface; FAR, on cubes of half-width 8 .. 32 M about the origin
of the coordinates.

Time = rt_side_query_stats.ms (HIP events around the launch of pt_query_sides), median of --repeats after --warmup, with
tune_refill_min swept over 8, 24 and 48 (24 is the default).  Walks per point and nodes and triangles per walk come from one more run
with count_traversal = 1, outside the timed ones.  Two yardsticks are timed in the same process on the same batch, default tuning,
the same median: query_points (rt_point_query_stats.ms) and a closest-hit query_rays of the same points along D[0]
(rt_ray_query_stats.ms) - the walk that a crossing walk would be if a hit could shrink its tmax.  There is no bar: the capability is
new, and how much more a crossing walk costs than a closest-hit ray is the finding."""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from point_query import distributions  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

D0 = (0.6350, 0.5127, 0.5779)  # kParityDir[0] of csrc/ray_parity.h
SCENES = {"planet": ("planet 1M", lambda: scenes.planet_scene(1_000_000, seed=1)), "soup": ("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08))}


def median_ms(run, stats, warmup, repeats):
    ms = []
    for k in range(warmup + repeats):
        run()
        st = stats()
        if k >= warmup:
            ms.append(st["ms"])
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="planet,soup")
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
    lines = [f"# tools/side_query.py --points {a.points} --repeats {a.repeats} --warmup {a.warmup} --scenes {a.scenes}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# ms = rt_side_query_stats.ms (HIP events around the launch of pt_query_sides), median of the repeats; Mpoints/s = points / that",
             "# walks = ray walks per point (2 + the share of points that needed the third); nodes, tris = node records fetched and triangles tested per WALK",
             "#   (one run with count_traversal = 1, not timed); inside = share of the points answered 1",
             "# points ms / ray ms = query_points and a closest-hit query_rays along D[0] on the same batch, default tuning, same median: the two yardsticks"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    for key in a.scenes.split(","):
        name, make = SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        emit(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {a.points} points per batch")
        emit(f"{'points':8} {'refill_min':>10} {'ms':>9} {'min':>9} {'max':>9} {'Mpoints/s':>10} {'walks':>7} {'nodes':>8} {'tris':>8} {'inside':>7} {'points ms':>10} {'ray ms':>9}")
        for label, p in distributions(mesh[0], a.points, dev):
            inside = r.query_sides(p, count_traversal=True)
            c = r.side_query_stats()
            if c["stack_overflow"] or c["invalid_points"]:
                raise SystemExit(f"{name} {label}: {c}")
            share = float((inside == 1).float().mean())
            dirs = torch.tensor(D0, dtype=torch.float32, device=dev).repeat(a.points, 1).contiguous()
            pts_ms = median_ms(lambda: r.query_points(p, want_points=False), r.point_query_stats, a.warmup, a.repeats)
            ray_ms = median_ms(lambda: r.query_rays(p, dirs), r.ray_query_stats, a.warmup, a.repeats)
            del dirs
            for refill in (8, 24, 48):
                ms = []
                for k in range(a.warmup + a.repeats):
                    got = r.query_sides(p, tune_refill_min=refill)
                    st = r.side_query_stats()
                    if k >= a.warmup:
                        ms.append(st["ms"])
                med, lo, hi = statistics.median(ms), min(ms), max(ms)
                if st["stack_overflow"] or st["invalid_points"]:
                    raise SystemExit(f"{name} {label}: {st}")
                if not torch.equal(got, inside):
                    raise SystemExit(f"{name} {label} refill_min {refill}: answers differ from the counted run's")
                emit(f"{label:8} {refill:10d} {med:9.3f} {lo:9.3f} {hi:9.3f} {a.points / med * 1e-3:10.1f} {c['walks'] / a.points:7.3f} "
                     f"{c['nodes_visited'] / c['walks']:8.2f} {c['tris_tested'] / c['walks']:8.2f} {share:7.3f} {pts_ms:10.3f} {ray_ms:9.3f}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
