#!/usr/bin/env python3
"""Cost of the neighbour queries on device arrays (rt_count / rt_fill / rt_list_neighbors_device) on 1 M-triangle scenes.

    python tools/neighbor_query.py [--points 8388608] [--repeats 20] [--warmup 3] [--scenes soup,terrain] [--budget-ms 6000] [--out profiles/neighbor_queries.txt]

Scenes: the 1 M-triangle soup and the 1 M-triangle terrain of raytracing_engine_amd/scenes.py.  Point distributions per scene, made as
tools/point_query.py makes them: NEAR, within 1e-3 M of the surface, and UNIFORM in the mesh's bounding box.  One radius for all points
of a batch, three per batch: the radii at which the mean list length is about 1, 8 and 64, found by bisection over count passes on the
first 2^17 points of the batch (nothing is chosen by hand; the line says what the whole batch then gives).

Time = rt_neighbor_query_stats.ms (HIP events from the first to the last launch of the call), median of --repeats after --warmup, for
the three entries - count (the walk and the scan into offsets), fill (the walk that writes the sorted lists, on the count step's
offsets) and list (both, capacity = the total) - with tune_refill_min swept over 8, 24 and 48 (24 is the default).  An entry so long
that its repeats would take more than --budget-ms of device time is repeated less often, and its line says how often.  Neighbours per point
(mean and longest) and nodes and triangles per walk come from one more count with count_traversal = 1, outside the timed ones.  The
yardstick, timed in the same process on the same batch with the same radius, default tuning and the same median: query_points
(rt_point_query_stats.ms), the walk that keeps the nearest only and shrinks its bound as it goes.  There is no bar: the capability is new."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from point_query import distributions  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

SCENES = {"soup": ("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08)), "terrain": ("terrain 1M", lambda: scenes.terrain_scene(708, seed=1))}
TARGETS = (1, 8, 64)
SAMPLE = 1 << 17


def median_ms(run, stats, warmup, repeats, budget_ms=float("inf")):
    """(median ms, the last statistics, timed repeats).  A call whose first run says that warmup + repeats of it would take more than
    budget_ms is timed max(3, budget_ms / that) times after that one warm-up; the line that reports it says how often."""
    run()
    st = stats()
    if st["ms"] * (warmup + repeats) > budget_ms:
        warmup, repeats = 1, min(repeats, max(3, int(budget_ms / st["ms"])))
    ms = []
    for k in range(1, warmup + repeats):
        run()
        st = stats()
        if k >= warmup:
            ms.append(st["ms"])
    return statistics.median(ms), st, len(ms)


def radius_for(r, sample, start, target):
    """The radius at which the mean number of neighbours of `sample` is about `target`: grow from `start` until it is reached, then
    bisect (geometrically) between the last two."""
    def mean(radius):
        r.count_neighbors(sample, radius)
        return r.neighbor_query_stats()["neighbors"] / len(sample)

    lo, hi = 0.0, start
    while mean(hi) < target:
        lo, hi = hi, hi * 1.5
    lo = lo or hi / 64.0
    for _ in range(12):
        mid = (lo * hi) ** 0.5
        if mean(mid) < target:
            lo = mid
        else:
            hi = mid
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="soup,terrain")
    ap.add_argument("--budget-ms", type=float, default=6000.0, help="device time one timed entry of one line may take; longer ones get fewer repeats (the line says how many)")
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
    lines = [f"# tools/neighbor_query.py --points {a.points} --repeats {a.repeats} --warmup {a.warmup} --budget-ms {a.budget_ms:g} --scenes {a.scenes}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# count / fill / list ms = rt_neighbor_query_stats.ms (HIP events from the first to the last launch of the call), median of the repeats:",
             "#   count = walk + scan into offsets, fill = the walk that writes the sorted lists on those offsets, list = both in one call (capacity = the total)",
             "# rmax = one radius for the whole batch, found by bisection over count passes on its first 2^17 points for a mean list length of 1, 8, 64",
             "# nbrs = neighbours per point (most: the longest list); nodes, tris = node records fetched and triangles tested per WALK (one count with count_traversal = 1, not timed)",
             f"# repeats = timed repeats of count / fill / list behind that line's medians (fewer than --repeats where one entry would have taken more than {a.budget_ms:g} ms of device time)",
             "# point ms = query_points on the same batch with the same rmax, default tuning, same median (its nodes and triangles per point behind it)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    lib = R.load()
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    n = a.points
    for key in a.scenes.split(","):
        name, make = SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        emit(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {n} points per batch")
        emit(f"{'points':8} {'rmax':>10} {'refill_min':>10} {'count ms':>9} {'fill ms':>9} {'list ms':>9} {'Mpoints/s list':>14} {'nbrs':>7} {'most':>5} {'nodes':>8} {'tris':>8} "
             f"{'point ms':>9} {'p.nodes':>8} {'p.tris':>8} {'repeats':>9}")
        dists = {label: p for label, p in distributions(mesh[0], n, dev)}
        for label in ("near", "uniform"):
            p = dists[label]
            sample = p[:min(n, SAMPLE)].contiguous()
            nearest, _, _ = r.query_points(sample, want_points=False)
            start = max(float(nearest.median()), 1e-6)
            for target in TARGETS:
                rmax = radius_for(r, sample, start, target)
                start = rmax
                counts = r.count_neighbors(p, rmax, count_traversal=True)
                c = r.neighbor_query_stats()
                if c["stack_overflow"] or c["invalid_points"]:
                    raise SystemExit(f"{name} {label}: {c}")
                most, total = int(counts.max()), c["neighbors"]
                offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
                nd, ni = torch.empty(max(total, 1), dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
                rt = torch.full((n,), rmax, dtype=torch.float32, device=dev)
                r.query_points(p, rt, want_points=False, count_traversal=True)
                pc = r.point_query_stats()
                point_ms, _, _ = median_ms(lambda: r.query_points(p, rt, want_points=False), r.point_query_stats, a.warmup, a.repeats)
                first = None
                for refill in (8, 24, 48):
                    prm = R.NeighborQueryParams(tune_refill_min=refill)

                    def call(fn, *args):
                        torch.cuda.current_stream(0).synchronize()
                        r._check(fn(r._ctx, ptr(p), None, rmax, n, C.byref(prm), *args))

                    count_ms, _, k1 = median_ms(lambda: call(lib.rt_count_neighbors_device, ptr(counts), ptr(offsets)), r.neighbor_query_stats, a.warmup, a.repeats, a.budget_ms)
                    fill_ms, fs, k2 = median_ms(lambda: call(lib.rt_fill_neighbors_device, ptr(offsets), total, ptr(nd), ptr(ni)), r.neighbor_query_stats, a.warmup, a.repeats, a.budget_ms)
                    list_ms, ls, k3 = median_ms(lambda: call(lib.rt_list_neighbors_device, ptr(counts), ptr(offsets), total, ptr(nd), ptr(ni)), r.neighbor_query_stats,
                                                a.warmup, a.repeats, a.budget_ms)
                    for s in (fs, ls):
                        if s["stack_overflow"] or s["slice_overflow"] or s["incomplete_points"] or s["neighbors_written"] != total or s["neighbors"] != total:
                            raise SystemExit(f"{name} {label} refill_min {refill}: {s}")
                    if int(offsets[n]) != total:
                        raise SystemExit(f"{name} {label}: offsets[n] {int(offsets[n])} != neighbours {total}")
                    got = (nd[:total].clone(), ni[:total].clone())
                    if first is None:
                        first = got
                    elif not (torch.equal(got[0].view(torch.int32), first[0].view(torch.int32)) and torch.equal(got[1], first[1])):
                        raise SystemExit(f"{name} {label} refill_min {refill}: the lists differ from refill_min 8's")
                    emit(f"{label:8} {rmax:10.4g} {refill:10d} {count_ms:9.3f} {fill_ms:9.3f} {list_ms:9.3f} {n / list_ms * 1e-3:14.1f} {total / n:7.3f} {most:5d} "
                         f"{c['nodes_visited'] / n:8.2f} {c['tris_tested'] / n:8.2f} {point_ms:9.3f} {pc['nodes_visited'] / n:8.2f} {pc['tris_tested'] / n:8.2f} {f'{k1}/{k2}/{k3}':>9}")
                del first, got, nd, ni, offsets, rt, counts
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
