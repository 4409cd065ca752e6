#!/usr/bin/env python3
"""Cost of the k-nearest queries on device arrays (rt_query_knn_device) on 1 M-triangle scenes, beside the two calls that were there before.

    python tools/knn_query.py [--points 8388608] [--repeats 20] [--warmup 3] [--scenes soup,terrain] [--ks 1,8,64] [--budget-ms 6000] [--out profiles/knn_queries.txt]

Scenes, point distributions (NEAR: within 1e-3 M of the surface; UNIFORM: in the mesh's bounding box) and the median are those of
tools/neighbor_query.py, whose helpers this tool uses.  Per batch and k: query_knn without a radius, default tuning; time =
rt_knn_query_stats.ms (HIP events around the launch), median of --repeats after --warmup; nodes and triangles per point from one more
call with count_traversal = 1, outside the timed ones.  The yardsticks are timed in the same process on the same batch with the same
median: for k = 1, query_points without a radius (the same walk, one answer instead of a row of one); for k = 8 and 64, list_neighbors
(capacity = the total) at the one radius for the whole batch at which the mean list length is about k - found by neighbor_query.py's
bisection over count passes on the first 2^17 points - with its longest list, and its count step alone.  A call so long that its
repeats would take more than --budget-ms of device time is repeated less often, and its line says how often.  There is no bar: the
capability is new; the two yardsticks answer other questions (the nearest only; everything within a guessed radius)."""
import argparse
import ctypes as C
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from neighbor_query import SAMPLE, SCENES, median_ms, radius_for  # noqa: E402
from point_query import distributions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="soup,terrain")
    ap.add_argument("--ks", default="1,8,64")
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
    ks = [int(x) for x in a.ks.split(",")]
    lines = [f"# tools/knn_query.py --points {a.points} --repeats {a.repeats} --warmup {a.warmup} --budget-ms {a.budget_ms:g} --scenes {a.scenes} --ks {a.ks}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# knn ms = rt_knn_query_stats.ms of query_knn(points, k) without a radius, default tuning (HIP events around the launch), median of the repeats;",
             "#   nodes, tris = node records fetched and triangles tested per point (one call with count_traversal = 1, not timed); full = rows that hold k entries",
             "# yardstick, same process, same batch, same median:",
             "#   k = 1:  query_points without a radius (y.ms, y.nodes, y.tris per point); ratio = knn ms / y.ms",
             "#   k > 1:  list_neighbors at ONE radius for the batch (rmax: the mean list length is about k; bisection over count passes on the first 2^17 points),",
             "#           capacity = the total: y.ms = the list call, count ms = its count step alone, nbrs = neighbours per point, most = the longest list,",
             "#           y.nodes, y.tris per WALK (the list call walks twice); ratio = knn ms / y.ms",
             f"# repeats = timed repeats of knn / yardstick behind that line's medians (fewer than --repeats where one entry would have taken more than {a.budget_ms:g} ms of device time)"]

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
        emit(f"{'points':8} {'k':>4} {'knn ms':>9} {'Mpoints/s':>10} {'nodes':>8} {'tris':>8} {'full':>6} | {'yardstick':>14} {'rmax':>9} {'y.ms':>9} {'count ms':>9} {'nbrs':>7} {'most':>5} "
             f"{'y.nodes':>8} {'y.tris':>8} {'ratio':>7} {'repeats':>7}")
        dists = {label: p for label, p in distributions(mesh[0], n, dev)}
        for label in ("near", "uniform"):
            p = dists[label]
            sample = p[:min(n, SAMPLE)].contiguous()
            nearest, _, _ = r.query_points(sample, want_points=False)
            start = max(float(nearest.median()), 1e-6)
            for k in ks:
                dist = torch.empty((n, k), dtype=torch.float32, device=dev)
                tri = torch.empty((n, k), dtype=torch.int32, device=dev)
                counts = torch.empty(n, dtype=torch.int32, device=dev)
                out = (dist, tri, counts)
                r.query_knn(p, k, out=out, count_traversal=True)
                kc = r.knn_query_stats()
                if kc["stack_overflow"] or kc["invalid_points"]:
                    raise SystemExit(f"{name} {label} k {k}: {kc}")
                full = float((counts == k).float().mean())
                knn_ms, _, k1 = median_ms(lambda: r.query_knn(p, k, out=out), r.knn_query_stats, a.warmup, a.repeats, a.budget_ms)
                if k == 1:
                    r.query_points(p, want_points=False, count_traversal=True)
                    pc = r.point_query_stats()
                    pd, pt, _ = r.query_points(p, want_points=False)
                    if not (torch.equal(pd.view(torch.int32), dist[:, 0].view(torch.int32)) and torch.equal(pt, tri[:, 0])):
                        raise SystemExit(f"{name} {label}: k = 1 differs from query_points")
                    y_ms, _, k2 = median_ms(lambda: r.query_points(p, want_points=False, out=(pd, pt)), r.point_query_stats, a.warmup, a.repeats, a.budget_ms)
                    yard = f"{'query_points':>14} {'-':>9} {y_ms:9.3f} {'-':>9} {'-':>7} {'-':>5} {pc['nodes_visited'] / n:8.2f} {pc['tris_tested'] / n:8.2f}"
                    del pd, pt
                else:
                    rmax = radius_for(r, sample, start, k)
                    start = rmax
                    cnt = r.count_neighbors(p, rmax, count_traversal=True)
                    c = r.neighbor_query_stats()
                    most, total = int(cnt.max()), c["neighbors"]
                    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
                    nd, ni = torch.empty(max(total, 1), dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
                    prm = R.NeighborQueryParams()

                    def call(fn, *args):
                        torch.cuda.current_stream(0).synchronize()
                        r._check(fn(r._ctx, ptr(p), None, rmax, n, C.byref(prm), *args))

                    count_ms, _, _ = median_ms(lambda: call(lib.rt_count_neighbors_device, ptr(cnt), ptr(offsets)), r.neighbor_query_stats, a.warmup, a.repeats, a.budget_ms)
                    y_ms, ls, k2 = median_ms(lambda: call(lib.rt_list_neighbors_device, ptr(cnt), ptr(offsets), total, ptr(nd), ptr(ni)), r.neighbor_query_stats,
                                             a.warmup, a.repeats, a.budget_ms)
                    if ls["stack_overflow"] or ls["slice_overflow"] or ls["incomplete_points"] or ls["neighbors_written"] != total:
                        raise SystemExit(f"{name} {label} k {k}: {ls}")
                    # the two calls agree where they must: a point's row is the head of its list
                    head = torch.minimum(cnt, torch.full_like(cnt, k))
                    rows = torch.nonzero(head > 0)[:65536, 0]
                    if not (torch.equal(nd[offsets[rows]].view(torch.int32), dist[rows, 0].view(torch.int32)) and torch.equal(ni[offsets[rows]], tri[rows, 0])):
                        raise SystemExit(f"{name} {label} k {k}: the first list entry differs from the row's")
                    yard = (f"{'list_neighbors':>14} {rmax:9.4g} {y_ms:9.3f} {count_ms:9.3f} {total / n:7.3f} {most:5d} {c['nodes_visited'] / n:8.2f} {c['tris_tested'] / n:8.2f}")
                    del nd, ni, offsets, cnt
                emit(f"{label:8} {k:4d} {knn_ms:9.3f} {n / knn_ms * 1e-3:10.1f} {kc['nodes_visited'] / n:8.2f} {kc['tris_tested'] / n:8.2f} {full:6.3f} | {yard} {knn_ms / y_ms:7.2f} {f'{k1}/{k2}':>7}")
                del dist, tri, counts, out
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
