#!/usr/bin/env python3
"""Cost of the overlap queries on device arrays (rt_count / rt_fill / rt_list_overlaps_device) on 1 M-triangle scenes.

    python tools/overlap_query.py [--tris 1048576] [--repeats 10] [--warmup 2] [--scenes soup,terrain] [--budget-ms 4000] [--out profiles/overlap_queries.txt]

Scenes: the 1 M-triangle soup and the 1 M-triangle terrain of raytracing_engine_amd/scenes.py.  Query triangles: mesh triangles drawn
at random (fixed seed), each displaced as a whole in a random direction by a fraction of its size (its longest edge).  The fraction
is found, not chosen: the mean list length of the first 2^17 queries is scanned over fractions 2^-8 .. 2^4 and bisected (geometrically)
inside the first bracket of the target, for targets of about 1 and 8 overlaps per query.  A copy of a mesh triangle cuts only so many
of its neighbours however it is displaced (for small displacements only the direction matters), so where no fraction reaches a target
the one that comes closest is kept and the query triangles are GROWN about their centroids instead, by a factor found the same way
over 2^0 .. 2^7; the line names both and says what the whole batch then gives.

Time = rt_overlap_query_stats.ms (HIP events from the first to the last launch of the call), median of --repeats after --warmup, for the
three entries - count (the walk and the scan into offsets), fill (the walk that writes the sorted lists, on the count step's offsets)
and list (both, capacity = the total).  Overlaps per query (mean and longest) and nodes and records per walk come from one more count
with count_traversal = 1, outside the timed ones.  The yardstick is what a caller has without these entries: three list_ray_hits
batches per query triangle, one per edge (origin, direction, tmax = 1; capacity = that batch's total), rt_hit_query_stats.ms of the
three added, same median.  It gives bits 0-2 only - the mesh's edges through the query triangle are missing - and each of its walks
follows the whole ray, since a segment's limit may not prune.  There is no bar: the capability is new."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

SCENES = {"soup": ("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08)), "terrain": ("terrain 1M", lambda: scenes.terrain_scene(708, seed=1))}
TARGETS = (1, 8)
SAMPLE = 1 << 17


def median_ms(run, warmup, repeats, budget_ms=float("inf")):
    """(median of run()'s ms, timed repeats); fewer repeats where warmup + repeats would take more than budget_ms of device time."""
    first = run()
    if first * (warmup + repeats) > budget_ms:
        warmup, repeats = 1, min(repeats, max(3, int(budget_ms / first)))
    ms = [run() for _ in range(1, warmup + repeats)][warmup - 1:]
    return statistics.median(ms), len(ms)


def knob_for(mean, target, exponents):
    """The knob setting (a displacement in triangle sizes, or a growth factor) at which mean(setting) is about target: (setting, True), or
    the closest of the scan over 2^exponents and False.  The scan stops at the first bracket: settings beyond it (long lists) are not walked."""
    grid = [2.0 ** k for k in exponents]
    got = [mean(grid[0])]
    for k in range(len(grid) - 1):
        got.append(mean(grid[k + 1]))
        if (got[k] - target) * (got[k + 1] - target) <= 0 and got[k] != got[k + 1]:
            lo, hi, rising = grid[k], grid[k + 1], got[k] < got[k + 1]
            for _ in range(8):
                mid = (lo * hi) ** 0.5
                if (mean(mid) < target) == rising:
                    lo = mid
                else:
                    hi = mid
            return (lo * hi) ** 0.5, True
    k = min(range(len(grid)), key=lambda i: abs(got[i] - target))
    return grid[k], False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="soup,terrain")
    ap.add_argument("--budget-ms", type=float, default=4000.0, help="device time one timed entry of one line may take; longer ones get fewer repeats (the line says how many)")
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
    lines = [f"# tools/overlap_query.py --tris {a.tris} --repeats {a.repeats} --warmup {a.warmup} --budget-ms {a.budget_ms:g} --scenes {a.scenes}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# count / fill / list ms = rt_overlap_query_stats.ms (HIP events from the first to the last launch of the call), median of the repeats:",
             "#   count = walk + scan into offsets, fill = the walk that writes the sorted lists on those offsets, list = both in one call (capacity = the total)",
             "# shift = the displacement of every query triangle in units of its longest edge, grow = its magnification about its centroid (1 where a shift alone reaches the target),",
             "#   both found on the first 2^17 queries for a mean list of about 1 and 8 (found = no: neither reaches it, the closest)",
             "# ovl = overlaps per query (most: the longest list); nodes, recs = node records and triangle records fetched per WALK (one count with count_traversal = 1, not timed)",
             "# emul ms = three list_ray_hits batches (one per edge of the query triangles, tmax = 1, capacity = the batch's total), rt_hit_query_stats.ms added; e.hits = their hits per query",
             "#   triangle (bits 0-2 only: the emulation does not see the mesh's edges through the query triangle); ratio = emul ms / list ms",
             "# repeats = timed repeats of count / fill / list / emulation behind that line's medians"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    lib = R.load()
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    n = a.tris
    for key in a.scenes.split(","):
        name, make = SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        emit(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {n} query triangles per batch")
        emit(f"{'target':>6} {'shift':>9} {'grow':>7} {'found':>5}{'count ms':>9} {'fill ms':>9} {'list ms':>9} {'Mtris/s list':>12} {'ovl':>7} {'most':>5} {'nodes':>8} {'recs':>8} "
             f"{'emul ms':>9} {'e.hits':>7} {'ratio':>6} {'repeats':>11}")
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        verts = torch.from_numpy(mesh[0]).to(dev).view(-1, 3, 3)
        base = verts[torch.randint(0, len(verts), (n,), generator=gen, device=dev)]
        size = torch.stack([(base[:, 1] - base[:, 0]).norm(dim=1), (base[:, 2] - base[:, 1]).norm(dim=1), (base[:, 0] - base[:, 2]).norm(dim=1)]).max(0).values
        way = torch.randn(n, 3, generator=gen, device=dev)
        way = way / way.norm(dim=1, keepdim=True)
        del verts

        centre = base.mean(dim=1, keepdim=True)

        def queries(shift, grow, count=n):
            grown = centre[:count] + (base[:count] - centre[:count]) * grow
            return (grown + (way[:count] * (shift * size[:count])[:, None])[:, None, :]).contiguous().view(count, 9)

        def mean(shift, grow):
            r.count_overlaps(queries(shift, grow, min(n, SAMPLE)))
            return r.overlap_query_stats()["overlaps"] / min(n, SAMPLE)

        for target in TARGETS:
            grow = 1.0
            shift, found = knob_for(lambda s: mean(s, 1.0), target, range(-8, 5))
            if not found:
                grow, found = knob_for(lambda g: mean(shift, g), target, range(0, 8))
            q = queries(shift, grow)
            counts = r.count_overlaps(q, count_traversal=True)
            c = r.overlap_query_stats()
            if c["stack_overflow"] or c["invalid_triangles"]:
                raise SystemExit(f"{name}: {c}")
            most, total = int(counts.max()), c["overlaps"]
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
            tri, edges = torch.empty(max(total, 1), dtype=torch.int32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            prm = R.OverlapQueryParams()

            def call(fn, *args):
                torch.cuda.current_stream(0).synchronize()
                r._check(fn(r._ctx, ptr(q), n, C.byref(prm), *args))
                return r.overlap_query_stats()

            count_ms, k1 = median_ms(lambda: call(lib.rt_count_overlaps_device, ptr(counts), ptr(offsets))["ms"], a.warmup, a.repeats, a.budget_ms)
            fill_ms, k2 = median_ms(lambda: call(lib.rt_fill_overlaps_device, ptr(offsets), total, ptr(tri), ptr(edges))["ms"], a.warmup, a.repeats, a.budget_ms)
            list_ms, k3 = median_ms(lambda: call(lib.rt_list_overlaps_device, ptr(counts), ptr(offsets), total, ptr(tri), ptr(edges))["ms"], a.warmup, a.repeats, a.budget_ms)
            s = r.overlap_query_stats()
            if s["stack_overflow"] or s["slice_overflow"] or s["incomplete_triangles"] or s["overlaps_written"] != total or s["overlaps"] != total or int(offsets[n]) != total:
                raise SystemExit(f"{name}: {s}")
            # the emulation: one list_ray_hits batch per edge
            t3 = q.view(n, 3, 3)
            rays = [(t3[:, k].contiguous(), (t3[:, (k + 1) % 3] - t3[:, k]).contiguous()) for k in range(3)]
            one = torch.ones(n, dtype=torch.float32, device=dev)
            caps, hits = [], 0
            for o, d in rays:
                r.count_ray_hits(o, d, one)
                caps.append(r.hit_query_stats()["hits"])
                hits += caps[-1]
            outs = [(torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(max(cap, 1), dtype=torch.float32, device=dev)[:cap],
                     torch.empty(max(cap, 1), dtype=torch.int32, device=dev)[:cap], torch.empty(n, dtype=torch.int32, device=dev)) for cap in caps]

            def emulate():
                ms = 0.0
                for (o, d), cap, out in zip(rays, caps, outs):
                    r.list_ray_hits(o, d, one, capacity=cap, out=out)
                    ms += r.hit_query_stats()["ms"]
                return ms

            emul_ms, k4 = median_ms(emulate, a.warmup, a.repeats, a.budget_ms)
            emit(f"{target:6d} {shift:9.4g} {grow:7.3g} {'yes' if found else 'no':>5}{count_ms:9.3f} {fill_ms:9.3f} {list_ms:9.3f} {n / list_ms * 1e-3:12.1f} {total / n:7.3f} {most:5d} "
                 f"{c['nodes_visited'] / n:8.2f} {c['tris_tested'] / n:8.2f} {emul_ms:9.3f} {hits / n:7.3f} {emul_ms / list_ms:6.2f} {f'{k1}/{k2}/{k3}/{k4}':>11}")
            del q, counts, offsets, tri, edges, rays, outs, one
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
