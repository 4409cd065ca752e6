#!/usr/bin/env python3
"""Cost of the all-hits ray queries on device arrays (rt_count / rt_fill / rt_list_ray_hits_device) on 1 M-triangle scenes.

    python tools/hit_query.py [--rays 8388608] [--repeats 20] [--warmup 3] [--scenes planet,soup] [--out profiles/hit_queries.txt]

Scenes: the 1 M-triangle planet and the 1 M-triangle soup of raytracing_engine_amd/scenes.py.  Batches per scene, made as
tools/ray_query.py makes them: a COHERENT one, the fan of a pinhole camera that looks at the scene, and an INCOHERENT one,
cosine-distributed directions from the surface points the fan hits.  No limits: every ray is walked to the end of the scene.

Time = rt_hit_query_stats.ms (HIP events from the first to the last launch of the call), median of --repeats after --warmup, for the
three entries - count (the walk and the scan into offsets), fill (the walk that writes the sorted lists, on the count step's offsets)
and list (both, capacity = the total) - with tune_refill_min swept over 8, 24 and 48 (24 is the default).  Hits per ray and nodes and
triangles per walk come from one more count with count_traversal = 1, outside the timed ones.  Yardsticks, timed in the same process
on the same batch with default tuning and the same median: a closest-hit query_rays of the same rays (rt_ray_query_stats.ms); and, for
rays along D[0] from the same origins, the count step against the per-walk cost of query_sides(want_crossings=True)
(rt_side_query_stats.ms / 3): the same walk, so the two should be close.  There is no bar: the capability is new."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from ray_query import cosine_from_hits, fan  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

D0 = (0.6350, 0.5127, 0.5779)  # kParityDir[0] of csrc/ray_parity.h
# name, mesh, the fan's (yaw, pitch) and position: the planet (centre (0, 20, 0), radius 10) from (0, 5, 0), the soup from its middle
SCENES = {"planet": ("planet 1M", lambda: scenes.planet_scene(1_000_000, seed=1), (0.0, 0.0), (0, 5, 0)),
          "soup": ("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08), (0.0, 0.0), (0, 0, 0))}


def median_ms(run, stats, warmup, repeats):
    ms = []
    for k in range(warmup + repeats):
        run()
        st = stats()
        if k >= warmup:
            ms.append(st["ms"])
    return statistics.median(ms), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 23)
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
    lines = [f"# tools/hit_query.py --rays {a.rays} --repeats {a.repeats} --warmup {a.warmup} --scenes {a.scenes}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# count / fill / list ms = rt_hit_query_stats.ms (HIP events from the first to the last launch of the call), median of the repeats:",
             "#   count = walk + scan into offsets, fill = the walk that writes the sorted lists on those offsets, list = both in one call (capacity = the total)",
             "# hits = hits per ray (most: the longest list); nodes, tris = node records fetched and triangles tested per WALK (one count with count_traversal = 1, not timed)",
             "# ray ms = a closest-hit query_rays on the same batch, default tuning, same median",
             "# the D[0] lines: rays along D[0] from the batch's origins - count ms of the count step (counts only, no scan) against side/3 ms =",
             "#   rt_side_query_stats.ms / 3 of query_sides(want_crossings=True) on those origins: three of the same walks per point"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    lib = R.load()
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    n = a.rays
    for key in a.scenes.split(","):
        name, make, yaw_pitch, pos = SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        emit(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {n} rays per batch")
        emit(f"{'rays':10} {'refill_min':>10} {'count ms':>9} {'fill ms':>9} {'list ms':>9} {'Mrays/s list':>12} {'hits':>7} {'most':>5} {'nodes':>8} {'tris':>8} {'ray ms':>9}")
        o, d = fan(n, yaw_pitch, pos)
        t, tri = r.trace_rays(o, d)
        oi, di = cosine_from_hits(np.asarray(mesh[0], np.float32), o, d, t, tri, n, seed=7)
        for label, bo, bd in (("coherent", o, d), ("incoherent", oi, di)):
            to, td = torch.from_numpy(bo).to(dev), torch.from_numpy(bd).to(dev)
            counts = r.count_ray_hits(to, td, count_traversal=True)
            c = r.hit_query_stats()
            if c["stack_overflow"] or c["invalid_rays"]:
                raise SystemExit(f"{name} {label}: {c}")
            most = int(counts.max())
            total = c["hits"]
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
            ht, hi = torch.empty(max(total, 1), dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            ray_ms, _ = median_ms(lambda: r.query_rays(to, td), r.ray_query_stats, a.warmup, a.repeats)
            first = None
            for refill in (8, 24, 48):
                prm = R.HitQueryParams(tune_refill_min=refill)

                def call(fn, *args):
                    torch.cuda.current_stream(0).synchronize()
                    r._check(fn(r._ctx, ptr(to), ptr(td), None, n, C.byref(prm), *args))

                count_ms, _ = median_ms(lambda: call(lib.rt_count_ray_hits_device, ptr(counts), ptr(offsets)), r.hit_query_stats, a.warmup, a.repeats)
                fill_ms, fs = median_ms(lambda: call(lib.rt_fill_ray_hits_device, ptr(offsets), total, ptr(ht), ptr(hi)), r.hit_query_stats, a.warmup, a.repeats)
                list_ms, ls = median_ms(lambda: call(lib.rt_list_ray_hits_device, ptr(counts), ptr(offsets), total, ptr(ht), ptr(hi)), r.hit_query_stats, a.warmup, a.repeats)
                for s in (fs, ls):
                    if s["stack_overflow"] or s["slice_overflow"] or s["incomplete_rays"] or s["hits_written"] != total or s["hits"] != total:
                        raise SystemExit(f"{name} {label} refill_min {refill}: {s}")
                if int(offsets[n]) != total:
                    raise SystemExit(f"{name} {label}: offsets[n] {int(offsets[n])} != hits {total}")
                got = (ht[:total].clone(), hi[:total].clone())
                if first is None:
                    first = got
                elif not (torch.equal(got[0].view(torch.int32), first[0].view(torch.int32)) and torch.equal(got[1], first[1])):
                    raise SystemExit(f"{name} {label} refill_min {refill}: the lists differ from refill_min 8's")
                emit(f"{label:10} {refill:10d} {count_ms:9.3f} {fill_ms:9.3f} {list_ms:9.3f} {n / list_ms * 1e-3:12.1f} {total / n:7.3f} {most:5d} "
                     f"{c['nodes_visited'] / n:8.2f} {c['tris_tested'] / n:8.2f} {ray_ms:9.3f}")
            del first, got, ht, hi
            # the same walk twice: the count step along D[0] against a third of query_sides with all three crossings
            d0 = torch.tensor(D0, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
            c0 = r.count_ray_hits(to, d0, count_traversal=True)
            cs = r.hit_query_stats()
            _, crossings = r.query_sides(to, want_crossings=True, count_traversal=True)
            ss = r.side_query_stats()
            valid = crossings[:, 0] >= 0
            if cs["invalid_rays"] or ss["invalid_points"] or not torch.equal(c0[valid], crossings[valid, 0]):
                raise SystemExit(f"{name} {label}: the counts along D[0] differ from query_sides' crossings")
            d0_ms, _ = median_ms(lambda: r.count_ray_hits(to, d0), r.hit_query_stats, a.warmup, a.repeats)
            side_ms, _ = median_ms(lambda: r.query_sides(to, want_crossings=True), r.side_query_stats, a.warmup, a.repeats)
            emit(f"{label:10} along D[0]: count ms {d0_ms:9.3f}   side/3 ms {side_ms / 3:9.3f}   ratio {d0_ms / (side_ms / 3):6.3f}   hits {cs['hits'] / n:.3f}   "
                 f"nodes {cs['nodes_visited'] / n:.2f} (side, per walk: {ss['nodes_visited'] / ss['walks']:.2f})   tris {cs['tris_tested'] / n:.2f} ({ss['tris_tested'] / ss['walks']:.2f})")
            del d0, c0, crossings, to, td
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
