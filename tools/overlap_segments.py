#!/usr/bin/env python3
"""Cost of the overlap segments on device arrays (rt_overlap_segments_device) beside the list call that produced their list.

    python tools/overlap_segments.py [--tris 1048576] [--repeats 10] [--warmup 2] [--scenes soup,terrain] [--budget-ms 4000] [--out profiles/overlap_segments.txt]

The four workloads of tools/overlap_query.py, found the same way (its scenes, its query triangles, its search for the displacement and
the growth that give about 1 and 8 overlaps per query triangle).  Per workload: the list (rt_list_overlaps_device, capacity = the total,
rt_overlap_query_stats.ms), then on that list
  seg ms   rt_overlap_segment_stats.ms of rt_overlap_segments_device with `ends`: HIP events round the map kernel and the segment kernel
  map ms   the same call on offsets that are all 0 (no entry is visited): the map from original index to leaf position, written by
           every call, and the launch of a segment kernel that returns at once
  Ment/s   entries per second of the segment call
each the median of --repeats after --warmup.  Then the question the long lists ask: the segment call on the ONE longest list of the
batch alone (n = 1), and on as many entries of the batch's first lists (short ones), both a single small launch: the fill walk inserts
a list of k entries in O(k^2) in one lane, the segment call has one lane per entry whoever owns it.  There is no bar: the capability is new."""
import argparse
import ctypes as C
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_query as OQ  # noqa: E402
import raytracing_engine_amd as R  # noqa: E402


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
    lines = [f"# tools/overlap_segments.py --tris {a.tris} --repeats {a.repeats} --warmup {a.warmup} --budget-ms {a.budget_ms:g} --scenes {a.scenes}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# list ms = rt_overlap_query_stats.ms of rt_list_overlaps_device (capacity = the total); seg ms = rt_overlap_segment_stats.ms of rt_overlap_segments_device with ends",
             "#   on that list (the map kernel and the segment kernel); map ms = the same call on offsets of zeros: the map and an empty segment kernel; medians of the repeats",
             "# shift, grow, ovl (overlaps per query) and most (the longest list) as in tools/overlap_query.py; seg / list = seg ms / list ms; Ment/s = entries per second of the segment call",
             "# touch = the share of one-bit entries (the same point twice); bad = bad_entries (must be 0)",
             "# longest ms = the segment call on the longest list alone (n = 1, `most` entries); short ms = on the first lists of the batch that hold as many entries; one launch each",
             "# repeats = timed repeats of list / seg / map behind that line's medians"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    lib = R.load()
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    n = a.tris
    for key in a.scenes.split(","):
        name, make = OQ.SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        emit(f"\n## {name}: {len(mesh[0])} triangles, depth {st['bvh_depth']}, {n} query triangles per batch")
        emit(f"{'target':>6} {'shift':>9} {'grow':>7} {'entries':>9} {'ovl':>7} {'most':>5} {'list ms':>9} {'seg ms':>8} {'map ms':>8} {'seg / list':>10} {'Ment/s':>8} {'touch':>6} {'bad':>4} "
             f"{'longest ms':>10} {'short ms':>9} {'repeats':>9}")
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
            r.count_overlaps(queries(shift, grow, min(n, OQ.SAMPLE)))
            return r.overlap_query_stats()["overlaps"] / min(n, OQ.SAMPLE)

        for target in OQ.TARGETS:
            grow = 1.0
            shift, found = OQ.knob_for(lambda s: mean(s, 1.0), target, range(-8, 5))
            if not found:
                grow, found = OQ.knob_for(lambda g: mean(shift, g), target, range(0, 8))
            q = queries(shift, grow)
            counts = r.count_overlaps(q)
            total, most = r.overlap_query_stats()["overlaps"], int(counts.max())
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
            tri, edges = torch.empty(max(total, 1), dtype=torch.int32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            seg, ends = torch.empty(max(total, 1), 6, dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            prm = R.OverlapQueryParams()

            def list_call():
                torch.cuda.current_stream(0).synchronize()
                r._check(lib.rt_list_overlaps_device(r._ctx, ptr(q), n, C.byref(prm), ptr(counts), ptr(offsets), total, ptr(tri), ptr(edges)))
                return r.overlap_query_stats()["ms"]

            def seg_call(tq, count, off, cap, t):
                torch.cuda.current_stream(0).synchronize()
                r._check(lib.rt_overlap_segments_device(r._ctx, ptr(tq), count, ptr(off), cap, ptr(t), ptr(seg), ptr(ends)))
                return r.overlap_segment_stats()

            list_ms, k1 = OQ.median_ms(list_call, a.warmup, a.repeats, a.budget_ms)
            if int(offsets[n]) != total:
                raise SystemExit(f"{name}: the list holds {int(offsets[n])} entries, the count step found {total}")
            seg_ms, k2 = OQ.median_ms(lambda: seg_call(q, n, offsets, total, tri)["ms"], a.warmup, a.repeats, a.budget_ms)
            s = seg_call(q, n, offsets, total, tri)
            if s["entries"] != total or s["bad_entries"] or s["skipped_incomplete"] or s["segments"] + s["touches"] != total:
                raise SystemExit(f"{name}: {s}")
            zeros = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            map_ms, k3 = OQ.median_ms(lambda: seg_call(q, n, zeros, total, tri)["ms"], a.warmup, a.repeats, a.budget_ms)
            # the longest list alone, and as many entries of short lists
            i = int(counts.argmax())
            lo = int(offsets[i])
            one_off = torch.tensor([0, most], dtype=torch.int64, device=dev)
            longest_ms, _ = OQ.median_ms(lambda: seg_call(q[i:i + 1].contiguous(), 1, one_off, most, tri[lo:lo + most].contiguous())["ms"], a.warmup, a.repeats, a.budget_ms)
            m = int(torch.searchsorted(offsets, torch.tensor([most], dtype=torch.int64, device=dev), right=True)[0])  # the first m - 1 lists end at or below `most` entries
            m = max(2, min(m, n + 1))
            short_cap = int(offsets[m - 1])
            short_ms, _ = OQ.median_ms(lambda: seg_call(q[:m - 1].contiguous(), m - 1, offsets[:m].contiguous(), short_cap, tri)["ms"], a.warmup, a.repeats, a.budget_ms) \
                if short_cap else (float("nan"), 0)
            emit(f"{target:6d} {shift:9.4g} {grow:7.3g} {total:9d} {total / n:7.3f} {most:5d} {list_ms:9.3f} {seg_ms:8.3f} {map_ms:8.3f} {seg_ms / list_ms:10.4f} {total / seg_ms * 1e-3:8.1f} "
                 f"{s['touches'] / max(total, 1):6.3f} {s['bad_entries']:4d} {longest_ms:10.4f} {short_ms:9.4f} {f'{k1}/{k2}/{k3}':>9}   (short: {short_cap} entries of {m - 1} lists)")
            del q, counts, offsets, tri, edges, seg, ends, zeros
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
