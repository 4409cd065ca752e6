#!/usr/bin/env python3
"""Rate of the ray queries on device arrays (rt_query_rays_device) on 1 M-triangle scenes, against the kernel of the rt_trace_rays
test hook on the same rays.

    python tools/ray_query.py [--rays 8388608] [--repeats 20] [--warmup 3] [--sweep] [--attributes] [--baseline DIR] [--out profiles/ray_queries.txt]
    python tools/ray_query.py --hook [--rays N]      # the hook on the same batches, nothing else: the run to put under
                                                     # rocprofv3 --kernel-trace --stats --output-format csv -d DIR

Scenes: the 1 M-triangle soup and the 1 M-triangle terrain (raytracing_engine_amd/scenes.py).  Batches per scene: a COHERENT one,
the fan of a pinhole camera (the scene's benchmark view, row-major pixels), and an INCOHERENT one, cosine-distributed directions
(hashed uniforms) from the surface points the fan hits - what a path tracer's first bounce or an ambient-occlusion bake asks.
Closest hit runs along the rays; any hit on segments of length 40 along them (limit 0.999, as the hook has it).

The query's time is rt_ray_query_stats.ms (HIP events around its launch), median of --repeats after --warmup.  The hook's CALL time
includes four allocations and four synchronous copies and is not the comparison: its KERNEL time comes from a rocprofv3 kernel trace
of the --hook run, a separate process, handed over with --baseline DIR (dispatches of pt_trace_rays in order; the --hook run
prints the order).  Both processes make the batches with the same code from the same seeds; the fan's hits come from the hook in
both.  --attributes: every closest-hit batch once more through rt_query_rays_attr_device (barycentrics and normals, DESIGN.md
section 6.18), in the same process under the same protocol; its t and tri must be the plain query's."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

f32 = np.float32
SEGMENT = f32(40.0)
HOOK_REPEATS = 3


def scene_list():
    return [("soup 1M", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08), (0.0, 0.0), (0, 0, 0)),
            ("terrain 1M", lambda: scenes.terrain_scene(708, seed=1), (0.0, -0.25), (0, 0, 4))]


def hash32(x):
    x = x.astype(np.uint32)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def uniform(seed, stream, n):
    with np.errstate(over="ignore"):
        base = hash32(np.array([(seed * 0x9E3779B9 + stream) & 0xFFFFFFFF], np.uint32))[0]
        h = hash32(np.arange(n, dtype=np.uint32) + base)
    return (h >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)


def rotate(q, v):
    q = np.asarray(q, np.float64)
    b, w = q[:3], q[3]
    return 2.0 * (v @ b)[:, None] * b + (w * w - b @ b) * v + 2.0 * w * np.cross(b, v)


def fan(n, yaw_pitch, pos):
    """n rays of a pinhole camera at pos (16:9, FOV 1 as the reference's camera), row-major over the pixel grid."""
    h = int(np.sqrt(n * 9 / 16))
    w = -(-n // h)
    i = np.arange(n)
    px, py = (i % w).astype(np.float64), (i // w).astype(np.float64)
    v = np.stack([((px + 0.5) * 2 / w - 1), np.ones(n), ((py + 0.5) * 2 / h - 1) * (h / w)], 1)
    d = rotate(R.camera_quat(*yaw_pitch), v)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(np.asarray(pos, f32), (n, 3)).copy(), d.astype(f32)


def cosine_from_hits(verts, o, d, t, tri, n, seed):
    """n rays from the surface points (o + t d, on triangle tri) of the rays that hit: origin lifted 1e-3 off the surface towards the
    side the ray came from, direction cosine-distributed about that normal; the hits are reused in a hashed order until n are made."""
    hit = np.nonzero(tri >= 0)[0]
    if len(hit) == 0:
        raise SystemExit("the fan hits nothing")
    pick = hit[(hash32(np.arange(n, dtype=np.uint32) + np.uint32(seed)) % np.uint32(len(hit))).astype(np.int64)]
    v = verts.reshape(-1, 3, 3)[tri[pick]].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    din = d[pick].astype(np.float64)
    nrm = np.where(((nrm * din).sum(1) > 0)[:, None], -nrm, nrm)
    p = o[pick].astype(np.float64) + t[pick].astype(np.float64)[:, None] * din + 1e-3 * nrm
    u1, u2 = uniform(seed, 1, n).astype(np.float64), uniform(seed, 2, n).astype(np.float64)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    b1 = np.cross(nrm, a)
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = np.cross(nrm, b1)
    out = b1 * (r * np.cos(phi))[:, None] + b2 * (r * np.sin(phi))[:, None] + nrm * np.sqrt(np.maximum(0.0, 1 - u1))[:, None]
    return p.astype(f32), out.astype(f32)


def batches(r, mesh, view, n):
    """[(label, origins, directions)] of one scene; the renderer holds the scene's mesh."""
    o, d = fan(n, *view)
    t, tri = r.trace_rays(o, d)
    oi, di = cosine_from_hits(np.asarray(mesh[0], f32), o, d, t, tri, n, seed=7)
    return [("coherent", o, d), ("incoherent", oi, di)], float((tri >= 0).mean())


def hook_run(a):
    """The hook on every batch; prints, in order, what each dispatch of pt_trace_rays is."""
    r = R.Renderer(0)
    order = []
    for name, make, yaw_pitch, pos in scene_list():
        mesh = make()
        r.set_mesh(*mesh)
        order.append(f"{name}|setup|fan hits")
        bs, _ = batches(r, mesh, (yaw_pitch, pos), a.rays)
        for label, o, d in bs:
            for kind, dirs, any_hit in (("closest", d, False), ("any", d * SEGMENT, True)):
                for _ in range(HOOK_REPEATS):
                    r.trace_rays(o, dirs, any_hit=any_hit)
                    order.append(f"{name}|{label}|{kind}")
    print("HOOK_ORDER " + ";".join(order))


def read_baseline(directory):
    """{(scene, batch, kind): median kernel ms} from the kernel trace of a --hook run and the order it printed (hook_order.txt)."""
    order = None
    for f in glob.glob(os.path.join(directory, "**", "hook_order.txt"), recursive=True):
        for line in open(f):
            if line.startswith("HOOK_ORDER "):
                order = line[len("HOOK_ORDER "):].strip().split(";")
    traces = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if order is None or not traces:
        raise SystemExit(f"{directory}: no hook_order.txt / *kernel_trace.csv")
    rows = []
    for f in traces:
        for row in csv.DictReader(open(f)):
            if "pt_trace_rays" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    if len(rows) != len(order):
        raise SystemExit(f"{directory}: {len(rows)} dispatches of pt_trace_rays, the run announced {len(order)}")
    per = {}
    for (s, e), what in zip(rows, order):
        per.setdefault(tuple(what.split("|")), []).append((e - s) * 1e-6)
    return {k: statistics.median(v) for k, v in per.items() if k[1] != "setup"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="tune_refill_min 8, 24, 48 beside the default")
    ap.add_argument("--attributes", action="store_true", help="the closest-hit batches with barycentrics and normals too")
    ap.add_argument("--baseline", default="", help="directory of the rocprofv3 kernel trace of a --hook run")
    ap.add_argument("--hook", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="what to name as the commit (default: git rev-parse of this checkout)")
    a = ap.parse_args()
    if a.hook:
        hook_run(a)
        return
    import torch

    base = read_baseline(a.baseline) if a.baseline else {}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        if a.commit:
            raise OSError
        commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        if subprocess.run(["git", "-C", root, "status", "--porcelain", "-uno"], capture_output=True, text=True).stdout.strip():
            commit += " + uncommitted changes"
    except (OSError, subprocess.CalledProcessError):
        commit = a.commit or "unknown (not a git checkout)"
    lines = [f"# tools/ray_query.py --rays {a.rays} --repeats {a.repeats} --warmup {a.warmup}{' --sweep' if a.sweep else ''}{' --attributes' if a.attributes else ''}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# query ms = rt_ray_query_stats.ms (HIP events around the launch of pt_query_rays), median of the repeats; Mrays/s = rays / that",
             "# hook kernel ms = pt_trace_rays in a rocprofv3 kernel trace of `tools/ray_query.py --hook` (a separate process, the same batches),"
             f" median of {HOOK_REPEATS}" + ("" if base else ": NOT MEASURED in this run"),
             "# closest hit along the rays; any hit on segments of length 40 along them (limit 0.999 of the segment)"]
    settings = [("default", {})] + ([(f"refill_min {v}", dict(tune_refill_min=v)) for v in (8, 24, 48)] if a.sweep else [])
    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    for name, make, yaw_pitch, pos in scene_list():
        mesh = make()
        r.set_mesh(*mesh)
        bs, hit_share = batches(r, mesh, (yaw_pitch, pos), a.rays)
        lines.append(f"\n## {name}: {len(mesh[0])} triangles, {a.rays} rays per batch ({hit_share:.3f} of the fan hits)")
        lines.append(f"{'batch':11} {'query':8} {'setting':14} {'query ms':>9} {'min':>8} {'max':>8} {'Mrays/s':>9} {'hook kernel ms':>15} {'hook Mrays/s':>13} {'hook / query':>13}")
        for label, o, d in bs:
            to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
            tseg = td * float(SEGMENT)
            for kind, dirs, any_hit in (("closest", td, False), ("any", tseg, True)):
                ref = None
                for sname, kw in settings + ([("attributes", dict(attributes=True))] if a.attributes and not any_hit else []):
                    ms = []
                    for k in range(a.warmup + a.repeats):
                        got = r.query_rays(to, dirs, any_hit=any_hit, **kw)
                        st = r.ray_query_stats()
                        if k >= a.warmup:
                            ms.append(st["ms"])
                    if st["stack_overflow"] or st["invalid_rays"]:
                        raise SystemExit(f"{name} {label} {kind}: {st}")
                    tri = got if any_hit else got[1]
                    if ref is None:
                        ref = tri.clone()
                    elif not torch.equal(ref, tri):
                        raise SystemExit(f"{name} {label} {kind} {sname}: answers differ from the default setting's")
                    med = statistics.median(ms)
                    hk = base.get((name, label, kind))
                    lines.append(f"{label:11} {kind:8} {sname:14} {med:9.3f} {min(ms):8.3f} {max(ms):8.3f} {a.rays / med * 1e-3:9.1f} "
                                 + (f"{hk:15.3f} {a.rays / hk * 1e-3:13.1f} {hk / med:13.3f}" if hk else f"{'not measured':>15}"))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
