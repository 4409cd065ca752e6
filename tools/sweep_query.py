#!/usr/bin/env python3
"""Cost of the sphere-cast queries on device arrays (rt_query_sweeps_device) on 1 M-triangle scenes, beside the ray query on the same
paths and beside the loop a caller had to write before.

    python tools/sweep_query.py [--sweeps 8388608] [--repeats 20] [--warmup 3] [--scenes soup,terrain] [--radii 0,1,8] [--budget-ms 3000] [--out profiles/sweep_queries.txt]

Scenes and the median are those of tools/neighbor_query.py, whose helpers this tool uses.  Paths: origins uniform in the mesh's
bounding box (tools/point_query.py's UNIFORM), unit directions uniform on the sphere, tmax = the box's diagonal.  Radii are given in
mean edge lengths of the scene.  Per radius: query_sweeps, default tuning; time = rt_sweep_query_stats.ms (HIP events around the
launch), median of --repeats after --warmup; nodes and triangle records per sweep from one more call with count_traversal = 1,
outside the timed ones; hit = sweeps answered with a triangle, start = those answered at t = 0.
FLOOR: query_rays on the same origins, directions and tmax, timed the same way: one walk, no inflation, one test per triangle.
EMULATION: conservative advancement, what a caller writes without this query: query_points at the centres, every centre advanced
by (distance - r) along its unit direction, the sweeps whose gap is at most 64 x 2^-24 S (the contract's band, tests/sweep_exact.py; S =
the largest |coordinate| of the mesh and the origins) or whose path is used up retired, the rest compacted and asked again, up to 32
rounds.  Its time is torch's events around the whole loop (the point queries and the glue between them), median of 3; rounds = the
rounds it ran, open = the share of sweeps still advancing after the last.  A call so long that its repeats would take more than
--budget-ms of device time is repeated less often, and its line says how often.  There is no bar: the capability is new."""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from neighbor_query import SCENES, median_ms  # noqa: E402
from point_query import distributions  # noqa: E402

ROUNDS = 32
BAND = 64.0 * 2.0 ** -24


def advance(r, o, d, radius, tmax, tol):
    """Conservative advancement with query_points; returns (t, rounds run, sweeps still open)."""
    import torch

    n = len(o)
    t = torch.zeros(n, dtype=torch.float32, device=o.device)
    live = torch.arange(n, device=o.device)
    rounds = 0
    while rounds < ROUNDS and len(live):
        rounds += 1
        c = torch.addcmul(o[live], d[live], t[live, None]).contiguous()
        dist, _, _ = r.query_points(c, want_points=False)
        gap = dist - radius
        t[live] = t[live] + gap.clamp(min=0.0)
        live = live[(gap > tol) & (t[live] < tmax)]
    return t, rounds, len(live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=1 << 23)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="soup,terrain")
    ap.add_argument("--radii", default="0,1,8", help="in mean edge lengths of the scene")
    ap.add_argument("--budget-ms", type=float, default=3000.0, help="device time one timed entry of one line may take; longer ones get fewer repeats (the line says how many)")
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
    radii = [float(x) for x in a.radii.split(",")]
    lines = [f"# tools/sweep_query.py --sweeps {a.sweeps} --repeats {a.repeats} --warmup {a.warmup} --budget-ms {a.budget_ms:g} --scenes {a.scenes} --radii {a.radii}   ({torch.cuda.get_device_name(0)})",
             f"# commit {commit}",
             "# sweep ms = rt_sweep_query_stats.ms of query_sweeps(origins, dirs, r, tmax), default tuning (HIP events around the launch), median of the repeats;",
             "#   nodes, tris = node records and triangle records fetched per sweep (one call with count_traversal = 1, not timed); hit, start = share answered with a triangle / at t = 0",
             "# floor: query_rays on the same origins, directions and tmax (ray ms), same median; x rays = sweep ms / ray ms",
             f"# emulation: conservative advancement by query_points batches until the gap is at most 64 x 2^-24 S or {ROUNDS} rounds (adv ms: torch events round the loop, median of 3);",
             "#   rounds = rounds run, open = share of sweeps still advancing after the last, x adv = adv ms / sweep ms",
             f"# repeats = timed repeats of the sweeps / the rays (fewer than --repeats where one entry would have taken more than {a.budget_ms:g} ms of device time)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    r = R.Renderer(0)
    dev = torch.device("cuda", 0)
    n = a.sweeps
    for key in a.scenes.split(","):
        name, make = SCENES[key]
        mesh = make()
        r.set_mesh(*mesh)
        st = r.pt_stats()
        v = np.asarray(mesh[0], np.float32).reshape(-1, 3, 3)
        sample = v[:: max(1, len(v) // 100000)].astype(np.float64)
        edge = float(np.mean([np.linalg.norm(sample[:, (k + 1) % 3] - sample[:, k], axis=1).mean() for k in range(3)]))
        lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
        diag = float(np.linalg.norm(hi.astype(np.float64) - lo))
        o = dict(distributions(mesh[0], n, dev))["uniform"].contiguous()
        g = torch.Generator(device=dev)
        g.manual_seed(23)
        d = torch.randn(n, 3, generator=g, device=dev, dtype=torch.float32)
        d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        tmax = torch.full((n,), diag, dtype=torch.float32, device=dev)
        S = max(float(np.abs(v).max()), float(o.abs().max()))
        emit(f"\n## {name}: {len(v)} triangles, depth {st['bvh_depth']}, mean edge {edge:.4g}, {n} sweeps per batch, tmax {diag:.4g}")
        emit(f"{'r/edge':>6} {'r':>9} {'sweep ms':>9} {'Msweeps/s':>10} {'nodes':>8} {'tris':>8} {'hit':>6} {'start':>6} | {'ray ms':>8} {'x rays':>7} | {'adv ms':>9} {'rounds':>6} {'open':>8} "
             f"{'x adv':>7} {'repeats':>7}")
        rt, rtri = r.query_rays(o, d, tmax)
        ray_ms, rs, k2 = median_ms(lambda: r.query_rays(o, d, tmax, out=(rt, rtri)), r.ray_query_stats, a.warmup, a.repeats, a.budget_ms)
        if rs["stack_overflow"] or rs["invalid_rays"]:
            raise SystemExit(f"{name}: {rs}")
        for rel in radii:
            radius = rel * edge
            rad = torch.full((n,), radius, dtype=torch.float32, device=dev)
            t, tri, _ = r.query_sweeps(o, d, rad, tmax, want_points=False, count_traversal=True)
            sc = r.sweep_query_stats()
            if sc["stack_overflow"] or sc["invalid_sweeps"]:
                raise SystemExit(f"{name} r {radius}: {sc}")
            hit, start = float((tri >= 0).float().mean()), float(((tri >= 0) & (t == 0)).float().mean())
            sweep_ms, _, k1 = median_ms(lambda: r.query_sweeps(o, d, rad, tmax, want_points=False, out=(t, tri)), r.sweep_query_stats, a.warmup, a.repeats, a.budget_ms)
            adv = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                _, rounds, still = advance(r, o, d, radius, diag, BAND * S)
                e1.record()
                torch.cuda.synchronize()
                adv.append(e0.elapsed_time(e1))
            adv_ms = sorted(adv)[1]
            emit(f"{rel:6g} {radius:9.4g} {sweep_ms:9.3f} {n / sweep_ms * 1e-3:10.1f} {sc['nodes_visited'] / n:8.2f} {sc['tris_tested'] / n:8.2f} {hit:6.3f} {start:6.3f} | {ray_ms:8.3f} "
                 f"{sweep_ms / ray_ms:7.2f} | {adv_ms:9.1f} {rounds:6d} {still / n:8.5f} {adv_ms / sweep_ms:7.2f} {f'{k1}/{k2}':>7}")
            del rad, t, tri
        del o, d, tmax, rt, rtri
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
