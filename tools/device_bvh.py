#!/usr/bin/env python3
"""Host-built (binned SAH + optimal-cut collapse) against device-built (LBVH + greedy collapse, rt_set_mesh_device) path B
trees, in one process, alternating the two builders on each scene: build time, tree shape, the sum of child half-areas and
the frame time at 1920x1080, 4 spp, 1 bounce (rt_render_pt_device, HIP events).

    python tools/device_bvh.py [--repeats 7] [--frames 10] [--out profiles/device_bvh.txt]
    python tools/device_bvh.py --profile-build      # one warm-up and one device build of the 1 M soup, nothing else:
                                                    # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402


def scene_list():
    return [("tri1m soup (bench headline)", lambda: scenes.soup_scene(1_000_000, seed=1, edge=0.08), (0, 0, 0, 1), (0, 0, 0), (0.2, 0.2, 0.25)),
            ("soup 100k (BASELINE configs[2] size)", lambda: scenes.soup_scene(100_000, seed=1), (0, 0, 0, 1), (0, 0, 0), (0.2, 0.2, 0.25)),
            ("terrain 1M (708x708 height field)", lambda: scenes.terrain_scene(708, seed=1), tuple(R.camera_quat(0.0, -0.25)), (0, 0, 4), (0.4, 0.5, 0.7))]


def to_device(mesh):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0") for x in mesh)


def half_area_sum(nodes):
    """Sum over occupied child slots of the de-quantised box's half-area (the quality metric of bvh_build.cpp, on the final
    8-wide boxes so that both trees are measured alike)."""
    w3 = nodes[:, 3]
    occ = (((w3 >> 24) | nodes[:, 6])[:, None] >> np.arange(8, dtype=np.uint32)) & 1
    q = np.ascontiguousarray(nodes[:, 8:20]).view(np.uint8).reshape(-1, 6, 8).astype(np.float64)
    scale = ((np.stack([(w3 >> (8 * a)) & 0xFF for a in range(3)], 1).astype(np.uint32)) << np.uint32(23)).view(np.float32).astype(np.float64)
    ext = (q[:, 3:, :] - q[:, :3, :]) * scale[:, :, None]  # (node, axis, slot)
    ha = ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0]
    return float((ha * occ).sum())


def build(r, which, mesh, dmesh):
    t0 = time.perf_counter()
    if which == "host":
        r.set_mesh(*mesh)
    else:
        r.set_mesh_device(*dmesh)
    wall = (time.perf_counter() - t0) * 1e3
    return r.pt_stats()["bvh_build_ms"], wall


def frame_ms(r, rot, pos, sky, frames, buf):
    """Median per-frame time between HIP events recorded on the stream the frames run on: an explicit torch stream lent to
    the context (not the null stream: rt_set_stream(NULL) selects the context's own stream)."""
    import torch

    prm = r.pt_params(spp=4, bounces=1, seed=1, sky=sky)
    s = torch.cuda.Stream(device=0)
    r.set_stream(s.cuda_stream)
    try:
        for _ in range(2):
            r.render_pt_device(rot, pos, prm, buf.data_ptr())
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
        for e0, e1 in ev:
            e0.record(s)
            r.render_pt_device(rot, pos, prm, buf.data_ptr())
            e1.record(s)
        s.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)
    finally:
        r.set_stream(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile-build", action="store_true")
    a = ap.parse_args()
    import torch

    r = R.Renderer(0)
    if a.profile_build:
        mesh = scenes.soup_scene(1_000_000, seed=1, edge=0.08)
        dmesh = to_device(mesh)
        for _ in range(2):
            r.set_mesh_device(*dmesh)
        print(f"device build of the 1 M soup: {r.pt_stats()['bvh_build_ms']:.3f} ms (HIP events)")
        return
    lines = [f"# tools/device_bvh.py --repeats {a.repeats} --frames {a.frames}   ({torch.cuda.get_device_name(0)})",
             "# build ms: median over the repeats after a warm-up build of each kind, host and device builds alternating;",
             "#   host = wall time of build_bvh on this process's CPUs, device = HIP events from the first build kernel to the last;",
             "#   call ms = wall time of the whole rt_set_mesh / rt_set_mesh_device call (uploads, validation, allocation included)",
             "# SAH = sum of the de-quantised child-box half-areas over all occupied slots (lower is better)",
             "# frame ms: 1920x1080, 4 spp, 1 bounce, rt_render_pt_device, HIP events, median of the frames"]
    r.resize(1920, 1080)
    buf = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda:0")
    for name, make, rot, pos, sky in scene_list():
        mesh = make()
        dmesh = to_device(mesh)
        times = {"host": [], "device": []}
        calls = {"host": [], "device": []}
        for which in ("host", "device"):
            build(r, which, mesh, dmesh)  # warm-up
        for _ in range(a.repeats):
            for which in ("host", "device"):
                ms, wall = build(r, which, mesh, dmesh)
                times[which].append(ms)
                calls[which].append(wall)
        lines.append(f"\n## {name}: {len(mesh[0])} triangles")
        lines.append(f"{'tree':8} {'build ms':>9} {'min':>8} {'max':>8} {'call ms':>8} {'nodes':>8} {'depth':>5} {'stack':>5} {'SAH':>14} {'frame ms':>9}")
        res = {}
        for which in ("host", "device"):
            build(r, which, mesh, dmesh)
            st = r.pt_stats()
            nodes, _ = r.read_bvh()
            fm = frame_ms(r, rot, pos, sky, a.frames, buf)
            res[which] = fm
            lines.append(f"{which:8} {statistics.median(times[which]):9.2f} {min(times[which]):8.2f} {max(times[which]):8.2f} "
                         f"{statistics.median(calls[which]):8.1f} {st['n_nodes']:8d} {st['bvh_depth']:5d} {st['stack_need']:5d} "
                         f"{half_area_sum(nodes):14.6g} {fm:9.3f}")
        lines.append(f"build speed-up {statistics.median(times['host']) / statistics.median(times['device']):.1f}x, "
                     f"frame time device / host {res['device'] / res['host']:.3f}")
        print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
