#!/usr/bin/env python3
"""Refit of a path B tree to new vertices (rt_refit_mesh_device) against a device build (rt_set_mesh_device) and a host build
(rt_set_mesh), in one process: the cost of one update of a moving mesh, and what a refitted tree costs in frame time as the
mesh moves away from the vertices the tree was built for.

    python tools/refit_bvh.py [--repeats 21] [--steps 30] [--frames 5] [--out profiles/refit_bvh.txt]
    python tools/refit_bvh.py --profile-refit     # one warm-up and ten refits of the 1 M soup, nothing else:
                                                  # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracing_engine_amd as R  # noqa: E402
from device_bvh import frame_ms, half_area_sum, scene_list, to_device  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E spec peak (MI355X_MICROARCH.md; about 6.3 TB/s achievable)
f32 = np.float32


def level_sizes(nodes):
    """Node count per level of the breadth-first tree (one refit launch per level below the top)."""
    m = (nodes[:, 3] >> 24).astype(np.uint32)
    n_in = sum(((m >> b) & 1) for b in range(8)).astype(np.int64)
    out, first, count = [], 0, 1
    while count:
        out.append(count)
        first, count = first + count, int(n_in[first:first + count].sum())
    return out


def refit_bytes(n_tris, nodes):
    """Algorithmic bytes of one refit: what its kernels must read and write at least once."""
    n_nodes = len(nodes)
    inner = int(sum((((nodes[:, 3] >> 24) >> b) & 1).sum() for b in range(8)))
    return {
        "validate: vertex reads": 36 * n_tris,
        "records: vertex reads (gathered)": 36 * n_tris,
        "records: word 9-11 reads": 16 * n_tris,
        "records: writes": 48 * n_tris,
        "nodes: leaf record reads": 36 * n_tris,
        "nodes: header reads (words 0-7)": 32 * n_nodes,
        "nodes: box word writes (0-3, 8-19)": 64 * n_nodes,
        "nodes: exact box writes": 24 * n_nodes,
        "nodes: child box reads": 24 * inner,
    }


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


# ---- animations: seeded, deterministic; step k -> vertices (n, 9) float32 --------------------------------------------------

def wave(v, k, amp=1.5):
    """Travelling wave on the height field's heights (z), the light quad (last two triangles) fixed."""
    out = v.reshape(-1, 3, 3).copy()
    body = out[:-2]
    x, y = body[..., 0].astype(np.float64), body[..., 1].astype(np.float64)
    body[..., 2] += (amp * np.sin(0.25 * x + 0.15 * y - 0.35 * k)).astype(f32)
    return out.reshape(-1, 9)


class Drift:
    """Random walk of every soup triangle but the light: a rigid offset per triangle, N(0, sigma^2) per axis per step."""

    def __init__(self, v, sigma=0.04, seed=1):
        self.v = v.reshape(-1, 3, 3)
        self.sigma, self.rng = sigma, np.random.default_rng(seed)
        self.off = np.zeros((len(self.v) - 2, 1, 3), f32)
        self.k = 0

    def __call__(self, v, k):
        while self.k < k:
            self.off += self.rng.normal(scale=self.sigma, size=self.off.shape).astype(f32)
            self.k += 1
        out = self.v.copy()
        out[:-2] += self.off
        return out.reshape(-1, 9)


def explode(v, k, rate=0.05):
    """Triangle centroids scaled outward from the soup's centre by 1 + rate * k, shapes kept: refit's adversarial case."""
    out = v.reshape(-1, 3, 3).copy()
    body = out[:-2]
    c = body.mean(1, keepdims=True)
    centre = c.reshape(-1, 3).mean(0)
    body += ((c - centre) * f32(rate * k)).astype(f32)
    return out.reshape(-1, 9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile-refit", action="store_true")
    a = ap.parse_args()
    import torch

    scenes_ = scene_list()
    if a.profile_refit:
        r = R.Renderer(0)
        mesh = scenes_[0][1]()
        dmesh = to_device(mesh)
        r.set_mesh_device(*dmesh)
        moved = torch.from_numpy(Drift(np.asarray(mesh[0], f32), seed=2)(None, 3)).to("cuda:0")
        for k in range(11):
            r.refit_mesh_device(moved if k % 2 else dmesh[0])
        print(f"refit of the 1 M soup: {r.pt_stats()['bvh_build_ms']:.3f} ms (HIP events, last of 11)")
        return

    dev_name = torch.cuda.get_device_name(0)
    lines = [f"# tools/refit_bvh.py --repeats {a.repeats} --steps {a.steps} --frames {a.frames}   ({dev_name})",
             "# update cost: every kind of update alternates with the others, after a warm-up of each; median over the repeats",
             "#   call ms = host clock around the synchronous call; event ms = rt_pt_stats.bvh_build_ms (HIP events from the first",
             "#   kernel to the last: for the refit the validation read-back is inside it; for rt_set_mesh the host build's wall time)",
             "#   refits alternate between the original vertices and a drifted copy, both device tensors",
             "# frame ms: 1920x1080, 4 spp, 1 bounce, rt_render_pt_device, HIP events, median of the frames",
             "# SAH = sum of the de-quantised child-box half-areas over all occupied slots (lower is better)"]
    r = R.Renderer(0)
    r.resize(1920, 1080)
    buf = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda:0")
    meshes = {}

    # ---- 1. update cost ----------------------------------------------------------------------------------------------------
    for name, make, rot, pos, sky in scenes_:
        mesh = make()
        meshes[name] = mesh
        dmesh = to_device(mesh)
        v = np.asarray(mesh[0], f32)
        moved = torch.from_numpy(Drift(v, seed=2)(None, 3)).to("cuda:0")
        kinds = {
            "refit (device tree)": None,
            "rt_set_mesh_device": lambda: r.set_mesh_device(*dmesh),
            "rt_set_mesh (host)": lambda: r.set_mesh(*mesh),
        }
        calls = {k: [] for k in kinds}
        events = {k: [] for k in kinds}
        flip = [0]

        def do_refit():
            flip[0] ^= 1
            r.refit_mesh_device(moved if flip[0] else dmesh[0])

        def run(kind, record):
            if kind.startswith("refit"):
                r.set_mesh_device(*dmesh)  # the refit starts from a device-built tree of the original vertices
                do_refit()  # first refit of a mesh allocates its scratch
                ms = []
                for _ in range(3):
                    ms.append((timed(do_refit), r.pt_stats()["bvh_build_ms"]))
                if record:
                    calls[kind] += [c for c, _ in ms]
                    events[kind] += [e for _, e in ms]
            else:
                c = timed(kinds[kind])
                if record:
                    calls[kind].append(c)
                    events[kind].append(r.pt_stats()["bvh_build_ms"])

        for kind in kinds:
            run(kind, False)
        reps = {k: (a.repeats + 2) // 3 if k.startswith("refit") else a.repeats for k in kinds}
        for i in range(max(reps.values())):
            for kind in kinds:
                if i < reps[kind]:
                    run(kind, True)
        # the refit of a host-built tree, same vertices
        r.set_mesh(*mesh)
        do_refit()
        host_refit = [(timed(do_refit), r.pt_stats()["bvh_build_ms"]) for _ in range(a.repeats)]
        calls["refit (host tree)"] = [c for c, _ in host_refit]
        events["refit (host tree)"] = [e for _, e in host_refit]
        r.set_mesh_device(*dmesh)
        nodes, _ = r.read_bvh()
        st = r.pt_stats()
        by = refit_bytes(len(v), nodes)
        total = sum(by.values())
        ev_med = statistics.median(events["refit (device tree)"])
        lines.append(f"\n## {name}: {len(v)} triangles; device tree {st['n_nodes']} nodes, depth {st['bvh_depth']}, "
                     f"level sizes {level_sizes(nodes)}")
        lines.append(f"{'update':24} {'call ms':>8} {'min':>8} {'max':>8} {'event ms':>9} {'n':>4}")
        for kind in ("refit (device tree)", "refit (host tree)", "rt_set_mesh_device", "rt_set_mesh (host)"):
            c = calls[kind]
            lines.append(f"{kind:24} {statistics.median(c):8.3f} {min(c):8.3f} {max(c):8.3f} {statistics.median(events[kind]):9.3f} {len(c):4d}")
        lines.append(f"refit call / device build call {statistics.median(calls['refit (device tree)']) / statistics.median(calls['rt_set_mesh_device']):.3f}"
                     f", / host build call {statistics.median(calls['refit (device tree)']) / statistics.median(calls['rt_set_mesh (host)']):.4f}")
        lines.append(f"algorithmic bytes of one refit: {total / 1e6:.1f} MB = " + ", ".join(f"{k} {x / 1e6:.1f}" for k, x in by.items()))
        lines.append(f"  over the event time {ev_med:.3f} ms: {total / (ev_med * 1e-3) / 1e12:.2f} TB/s = {total / (ev_med * 1e-3) / HBM_PEAK:.3f} of the "
                     f"8 TB/s HBM peak (least time at peak {total / HBM_PEAK * 1e6:.1f} us; kernel time: the rocprofv3 table)")
        print("\n".join(lines[-9:]), flush=True)

    # ---- 2. tree quality under motion --------------------------------------------------------------------------------------
    lines.append("\n## tree quality under motion: the tree built at step 0 and refitted to step k, against a fresh device build of step k")
    lines.append("## (frame ms and SAH of both; ratio = refit / fresh)")
    anims = [("terrain wave", scenes_[2], wave), ("soup drift (random walk, sigma 0.04 per step)", scenes_[0], None),
             ("soup explosion (centroids x (1 + 0.05 k))", scenes_[0], explode)]
    rb = R.Renderer(0)
    rb.resize(1920, 1080)
    for title, (name, _, rot, pos, sky), fn in anims:
        mesh = meshes[name]
        v = np.asarray(mesh[0], f32)
        if fn is None:
            fn = Drift(v, seed=5)
        dmesh = to_device(mesh)
        r.set_mesh_device(*dmesh)
        lines.append(f"\n### {title} on {name}")
        lines.append(f"{'step':>4} {'refit ms':>9} {'build ms':>9} {'frame refit':>12} {'frame fresh':>12} {'ratio':>6} {'SAH refit':>12} {'SAH fresh':>12} {'ratio':>6}")
        for k in range(a.steps + 1):
            vk = torch.from_numpy(np.ascontiguousarray(fn(v, k))).to("cuda:0")
            r.refit_mesh_device(vk)
            refit_ms = r.pt_stats()["bvh_build_ms"]
            rb.set_mesh_device(vk, dmesh[1], dmesh[2])
            build_ms = rb.pt_stats()["bvh_build_ms"]
            fr = frame_ms(r, rot, pos, sky, a.frames, buf)
            ff = frame_ms(rb, rot, pos, sky, a.frames, buf)
            sr, sf = half_area_sum(r.read_bvh()[0]), half_area_sum(rb.read_bvh()[0])
            lines.append(f"{k:4d} {refit_ms:9.3f} {build_ms:9.3f} {fr:12.3f} {ff:12.3f} {fr / ff:6.3f} {sr:12.6g} {sf:12.6g} {sr / sf:6.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
