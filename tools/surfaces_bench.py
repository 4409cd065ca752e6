#!/usr/bin/env python3
"""What mirror and glass surfaces cost on path B (rt_set_mesh_surfaces): the headline workload's scene (1 M soup,
1920x1080, 4 spp) at 1 and 3 bounces under four surface settings, in one process, the variants alternated round by round.

    python tools/surfaces_bench.py [--frames 20] [--rounds 3] [--out profiles/surfaces.txt]
    python tools/surfaces_bench.py --profile    # two frames of every variant at 3 bounces, nothing else: the run to put under
                                                # rocprofv3 --kernel-trace --stats (pt_shade<false> against pt_shade<true>)

Variants: "none" = a context whose mesh never saw the call; "lambert" = every kind 0 through the call (pt_shade<false> as well);
"m10_g10" = 10 % mirror + 10 % glass (index 1.5); "g50" = 50 % glass (index 1.5), kinds from scenes.soup_surfaces.  Times are
HIP events around each frame on an explicit stream (median of --frames after two warm-up frames, per round); rays per frame are
the frame's camera + bounce + shadow rays from rt_pt_stats."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402
from raytracing_engine_amd import scenes  # noqa: E402

N_TRIS, EDGE, W, H, SPP, SKY = 1_000_000, 0.08, 1920, 1080, 4, (0.2, 0.2, 0.25)
VARIANTS = ("none", "lambert", "m10_g10", "g50")


def surfaces(variant):
    if variant == "lambert":
        return np.zeros(N_TRIS, np.uint32), None
    if variant == "m10_g10":
        return scenes.soup_surfaces(N_TRIS, 1, 0.1, 0.1, 1.5)
    return scenes.soup_surfaces(N_TRIS, 1, 0.0, 0.5, 1.5)


def frame_ms(r, prm, frames, buf, stream):
    import torch

    for _ in range(2):
        r.render_pt_device((0, 0, 0, 1), (0, 0, 0), prm, buf.data_ptr())
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
    for e0, e1 in ev:
        e0.record(stream)
        r.render_pt_device((0, 0, 0, 1), (0, 0, 0), prm, buf.data_ptr())
        e1.record(stream)
    stream.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bounces", default="1,3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    mesh = scenes.soup_scene(N_TRIS, seed=1, edge=EDGE)
    plain, surf = R.Renderer(0), R.Renderer(0)  # "none" renders with a context that never calls rt_set_mesh_surfaces
    for r in (plain, surf):
        r.set_mesh(*mesh)
        r.resize(W, H)
    ctx = {v: plain if v == "none" else surf for v in VARIANTS}
    stream = torch.cuda.Stream(device=0)
    buf = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    bounces = [int(b) for b in a.bounces.split(",")]
    if a.profile:
        for v in VARIANTS:
            if v != "none":
                surf.set_surfaces(*surfaces(v))
            prm = ctx[v].pt_params(spp=SPP, bounces=3, seed=1, sky=SKY)
            for _ in range(2):
                ctx[v].render_pt_device((0, 0, 0, 1), (0, 0, 0), prm, buf.data_ptr())
            ctx[v].synchronize()
        print("profile run done")
        return
    rays, ms = {}, {}
    for b in bounces:
        for v in VARIANTS:  # rays per frame (synchronous frame; not timed)
            if v != "none":
                surf.set_surfaces(*surfaces(v))
            ctx[v].render_pt(params=ctx[v].pt_params(spp=SPP, bounces=b, seed=1, sky=SKY))
            st = ctx[v].pt_stats()
            rays[b, v] = (st["camera_rays"], st["bounce_rays"], st["shadow_rays"])
    for rnd in range(a.rounds):
        for b in bounces:
            for v in VARIANTS:
                if v != "none":
                    surf.set_surfaces(*surfaces(v))
                r = ctx[v]
                r.set_stream(stream.cuda_stream)
                try:
                    ms.setdefault((b, v), []).append(frame_ms(r, r.pt_params(spp=SPP, bounces=b, seed=1, sky=SKY), a.frames, buf, stream))
                finally:
                    r.set_stream(None)
    lines = [f"# tools/surfaces_bench.py --frames {a.frames} --rounds {a.rounds}: 1 M soup (edge {EDGE}), {W}x{H}, {SPP} spp, one MI355X",
             f"# device: {torch.cuda.get_device_name(0)}; ms = per-frame HIP-event median of {a.frames} frames per round; rounds alternate the variants",
             f"{'bounces':>7} {'variant':>8} {'ms/frame (rounds)':>30} {'median':>8} {'camera':>10} {'bounce':>10} {'shadow':>10} {'rays':>10} {'Mrays/s':>8} {'vs none':>8}"]
    for b in bounces:
        base = statistics.median(ms[b, "none"])
        for v in VARIANTS:
            m = statistics.median(ms[b, v])
            tot = sum(rays[b, v])
            lines.append(f"{b:>7} {v:>8} {' '.join(f'{x:.3f}' for x in ms[b, v]):>30} {m:8.3f} {rays[b, v][0]:>10} {rays[b, v][1]:>10} {rays[b, v][2]:>10} "
                         f"{tot:>10} {tot / m / 1e3:8.1f} {m / base:8.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    plain.close()
    surf.close()


if __name__ == "__main__":
    main()
