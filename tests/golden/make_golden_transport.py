"""Writes tests/golden/transport_<scene>.npz: the float64 reference values of path B's light transport (DESIGN.md sections 3, 6.4).

Run on the CPU from the repository root:  python tests/golden/make_golden_transport.py [scene ...]
It is imported by no test.  It runs tests/native/pt_transport_ref.cpp (through tests/transport_ref.py) at each scene's budget, checks
the conditions the reference alone must meet (relative standard error of the frame mean <= 0.05 % per channel, of every cell
brighter than a tenth of the frame mean <= 0.25 %, dimmer cells on that scale), runs oracle B (tests/native/pt_surfaces_ref.c where
there are mirrors or glass) through compare() at the CPU tests' budget, and prints one table row per scene.  A scene that misses a
condition or whose oracle frames exceed the cap on the seed-to-seed scatter is not written.

Each file holds the scene arrays (verts, albedo, emission, kind, ior), the view (pos, rot, sky, bounces, ray_eps, width, height), the
cell grid, the reference's seed, batches, paths per pixel and batch and path count, the means, standard errors and per-path
deviations per cell and channel and for the frame, the frame mean by gathering depth, and the measured conditions.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import transport_ref as TR  # noqa: E402

REF_SEED = 20261019
BATCHES = 128
# paths per pixel and batch; 256 pixels x 128 batches x 16384 = 2^29 paths in the rooms with a light.  The frame mean alone would be
# content with 2^25; the 0.25 % of the cells that see little of the light directly needs sixteen times that (at 2^27 the worst cell of
# cornell_b0 stood at 0.34 %, at 2^29 at 0.18 %).
SPP = {"cornell": 16384, "surfaces": 16384, "sky_room": 2048, "tess_light": 4096, "cornell_b0": 16384, "cornell_b1": 16384}
GPU_SPP = 4096  # tests/test_gpu_transport.py


def main(names):
    f32 = np.float32
    rows = []
    for name in names:
        s = TR.scene(name)
        v, a, e = (np.ascontiguousarray(x, f32) for x in s["mesh"])
        n = len(v)
        kind = np.zeros(n, np.uint32) if s["kind"] is None else np.ascontiguousarray(s["kind"], np.uint32)
        ior = np.ones(n, f32) if s["ior"] is None else np.ascontiguousarray(s["ior"], f32)
        view = s["view"]
        t0 = time.time()
        r = TR.reference((v, a, e), kind, ior, seed=REF_SEED, batches=BATCHES, spp=SPP[name], threads=os.cpu_count() or 16, **view)
        t_ref = time.time() - t0
        g = dict(verts=v.reshape(n, 9), albedo=a.reshape(n, 3), emission=e.reshape(n, 3), kind=kind, ior=ior,
                 pos=np.array(view["pos"], f32), rot=np.array(view["rot"], f32), sky=np.array(view["sky"], f32), bounces=np.int32(view["bounces"]),
                 ray_eps=f32(view["ray_eps"]), width=np.int32(TR.WIDTH), height=np.int32(TR.HEIGHT), cells=np.array([TR.CELLS, TR.CELLS], np.int32),
                 ref_seed=np.int64(REF_SEED), ref_batches=np.int32(BATCHES), ref_spp=np.int32(SPP[name]), paths=np.int64(r["paths"]),
                 mean=r["mean"], se=r["se"], sd=r["sd"], frame_mean=r["frame_mean"], frame_se=r["frame_se"], frame_sd=r["frame_sd"], by_depth=r["by_depth"])
        frame, cell = TR.reference_conditions(g)
        g["frame_rel_se"], g["cell_rel_se"] = np.float64(frame), np.float64(cell)
        t0 = time.time()
        spp = TR.CPU_SPP[name]
        rep = TR.compare(TR.cpu_frames(s["mesh"], s["kind"], s["ior"], view, spp), g, spp, check=False)
        t_cpu = time.time() - t0
        det_f, det_c = TR.detectable_bias(g, GPU_SPP)
        ok = frame <= TR.FRAME_REL_SE and cell <= TR.CELL_REL_SE and not rep["failures"]
        rows.append(f"{name:11s} {n:4d} tris  {r['paths']:>10d} paths {t_ref:6.1f} s  frame mean " + " ".join(f"{x:.5f}" for x in r["frame_mean"]) +
                    f"  rel se frame {frame:.2e} cell {cell:.2e}  sd/mean {np.max(r['frame_sd'] / np.maximum(r['frame_mean'], 1e-300)):.2f}"
                    f" | CPU {spp} spp {t_cpu:4.1f} s: {TR.summary(rep)} | GPU leg detects {det_f:.2%} frame, {det_c:.2%} cell | {'ok' if ok else 'NOT WRITTEN'}")
        print(rows[-1], flush=True)
        for f in rep["failures"]:
            print("    " + f)
        if ok:
            np.savez_compressed(TR.golden_path(name), **g)
    print("\n".join(["", "summary:"] + rows))


if __name__ == "__main__":
    main(sys.argv[1:] or TR.SCENES)
