"""The lifetime of everything a context holds (csrc/rt_internal.h): a context that has used every buffer, event,
stream, frame slot and query kind it can hold closes, and the next one computes the same; a context closes with frames in flight.

Nothing here measures free device memory: the figure is device-wide and other processes move it.  That no handle leaks or is
destroyed twice is tests/test_owned_host.py's to say; this file pins that the lifetimes work on the device.

Statistics are compared without their times.  A time is a member named `ms`, `ms_*` or `*_ms` (one rule for all the statistics structs:
`ms` of a query, `ms_total` and the stage times of a frame, `bvh_build_ms`); a member so named that is not a time would escape the
comparison, so none may be.

Every shape is the smallest that reaches the code: views of 64x64 and 32x32, the default sphere scene, a closed box of 12 triangles
with one emissive face (sign_exact.box), 8 items per query."""
import numpy as np
import pytest

import raytracing_engine_amd as R
import sign_exact as SX
from gpu_query import tdev

pytestmark = pytest.mark.gpu

f32 = np.float32
W = H = 64
BOX = np.ascontiguousarray(SX.box(cells=1), f32).reshape(12, 9)
ALBEDO = np.full((12, 3), 0.7, f32)
EMISSION = np.zeros((12, 3), f32)
EMISSION[:2] = 8.0  # the two triangles of the face x = -1
OFFSET = f32(0.015625)  # the refit moves the box by 2^-6 along every axis
EYE = (0.25, -0.125, 0.5)  # inside the box
_rng = np.random.default_rng(11)
POINTS = _rng.uniform(-0.9, 0.9, (8, 3)).astype(f32)
DIRS = _rng.normal(size=(8, 3)).astype(f32)
TRIS = _rng.uniform(-1.5, 1.5, (8, 9)).astype(f32)  # corners inside and outside the box: they cross its faces
KINDS = ("ray", "point", "side", "hit", "neighbor", "overlap", "clearance", "knn", "sweep")


def arrays(result):
    """A call's answer - a tensor, an array or a tuple of them with None for what was not asked for - as a list of host arrays."""
    items = result if isinstance(result, (tuple, list)) else (result,)
    return [x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in items if x is not None]


def path_a_frames(r):
    """The path A frames of a round on `r`, already at 64 x 64 with the default scene and configuration."""
    return [r.render(spp=spp) for spp in (1, 4, 16)]


def one_round():
    """Everything a context can hold, used once; returns what the round computed: {name: list of arrays} and {name: statistics}."""
    got, stats = {}, {}
    r = R.Renderer(0)
    r.resize(W, H)
    r.set_scene(R.default_scene())
    got["path_a"] = path_a_frames(r)  # the level images regrow 1 -> 4 -> 16
    got["rgba8"] = [r.read_rgba8()]
    cfg = r.default_config()
    cfg.reflections = 1
    r.set_config(cfg)
    got["chains"] = arrays(r.render_chains())
    staged = r.default_config()
    staged.profile_stages = 1
    r.set_config(staged)
    got["path_a_staged"] = [r.render()]

    r.set_config(r.default_config())
    r.set_mesh(BOX, ALBEDO, EMISSION)
    pt = dict(pos=EYE, spp=1, bounces=1)
    got["pt"] = [r.render_pt(**pt), r.render_pt(tune_no_overlap=2, **pt)]  # the second on two streams: the auxiliary stream and its two events
    r.set_config(staged)
    got["pt"].append(r.render_pt(**pt))  # under per-stage timing: the event pool fills
    stats["pt"] = r.pt_stats()

    points, dirs, tris = tdev(POINTS), tdev(DIRS), tdev(TRIS)
    got["ray"] = arrays(r.query_rays(points, dirs))
    got["point"] = arrays(r.query_points(points))
    got["side"] = arrays(r.query_sides(points))
    got["signed_distance"] = arrays(r.query_signed_distance(points))
    got["hit"] = arrays(r.list_ray_hits(points, dirs))
    got["neighbor"] = arrays(r.list_neighbors(points, 1.0))
    offsets, tri, edges, counts = r.list_overlaps(tris)
    got["overlap"] = arrays((offsets, tri, edges, counts))
    got["overlap_segment"] = arrays(r.overlap_segments(tris, offsets, tri))
    got["clearance"] = arrays(r.query_clearance(tris))
    got["knn"] = arrays(r.query_knn(points, 3))
    got["sweep"] = arrays(r.query_sweeps(points, dirs, 0.0625))
    for kind in KINDS:
        stats[kind] = getattr(r, kind + "_query_stats")()
    stats["overlap_segment"] = r.overlap_segment_stats()

    r.set_mesh_device(tdev(BOX), tdev(ALBEDO), tdev(EMISSION))
    r.refit_mesh_device(tdev(BOX + OFFSET))
    got["pt_refit"] = [r.render_pt(**pt)]

    r.frames_configure(2, r.FRAME_RGBA8)
    r.frame_submit(0)
    r.frame_submit(1, pos=EYE, pt_params=r.pt_params(spp=1, bounces=1))
    got["frames"] = [r.frame_wait(0), r.frame_wait(1)]
    r.set_mesh(BOX, ALBEDO, EMISSION)  # replaced while the lanes have borrowed it
    r.resize(32, 32)  # the slots and the levels go
    got["path_a_32"] = [r.render()]
    r.close()
    r.close()  # harmless
    for st in stats.values():
        for key in [k for k in st if k == "ms" or k.startswith("ms_") or k.endswith("_ms")]:  # times differ from run to run
            del st[key]
    return got, stats


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_a_context_that_used_everything_closes_and_the_next_renders_the_same(renderer):
    rounds = [one_round() for _ in range(3)]
    first, first_stats = rounds[0]
    for k, (got, stats) in enumerate(rounds[1:], 1):
        assert got.keys() == first.keys()
        for name in first:
            assert len(got[name]) == len(first[name]) and all(same(a, b) for a, b in zip(got[name], first[name])), (k, name)
        assert stats == first_stats, (k, {n: (stats[n], first_stats[n]) for n in stats if stats[n] != first_stats[n]})

    r = renderer
    r.set_config(r.default_config())
    r.set_scene(R.default_scene())
    r.resize(W, H)
    want = path_a_frames(r)
    assert all(same(a, b) for a, b in zip(first["path_a"], want))
    assert same(first["path_a_staged"][0], want[0])  # per-stage timing changes no pixel
    r.resize(32, 32)
    assert same(first["path_a_32"][0], r.render())


def test_closing_with_frames_in_flight_waits_for_them(renderer):
    r = R.Renderer(0)
    r.resize(W, H)
    r.set_scene(R.default_scene())
    r.frames_configure(3, r.FRAME_F32)
    for slot in range(3):
        r.frame_submit(slot, spp=16)
    r.close()  # nobody waited: the close does
    with R.Renderer(0) as fresh:
        fresh.resize(W, H)
        fresh.set_scene(R.default_scene())
        got = fresh.render()
    renderer.set_config(renderer.default_config())
    renderer.set_scene(R.default_scene())
    renderer.resize(W, H)
    assert same(got, renderer.render())
