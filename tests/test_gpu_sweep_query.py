"""Sphere-cast queries on device tensors (Renderer.query_sweeps / rt_query_sweeps_device) on the GPU.

The reference is the native brute force over all triangles (tests/native/sweep_query_ref.cpp through tests/sweep_exact.py: the
arithmetic of csrc/sweep_tri.h without a tree), which the kernel must match bit for bit in every element of t, tri and point; that
reference is held to the float64 contract on the CPU (tests/test_sweep_query_host.py).  The first tests run every family on its own
meshes; the others use one batch on the terrain."""
import functools

import numpy as np
import pytest

import raytracing_engine_amd as R
import sweep_exact as SX
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, busy_stream, ptr, same_floats, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_px_surface as set_mesh

pytestmark = pytest.mark.gpu

PX = SX.PX
f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = -1, -2


def query(renderer, o, d, r, tmax=None, **kw):
    """Numpy in, numpy out, through device tensors: (t, tri, point)."""
    got = renderer.query_sweeps(tdev(o), tdev(d), r if isinstance(r, float) else tdev(r), None if tmax is None else tdev(tmax), **kw)
    return tuple(None if x is None else x.cpu().numpy() for x in got)


def assert_answers(got, ref, sel=slice(None), what=None):
    t, tri, point = got
    assert np.array_equal(tri, ref["tri"][sel]), (what, np.nonzero(tri != ref["tri"][sel])[0][:8])
    assert same_floats(t, ref["t"][sel]), what
    if point is not None:
        assert same_floats(point, ref["point"][sel]), what


def check_case(renderer, name, c, what):
    got = query(renderer, c["o"], c["d"], c["r"], c.get("tmax"))
    t, tri, point = got
    n = len(tri)
    assert tri.dtype == np.int32 and t.dtype == f32 and point.dtype == f32 and point.shape == (n, 3)
    ref = c["ref"]["brute"]
    assert_answers(got, ref, what=(name, c["mesh"], what))
    st = renderer.sweep_query_stats()
    assert (st["sweeps"], st["invalid_sweeps"], st["hits"], st["stack_overflow"], st["launches"]) == (n, int((ref["tri"] == INVALID).sum()), int((ref["tri"] >= 0).sum()), 0, 1)
    assert st["ms"] > 0


# ---- 1. every family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SX.FAMILIES + ("h",))
def test_every_family_on_the_host_built_tree(renderer, name):
    hits = 0
    for c in SX.family_case(name):
        set_mesh(renderer, c["verts"])
        check_case(renderer, name, c, "host")
        hits += int((c["ref"]["brute"]["tri"] >= 0).sum())
    assert hits >= 10
    if name == "h":
        assert all((c["ref"]["brute"]["tri"] == INVALID).sum() == 28 for c in SX.family_case("h"))


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, name):
    for c, cm in zip(SX.family_case(name), SX.family_case(name, 2400, True)):
        v = c["verts"]
        if len(v) < 8:
            continue  # (the tetrahedron: the host-built tree has it)
        a, e = PX.surface(v)
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_case(renderer, name, c, "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_case(renderer, name, c, "device build")
        renderer.refit_mesh_device(tdev(cm["verts"]))
        check_case(renderer, name, cm, "refit to moved vertices")


# ---- 2. one batch on the terrain ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    """Family a and family b of the terrain in one shuffled batch, and the brute-force answers."""
    parts = [next(c for c in SX.family_case(name) if c["mesh"] == "terrain") for name in ("a", "b")]
    rng = np.random.default_rng(17)
    n = sum(len(p["r"]) for p in parts)
    perm = rng.permutation(n)
    o, d, r = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])[perm]) for k in ("o", "d", "r"))
    v = parts[0]["verts"]
    ref = SX.reference(v, o, d, r)
    assert SX.walk_is_brute(ref) and (ref["brute"]["tri"] >= 0).sum() > n // 4 and (ref["brute"]["tri"] == MISS).sum() > n // 8
    return dict(v=v, o=o, d=d, r=r, ref=ref["brute"], n=n, reach=PX.reach_of(v))


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


def test_refill_and_the_exit_rule(renderer):
    """4 000 invalid items through one workgroup; 1 024 invalid items in front of valid ones: refills that hand out 64 entries and
    leave no lane alive; whole blocks of tmax <= 0, which miss without a walk."""
    b = set_batch(renderer)
    N = b["n"]
    sel = np.arange(4000) % N
    o = b["o"][sel].copy()
    o[:, 1] = np.array([np.nan, np.inf, -np.inf, 2 * float(b["reach"])], f32)[np.arange(4000) % 4]
    t, tri, point = query(renderer, o, b["d"][sel], b["r"][sel], tune_max_blocks=1)
    assert (tri == INVALID).all() and np.isnan(t).all() and np.isnan(point).all()
    st = renderer.sweep_query_stats()
    assert (st["sweeps"], st["invalid_sweeps"], st["hits"]) == (4000, 4000, 0)
    r_bad = b["r"][:1024].copy()
    r_bad[:] = np.array([np.nan, -1.0, np.inf, 2 * float(b["reach"])], f32)[np.arange(1024) % 4]
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3, tune_refill_min=1)):
        t, tri, point = query(renderer, np.concatenate([b["o"][:1024], b["o"]]), np.concatenate([b["d"][:1024], b["d"]]), np.concatenate([r_bad, b["r"]]), **kw)
        assert (tri[:1024] == INVALID).all() and np.isnan(t[:1024]).all() and np.isnan(point[:1024]).all(), kw
        assert_answers((t[1024:], tri[1024:], point[1024:]), b["ref"], what=kw)
        st = renderer.sweep_query_stats()
        assert (st["sweeps"], st["invalid_sweeps"], st["hits"]) == (1024 + N, 1024, int((b["ref"]["tri"] >= 0).sum()))
    tmax = np.full(N, INF, f32)
    tmax[:512] = np.array([0.0, -0.0, -1.0, -np.inf], f32)[np.arange(512) % 4]
    tmax[700:764] = 0.0
    t, tri, point = query(renderer, b["o"], b["d"], b["r"], tmax, tune_max_blocks=1)
    walked = tmax > 0
    assert (tri[~walked] == MISS).all() and (t[~walked] == INF).all() and np.isnan(point[~walked]).all()
    assert_answers((t[walked], tri[walked], point[walked]), b["ref"], walked)
    assert renderer.sweep_query_stats()["invalid_sweeps"] == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_edges(renderer, n):
    b = set_batch(renderer)
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=64)):
        assert_answers(query(renderer, b["o"][:n], b["d"][:n], b["r"][:n], **kw), b["ref"], slice(0, n), (n, kw))
        if n:
            st = renderer.sweep_query_stats()
            assert (st["sweeps"], st["stack_overflow"], st["launches"]) == (n, 0, 1)


def test_stack_spill_and_counters(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest of the 7 per level in global memory: the same bits.  The
    walk fetches fewer nodes than the tree has; without count_traversal nothing is counted."""
    b = set_batch(renderer)
    assert renderer.pt_stats()["bvh_depth"] > 1
    assert_answers(query(renderer, b["o"], b["d"], b["r"], tune_lds_stack=1, count_traversal=True), b["ref"])
    st = renderer.sweep_query_stats()
    print(f"terrain: {st['nodes_visited'] / b['n']:.2f} nodes and {st['tris_tested'] / b['n']:.2f} records per item ({len(b['v'])} triangles)")
    assert st["stack_overflow"] == 0 and 0 < st["tris_tested"] / b["n"] < len(b["v"]) / 8 and st["nodes_visited"] > 0
    assert_answers(query(renderer, b["o"], b["d"], b["r"]), b["ref"])
    st = renderer.sweep_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)


def test_a_scalar_radius_is_the_tensor_of_that_radius(renderer):
    b = set_batch(renderer)
    for radius in (0.0, 0.25):
        full = np.full(b["n"], radius, f32)
        ref = SX.reference(b["v"], b["o"], b["d"], full)["brute"]
        assert_answers(query(renderer, b["o"], b["d"], radius), ref, what=radius)
        assert_answers(query(renderer, b["o"], b["d"], full), ref, what=radius)
    assert (ref["tri"] >= 0).sum() > 100


def test_out_tensors_and_want_points(renderer):
    import torch

    b = set_batch(renderer)
    for n in (1, 65, 600):
        o, d, r = tdev(b["o"][:n]), tdev(b["d"][:n]), tdev(b["r"][:n])
        tm = tdev(np.full(n, INF, f32))
        before = [x.clone() for x in (o, d, r, tm)]
        t_buf, i_buf, p_buf = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64), sentinel(n, torch.float32, 64, cols=3)
        t, tri, point = renderer.query_sweeps(o, d, r, tm, out=(t_buf[:n], i_buf[:n], p_buf[:n]))
        assert t.data_ptr() == t_buf.data_ptr() and tri.data_ptr() == i_buf.data_ptr() and point.data_ptr() == p_buf.data_ptr()
        assert still_sentinel(t_buf, 0, n) and still_sentinel(i_buf, 0, n) and still_sentinel(p_buf, 0, n)
        assert_answers(tuple(x.cpu().numpy() for x in (t, tri, point)), b["ref"], slice(0, n))
        for x, x0 in zip((o, d, r, tm), before):
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
        for buf in (t_buf, i_buf, p_buf):
            buf.fill_(-7)
        t, tri, none = renderer.query_sweeps(o, d, r, out=(t_buf[:n], i_buf[:n]), want_points=False)
        assert none is None and still_sentinel(t_buf, 0, n) and still_sentinel(i_buf, 0, n) and still_sentinel(p_buf)
        assert_answers((t.cpu().numpy(), tri.cpu().numpy(), None), b["ref"], slice(0, n))
    t, tri, none = renderer.query_sweeps(o, d, r, want_points=False)
    assert none is None
    assert_answers((t.cpu().numpy(), tri.cpu().numpy(), None), b["ref"], slice(0, n))
    with pytest.raises(ValueError):
        renderer.query_sweeps(o, d, r, out=(t_buf[:n], i_buf[:n - 1], p_buf[:n]))


def test_no_sync_on_a_busy_stream(renderer):
    import torch

    b = set_batch(renderer)
    n = b["n"]
    o, d, r = tdev(b["o"]), tdev(b["d"]), tdev(b["r"])
    t, tri, point = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3)
    with busy_stream(renderer):
        renderer.query_sweeps(o, d, r, out=(t, tri, point), sync=False)
    assert_answers(tuple(x.cpu().numpy() for x in (t, tri, point)), b["ref"])


def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_batch(renderer)
    n = 500
    o, d, r = tdev(b["o"][:n]), tdev(b["d"][:n]), tdev(b["r"][:n])
    t, tri, point = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3)
    good = (ptr(o), ptr(d), ptr(r), None, n, None, ptr(t), ptr(tri), ptr(point))
    fresh = R.Renderer(0)
    try:
        assert lib.rt_query_sweeps_device(fresh._ctx, *good) == RT_ERR_STATE  # no mesh
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short3=12, short1=4)  # n - 1 rows from the short ones
    hp, big, short3, short1 = bp.hp, bp.big, bp.short3, bp.short1

    def with_arg(k, value):
        args = list(good)
        args[k] = value
        return tuple(args)

    calls = [with_arg(0, None), with_arg(1, None), with_arg(2, None), with_arg(6, None), with_arg(7, None),  # NULL where a pointer is due
             with_arg(0, hp), with_arg(1, hp), with_arg(2, hp), with_arg(3, hp), with_arg(6, hp), with_arg(7, hp), with_arg(8, hp),  # host memory
             with_arg(0, short3), with_arg(1, short3), with_arg(2, short1), with_arg(3, short1), with_arg(6, short1), with_arg(7, short1), with_arg(8, short3),  # too short
             with_arg(4, (1 << 30) + 1)] + [with_arg(5, prm) for prm in bad_params(R.SweepQueryParams)]
    for k, args in enumerate(calls):
        assert lib.rt_query_sweeps_device(ctx, *args) == RT_ERR_INVALID, k
        assert_untouched(renderer, (t, tri, point), big, k)
    assert lib.rt_query_sweeps_device(ctx, *with_arg(4, 0)) == 0  # n = 0 is accepted, and does nothing
    assert lib.rt_query_sweeps_device(ctx, None, None, None, None, 0, None, None, None, None) == 0
    renderer.synchronize()
    assert still_sentinel(t) and still_sentinel(tri) and still_sentinel(point)
    got = renderer.query_sweeps(o, d, r, out=(t, tri, point))
    assert_answers(tuple(x.cpu().numpy() for x in got), b["ref"], slice(0, n))


def test_between_two_other_kinds_their_statistics_and_answers_stay(renderer):
    """A closest-point query, a sphere cast, a ray query on one context: each kind's statistics are its own query's whatever ran after
    it, and the other kinds answer as they did before."""
    b = set_batch(renderer)
    o, d = tdev(b["o"]), tdev(b["d"])
    dist0, ptri0, _ = renderer.query_points(o[:700], want_points=False, count_traversal=True)
    rt0, rtri0 = renderer.query_rays(o, d)
    points_before, rays_before = renderer.point_query_stats(), renderer.ray_query_stats()
    renderer.query_points(o[:700], want_points=False, count_traversal=True)
    assert_answers(query(renderer, b["o"], b["d"], b["r"], count_traversal=True), b["ref"])
    rt1, rtri1 = renderer.query_rays(o, d)
    points_after, rays_after, sweeps = renderer.point_query_stats(), renderer.ray_query_stats(), renderer.sweep_query_stats()
    for before, after in ((points_before, points_after), (rays_before, rays_after)):
        assert {k: v for k, v in before.items() if k != "ms"} == {k: v for k, v in after.items() if k != "ms"}
    assert points_after["points"] == 700 and rays_after["rays"] == b["n"] and sweeps["sweeps"] == b["n"] and sweeps["nodes_visited"] > 0
    dist1, ptri1, _ = renderer.query_points(o[:700], want_points=False, count_traversal=True)
    assert same_floats(dist0.cpu().numpy(), dist1.cpu().numpy()) and np.array_equal(ptri0.cpu().numpy(), ptri1.cpu().numpy())
    assert same_floats(rt0.cpu().numpy(), rt1.cpu().numpy()) and np.array_equal(rtri0.cpu().numpy(), rtri1.cpu().numpy())
    assert renderer.sweep_query_stats() == sweeps  # a second read returns the same
