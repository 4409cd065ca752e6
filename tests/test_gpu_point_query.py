"""Closest-point queries on device tensors (Renderer.query_points / rt_query_points_device) on the GPU.

Two references, both from tests/point_exact.py: the native brute force over all triangles (tests/native/point_query_ref.cpp, the
arithmetic of csrc/point_tri.h without a tree), which the kernel must match bit for bit in tri, dist and point, and the float64
contract, which its answers must satisfy on their own.  The first tests run every family on its own meshes; the others need ONE batch
on ONE mesh whose size they can cut, tile and plant points into: the 4 000 points of soup_batch() against the 2 000-triangle soup.  A
distance limit needs no tolerance: the answer is defined as the (d2, index)-minimal triangle, so "hit when d2 < rmax * rmax" is decided
by the reference's own d2."""
import functools

import numpy as np
import pytest

import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, busy_stream, dev, pt_frame, ptr, same_floats, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_px_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = -1, -2
N = 4000


def query(renderer, p, rmax=None, **kw):
    """Numpy in, numpy out, through device tensors: (dist, tri, point)."""
    d, t, c = renderer.query_points(tdev(p), None if rmax is None else tdev(rmax), **kw)
    return d.cpu().numpy(), t.cpu().numpy(), None if c is None else c.cpu().numpy()


@functools.lru_cache(maxsize=None)
def family_data(name, moved=False):
    """[dict(part, ref (the brute force), em)] of one family, on its meshes or on ray_exact.moved() vertices; computed once."""
    parts = PX.family(name, N, moved=X.moved if moved else None)
    return [dict(part=p, ref=PX.reference(p["verts"], p["p"])["brute"], em=PX.ExactTris(p["verts"])) for p in parts]


def check_part(renderer, name, d, what):
    part, ref = d["part"], d["ref"]
    dist, tri, c = query(renderer, part["p"])
    assert tri.dtype == np.int32 and dist.dtype == f32 and c.dtype == f32 and c.shape == (len(tri), 3)
    assert np.array_equal(tri, ref["tri"]), (name, part["mesh"], what, np.nonzero(tri != ref["tri"])[0][:8])
    assert same_floats(dist, ref["dist"]), (name, part["mesh"], what)
    assert same_floats(c, ref["c"]), (name, part["mesh"], what)
    ok = PX.check(d["em"], part["p"], tri, dist, c)
    assert ok.all(), (name, part["mesh"], what, "outside the contract", np.nonzero(~ok)[0][:8])
    st = renderer.point_query_stats()
    assert (st["points"], st["invalid_points"], st["stack_overflow"], st["launches"]) == (len(tri), 0, 0, 1) and st["ms"] > 0


# ---- 1. every family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PX.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, name):
    for d in family_data(name):
        set_mesh(renderer, d["part"]["verts"])
        check_part(renderer, name, d, "host")
    if name == "f":  # every triangle twice: the first copy
        assert (family_data("f")[0]["ref"]["tri"] < len(PX.mesh("soup_dup")) // 2).all()


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, name):
    for d, dm in zip(family_data(name), family_data(name, True)):
        v = d["part"]["verts"]
        a, e = PX.surface(v)
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_part(renderer, name, d, "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_part(renderer, name, d, "device build")
        renderer.refit_mesh_device(tdev(dm["part"]["verts"]))
        check_part(renderer, name, dm, "refit to moved vertices")


# ---- 2. one batch on the soup ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soup_batch():
    """4 000 points about the 2 000-triangle soup - in its inflated box, on it, just off it, far from it - and the brute-force answers."""
    v = PX.mesh("soup")
    rng = np.random.default_rng(7)
    on, tri = X._targets(rng, v, 1000, "iev")
    off = on.astype(np.float64) + PX._normals(v, tri) * (rng.choice([-1.0, 1.0], 1000) * np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), 1000)))[:, None]
    p = np.concatenate([PX._in_box(rng, v, 1500), on, off.astype(f32), PX._far(rng, v, 500)]).astype(f32)
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    ref = PX.reference(v, p)["brute"]
    assert (ref["tri"] >= 0).all()
    return dict(v=v, p=p, ref=ref, reach=PX.reach_of(v))


def set_soup(renderer):
    b = soup_batch()
    set_mesh(renderer, b["v"])
    return b


def assert_answers(got, ref, sel=slice(None), what=None):
    dist, tri, c = got
    assert np.array_equal(tri, ref["tri"][sel]), (what, np.nonzero(tri != ref["tri"][sel])[0][:8])
    assert same_floats(dist, ref["dist"][sel]), what
    if c is not None:
        assert same_floats(c, ref["c"][sel]), what


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 1 000 points every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not."""
    b = set_soup(renderer)
    for kw in TUNINGS:
        assert_answers(query(renderer, b["p"][:n], **kw), b["ref"], slice(0, n), (n, kw))
        st = renderer.point_query_stats()
        assert (st["points"], st["stack_overflow"]) == (n, 0)


def test_more_points_than_lanes(renderer):
    import torch

    b = set_soup(renderer)
    n = 600000
    assert n > 256 * 8 * 256
    perm = torch.from_numpy(((np.arange(n, dtype=np.int64) * 2654435761) % N)).to(dev())  # a fixed scatter of the 4 000 points
    p = tdev(b["p"])[perm].contiguous()
    dist, tri, c = renderer.query_points(p)
    st = renderer.point_query_stats()
    assert (st["points"], st["invalid_points"], st["stack_overflow"]) == (n, 0, 0)
    spot = np.arange(0, n, n // N)[:N]  # 4 000 of them against the reference
    src = perm.cpu().numpy()[spot]
    assert_answers((dist.cpu().numpy()[spot], tri.cpu().numpy()[spot], c.cpu().numpy()[spot]), b["ref"], src)
    # and all of them against the batch's own answers
    assert torch.equal(tri, tdev(b["ref"]["tri"])[perm]) and torch.equal(dist.view(torch.int32), tdev(b["ref"]["dist"]).view(torch.int32)[perm])


def test_distance_limits(renderer):
    b = set_soup(renderer)
    ref = b["ref"]
    d = ref["dist"]
    kind = np.arange(N) % 7
    rng = np.random.default_rng(41)
    rmax = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                     [d, np.nextafter(d, INF), f32(0.5) * d, np.full(N, INF), np.zeros(N, f32), np.full(N, f32(-1))],
                     (d * rng.uniform(0.5, 1.5, N)).astype(f32)).astype(f32)
    rmax[6] = f32(1e-30)  # its square underflows to 0: nothing is nearer
    within = (ref["d2"] < rmax * rmax) & (rmax > 0)  # rmax * rmax: one fp32 product
    pos = d > 0
    assert within[(kind == 1) & pos].all() and not within[(kind == 2) & pos].any() and within[kind == 3].all() and not within[(kind == 4) | (kind == 5)].any()
    assert within[kind == 6].any() and (~within)[kind == 6].any() and not within[6]
    exp = dict(tri=np.where(within, ref["tri"], MISS), dist=np.where(within, d, INF).astype(f32), c=np.where(within[:, None], ref["c"], f32(np.nan)).astype(f32))
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        assert_answers(query(renderer, b["p"], rmax, **kw), exp, what=kw)
        st = renderer.point_query_stats()
        assert (st["invalid_points"], st["stack_overflow"]) == (0, 0)
    ok = PX.check(PX.ExactTris(b["v"]), b["p"], exp["tri"], exp["dist"], exp["c"], rmax=np.where(rmax > 0, rmax, 0))
    assert ok.all(), np.nonzero(~ok)[0][:8]


def test_invalid_points(renderer):
    b = set_soup(renderer)
    ref, reach = b["ref"], b["reach"]
    rng = np.random.default_rng(43)
    where = rng.permutation(N)
    p, rmax = b["p"].copy(), np.full(N, INF, f32)
    invalid = np.zeros(N, bool)
    k = 0
    for comp in range(3):  # a NaN or an infinity in one component
        for bad in (np.nan, np.inf, -np.inf):
            for _ in range(3):
                p[where[k], comp] = bad
                invalid[where[k]] = True
                k += 1
    for _ in range(9):
        rmax[where[k]] = np.nan
        invalid[where[k]] = True
        k += 1
    for comp in range(3):  # one step beyond the reach
        for sign in (1, -1):
            p[where[k], comp] = sign * np.nextafter(reach, INF)
            invalid[where[k]] = True
            k += 1
    edge = where[k:k + 12]  # exactly at it: valid
    for j, i in enumerate(edge):
        p[i, j % 3] = (1 if j % 2 else -1) * reach
    exp = PX.reference(b["v"], p, rmax)["brute"]
    assert np.array_equal(exp["tri"] == INVALID, invalid) and (exp["tri"][edge] >= 0).all()
    assert np.array_equal(exp["tri"][~invalid & ~np.isin(np.arange(N), edge)], ref["tri"][~invalid & ~np.isin(np.arange(N), edge)])
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        got = query(renderer, p, rmax, **kw)
        assert_answers(got, exp, what=kw)
        assert np.isnan(got[0][invalid]).all() and np.isnan(got[2][invalid]).all()
        assert renderer.point_query_stats()["invalid_points"] == invalid.sum()
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive
    p_bad = b["p"].copy()
    p_bad[:, 1] = np.nan
    dist, tri, c = query(renderer, p_bad, tune_max_blocks=1)
    assert (tri == INVALID).all() and np.isnan(dist).all() and np.isnan(c).all() and renderer.point_query_stats()["invalid_points"] == N
    p_bad = b["p"].copy()
    p_bad[:1024, 2] = -np.inf
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        dist, tri, c = query(renderer, p_bad, **kw)
        assert (tri[:1024] == INVALID).all(), kw
        assert_answers((dist[1024:], tri[1024:], c[1024:]), ref, slice(1024, None), kw)
        assert renderer.point_query_stats()["invalid_points"] == 1024


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest of the 7 per level in global memory."""
    for d in (family_data("a")[0], family_data("a")[3]):
        assert d["part"]["mesh"] in ("soup", "terrain")
        set_mesh(renderer, d["part"]["verts"])
        assert renderer.pt_stats()["bvh_depth"] > 1
        assert_answers(query(renderer, d["part"]["p"], tune_lds_stack=1), d["ref"])
        assert renderer.point_query_stats()["stack_overflow"] == 0


def test_pruning_happens(renderer):
    """Family b of the terrain: mean triangles tested per point <= n_tris / 8 (brute force: n_tris).  The cap is a condition, not a
    measurement: the CPU reference walk tests 6.8 per point on this input (test_point_query_host.py)."""
    d = family_data("b")[0]
    assert d["part"]["mesh"] == "terrain"
    set_mesh(renderer, d["part"]["verts"])
    n, n_tris = len(d["part"]["p"]), len(d["part"]["verts"])
    assert_answers(query(renderer, d["part"]["p"], count_traversal=True), d["ref"])
    st = renderer.point_query_stats()
    print(f"terrain, family b: {st['tris_tested'] / n:.2f} triangles and {st['nodes_visited'] / n:.2f} nodes per point ({n_tris} triangles)")
    assert st["stack_overflow"] == 0 and st["nodes_visited"] >= n
    assert 0 < st["tris_tested"] / n <= n_tris / 8
    query(renderer, d["part"]["p"][:100])
    st = renderer.point_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted


def test_bounds_and_out_tensors(renderer):
    import torch

    b = set_soup(renderer)
    for n in (1, 65, N):
        p, rm = tdev(b["p"][:n]), tdev(np.full(n, INF, f32))
        p0, rm0 = p.clone(), rm.clone()
        d_buf, t_buf, c_buf = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64), sentinel(n, torch.float32, 64, cols=3)
        dist, tri, c = renderer.query_points(p, rm, out=(d_buf[:n], t_buf[:n], c_buf[:n]))
        assert dist.data_ptr() == d_buf.data_ptr() and tri.data_ptr() == t_buf.data_ptr() and c.data_ptr() == c_buf.data_ptr()
        assert still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n) and still_sentinel(c_buf, 0, n)
        assert_answers((dist.cpu().numpy(), tri.cpu().numpy(), c.cpu().numpy()), b["ref"], slice(0, n))
        for x, x0 in ((p, p0), (rm, rm0)):
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
        # point_out = NULL
        d_buf.fill_(-7.0)
        t_buf.fill_(-7)
        dist, tri, none = renderer.query_points(p, out=(d_buf[:n], t_buf[:n]), want_points=False)
        assert none is None and still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n)
        assert_answers((dist.cpu().numpy(), tri.cpu().numpy(), None), b["ref"], slice(0, n))
    with pytest.raises(ValueError):
        renderer.query_points(p, out=(d_buf[:N], t_buf[:N - 1], c_buf[:N]))
    with pytest.raises(ValueError):
        renderer.query_points(p, out=(t_buf[:N], t_buf[:N], c_buf[:N]))


def test_stream_order(renderer):
    """Points made by torch on a stream, the query behind them on that stream without a host synchronisation, a torch reduction of the
    answers behind the query; one synchronisation at the end.  (Halving and doubling is exact: the points are the batch's bit for bit.)"""
    import torch

    b = set_soup(renderer)
    p_half = tdev(b["p"] * f32(0.5))
    ref_d, ref_t, ref_c = tdev(b["ref"]["dist"]).view(torch.int32), tdev(b["ref"]["tri"]), tdev(b["ref"]["c"]).view(torch.int32)
    dist, tri, c = sentinel(N, torch.float32), sentinel(N, torch.int32), sentinel(N, torch.float32, cols=3)
    with busy_stream(renderer):
        p = p_half * 2.0
        renderer.query_points(p, out=(dist, tri, c), sync=False)
        wrong = (dist.view(torch.int32) != ref_d).sum() + (tri != ref_t).sum() + (c.view(torch.int32) != ref_c).sum()
    assert int(wrong) == 0


def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_soup(renderer)
    n = 1000
    p = tdev(b["p"][:n])
    dist, tri, c = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3)
    fresh = R.Renderer(0)
    try:
        assert lib.rt_query_points_device(fresh._ctx, ptr(p), None, n, None, ptr(dist), ptr(tri), ptr(c)) == RT_ERR_STATE  # no mesh
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short3=12, short1=4)  # the allocation holds n - 1 rows from the short ones
    hp, big, short3, short1 = bp.hp, bp.big, bp.short3, bp.short1
    calls = [(None, None, n, None, ptr(dist), ptr(tri), ptr(c)), (ptr(p), None, n, None, None, ptr(tri), ptr(c)), (ptr(p), None, n, None, ptr(dist), None, ptr(c)),
             (hp, None, n, None, ptr(dist), ptr(tri), ptr(c)), (ptr(p), hp, n, None, ptr(dist), ptr(tri), ptr(c)), (ptr(p), None, n, None, hp, ptr(tri), ptr(c)),
             (ptr(p), None, n, None, ptr(dist), hp, ptr(c)), (ptr(p), None, n, None, ptr(dist), ptr(tri), hp),
             (short3, None, n, None, ptr(dist), ptr(tri), ptr(c)), (ptr(p), short1, n, None, ptr(dist), ptr(tri), ptr(c)),
             (ptr(p), None, n, None, short1, ptr(tri), ptr(c)), (ptr(p), None, n, None, ptr(dist), short1, ptr(c)), (ptr(p), None, n, None, ptr(dist), ptr(tri), short3),
             (ptr(p), None, (1 << 30) + 1, None, ptr(dist), ptr(tri), ptr(c))] + [(ptr(p), None, n, prm, ptr(dist), ptr(tri), ptr(c)) for prm in bad_params(R.PointQueryParams)]
    for k, args in enumerate(calls):
        assert lib.rt_query_points_device(ctx, *args) == RT_ERR_INVALID, k
        assert_untouched(renderer, (dist, tri, c), big, k)
    assert lib.rt_query_points_device(ctx, ptr(p), None, 0, None, ptr(dist), ptr(tri), ptr(c)) == 0  # n = 0 is accepted, and does nothing
    assert lib.rt_query_points_device(ctx, None, None, 0, None, None, None, None) == 0
    renderer.synchronize()
    assert still_sentinel(dist) and still_sentinel(tri) and still_sentinel(c)
    e = renderer.query_points(p[:0])
    assert len(e[0]) == 0 and len(e[1]) == 0 and len(e[2]) == 0
    # the context still answers
    got = renderer.query_points(p, out=(dist, tri, c))
    assert_answers(tuple(x.cpu().numpy() for x in got), b["ref"], slice(0, n))


def test_ray_and_point_stats_do_not_mix(renderer):
    """Each query kind keeps its own counters until somebody reads them: a ray query's survive a later point query, and the other way
    round, and neither query's answers depend on what ran before it."""
    b = set_soup(renderer)
    parts = X.family("a")
    o, d = np.concatenate([p["o"] for p in parts]).copy(), np.concatenate([p["d"] for p in parts])
    assert len(o) == N
    rng = np.random.default_rng(47)
    bad_rays = rng.permutation(N)[:100]
    o[bad_rays, np.arange(100) % 3] = np.array([np.nan, np.inf, -np.inf], f32)[np.arange(100) % 3]
    p = b["p"].copy()
    p[rng.permutation(N)[:300], 0] = np.nan
    to, td, tp = tdev(o), tdev(d), tdev(p)

    def rays():
        t, tri = renderer.query_rays(to, td)
        return t.cpu().numpy(), tri.cpu().numpy()

    def points():
        return tuple(x.cpu().numpy() for x in renderer.query_points(tp, count_traversal=True))

    rays_alone, points_alone = rays(), points()
    assert (rays_alone[1][bad_rays] == INVALID).all() and (rays_alone[1] == INVALID).sum() == 100 and (points_alone[1] == INVALID).sum() == 300
    for first, second in ((rays, points), (points, rays)):
        got = {first: first(), second: second()}
        rs, ps = renderer.ray_query_stats(), renderer.point_query_stats()  # only now
        assert (rs["invalid_rays"], rs["rays"]) == (100, N), rs
        assert (ps["invalid_points"], ps["points"]) == (300, N) and ps["nodes_visited"] > 0, ps
        assert rs["ms"] > 0 and ps["ms"] > 0
        assert all(same_floats(x, y) for x, y in zip(got[rays], rays_alone)), first.__name__
        assert all(same_floats(x, y) for x, y in zip(got[points], points_alone)), first.__name__
        assert np.array_equal(got[rays][1], rays_alone[1]) and np.array_equal(got[points][1], points_alone[1])


def test_queries_leave_two_stream_frames_alone(renderer):
    """tune_no_overlap = 2: the shadow kernel runs beside the next closest-hit kernel on the second half of the spill columns - the one
    path that reads where that half begins.  Queries that size the columns for themselves in between must not move the frame.  With the
    default ten LDS entries this small tree never spills, so the same is asked of frames with one LDS entry, which do use both halves."""
    b = set_soup(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3), tune_no_overlap=2)
    parts = X.family("a")
    o, d = np.concatenate([p["o"] for p in parts]), np.concatenate([p["d"] for p in parts])

    def frame(**more):
        return pt_frame(renderer, **kw, **more)

    before, before_spilling = frame(), frame(tune_lds_stack=1)
    assert before[1][1] > 0 and before[1][2] > 0 and before[1][3] == 0
    assert renderer.pt_stats()["bvh_depth"] > 1  # one LDS entry is not the whole stack
    assert np.array_equal(before[0], before_spilling[0]) and before[1] == before_spilling[1]
    assert_answers(query(renderer, b["p"], tune_lds_stack=1), b["ref"])
    renderer.query_rays(tdev(o), tdev(d), tune_lds_stack=1)
    assert renderer.ray_query_stats()["stack_overflow"] == 0
    after, after_spilling = frame(), frame(tune_lds_stack=1)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before[0], after_spilling[0]) and before[1] == after_spilling[1]


def test_rendering_and_sharing_are_undisturbed(renderer):
    b = set_soup(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r):
        return pt_frame(r, **kw)

    before = frame(renderer)
    assert before[1][1] > 0 and before[1][2] > 0
    assert_answers(query(renderer, b["p"], tune_lds_stack=1), b["ref"])
    after = frame(renderer)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    # a shared mesh stays shared: the query only reads it
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        assert_answers(query(other, b["p"]), b["ref"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()
