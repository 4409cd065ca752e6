"""Clearance queries on device tensors (Renderer.query_clearance / rt_query_clearance_device) on the GPU.

Two references, both from tests/clearance_exact.py: the native brute force over all triangles (tests/native/clearance_query_ref.cpp, the
arithmetic of csrc/tri_dist.h without a tree), which the kernel must match bit for bit in tri, dist and both points, and the float64
contract, which its answers must satisfy on their own.  The first tests run every family on its own meshes; the others use one batch:
the 600 query triangles of soup_batch() against the 2 000-triangle soup.  A distance limit needs no tolerance: the answer is defined as
the (d2, index)-minimal triangle, so "hit when d2 < rmax * rmax" is decided by the reference's own d2."""
import functools

import numpy as np
import pytest

import clearance_exact as CX
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, dev, pt_frame, ptr, same_floats, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_px_surface as set_mesh

pytestmark = pytest.mark.gpu

PX, OX = CX.PX, CX.OX
f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = -1, -2
N = 600


def query(renderer, q, rmax=None, **kw):
    """Numpy in, numpy out, through device tensors: (dist, tri, point_query, point_mesh)."""
    got = renderer.query_clearance(tdev(q), None if rmax is None else tdev(rmax), **kw)
    return tuple(None if x is None else x.cpu().numpy() for x in got)


def assert_answers(got, ref, sel=slice(None), what=None):
    dist, tri, pq, pm = got
    assert np.array_equal(tri, ref["tri"][sel]), (what, np.nonzero(tri != ref["tri"][sel])[0][:8])
    assert same_floats(dist, ref["dist"][sel]), what
    if pq is not None:
        assert same_floats(pq, ref["pq"][sel]), what
    if pm is not None:
        assert same_floats(pm, ref["pm"][sel]), what


def check_case(renderer, name, c, ex, what):
    got = query(renderer, c["q"], c.get("rmax"))
    dist, tri, pq, pm = got
    assert tri.dtype == np.int32 and dist.dtype == f32 and pq.dtype == f32 and pq.shape == (len(tri), 3) and pm.shape == (len(tri), 3)
    assert_answers(got, c["ref"]["brute"], what=(name, c["mesh"], what))
    if ex is not None:
        ok = CX.check(ex, tri, dist, pq, pm)
        assert ok.all(), (name, c["mesh"], what, "outside the contract", np.nonzero(~ok)[0][:8])
    st = renderer.clearance_query_stats()
    assert (st["queries"], st["invalid_triangles"], st["stack_overflow"]) == (len(tri), int((c["ref"]["brute"]["tri"] == INVALID).sum()), 0) and st["ms"] > 0


# ---- 1. every family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CX.FAMILIES + ("h",))
def test_every_family_on_the_host_built_tree(renderer, name):
    exact = CX.family_exact(name) if name != "h" else [None] * 2
    for c, ex in zip(CX.family_case(name), exact):
        set_mesh(renderer, c["verts"])
        check_case(renderer, name, c, ex, "host")
    if name == "b":
        assert all((c["ref"]["brute"]["dist"] == 0).all() for c in CX.family_case("b"))
    if name == "f":  # every triangle twice: the first copy
        assert (CX.family_case("f")[0]["ref"]["brute"]["tri"] < 1000).all()
    if name == "h":
        assert all((c["ref"]["brute"]["tri"] == INVALID).sum() == 34 for c in CX.family_case("h"))


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, name):
    for c, cm, ex in zip(CX.family_case(name), CX.family_case(name, True), CX.family_exact(name)):
        v = c["verts"]
        a, e = PX.surface(v)
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_case(renderer, name, c, ex, "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_case(renderer, name, c, ex, "device build")
        renderer.refit_mesh_device(tdev(cm["verts"]))
        check_case(renderer, name, cm, None, "refit to moved vertices")


# ---- 2. one batch on the soup ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soup_batch():
    """600 query triangles about the 2 000-triangle soup - its own triangles displaced by 0.05, 1 and 5 of their size, planted through
    it, and far from it - and the brute-force answers."""
    v = PX.mesh("soup")
    rng = np.random.default_rng(11)
    q = np.concatenate([OX._displaced(rng, v, 130, 0.05), OX._displaced(rng, v, 130, 1.0), OX._displaced(rng, v, 130, 5.0), OX._planted(rng, v, 110), CX._far(rng, v, 100)])
    q = np.ascontiguousarray(q[rng.permutation(len(q))], f32)
    assert len(q) == N
    ref = CX.reference(v, q)
    assert (ref["brute"]["tri"] >= 0).all() and CX.walk_is_brute(ref)
    return dict(v=v, q=q, ref=ref["brute"], walk=ref, reach=PX.reach_of(v))


def set_soup(renderer):
    b = soup_batch()
    set_mesh(renderer, b["v"])
    return b


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 600, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 600 triangles every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not; beyond the batch's 600 its triangles repeat (no new geometry: these sizes are about the queue's streams),
    each against its own brute-force answer."""
    b = set_soup(renderer)
    sel = np.arange(n) % N
    for kw in TUNINGS:
        assert_answers(query(renderer, np.ascontiguousarray(b["q"][sel]), **kw), b["ref"], sel, (n, kw))
        st = renderer.clearance_query_stats()
        assert (st["queries"], st["stack_overflow"]) == (n, 0)


@pytest.mark.parametrize("n_tris", [1, 8, 9])
def test_tiny_meshes(renderer, n_tris):
    """A root that is all leaves (1, 8) and the smallest tree with an inner child (9)."""
    b = soup_batch()
    v = np.ascontiguousarray(b["v"][:n_tris])
    q = b["q"][:120]
    ref = CX.reference(v, q)
    assert CX.walk_is_brute(ref)
    set_mesh(renderer, v)
    assert_answers(query(renderer, q), ref["brute"], what=n_tris)
    assert (ref["brute"]["tri"] < n_tris).all()


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest of the 7 per level in global memory."""
    for c in (CX.family_case("a")[0], CX.family_case("a")[3]):
        assert c["mesh"] in ("soup", "terrain")
        set_mesh(renderer, c["verts"])
        assert renderer.pt_stats()["bvh_depth"] > 1
        assert_answers(query(renderer, c["q"], tune_lds_stack=1), c["ref"]["brute"])
        assert renderer.clearance_query_stats()["stack_overflow"] == 0


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
    nan3 = np.full((N, 3), np.nan, f32)
    exp = dict(tri=np.where(within, ref["tri"], MISS), dist=np.where(within, d, INF).astype(f32), pq=np.where(within[:, None], ref["pq"], nan3),
               pm=np.where(within[:, None], ref["pm"], nan3))
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        assert_answers(query(renderer, b["q"], rmax, **kw), exp, what=kw)
        st = renderer.clearance_query_stats()
        assert (st["invalid_triangles"], st["stack_overflow"]) == (0, 0)
    ok = CX.check(CX.Exact(b["v"], b["q"]), exp["tri"], exp["dist"], exp["pq"], exp["pm"], rmax=np.where(rmax > 0, rmax, 0))
    assert ok.all(), np.nonzero(~ok)[0][:8]


def test_invalid_queries_in_front_of_valid_ones(renderer):
    """1 024 invalid query triangles in front of valid ones: refills that hand out 64 entries and leave no lane alive."""
    b = set_soup(renderer)
    bad = np.tile(b["q"], (2, 1))[:1024].copy()
    bad[:, 5] = np.array([np.nan, np.inf, -np.inf, 2 * float(b["reach"])], f32)[np.arange(1024) % 4]
    q = np.concatenate([bad, b["q"]])
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        dist, tri, pq, pm = query(renderer, q, **kw)
        assert (tri[:1024] == INVALID).all() and np.isnan(dist[:1024]).all() and np.isnan(pq[:1024]).all() and np.isnan(pm[:1024]).all(), kw
        assert_answers((dist[1024:], tri[1024:], pq[1024:], pm[1024:]), b["ref"], what=kw)
        st = renderer.clearance_query_stats()
        assert (st["queries"], st["invalid_triangles"]) == (1024 + N, 1024)
    rmax = np.full(N, INF, f32)
    rmax[::5] = np.nan
    dist, tri, pq, pm = query(renderer, b["q"], rmax)
    assert (tri[::5] == INVALID).all() and np.isnan(dist[::5]).all() and renderer.clearance_query_stats()["invalid_triangles"] == len(rmax[::5])


def test_pruning_happens(renderer):
    """Family a of the terrain: mean records fetched per query <= n_tris / 8 = 144 (brute force: 1 154) on the kernel's own counter, and
    the reference walk's counts beside it.  The cap is a condition, not a measurement."""
    c = CX.family_case("a")[3]
    assert c["mesh"] == "terrain"
    set_mesh(renderer, c["verts"])
    n, n_tris = len(c["q"]), len(c["verts"])
    assert_answers(query(renderer, c["q"], count_traversal=True), c["ref"]["brute"])
    st = renderer.clearance_query_stats()
    print(f"terrain, family a: {st['tris_tested'] / n:.2f} records and {st['nodes_visited'] / n:.2f} nodes per query ({n_tris} triangles); "
          f"reference walk {c['ref']['tris_total'] / n:.2f} and {c['ref']['nodes_total'] / n:.2f}")
    assert st["stack_overflow"] == 0 and st["nodes_visited"] >= n
    assert n_tris // 8 == 144 and 0 < st["tris_tested"] / n <= 144
    query(renderer, c["q"][:100])
    st = renderer.clearance_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted


def test_bounds_and_out_tensors(renderer):
    import torch

    b = set_soup(renderer)
    for n in (1, 65, N):
        q, rm = tdev(b["q"][:n]), tdev(np.full(n, INF, f32))
        q0, rm0 = q.clone(), rm.clone()
        d_buf, t_buf = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64)
        a_buf, c_buf = sentinel(n, torch.float32, 64, cols=3), sentinel(n, torch.float32, 64, cols=3)
        dist, tri, pq, pm = renderer.query_clearance(q.view(n, 3, 3), rm, out=(d_buf[:n], t_buf[:n], a_buf[:n], c_buf[:n]))
        assert dist.data_ptr() == d_buf.data_ptr() and tri.data_ptr() == t_buf.data_ptr() and pq.data_ptr() == a_buf.data_ptr() and pm.data_ptr() == c_buf.data_ptr()
        assert still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n) and still_sentinel(a_buf, 0, n) and still_sentinel(c_buf, 0, n)
        assert_answers(tuple(x.cpu().numpy() for x in (dist, tri, pq, pm)), b["ref"], slice(0, n))
        for x, x0 in ((q, q0), (rm, rm0)):
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
        # both point outputs NULL
        d_buf.fill_(-7.0)
        t_buf.fill_(-7)
        dist, tri, none_q, none_m = renderer.query_clearance(q, out=(d_buf[:n], t_buf[:n]), want_points=False)
        assert none_q is None and none_m is None and still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n)
        assert_answers((dist.cpu().numpy(), tri.cpu().numpy(), None, None), b["ref"], slice(0, n))
        # each point output NULL in turn, through the library
        lib = R.load()
        for keep_query in (True, False):
            for buf in (d_buf, t_buf, a_buf, c_buf):
                buf.fill_(-7)
            torch.cuda.synchronize()
            assert lib.rt_query_clearance_device(renderer._ctx, ptr(q), None, n, None, ptr(t_buf), ptr(d_buf), ptr(a_buf) if keep_query else None,
                                                 None if keep_query else ptr(c_buf)) == 0
            renderer.synchronize()
            kept, left = (a_buf, c_buf) if keep_query else (c_buf, a_buf)
            assert still_sentinel(left) and still_sentinel(kept, 0, n) and still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n)
            assert_answers((d_buf[:n].cpu().numpy(), t_buf[:n].cpu().numpy(), a_buf[:n].cpu().numpy() if keep_query else None,
                            None if keep_query else c_buf[:n].cpu().numpy()), b["ref"], slice(0, n))
    with pytest.raises(ValueError):
        renderer.query_clearance(q, out=(d_buf[:N], t_buf[:N - 1], a_buf[:N], c_buf[:N]))
    with pytest.raises(ValueError):
        renderer.query_clearance(q, out=(t_buf[:N], t_buf[:N], a_buf[:N], c_buf[:N]))


def test_stream_order_behind_a_refit(renderer):
    """A refit and the query behind it on one stream, without a host synchronisation in between; one synchronisation at the end.  The
    answers are the moved mesh's."""
    import torch

    c, cm = CX.family_case("a")[0], CX.family_case("a", True)[0]
    v = c["verts"]
    a, e = PX.surface(v)
    renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
    q, moved = tdev(cm["q"]), tdev(cm["verts"])
    n = len(cm["q"])
    ref = cm["ref"]["brute"]
    assert not np.array_equal(ref["dist"], CX.reference(v, cm["q"])["brute"]["dist"])  # the unmoved mesh answers otherwise
    ref_d, ref_t, ref_q, ref_m = tdev(ref["dist"]).view(torch.int32), tdev(ref["tri"]), tdev(ref["pq"]).view(torch.int32), tdev(ref["pm"]).view(torch.int32)
    dist, tri, pq, pm = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3), sentinel(n, torch.float32, cols=3)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    renderer.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            renderer.refit_mesh_device(moved)
            renderer.query_clearance(q, out=(dist, tri, pq, pm), sync=False)
            wrong = (dist.view(torch.int32) != ref_d).sum() + (tri != ref_t).sum() + (pq.view(torch.int32) != ref_q).sum() + (pm.view(torch.int32) != ref_m).sum()
        s.synchronize()
        assert int(wrong) == 0
    finally:
        renderer.synchronize()
        renderer.set_stream(None)


def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_soup(renderer)
    n = 500
    q = tdev(b["q"][:n])
    dist, tri, pq, pm = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3), sentinel(n, torch.float32, cols=3)
    good = (ptr(q), None, n, None, ptr(tri), ptr(dist), ptr(pq), ptr(pm))
    fresh = R.Renderer(0)
    try:
        assert lib.rt_query_clearance_device(fresh._ctx, *good) == RT_ERR_STATE  # no mesh
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short9=36, short3=12, short1=4)  # n - 1 rows from the short ones
    hp, big, short9, short3, short1 = bp.hp, bp.big, bp.short9, bp.short3, bp.short1

    def with_arg(k, value):
        args = list(good)
        args[k] = value
        return tuple(args)

    calls = [with_arg(0, None), with_arg(4, None), with_arg(5, None),  # NULL where a pointer is due
             with_arg(0, hp), with_arg(1, hp), with_arg(4, hp), with_arg(5, hp), with_arg(6, hp), with_arg(7, hp),  # host memory
             with_arg(0, short9), with_arg(1, short1), with_arg(4, short1), with_arg(5, short1), with_arg(6, short3), with_arg(7, short3),  # too short
             with_arg(2, (1 << 30) + 1)] + [with_arg(3, prm) for prm in bad_params(R.ClearanceQueryParams)]
    for k, args in enumerate(calls):
        assert lib.rt_query_clearance_device(ctx, *args) == RT_ERR_INVALID, k
        assert_untouched(renderer, (dist, tri, pq, pm), big, k)
    assert lib.rt_query_clearance_device(ctx, *with_arg(2, 0)) == 0  # n = 0 is accepted, and does nothing
    assert lib.rt_query_clearance_device(ctx, None, None, 0, None, None, None, None, None) == 0
    renderer.synchronize()
    assert still_sentinel(dist) and still_sentinel(tri) and still_sentinel(pq) and still_sentinel(pm)
    e = renderer.query_clearance(q[:0])
    assert all(len(x) == 0 for x in e)
    # a mesh beyond the domain is refused too, and the context still answers afterwards
    far = (b["v"] * f32(2.0 ** 21)).astype(f32)
    set_mesh(renderer, far)
    assert lib.rt_query_clearance_device(ctx, *good) == RT_ERR_INVALID
    renderer.synchronize()
    assert still_sentinel(dist) and still_sentinel(tri)
    set_mesh(renderer, b["v"])
    got = renderer.query_clearance(q, out=(dist, tri, pq, pm))
    assert_answers(tuple(x.cpu().numpy() for x in got), b["ref"], slice(0, n))


def test_rendering_and_sharing_are_undisturbed(renderer):
    """A path B frame and its ray counts are bit-equal before and after a query, and a shared mesh stays shared: the query only reads it."""
    b = set_soup(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r):
        return pt_frame(r, **kw)

    before = frame(renderer)
    assert before[1][1] > 0 and before[1][2] > 0
    assert_answers(query(renderer, b["q"], tune_lds_stack=1), b["ref"])
    after = frame(renderer)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        assert_answers(query(other, b["q"]), b["ref"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()


def test_the_vertices_alone_are_not_the_answer(renderer):
    """What a caller could do before: three query_points batches on the vertices give an upper bound.  It is never below dist (beyond the
    roundings of two different evaluations), and for edge - edge and mesh-vertex - face pairs it is strictly above: the case the
    feature exists for."""
    above = 0
    for c, ex in zip(CX.family_case("a")[:4], CX.family_exact("a")[:4]):
        set_mesh(renderer, c["verts"])
        dist = query(renderer, c["q"], want_points=False)[0].astype(np.float64)
        corners = c["q"].reshape(-1, 3)
        by_vertex = renderer.query_points(tdev(corners), want_points=False)[0].cpu().numpy().astype(np.float64).reshape(-1, 3).min(1)
        assert (by_vertex >= dist - 2 * CX.KC * ex.unit).all(), c["mesh"]
        above += int((by_vertex > dist + 2 * CX.KC * ex.unit).sum())
    print(f"the three vertices overestimate the clearance of {above} of the {4 * 150} query triangles")
    assert above >= 1
