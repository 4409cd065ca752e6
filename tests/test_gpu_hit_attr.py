"""Hit attributes on device tensors (Renderer.query_rays / query_points with attributes=True, rt_query_rays_attr_device /
rt_query_points_attr_device) on the GPU.

The reference is native and tree-free: tests/native/hit_attr_ref.cpp (csrc/hit_attr.h over all triangles) for rays and for the normals
of points' winners, tests/native/point_query_ref.cpp for the points' (u, v).  The kernels must give its (t, tri, uv, normal) resp.
(dist, tri, point, uv, normal) bit for bit, and their t, tri resp. dist, tri, point must be the plain queries' on the same inputs bit for
bit.  Meshes, families and batches are those of tests/test_gpu_ray_query.py and tests/test_gpu_point_query.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import attr_exact as AX
import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
import test_gpu_point_query as TP
import test_gpu_ray_query as TR
from gpu_query import RT_ERR_INVALID, bad_pointers, busy_stream, pt_frame, ptr, same_floats, sentinel, still_sentinel, tdev  # same_floats: bit-equal, NaN for NaN

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = -1, -2
N = 4000
NS = [1, 63, 64, 65, 255, 256, 257, 4000]
REFILLS = [1, 24, 64]


def cpu(xs):
    return tuple(None if x is None else x.cpu().numpy() for x in xs)


def ray_attr(renderer, o, d, tmax=None, **kw):
    return cpu(renderer.query_rays(tdev(o), tdev(d), None if tmax is None else tdev(tmax), attributes=True, **kw))


def point_attr(renderer, p, rmax=None, **kw):
    return cpu(renderer.query_points(tdev(p), None if rmax is None else tdev(rmax), attributes=True, **kw))


def point_normals(verts, tri):
    """hit_attr.h's unit normals of the triangles tri (NaN rows for tri < 0), from the native reference."""
    return AX.reference(verts, np.zeros((0, 3), f32), np.zeros((0, 3), f32), tris=tri)["tri_normals"]


def assert_ray_answers(got, ref, sel=slice(None), what=None):
    t, tri, uv, nrm = got
    assert tri.dtype == np.int32 and uv.shape == (len(tri), 2) and nrm.shape == (len(tri), 3) and uv.dtype == f32 and nrm.dtype == f32
    assert np.array_equal(tri, ref["tri"][sel]), (what, np.nonzero(tri != ref["tri"][sel])[0][:8])
    assert same_floats(t, ref["t"][sel]), what
    assert same_floats(uv[:, 0], ref["ub"][sel]) and same_floats(uv[:, 1], ref["vb"][sel]), what
    assert same_floats(nrm, ref["normal"][sel]), what
    miss = tri < 0
    assert np.isnan(uv[miss]).all() and np.isnan(nrm[miss]).all() and np.isfinite(uv[~miss]).all() and np.isfinite(nrm[~miss]).all(), what


def assert_point_answers(got, ref, sel=slice(None), what=None):
    dist, tri, c, uv, nrm = got
    assert np.array_equal(tri, ref["tri"][sel]), (what, np.nonzero(tri != ref["tri"][sel])[0][:8])
    assert same_floats(dist, ref["dist"][sel]), what
    if c is not None:
        assert same_floats(c, ref["c"][sel]), what
    assert same_floats(uv[:, 0], ref["u"][sel]) and same_floats(uv[:, 1], ref["v"][sel]), what
    assert same_floats(nrm, ref["normal"][sel]), what
    miss = tri < 0
    assert np.isnan(uv[miss]).all() and np.isnan(nrm[miss]).all() and np.isfinite(uv[~miss]).all() and np.isfinite(nrm[~miss]).all(), what


# ---- 1. every family, every tree -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ray_family(name, moved=False):
    """[dict(part, verts, ref)] of one ray family: the native reference on the part's mesh, or on its moved vertices; computed once."""
    out = []
    for part in X.family(name, N):
        v = X.mesh(part["mesh"])[0]
        v = X.moved(v) if moved else v
        out.append(dict(part=part, verts=v, ref=AX.reference(v, part["o"], part["d"])))
    return out


@functools.lru_cache(maxsize=None)
def point_family(name, moved=False):
    """[dict(part, ref)] of one point family: point_query_ref's brute force with the winners' normals added; computed once."""
    out = []
    for d in TP.family_data(name, moved):
        ref = dict(d["ref"])
        ref["normal"] = point_normals(d["part"]["verts"], ref["tri"])
        out.append(dict(part=d["part"], ref=ref))
    return out


def check_rays(renderer, d, what):
    part, ref = d["part"], d["ref"]
    got = ray_attr(renderer, part["o"], part["d"])
    assert_ray_answers(got, ref, what=(part["mesh"], what))
    st = renderer.ray_query_stats()
    assert (st["rays"], st["invalid_rays"], st["stack_overflow"], st["launches"]) == (len(part["o"]), 0, 0, 1) and st["ms"] > 0
    t, tri = TR.query(renderer, part["o"], part["d"])  # the plain query on the same inputs
    assert np.array_equal(tri, got[1]) and same_floats(t, got[0]), (part["mesh"], what)


def check_points(renderer, d, what):
    part, ref = d["part"], d["ref"]
    got = point_attr(renderer, part["p"])
    assert_point_answers(got, ref, what=(part["mesh"], what))
    st = renderer.point_query_stats()
    assert (st["points"], st["invalid_points"], st["stack_overflow"], st["launches"]) == (len(part["p"]), 0, 0, 1) and st["ms"] > 0
    dist, tri, c = TP.query(renderer, part["p"])
    assert np.array_equal(tri, got[1]) and same_floats(dist, got[0]) and same_floats(c, got[2]), (part["mesh"], what)


@pytest.mark.parametrize("name", X.FAMILIES)
def test_every_ray_family_on_the_host_built_tree(renderer, name):
    hits = 0
    for d in ray_family(name):
        renderer.set_mesh(*X.mesh(d["part"]["mesh"]))
        check_rays(renderer, d, "host")
        hits += int((d["ref"]["tri"] >= 0).sum())
    assert hits > N // 4


@pytest.mark.parametrize("name", PX.FAMILIES)
def test_every_point_family_on_the_host_built_tree(renderer, name):
    for d in point_family(name):
        TP.set_mesh(renderer, d["part"]["verts"])
        check_points(renderer, d, "host")
    if name == "g":  # the needle mesh: winners without area have zero normals, the others unit ones
        ref = point_family("g")[0]["ref"]
        flat = np.isin(ref["tri"], (6, 9))
        assert flat.any() and (~flat).any() and (ref["normal"][flat] == 0).all() and (np.abs((ref["normal"][~flat].astype(np.float64) ** 2).sum(1) - 1) <= 2.0 ** -21).all()


@pytest.mark.parametrize("name", ["a", "h"])
def test_rays_on_two_level_device_built_and_refitted_trees(renderer, name):
    for d, dm in zip(ray_family(name), ray_family(name, True)):
        v, a, e = X.mesh(d["part"]["mesh"])
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_rays(renderer, d, "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_rays(renderer, d, "device build")
        renderer.refit_mesh_device(tdev(dm["verts"]))
        check_rays(renderer, dm, "refit to moved vertices")
        # the moved mesh's normals are not the old ones: wherever both meshes are hit in the same triangle they differ
        both = (d["ref"]["tri"] >= 0) & (d["ref"]["tri"] == dm["ref"]["tri"])
        changed = (d["ref"]["normal"][both].view(np.uint32) != dm["ref"]["normal"][both].view(np.uint32)).any(1)
        assert both.sum() > 100 and changed.mean() > 0.9


def test_points_on_two_level_device_built_and_refitted_trees(renderer):
    for d, dm in zip(point_family("a"), point_family("a", True)):
        v = d["part"]["verts"]
        a, e = PX.surface(v)
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_points(renderer, d, "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_points(renderer, d, "device build")
        renderer.refit_mesh_device(tdev(dm["part"]["verts"]))
        check_points(renderer, dm, "refit to moved vertices")


# ---- 2. the sink under refill pressure -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed_rays():
    """The soup batch of test_gpu_ray_query.py with trouble mixed in: 1 024 invalid rays in front, every ninth ray behind them invalid
    too, and per-ray limits - none, at t, one ulp above t, half of t, 0, -1, in turn.  Rays 1 024 .. 1 024 + n are the small batches.
    The reference knows validity and limits: its answers are the expectation."""
    b = TR.soup_batch()
    o, d = b["o"].copy(), b["d"].copy()
    o[:1024, 2] = -np.inf
    k = np.arange(N)
    o[(k >= 1024) & (k % 9 == 4), 0] = np.nan
    d[(k >= 1024) & (k % 9 == 7), 1] = np.inf
    t = b["t"]
    tmax = np.select([k % 6 == 0, k % 6 == 1, k % 6 == 2, k % 6 == 3, k % 6 == 4], [np.full(N, INF), t, np.nextafter(t, INF), f32(0.5) * t, np.zeros(N, f32)], f32(-1)).astype(f32)
    ref = AX.reference(X.mesh("soup")[0], o, d, tmax)
    valid = ref["tri"] != INVALID
    hit0 = valid & (b["tri"] >= 0)
    assert (ref["tri"][:1024] == INVALID).all() and 300 < (~valid[1024:]).sum() < 900
    assert (ref["tri"][hit0 & (k % 6 == 1)] == MISS).all() and (ref["tri"][hit0 & (k % 6 == 3)] == MISS).all()  # cut off by the limit: a miss, NaN attributes
    assert np.array_equal(ref["tri"][hit0 & (k % 6 == 2)], b["tri"][hit0 & (k % 6 == 2)]) and (hit0 & (k % 6 == 2)).sum() > 100
    assert (ref["tri"][valid & (k % 6 >= 4)] == MISS).all() and np.isnan(ref["ub"][ref["tri"] < 0]).all()
    return dict(o=o, d=d, tmax=tmax, ref=ref)


@functools.lru_cache(maxsize=None)
def mixed_points():
    """The same for the point batch of test_gpu_point_query.py: invalid points in front and sprinkled, limits at dist, one ulp above, half, none, 0."""
    b = TP.soup_batch()
    p = b["p"].copy()
    p[:1024, 1] = np.nan
    k = np.arange(N)
    p[(k >= 1024) & (k % 9 == 4), 0] = np.inf
    dist = b["ref"]["dist"]
    rmax = np.select([k % 5 == 0, k % 5 == 1, k % 5 == 2, k % 5 == 3], [np.full(N, INF), dist, np.nextafter(dist, INF), f32(0.5) * dist], f32(0)).astype(f32)
    ref = dict(PX.reference(b["v"], p, rmax)["brute"])
    ref["normal"] = point_normals(b["v"], ref["tri"])
    assert (ref["tri"][:1024] == INVALID).all() and (ref["tri"][1024:] >= 0).sum() > 1000 and (ref["tri"][1024:] == MISS).sum() > 800
    return dict(p=p, rmax=rmax, ref=ref)


@pytest.mark.parametrize("n", NS)
def test_the_ray_sink_under_refill_pressure(renderer, n):
    """One workgroup, one LDS stack entry, refills at 1, 24 and 64 idle lanes: lanes retire while their neighbours are mid-walk and are
    handed the next ray at once, invalid rays and empty intervals are answered in the source.  The sink must write the retiring ray's
    attributes at the retiring ray's row."""
    TR.set_soup(renderer)
    m = mixed_rays()
    sel = slice(0, N) if n == N else slice(1024, 1024 + n)
    o, d, tmax = m["o"][sel], m["d"][sel], m["tmax"][sel]
    for refill in REFILLS:
        kw = dict(tune_max_blocks=1, tune_refill_min=refill, tune_lds_stack=1)
        got = ray_attr(renderer, o, d, tmax, **kw)
        assert_ray_answers(got, m["ref"], sel, (n, refill))
        st = renderer.ray_query_stats()
        assert (st["rays"], st["invalid_rays"], st["stack_overflow"]) == (n, int((m["ref"]["tri"][sel] == INVALID).sum()), 0)
        t, tri = TR.query(renderer, o, d, tmax=tmax, **kw)
        assert np.array_equal(tri, got[1]) and same_floats(t, got[0]), (n, refill)
    if n == N:  # and with the default grid
        assert_ray_answers(ray_attr(renderer, o, d, tmax), m["ref"], sel, "default")


@pytest.mark.parametrize("n", NS)
def test_the_point_sink_under_refill_pressure(renderer, n):
    TP.set_soup(renderer)
    m = mixed_points()
    sel = slice(0, N) if n == N else slice(1024, 1024 + n)
    p, rmax = m["p"][sel], m["rmax"][sel]
    for refill in REFILLS:
        kw = dict(tune_max_blocks=1, tune_refill_min=refill, tune_lds_stack=1)
        got = point_attr(renderer, p, rmax, **kw)
        assert_point_answers(got, m["ref"], sel, (n, refill))
        st = renderer.point_query_stats()
        assert (st["points"], st["invalid_points"], st["stack_overflow"]) == (n, int((m["ref"]["tri"][sel] == INVALID).sum()), 0)
        dist, tri, c = TP.query(renderer, p, rmax, **kw)
        assert np.array_equal(tri, got[1]) and same_floats(dist, got[0]) and same_floats(c, got[2]), (n, refill)
    if n == N:
        assert_point_answers(point_attr(renderer, p, rmax, count_traversal=True), m["ref"], sel, "default, counted")
        assert renderer.point_query_stats()["nodes_visited"] > 0


# ---- 3. NULL arrays, bounds, inputs --------------------------------------------------------------------------------------------

def test_each_attribute_array_may_be_null_and_nothing_else_is_written(renderer):
    import torch

    lib = R.load()
    TR.set_soup(renderer)
    m = mixed_rays()
    for n in (1, 65, N):
        sel = slice(0, N) if n == N else slice(1024, 1024 + n)
        o, d, tm = tdev(m["o"][sel]), tdev(m["d"][sel]), tdev(m["tmax"][sel])
        o0, d0, tm0 = o.clone(), d.clone(), tm.clone()
        for want_uv, want_n in ((True, True), (True, False), (False, True), (False, False)):
            t, tri = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64)
            uv, nrm = sentinel(n, torch.float32, 64, cols=2), sentinel(n, torch.float32, 64, cols=3)
            assert lib.rt_query_rays_attr_device(renderer._ctx, ptr(o), ptr(d), ptr(tm), n, None, ptr(t), ptr(tri), ptr(uv if want_uv else None), ptr(nrm if want_n else None)) == 0
            renderer.synchronize()
            ref = m["ref"]
            assert np.array_equal(tri[:n].cpu().numpy(), ref["tri"][sel]) and same_floats(t[:n].cpu().numpy(), ref["t"][sel]), (n, want_uv, want_n)
            assert still_sentinel(t, 0, n) and still_sentinel(tri, 0, n) and still_sentinel(uv, 0, n) and still_sentinel(nrm, 0, n)
            if want_uv:
                assert same_floats(uv[:n, 0].cpu().numpy(), ref["ub"][sel]) and same_floats(uv[:n, 1].cpu().numpy(), ref["vb"][sel])
            else:
                assert still_sentinel(uv)
            if want_n:
                assert same_floats(nrm[:n].cpu().numpy(), ref["normal"][sel])
            else:
                assert still_sentinel(nrm)
        for x, x0 in ((o, o0), (d, d0), (tm, tm0)):
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
    # points
    TP.set_soup(renderer)
    mp = mixed_points()
    n = 257
    sel = slice(1024, 1024 + n)
    p, rm = tdev(mp["p"][sel]), tdev(mp["rmax"][sel])
    p0, rm0 = p.clone(), rm.clone()
    for want_c, want_uv, want_n in ((True, True, True), (False, True, False), (False, False, True), (True, False, False), (False, False, False)):
        dist, tri, c = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64), sentinel(n, torch.float32, 64, cols=3)
        uv, nrm = sentinel(n, torch.float32, 64, cols=2), sentinel(n, torch.float32, 64, cols=3)
        assert lib.rt_query_points_attr_device(renderer._ctx, ptr(p), ptr(rm), n, None, ptr(dist), ptr(tri), ptr(c if want_c else None), ptr(uv if want_uv else None),
                                               ptr(nrm if want_n else None)) == 0
        renderer.synchronize()
        ref = mp["ref"]
        assert np.array_equal(tri[:n].cpu().numpy(), ref["tri"][sel]) and same_floats(dist[:n].cpu().numpy(), ref["dist"][sel])
        assert still_sentinel(dist, 0, n) and still_sentinel(tri, 0, n) and still_sentinel(c, 0, n) and still_sentinel(uv, 0, n) and still_sentinel(nrm, 0, n)
        assert same_floats(c[:n].cpu().numpy(), ref["c"][sel]) if want_c else still_sentinel(c)
        assert (same_floats(uv[:n, 0].cpu().numpy(), ref["u"][sel]) and same_floats(uv[:n, 1].cpu().numpy(), ref["v"][sel])) if want_uv else still_sentinel(uv)
        assert same_floats(nrm[:n].cpu().numpy(), ref["normal"][sel]) if want_n else still_sentinel(nrm)
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(rm.view(torch.int32), rm0.view(torch.int32))
    # the wrapper's out tensors are the ones it returns
    t, tri, uv, nrm = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=2), sentinel(n, torch.float32, cols=3)
    got = renderer.query_rays(tdev(m["o"][sel]), tdev(m["d"][sel]), attributes=True, out=(t, tri, uv, nrm))
    assert [g.data_ptr() for g in got] == [x.data_ptr() for x in (t, tri, uv, nrm)]


def test_refusals_leave_all_outputs_untouched(renderer):
    import torch

    lib = R.load()
    n = 1000
    ends = bad_pointers(n, short3=12, short2=8, short1=4)  # the allocation holds n - 1 rows from the short ones
    hp, big, short3, short2, short1 = ends.hp, ends.big, ends.short3, ends.short2, ends.short1
    outs = [sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3), sentinel(n, torch.float32, cols=2), sentinel(n, torch.float32, cols=3)]
    t, tri, c, uv, nrm = outs

    def untouched():
        renderer.synchronize()
        return all(still_sentinel(x) for x in outs) and bool((big == 0).all())

    b = TR.set_soup(renderer)
    o, d = tdev(b["o"][:n]), tdev(b["d"][:n])
    Q = R.RayQueryParams
    ok = (ptr(o), ptr(d), None, n, None, ptr(t), ptr(tri), ptr(uv), ptr(nrm))

    def ray_call(**change):
        names = ("o", "d", "tmax", "n", "prm", "t", "tri", "uv", "nrm")
        return lib.rt_query_rays_attr_device(renderer._ctx, *(change.get(k, v) for k, v in zip(names, ok)))

    for k, change in enumerate([dict(prm=C.byref(Q(any_hit=1))), dict(prm=C.byref(Q(any_hit=1)), uv=None, nrm=None), dict(prm=C.byref(Q(any_hit=2))), dict(o=None), dict(d=hp),
                                dict(tmax=short1), dict(t=None), dict(tri=None), dict(t=hp), dict(uv=hp), dict(nrm=hp), dict(uv=short2), dict(nrm=short3), dict(o=short3),
                                dict(n=(1 << 30) + 1), dict(prm=C.byref(Q(tune_refill_min=65))), dict(prm=C.byref(Q(tune_blocks_per_cu=9))), dict(prm=C.byref(Q(tune_lds_stack=79)))]):
        assert ray_call(**change) == RT_ERR_INVALID, (k, change)
        assert untouched(), (k, change)
    assert ray_call(n=0) == 0 and lib.rt_query_rays_attr_device(renderer._ctx, None, None, None, 0, None, None, None, None, None) == 0 and untouched()
    with pytest.raises(ValueError):
        renderer.query_rays(o, d, any_hit=True, attributes=True)
    e = renderer.query_rays(o[:0], d[:0], attributes=True)
    assert [tuple(x.shape) for x in e] == [(0,), (0,), (0, 2), (0, 3)]

    bp = TP.set_soup(renderer)
    p = tdev(bp["p"][:n])
    P = R.PointQueryParams
    okp = (ptr(p), None, n, None, ptr(t), ptr(tri), ptr(c), ptr(uv), ptr(nrm))

    def point_call(**change):
        names = ("p", "rmax", "n", "prm", "dist", "tri", "c", "uv", "nrm")
        return lib.rt_query_points_attr_device(renderer._ctx, *(change.get(k, v) for k, v in zip(names, okp)))

    for k, change in enumerate([dict(p=None), dict(p=hp), dict(rmax=hp), dict(dist=None), dict(tri=None), dict(c=hp), dict(uv=hp), dict(nrm=hp), dict(uv=short2), dict(nrm=short3),
                                dict(c=short3), dict(n=(1 << 30) + 1), dict(prm=C.byref(P(count_traversal=2))), dict(prm=C.byref(P(tune_refill_min=65)))]):
        assert point_call(**change) == RT_ERR_INVALID, (k, change)
        assert untouched(), (k, change)
    assert point_call(n=0) == 0 and untouched()
    # the context still answers
    got = cpu(renderer.query_points(p, attributes=True, out=(t, tri, c, uv, nrm)))
    assert np.array_equal(got[1], bp["ref"]["tri"][:n]) and same_floats(got[3][:, 0], bp["ref"]["u"][:n])


# ---- 4. stream order -----------------------------------------------------------------------------------------------------------

def test_stream_order_with_interpolate_behind_the_query(renderer):
    """Rays made by torch on a stream, the attribute query behind them on that stream without a host synchronisation, interpolate() of
    the vertex positions behind the query, a torch comparison behind that; one synchronisation at the end."""
    import torch

    b = TR.set_soup(renderer)
    n = len(b["o"])
    verts = X.mesh("soup")[0]
    ref = AX.reference(verts, b["o"], b["d"])
    em = X.ExactMesh(verts)
    hit = ref["tri"] >= 0
    expect = np.full((n, 3), np.nan)
    expect[hit] = AX.bary_point(em, ref["tri"][hit], ref["ub"][hit], ref["vb"][hit])
    o_half, d_half = tdev(b["o"] * f32(0.5)), tdev(b["d"] * f32(0.5))
    vattr = tdev(verts.reshape(-1, 3, 3)).double()
    ref_uv, ref_tri, ref_p = tdev(np.stack([ref["ub"], ref["vb"]], 1)).view(torch.int32), tdev(ref["tri"]), tdev(expect)
    outs = [sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=2), sentinel(n, torch.float32, cols=3)]
    pouts = [sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3), sentinel(n, torch.float32, cols=2), sentinel(n, torch.float32, cols=3)]
    with busy_stream(renderer):
        o, d = o_half * 2.0, d_half * 2.0  # (halving and doubling is exact)
        t, tri, uv, nrm = renderer.query_rays(o, d, out=tuple(outs), sync=False, attributes=True)
        P = R.Renderer.interpolate(tri, uv.double(), vattr)
        wrong = (uv.view(torch.int32) != ref_uv).sum() + (tri != ref_tri).sum() + (~((P == ref_p) | (P.isnan() & ref_p.isnan()))).sum()
        # the hit points as query points: their nearest triangle is at distance ~0, and the chained query reads what interpolate wrote
        pts = torch.where(P.isnan(), torch.zeros_like(P), P).float().contiguous()
        dist, ptri, c, puv, pn = renderer.query_points(pts, out=tuple(pouts), sync=False, attributes=True)
        far = ((dist > 1e-4) & (tri >= 0)).sum()  # (miss rows ask about the origin of the coordinates)
    assert int(wrong) == 0 and int(far) == 0 and bool((ptri >= 0).all()) and bool(puv.isfinite().all())


# ---- 5. frames, sharing, statistics --------------------------------------------------------------------------------------------

def test_frames_sharing_and_statistics_are_undisturbed(renderer):
    b = TR.set_soup(renderer)
    bp = TP.soup_batch()
    renderer.resize(64, 64)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r):
        return pt_frame(r, **kw)

    before = frame(renderer)
    assert before[1][1] > 0 and before[1][2] > 0
    m = mixed_rays()
    other = R.Renderer(0)
    try:
        other.set_mesh(*X.mesh("soup"))
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        assert_ray_answers(ray_attr(renderer, m["o"], m["d"], m["tmax"], tune_lds_stack=1), m["ref"])
        got = point_attr(other, bp["p"])
        assert np.array_equal(got[1], bp["ref"]["tri"]) and same_floats(got[3][:, 0], bp["ref"]["u"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2  # the queries only read the mesh
        after, theirs = frame(renderer), frame(other)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
        assert np.array_equal(before[0], theirs[0]) and before[1] == theirs[1]
    finally:
        other.close()
    # the statistics are the kinds' own and do not mix: an attribute query of one kind leaves the other kind's unread counters alone
    n_bad = int((m["ref"]["tri"] == INVALID).sum())
    p = bp["p"].copy()
    p[:300, 0] = np.nan
    ray_attr(renderer, m["o"], m["d"], m["tmax"])
    point_attr(renderer, p, count_traversal=True)
    rs, ps = renderer.ray_query_stats(), renderer.point_query_stats()  # only now
    assert (rs["rays"], rs["invalid_rays"], rs["launches"]) == (N, n_bad, 1) and rs["ms"] > 0, rs
    assert (ps["points"], ps["invalid_points"], ps["launches"]) == (N, 300, 1) and ps["nodes_visited"] > 0 and ps["ms"] > 0, ps
    point_attr(renderer, p)
    ray_attr(renderer, m["o"], m["d"], m["tmax"])
    rs, ps = renderer.ray_query_stats(), renderer.point_query_stats()
    assert (rs["rays"], rs["invalid_rays"]) == (N, n_bad) and (ps["points"], ps["invalid_points"], ps["nodes_visited"]) == (N, 300, 0)
