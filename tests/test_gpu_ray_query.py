"""Ray queries on device tensors (Renderer.query_rays / rt_query_rays_device) on the GPU.

Two references, both from tests/ray_exact.py: the oracle's brute-force answers, which the queries must give bit for bit, and the
float64 accuracy contract, which they must satisfy on their own.  Test 1 runs every ray family on its own meshes (the data of
tests/test_gpu_ray_contract.py, shared through its cache).  The other tests need ONE batch on ONE mesh whose size they can cut,
tile and plant rays into: the 4 000 rays of family (a) - aimed at the soup, the terrain and the flat grid - all traced against the
2 000-triangle soup, with the oracle's brute-force answers for exactly that (soup_batch()).  A distance limit needs no tolerance: the
closest hit is defined as the (t, index)-minimal triangle the fp32 test accepts with t > 0, so "hit when t < tmax" is decided by
the reference's own t."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import ray_exact as X
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, busy_stream, dev, pt_frame, ptr, same_floats, sentinel, still_sentinel, tdev
from test_gpu_ray_contract import family_data  # the per-family references, computed once for both modules

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = -1, -2


def query(renderer, o, d, tmax=None, any_hit=False, **kw):
    """Numpy in, numpy out, through device tensors."""
    got = renderer.query_rays(tdev(o), tdev(d), None if tmax is None else tdev(tmax), any_hit=any_hit, **kw)
    if any_hit:
        return got.cpu().numpy()
    return got[0].cpu().numpy(), got[1].cpu().numpy()


@functools.lru_cache(maxsize=None)
def soup_batch():
    """The 4 000 rays of family (a) against the soup: rays, the oracle's brute-force answers (closest along d, occlusion of (o, o + seg)
    and of (o, o + d)), the float64 candidates, and the origin range of the mesh."""
    parts = X.family("a")
    o = np.concatenate([p["o"] for p in parts])
    d = np.concatenate([p["d"] for p in parts])
    seg = np.concatenate([p["seg"] for p in parts])
    v, a, e = X.mesh("soup")
    sc = O.TriScene(v, a, e)
    t, tri, occ = X.oracle_answers(sc, o, d, seg, False)
    em = X.ExactMesh(v)
    reach = f32(32) * max(f32(1), np.abs(v).max().astype(f32))
    assert np.abs(o).max() < reach and (tri >= 0).sum() > 1000 and (tri < 0).sum() > 100
    return dict(o=o, d=d, seg=seg, t=t, tri=tri, occ=occ, sc=sc, cand=X.Candidates(o, d, em), cand_seg=X.Candidates(o, seg, em), reach=reach)


def set_soup(renderer):
    renderer.set_mesh(*X.mesh("soup"))
    return soup_batch()


# ---- 1. every family ---------------------------------------------------------------------------------------------------------

def check_part(renderer, name, part, ref, cand, what):
    cc, co = cand
    t, tri = query(renderer, part["o"], part["d"])
    assert tri.dtype == np.int32 and t.dtype == f32
    assert np.array_equal(tri, ref["tri"]), (name, part["mesh"], what, np.nonzero(tri != ref["tri"])[0][:8])
    assert same_floats(t, ref["t"]), (name, part["mesh"], what, np.nonzero(t != ref["t"])[0][:8])  # +inf on a miss, both
    if name in X.CLOSEST_FAMILIES:
        ok = cc.check_closest(tri, t)
        assert ok.all(), (name, part["mesh"], what, "closest hit outside the contract", np.nonzero(~ok)[0][:8])
    occ = query(renderer, part["o"], part["seg"], any_hit=True)
    assert occ.dtype == np.int32 and set(np.unique(occ)) <= {0, 1}
    assert np.array_equal(occ.astype(bool), ref["occ"]), (name, part["mesh"], what, np.nonzero(occ.astype(bool) != ref["occ"])[0][:8])
    ok = co.check_occluded(occ)
    assert ok.all(), (name, part["mesh"], what, "occlusion outside the contract", np.nonzero(~ok)[0][:8])
    st = renderer.ray_query_stats()
    assert (st["rays"], st["invalid_rays"], st["stack_overflow"], st["launches"]) == (len(part["o"]), 0, 0, 1) and st["ms"] > 0


@pytest.mark.parametrize("name", X.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, name):
    for p in family_data(name):
        renderer.set_mesh(*X.mesh(p["part"]["mesh"]))
        check_part(renderer, name, p["part"], p["ref"], p["cand"], "host")


@pytest.mark.parametrize("name", ["a", "h"])
def test_two_level_device_built_and_refitted_trees(renderer, name):
    for p in family_data(name):
        v, a, e = X.mesh(p["part"]["mesh"])
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_part(renderer, name, p["part"], p["ref"], p["cand"], "two-level")
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_part(renderer, name, p["part"], p["ref"], p["cand"], "device build")
        renderer.refit_mesh_device(tdev(p["moved"]))
        check_part(renderer, name, p["part"], p["ref_moved"], p["cand_moved"], "refit to moved vertices")


# ---- 2. batch edges and refill -----------------------------------------------------------------------------------------------

TUNINGS = [dict(), dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4000])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams and 256 lanes for up to 4 000 rays: every stream is reached
    only by waves moving on from a dry one, and every lane refills many times."""
    b = set_soup(renderer)
    for kw in TUNINGS:
        t, tri = query(renderer, b["o"][:n], b["d"][:n], **kw)
        assert np.array_equal(tri, b["tri"][:n]) and same_floats(t, b["t"][:n]), (n, kw)
        occ = query(renderer, b["o"][:n], b["seg"][:n], any_hit=True, **kw)
        assert np.array_equal(occ.astype(bool), b["occ"][:n]), (n, kw)
        assert renderer.ray_query_stats()["rays"] == n
    if n == 4000:  # the batch of the tests below, held to the contract on its own
        assert b["cand"].check_closest(tri, t).all() and b["cand_seg"].check_occluded(occ).all()


# ---- 3. more rays than lanes ---------------------------------------------------------------------------------------------------

def test_more_rays_than_lanes(renderer):
    import torch

    b = set_soup(renderer)
    n = 600000
    assert n > 256 * 8 * 256
    perm = torch.from_numpy(((np.arange(n, dtype=np.int64) * 2654435761) % 4000)).to(dev())  # a fixed scatter of the 4 000 rays
    o, d, seg = (tdev(b[k])[perm].contiguous() for k in ("o", "d", "seg"))
    t, tri = renderer.query_rays(o, d)
    st = renderer.ray_query_stats()
    assert (st["rays"], st["invalid_rays"], st["stack_overflow"]) == (n, 0, 0)
    assert torch.equal(tri, tdev(b["tri"])[perm]) and torch.equal(t.view(torch.int32), tdev(b["t"]).view(torch.int32)[perm])
    occ = renderer.query_rays(o, seg, any_hit=True)
    assert torch.equal(occ != 0, tdev(b["occ"])[perm])
    assert renderer.ray_query_stats()["rays"] == n


# ---- 4. tmax -------------------------------------------------------------------------------------------------------------------

def test_distance_limits(renderer):
    b = set_soup(renderer)
    n = len(b["o"])
    rng = np.random.default_rng(41)
    t_ref, hit = b["t"], b["tri"] >= 0
    kind = np.arange(n) % 7
    rand = rng.uniform(0.01, 40.0, n).astype(f32)
    tmax = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                     [f32(0.5) * t_ref, t_ref, np.nextafter(t_ref, INF), np.full(n, INF), np.zeros(n, f32), np.full(n, f32(-1))], rand).astype(f32)
    tmax = np.where((kind == 6) | np.isfinite(tmax), tmax, np.where(kind <= 2, rand, tmax)).astype(f32)  # a miss has no t_ref to scale: a random limit
    for k in range(7):
        assert (hit & (kind == k)).sum() > 100
    assert (~hit & (kind == 6)).sum() > 10
    within = hit & (t_ref < tmax)
    assert not within[kind == 0].any() and not within[kind == 1].any() and within[hit & (kind == 2)].all() and within[hit & (kind == 3)].all()
    assert not within[(kind == 4) | (kind == 5)].any() and within[kind == 6].any() and (hit & ~within)[kind == 6].any()
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        t, tri = query(renderer, b["o"], b["d"], tmax=tmax, **kw)
        assert np.array_equal(tri, np.where(within, b["tri"], MISS)), np.nonzero(tri != np.where(within, b["tri"], MISS))[0][:8]
        assert same_floats(t, np.where(within, t_ref, INF))
        occ = query(renderer, b["o"], b["d"], tmax=tmax, any_hit=True, **kw)
        assert np.array_equal(occ, within.astype(np.int32)), np.nonzero(occ != within)[0][:8]
        assert renderer.ray_query_stats()["invalid_rays"] == 0
    # without a tmax array the limits are the hook's: +inf, and 0.999 for any hit
    occ = query(renderer, b["o"], b["d"], any_hit=True)
    assert np.array_equal(occ, query(renderer, b["o"], b["d"], tmax=np.full(n, X.T_SHADOW, f32), any_hit=True))
    assert np.array_equal(occ, (hit & (t_ref < f32(X.T_SHADOW))).astype(np.int32))


# ---- 5. invalid rays -----------------------------------------------------------------------------------------------------------

def test_invalid_rays(renderer):
    b = set_soup(renderer)
    n = len(b["o"])
    reach = b["reach"]
    rng = np.random.default_rng(43)
    n_soup = len(X.family("a")[0]["o"])  # the rays aimed at the soup come first
    edge = rng.choice(np.nonzero(b["tri"][:n_soup] >= 0)[0], 24, replace=False)
    where = rng.permutation(np.setdiff1d(np.arange(n), edge))
    o, d, tmax = b["o"].copy(), b["d"].copy(), np.full(n, INF, f32)
    invalid = np.zeros(n, bool)
    k = 0
    for arr in (o, d):  # a NaN or an infinity in one component of o or d
        for comp in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                for _ in range(3):
                    arr[where[k], comp] = bad
                    invalid[where[k]] = True
                    k += 1
    for _ in range(9):
        tmax[where[k]] = np.nan
        invalid[where[k]] = True
        k += 1
    for comp in range(3):  # one step beyond the range
        for sign in (1, -1):
            o[where[k], comp] = sign * np.nextafter(reach, INF)
            invalid[where[k]] = True
            k += 1
    for j, i in enumerate(edge):  # exactly at its end: valid; re-aimed at the point the ray hit, so that it has something to hit
        target = (o[i].astype(np.float64) + np.float64(b["t"][i]) * d[i].astype(np.float64)).astype(f32)
        o[i, j % 3] = (1 if j % 2 else -1) * reach
        d[i] = target - o[i]
    assert k < n // 4 and (np.abs(o[edge]).max(1) == reach).all() and not invalid[edge].any()
    te, trie, _ = X.oracle_answers(b["sc"], o[edge], d[edge], d[edge], False)
    assert (trie >= 0).sum() >= 12
    exp_t, exp_tri = b["t"].copy(), b["tri"].copy()
    exp_t[edge], exp_tri[edge] = te, trie
    exp_occ = (exp_tri >= 0) & (exp_t < f32(X.T_SHADOW))
    exp_t[invalid], exp_tri[invalid] = np.nan, INVALID
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        t, tri = query(renderer, o, d, tmax=tmax, **kw)
        assert np.array_equal(tri, exp_tri), np.nonzero(tri != exp_tri)[0][:8]
        assert np.isnan(t[invalid]).all() and same_floats(t[~invalid], exp_t[~invalid])
        assert renderer.ray_query_stats()["invalid_rays"] == invalid.sum()
        inv_no_tmax = invalid & ~np.isnan(tmax)
        occ = query(renderer, o, d, any_hit=True, **kw)  # the default limit: a NaN tmax is not among the faults here
        assert np.array_equal(occ, np.where(inv_no_tmax, INVALID, exp_occ.astype(np.int32)))
        assert renderer.ray_query_stats()["invalid_rays"] == inv_no_tmax.sum()
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive
    o_bad = b["o"].copy()
    o_bad[:, 1] = np.nan
    t, tri = query(renderer, o_bad, b["d"], tune_max_blocks=1)
    assert (tri == INVALID).all() and np.isnan(t).all() and renderer.ray_query_stats()["invalid_rays"] == n
    assert (query(renderer, o_bad, b["d"], any_hit=True, tune_max_blocks=1) == INVALID).all()
    o_bad = b["o"].copy()
    o_bad[:1024, 2] = -np.inf
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        t, tri = query(renderer, o_bad, b["d"], **kw)
        assert (tri[:1024] == INVALID).all() and np.array_equal(tri[1024:], b["tri"][1024:]) and same_floats(t[1024:], b["t"][1024:]), kw
        occ = query(renderer, o_bad, b["seg"], any_hit=True, **kw)
        assert (occ[:1024] == INVALID).all() and np.array_equal(occ[1024:].astype(bool), b["occ"][1024:]), kw
        assert renderer.ray_query_stats()["invalid_rays"] == 1024
    # a zero direction is valid and misses everything, as in the oracle
    t, tri = query(renderer, b["o"][:64], np.zeros((64, 3), f32))
    assert (tri == MISS).all() and np.isposinf(t).all() and renderer.ray_query_stats()["invalid_rays"] == 0


# ---- 6. spill ------------------------------------------------------------------------------------------------------------------

def test_stack_spill(renderer):
    data = family_data("a")
    for p in (data[0], data[2]):
        assert p["part"]["mesh"] in ("soup", "grid")
        renderer.set_mesh(*X.mesh(p["part"]["mesh"]))
        if p["part"]["mesh"] == "soup":
            assert renderer.pt_stats()["stack_need"] > 1  # one entry in LDS: the rest of every stack is in global memory
        t, tri = query(renderer, p["part"]["o"], p["part"]["d"], tune_lds_stack=1)
        assert np.array_equal(tri, p["ref"]["tri"]) and same_floats(t, p["ref"]["t"])
        assert renderer.ray_query_stats()["stack_overflow"] == 0
        occ = query(renderer, p["part"]["o"], p["part"]["seg"], any_hit=True, tune_lds_stack=1)
        assert np.array_equal(occ.astype(bool), p["ref"]["occ"])
        assert renderer.ray_query_stats()["stack_overflow"] == 0


# ---- 7. bounds -----------------------------------------------------------------------------------------------------------------

def test_bounds_and_out_tensors(renderer):
    import torch

    b = set_soup(renderer)
    for n in (1, 65, 4000):
        o, d, tm = tdev(b["o"][:n]), tdev(b["d"][:n]), tdev(np.full(n, INF, f32))
        o0, d0, tm0 = o.clone(), d.clone(), tm.clone()
        t_buf, tri_buf = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64)
        t, tri = renderer.query_rays(o, d, tm, out=(t_buf[:n], tri_buf[:n]))
        assert t.data_ptr() == t_buf.data_ptr() and tri.data_ptr() == tri_buf.data_ptr() and len(t) == len(tri) == n
        assert still_sentinel(t_buf, 0, n) and still_sentinel(tri_buf, 0, n)
        assert np.array_equal(tri.cpu().numpy(), b["tri"][:n]) and same_floats(t.cpu().numpy(), b["t"][:n])
        occ_buf = sentinel(n, torch.int32, 64)
        occ = renderer.query_rays(o, d, tm, any_hit=True, out=occ_buf[:n])
        assert occ.data_ptr() == occ_buf.data_ptr() and still_sentinel(occ_buf, 0, n)
        assert np.array_equal(occ.cpu().numpy(), (b["tri"][:n] >= 0).astype(np.int32))
        for x, x0 in ((o, o0), (d, d0), (tm, tm0)):
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
    with pytest.raises(ValueError):
        renderer.query_rays(o, d, out=(t_buf[:n], tri_buf[:n - 1]))
    with pytest.raises(ValueError):
        renderer.query_rays(o, d, out=(tri_buf[:n], tri_buf[:n]))
    with pytest.raises(ValueError):
        renderer.query_rays(o, d, any_hit=True, out=t_buf[:n])


# ---- 8. stream order -----------------------------------------------------------------------------------------------------------

def test_stream_order(renderer):
    """Rays made by torch on a stream, the query behind them on that stream without a host synchronisation, a torch reduction of the
    answers behind the query; one synchronisation at the end.  (Halving and doubling is exact: the rays are family (a)'s bit for bit.)"""
    import torch

    b = set_soup(renderer)
    n = len(b["o"])
    o_half, d_half = tdev(b["o"] * f32(0.5)), tdev(b["d"] * f32(0.5))
    ref_t, ref_tri = tdev(b["t"]).view(torch.int32), tdev(b["tri"])
    ref_occ = tdev((b["tri"] >= 0) & (b["t"] < f32(X.T_SHADOW)))
    t, tri, occ = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.int32)
    with busy_stream(renderer):
        o, d = o_half * 2.0, d_half * 2.0
        renderer.query_rays(o, d, out=(t, tri), sync=False)
        renderer.query_rays(o, d, any_hit=True, out=occ, sync=False)
        wrong = (t.view(torch.int32) != ref_t).sum() + (tri != ref_tri).sum() + ((occ != 0) != ref_occ).sum()
    assert int(wrong) == 0


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_soup(renderer)
    n = 1000
    o, d = tdev(b["o"][:n]), tdev(b["d"][:n])
    t, tri = sentinel(n, torch.float32), sentinel(n, torch.int32)
    fresh = R.Renderer(0)
    try:
        assert lib.rt_query_rays_device(fresh._ctx, ptr(o), ptr(d), None, n, None, ptr(t), ptr(tri)) == RT_ERR_STATE  # no mesh
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short3=12, short1=4)  # the allocation holds n - 1 rays from the short ones
    hp, big, short3, short1 = bp.hp, bp.big, bp.short3, bp.short1
    anyp = R.RayQueryParams(any_hit=1)
    calls = [(None, ptr(d), None, n, None, ptr(t), ptr(tri)), (ptr(o), None, None, n, None, ptr(t), ptr(tri)),
             (ptr(o), ptr(d), None, n, None, None, ptr(tri)), (ptr(o), ptr(d), None, n, None, ptr(t), None),
             (ptr(o), ptr(d), None, n, C.byref(anyp), None, None),
             (hp, ptr(d), None, n, None, ptr(t), ptr(tri)), (ptr(o), hp, None, n, None, ptr(t), ptr(tri)), (ptr(o), ptr(d), hp, n, None, ptr(t), ptr(tri)),
             (ptr(o), ptr(d), None, n, None, hp, ptr(tri)), (ptr(o), ptr(d), None, n, None, ptr(t), hp),
             (short3, ptr(d), None, n, None, ptr(t), ptr(tri)), (ptr(o), short3, None, n, None, ptr(t), ptr(tri)),
             (ptr(o), ptr(d), short1, n, None, ptr(t), ptr(tri)), (ptr(o), ptr(d), None, n, None, short1, ptr(tri)),
             (ptr(o), ptr(d), None, n, None, ptr(t), short1),
             (ptr(o), ptr(d), None, (1 << 30) + 1, None, ptr(t), ptr(tri))] + \
        [(ptr(o), ptr(d), None, n, prm, ptr(t), ptr(tri)) for prm in bad_params(R.RayQueryParams, "any_hit")]
    for k, args in enumerate(calls):
        assert lib.rt_query_rays_device(ctx, *args) == RT_ERR_INVALID, k
        assert_untouched(renderer, (t, tri), big, k)
    assert lib.rt_query_rays_device(ctx, ptr(o), ptr(d), None, 0, None, ptr(t), ptr(tri)) == 0  # n = 0 is accepted, and does nothing
    assert lib.rt_query_rays_device(ctx, None, None, None, 0, None, None, None) == 0
    renderer.synchronize()
    assert still_sentinel(t) and still_sentinel(tri)
    e = renderer.query_rays(o[:0], d[:0])
    assert len(e[0]) == 0 and len(e[1]) == 0
    # the context still answers
    t2, tri2 = renderer.query_rays(o, d, out=(t, tri))
    assert np.array_equal(tri2.cpu().numpy(), b["tri"][:n])


# ---- 10. rendering is undisturbed ----------------------------------------------------------------------------------------------

def test_rendering_is_undisturbed(renderer):
    b = set_soup(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r):
        return pt_frame(r, **kw)

    before = frame(renderer)
    assert before[1][1] > 0 and before[1][2] > 0
    t, tri = query(renderer, b["o"], b["d"], tune_lds_stack=1)
    query(renderer, b["o"], b["seg"], any_hit=True)
    after = frame(renderer)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(tri, b["tri"])
    # a shared mesh stays shared: the query only reads it
    other = R.Renderer(0)
    try:
        other.set_mesh(*X.mesh("soup"))
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        t2, tri2 = query(other, b["o"], b["d"])
        assert np.array_equal(tri2, b["tri"]) and same_floats(t2, b["t"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()
