"""Inside/outside and signed-distance queries on device tensors (Renderer.query_sides / query_signed_distance, rt_query_sides_device /
rt_query_signed_distance_device) on the GPU.

The reference is tests/sign_exact.py's native brute force (tests/native/side_query_ref.cpp: the arithmetic of csrc/ray_parity.h over
all triangles, no tree), which the kernel must match bit for bit in `inside` and in all three crossing counts; that reference in turn
is held to the float64 winding number on the CPU (tests/test_side_query_host.py).  The first tests run every family on every mesh;
the others need ONE batch on ONE mesh whose size they can cut, tile and plant points into: the 3 600 points of the sphere's case,
shuffled."""
import ctypes as C
import functools

import numpy as np
import pytest

import ray_exact as X
import sign_exact as SX
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, busy_stream, dev, pt_frame, ptr, same_floats, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
MISS, INVALID = SX.MISS, SX.INVALID
ALL = SX.CLOSED + SX.OPEN


def sides(renderer, p, **kw):
    """Numpy in, numpy out, through device tensors: inside, or (inside, crossings) with want_crossings."""
    out = renderer.query_sides(tdev(p), **kw)
    return tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()


def check_case(renderer, p, ref, what):
    """Both modes against the reference of points p: inside, crossings, the walk counts."""
    n = len(p)
    inside = sides(renderer, p)
    st = renderer.side_query_stats()
    assert inside.dtype == np.int32 and np.array_equal(inside, ref["inside"]), (what, np.nonzero(inside != ref["inside"])[0][:8])
    thirds = int(ref["third"].sum())
    assert (st["points"], st["invalid_points"], st["skipped_points"], st["stack_overflow"], st["launches"]) == (n, 0, 0, 0, 1) and st["ms"] > 0, (what, st)
    assert st["third_walks"] == thirds and st["walks"] == 2 * n + thirds, (what, st, thirds)
    inside3, crossings = sides(renderer, p, want_crossings=True)
    st = renderer.side_query_stats()
    assert crossings.dtype == np.int32 and crossings.shape == (n, 3)
    assert np.array_equal(crossings, ref["brute"]), (what, np.nonzero((crossings != ref["brute"]).any(1))[0][:8])
    assert np.array_equal(inside3, inside), what
    assert st["third_walks"] == thirds and st["walks"] == 3 * n and st["stack_overflow"] == 0, (what, st)


# ---- 1. every family on every mesh ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_every_family_on_the_host_built_tree(renderer, name):
    c = SX.case(name)
    set_mesh(renderer, c["verts"])
    check_case(renderer, c["p"], c["ref"], name)
    for f, r in c["rows"].items():  # (family by family, so that a failure names it)
        assert np.array_equal(sides(renderer, c["p"][r]), c["ref"]["inside"][r]), (name, f)


@functools.lru_cache(maxsize=None)
def moved_case(name):
    """Families a and d0 of case(name) against its vertices after ray_exact.moved()."""
    c = SX.case(name)
    p = np.concatenate([c["p"][c["rows"]["a"]], c["p"][c["rows"]["d0"]]])
    v = X.moved(c["verts"])
    return dict(verts=v, p=p, ref=SX.reference(v, p))


@pytest.mark.parametrize("name", ["sphere", "shell", "soup"])
def test_two_level_device_built_and_refitted_trees(renderer, name):
    c = SX.case(name)
    sel = np.r_[c["rows"]["a"], c["rows"]["d0"]]
    p = c["p"][sel]
    ref = {k: c["ref"][k][sel] for k in ("inside", "third", "brute")}
    v, a, e = X._with_surface(c["verts"])
    renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
    check_case(renderer, p, ref, (name, "two-level"))
    renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
    check_case(renderer, p, ref, (name, "device build"))
    m = moved_case(name)
    assert np.array_equal(m["p"], p) and (m["ref"]["inside"] >= 0).all()
    renderer.refit_mesh_device(tdev(m["verts"]))
    check_case(renderer, p, m["ref"], (name, "refit to moved vertices"))


# ---- 2. one batch on the sphere --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    c = SX.case("sphere")
    perm = np.random.default_rng(11).permutation(len(c["p"]))
    ref = {k: c["ref"][k][perm] for k in ("inside", "third", "brute")}
    return dict(v=c["verts"], p=np.ascontiguousarray(c["p"][perm]), ref=ref, n=len(perm), reach=SX.PX.reach_of(c["verts"]))


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 1 000 points every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not."""
    b = set_batch(renderer)
    assert n <= len(b["p"])
    for kw in TUNINGS:
        inside, crossings = sides(renderer, b["p"][:n], want_crossings=True, **kw)
        assert np.array_equal(inside, b["ref"]["inside"][:n]) and np.array_equal(crossings, b["ref"]["brute"][:n]), (n, kw)
        assert np.array_equal(sides(renderer, b["p"][:n], **kw), b["ref"]["inside"][:n]), (n, kw)
        st = renderer.side_query_stats()
        thirds = int(b["ref"]["third"][:n].sum())
        assert (st["points"], st["stack_overflow"], st["third_walks"], st["walks"]) == (n, 0, thirds, 2 * n + thirds), (n, kw, st)


def test_more_points_than_lanes(renderer):
    import torch

    b = set_batch(renderer)
    n, m = 600000, b["n"]
    assert n > 256 * 8 * 256
    perm = torch.from_numpy(((np.arange(n, dtype=np.int64) * 2654435761) % m)).to(dev())  # a fixed scatter of the batch's points
    p = tdev(b["p"])[perm].contiguous()
    inside, crossings = renderer.query_sides(p, want_crossings=True)
    st = renderer.side_query_stats()
    assert (st["points"], st["invalid_points"], st["stack_overflow"], st["walks"]) == (n, 0, 0, 3 * n)
    assert torch.equal(inside, tdev(b["ref"]["inside"])[perm]) and torch.equal(crossings, tdev(b["ref"]["brute"])[perm])
    assert torch.equal(renderer.query_sides(p), inside)
    st = renderer.side_query_stats()
    assert st["walks"] == 2 * n + st["third_walks"] and st["third_walks"] == int(tdev(b["ref"]["third"])[perm].sum())


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest in global memory."""
    for name in ("sphere", "soup"):
        c = SX.case(name)
        set_mesh(renderer, c["verts"])
        assert renderer.pt_stats()["bvh_depth"] > 1
        inside, crossings = sides(renderer, c["p"], want_crossings=True, tune_lds_stack=1)
        assert np.array_equal(inside, c["ref"]["inside"]) and np.array_equal(crossings, c["ref"]["brute"]), name
        assert renderer.side_query_stats()["stack_overflow"] == 0
        assert np.array_equal(sides(renderer, c["p"], tune_lds_stack=1), c["ref"]["inside"]), name
        assert renderer.side_query_stats()["stack_overflow"] == 0


def test_invalid_points(renderer):
    b = set_batch(renderer)
    ref, reach, n = b["ref"], b["reach"], b["n"]
    rng = np.random.default_rng(43)
    where = rng.permutation(n)
    p = b["p"].copy()
    invalid = np.zeros(n, bool)
    k = 0
    for comp in range(3):  # a NaN or an infinity in one component
        for bad in (np.nan, np.inf, -np.inf):
            for _ in range(3):
                p[where[k], comp] = bad
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
    exp = SX.reference(b["v"], p)
    assert np.array_equal(exp["inside"] == INVALID, invalid) and (exp["inside"][edge] >= 0).all()
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        import torch

        cr, ins = sentinel(n, torch.int32, cols=3), sentinel(n, torch.int32)
        renderer.query_sides(tdev(p), out=(ins, cr), want_crossings=True, **kw)
        assert np.array_equal(ins.cpu().numpy(), exp["inside"]), kw
        got = cr.cpu().numpy()
        assert np.array_equal(got[~invalid], exp["brute"][~invalid]) and (got[invalid] == -7).all(), kw  # an invalid point's crossings are not written
        st = renderer.side_query_stats()
        assert (st["invalid_points"], st["walks"]) == (invalid.sum(), 3 * (n - invalid.sum())), (kw, st)
        assert np.array_equal(sides(renderer, p, **kw), exp["inside"]), kw
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive - 4 000 invalid points through one workgroup
    p_bad = np.tile(b["p"], (2, 1))[:4000].copy()
    p_bad[:, 1] = np.nan
    assert (sides(renderer, p_bad, tune_max_blocks=1) == INVALID).all()
    st = renderer.side_query_stats()
    assert (st["invalid_points"], st["walks"], st["points"]) == (4000, 0, 4000)
    p_bad = b["p"].copy()
    p_bad[:1024, 2] = -np.inf
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        inside = sides(renderer, p_bad, **kw)
        assert (inside[:1024] == INVALID).all() and np.array_equal(inside[1024:], ref["inside"][1024:]), kw
        assert renderer.side_query_stats()["invalid_points"] == 1024


def test_dist_inout_entries(renderer):
    """rt_query_sides_device with a distance array: +inf is skipped (MISS, stays +inf), NaN is invalid (stays NaN), everything else -
    0 included - takes the sign; an entry is read before the point is looked at."""
    import torch

    lib = R.load()
    b = set_batch(renderer)
    n, ref = b["n"], b["ref"]
    rng = np.random.default_rng(45)
    dist = rng.uniform(0.1, 2.0, n).astype(f32)
    kind = np.arange(n) % 5
    dist[kind == 1] = INF
    dist[kind == 2] = np.nan
    dist[kind == 3] = 0.0
    p = b["p"].copy()
    p[10, 0] = np.nan  # kind 0: an invalid point with a finite distance
    p[11, 0] = np.nan  # kind 1: +inf is decided first
    exp_inside = np.where(kind == 1, MISS, np.where(kind == 2, INVALID, ref["inside"])).astype(np.int32)
    exp_inside[10] = INVALID
    walked = (exp_inside >= 0)
    exp_dist = np.where(walked & (ref["inside"] == 1), -dist, dist).astype(f32)
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        tp, td = tdev(p), tdev(dist)
        ins = sentinel(n, torch.int32, 64)
        prm = R.SideQueryParams(**kw)
        assert lib.rt_query_sides_device(renderer._ctx, ptr(tp), n, C.byref(prm), ptr(ins), None, ptr(td)) == 0
        st = renderer.side_query_stats()
        assert np.array_equal(ins.cpu().numpy()[:n], exp_inside) and still_sentinel(ins, 0, n), kw
        assert same_floats(td.cpu().numpy(), exp_dist), kw
        zero = td.cpu().numpy()[(kind == 3) & walked]
        assert np.array_equal(np.signbit(zero), ref["inside"][(kind == 3) & walked] == 1)  # 0 becomes -0 inside
        thirds = int(ref["third"][walked].sum())
        assert (st["skipped_points"], st["invalid_points"], st["third_walks"], st["walks"]) == ((kind == 1).sum(), (kind == 2).sum() + 1, thirds, 2 * walked.sum() + thirds), (kw, st)


def test_signed_distance(renderer):
    import torch

    b = set_batch(renderer)
    n, ref = b["n"], b["ref"]
    p = b["p"].copy()
    p[5, 1] = np.inf
    tp = tdev(p)
    dist, tri, c = renderer.query_points(tp)
    sd, tri2, c2 = renderer.query_signed_distance(tp)
    ps, ss = renderer.point_query_stats(), renderer.side_query_stats()
    valid = np.arange(n) != 5
    inside = np.where(valid, ref["inside"], 0)
    d, s = dist.cpu().numpy(), sd.cpu().numpy()
    assert same_floats(np.abs(s), d) and torch.equal(tri, tri2) and same_floats(c.cpu().numpy(), c2.cpu().numpy())
    assert np.isnan(s[5]) and int(tri2[5]) == INVALID
    assert (d[valid] > 0).all() and np.array_equal(np.signbit(s[valid]), inside[valid] == 1)  # the sign is the reference's
    assert (ps["points"], ps["invalid_points"]) == (n, 1) and (ss["points"], ss["invalid_points"], ss["skipped_points"]) == (n, 1, 0)
    thirds = int(ref["third"][valid].sum())
    assert (ss["third_walks"], ss["walks"], ss["stack_overflow"], ps["stack_overflow"]) == (thirds, 2 * (n - 1) + thirds, 0, 0)
    # a narrow band: beyond rmax nothing is walked and the entry stays +inf; want_points=False; out tensors with sentinels behind them
    rmax = np.full(n, f32(0.05))
    rmax[::7] = INF
    d_buf, t_buf = sentinel(n, torch.float32, 64), sentinel(n, torch.int32, 64)
    sd, tri3, none = renderer.query_signed_distance(tp, rmax=tdev(rmax), out=(d_buf[:n], t_buf[:n]), want_points=False)
    ps, ss = renderer.point_query_stats(), renderer.side_query_stats()
    dl, tl, _ = renderer.query_points(tp, tdev(rmax), want_points=False)
    beyond = np.isinf(dl.cpu().numpy()) & valid  # as the point query itself decides it (d2 < rmax * rmax in fp32)
    assert 0.3 < beyond.mean() < 0.95 and (d[beyond] >= f32(0.999) * rmax[beyond]).all() and (d[valid & ~beyond] <= f32(1.001) * rmax[valid & ~beyond]).all()
    assert none is None and sd.data_ptr() == d_buf.data_ptr() and still_sentinel(d_buf, 0, n) and still_sentinel(t_buf, 0, n)
    s = sd.cpu().numpy()
    assert same_floats(np.abs(s), dl.cpu().numpy()) and torch.equal(tri3, tl)
    assert (s[beyond] == INF).all() and (tri3.cpu().numpy()[beyond] == MISS).all()
    near = valid & ~beyond
    assert np.array_equal(np.signbit(s[near]), inside[near] == 1)
    thirds = int(ref["third"][near].sum())
    assert (ss["skipped_points"], ss["invalid_points"], ss["walks"]) == (beyond.sum(), 1, 2 * near.sum() + thirds), ss
    assert ps["points"] == n and torch.equal(tp.view(torch.int32), tdev(p).view(torch.int32))
    # inside_out through the C entry
    lib = R.load()
    ins, c_buf = sentinel(n, torch.int32, 64), sentinel(n, torch.float32, cols=3)
    assert lib.rt_query_signed_distance_device(renderer._ctx, ptr(tp), None, n, None, None, ptr(d_buf), ptr(t_buf), ptr(c_buf), ptr(ins)) == 0
    renderer.synchronize()
    assert np.array_equal(ins.cpu().numpy()[:n], np.where(valid, ref["inside"], INVALID)) and still_sentinel(ins, 0, n)
    assert same_floats(c_buf.cpu().numpy(), c.cpu().numpy()) and still_sentinel(d_buf, 0, n)


def test_pruning_happens(renderer):
    """Family a of the sphere: mean triangles tested per walk <= n_tris / 8 (brute force: n_tris).  The cap is a condition, not a
    measurement: the CPU reference walk tests about 4 per walk on this input (test_side_query_host.py)."""
    c = SX.case("sphere")
    set_mesh(renderer, c["verts"])
    p = c["p"][c["rows"]["a"]]
    n_tris = len(c["verts"])
    assert np.array_equal(sides(renderer, p, count_traversal=True), c["ref"]["inside"][c["rows"]["a"]])
    st = renderer.side_query_stats()
    print(f"sphere, family a: {st['tris_tested'] / st['walks']:.2f} triangles and {st['nodes_visited'] / st['walks']:.2f} nodes per walk ({n_tris} triangles)")
    assert st["stack_overflow"] == 0 and st["walks"] >= 2 * len(p) and st["nodes_visited"] >= st["walks"]
    assert 0 < st["tris_tested"] / st["walks"] <= n_tris / 8
    sides(renderer, p[:100])
    st = renderer.side_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted


def test_bounds_and_out_tensors(renderer):
    import torch

    b = set_batch(renderer)
    for n in (1, 65, b["n"]):
        p = tdev(b["p"][:n])
        p0 = p.clone()
        i_buf, x_buf = sentinel(n, torch.int32, 64), sentinel(n, torch.int32, 64, cols=3)
        inside, crossings = renderer.query_sides(p, out=(i_buf[:n], x_buf[:n]), want_crossings=True)
        assert inside.data_ptr() == i_buf.data_ptr() and crossings.data_ptr() == x_buf.data_ptr()
        assert still_sentinel(i_buf, 0, n) and still_sentinel(x_buf, 0, n)
        assert np.array_equal(inside.cpu().numpy(), b["ref"]["inside"][:n]) and np.array_equal(crossings.cpu().numpy(), b["ref"]["brute"][:n])
        i_buf.fill_(-7)
        inside = renderer.query_sides(p, out=i_buf[:n])
        assert inside.data_ptr() == i_buf.data_ptr() and still_sentinel(i_buf, 0, n) and np.array_equal(inside.cpu().numpy(), b["ref"]["inside"][:n])
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32))
    with pytest.raises(ValueError):
        renderer.query_sides(p, out=i_buf[:n - 1])
    with pytest.raises(ValueError):
        renderer.query_sides(p, out=(i_buf[:n], x_buf[:n - 1]), want_crossings=True)


def test_stream_order(renderer):
    """Points made by torch on a stream, the queries behind them on that stream without a host synchronisation, a torch reduction of
    the answers behind the queries; one synchronisation at the end.  (Halving and doubling is exact: the points are the batch's.)"""
    import torch

    b = set_batch(renderer)
    n = b["n"]
    p_half = tdev(b["p"] * f32(0.5))
    ref_i, ref_x = tdev(b["ref"]["inside"]), tdev(b["ref"]["brute"])
    inside, crossings, sd, tri = sentinel(n, torch.int32), sentinel(n, torch.int32, cols=3), sentinel(n, torch.float32), sentinel(n, torch.int32)
    with busy_stream(renderer):
        p = p_half * 2.0
        renderer.query_sides(p, out=(inside, crossings), want_crossings=True, sync=False)
        renderer.query_signed_distance(p, out=(sd, tri), want_points=False, sync=False)
        wrong = (inside != ref_i).sum() + (crossings != ref_x).sum() + ((sd < 0) != (ref_i == 1)).sum() + (tri < 0).sum()
    assert int(wrong) == 0


def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_batch(renderer)
    n = 1000
    p = tdev(b["p"][:n])
    ins, cr = sentinel(n, torch.int32), sentinel(n, torch.int32, cols=3)
    dist, tri, c = sentinel(n, torch.float32), sentinel(n, torch.int32), sentinel(n, torch.float32, cols=3)
    fresh = R.Renderer(0)
    try:
        assert lib.rt_query_sides_device(fresh._ctx, ptr(p), n, None, ptr(ins), ptr(cr), ptr(dist)) == RT_ERR_STATE  # no mesh
        assert lib.rt_query_signed_distance_device(fresh._ctx, ptr(p), None, n, None, None, ptr(dist), ptr(tri), ptr(c), ptr(ins)) == RT_ERR_STATE
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short3=12, short1=4)  # the allocation holds n - 1 rows from the short ones
    hp, short3, short1 = bp.hp, bp.short3, bp.short1
    S, P = R.SideQueryParams, R.PointQueryParams

    def untouched(k):
        assert_untouched(renderer, (ins, cr, dist, tri, c), bp.big, k)

    calls = [(None, n, None, ptr(ins), ptr(cr), ptr(dist)), (ptr(p), n, None, None, ptr(cr), ptr(dist)), (hp, n, None, ptr(ins), ptr(cr), ptr(dist)),
             (ptr(p), n, None, hp, ptr(cr), ptr(dist)), (ptr(p), n, None, ptr(ins), hp, ptr(dist)), (ptr(p), n, None, ptr(ins), ptr(cr), hp),
             (short3, n, None, ptr(ins), ptr(cr), ptr(dist)), (ptr(p), n, None, short1, ptr(cr), ptr(dist)), (ptr(p), n, None, ptr(ins), short3, ptr(dist)),
             (ptr(p), n, None, ptr(ins), ptr(cr), short1), (ptr(p), (1 << 30) + 1, None, ptr(ins), ptr(cr), ptr(dist))] + \
        [(ptr(p), n, prm, ptr(ins), ptr(cr), ptr(dist)) for prm in bad_params(S)]
    for k, args in enumerate(calls):
        assert lib.rt_query_sides_device(ctx, *args) == RT_ERR_INVALID, k
        untouched(k)
    # the pair: a refusal of the SECOND step comes before the first step is enqueued
    pair = [(None, None, n, None, None, ptr(dist), ptr(tri), ptr(c), ptr(ins)), (ptr(p), None, n, None, None, None, ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, n, None, None, ptr(dist), None, ptr(c), ptr(ins)), (ptr(p), hp, n, None, None, ptr(dist), ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, n, None, None, ptr(dist), ptr(tri), hp, ptr(ins)), (ptr(p), None, n, None, None, ptr(dist), ptr(tri), ptr(c), hp),
            (ptr(p), None, n, None, None, ptr(dist), ptr(tri), ptr(c), short1), (ptr(p), None, n, None, None, short1, ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, n, C.byref(P(count_traversal=2)), None, ptr(dist), ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, n, None, C.byref(S(count_traversal=2)), ptr(dist), ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, n, None, C.byref(S(tune_lds_stack=79)), ptr(dist), ptr(tri), ptr(c), ptr(ins)),
            (ptr(p), None, (1 << 30) + 1, None, None, ptr(dist), ptr(tri), ptr(c), ptr(ins))]
    for k, args in enumerate(pair):
        assert lib.rt_query_signed_distance_device(ctx, *args) == RT_ERR_INVALID, k
        untouched(("pair", k))
    assert lib.rt_query_sides_device(ctx, ptr(p), 0, None, ptr(ins), ptr(cr), ptr(dist)) == 0  # n = 0 is accepted, and does nothing
    assert lib.rt_query_sides_device(ctx, None, 0, None, None, None, None) == 0
    assert lib.rt_query_signed_distance_device(ctx, None, None, 0, None, None, None, None, None, None) == 0
    untouched("n = 0")
    assert len(renderer.query_sides(p[:0])) == 0 and len(renderer.query_signed_distance(p[:0])[0]) == 0
    # the context still answers
    assert np.array_equal(renderer.query_sides(p, out=ins).cpu().numpy(), b["ref"]["inside"][:n])


def test_the_three_kinds_of_stats_do_not_mix(renderer):
    """Each query kind keeps its own counters until somebody reads them: ray, point and side queries issued back to back, in every
    order, each report their own."""
    import itertools

    b = set_batch(renderer)
    n = b["n"]
    rng = np.random.default_rng(47)
    o = b["p"].copy()
    o[rng.permutation(n)[:100], 0] = np.nan
    pp = b["p"].copy()
    pp[rng.permutation(n)[:300], 1] = np.inf
    ps = b["p"].copy()
    bad = rng.permutation(n)[:500]
    ps[bad, 2] = np.nan
    to, td, tpp, tps = tdev(o), tdev(np.broadcast_to(SX.D[0], o.shape).copy()), tdev(pp), tdev(ps)
    thirds = int(np.delete(b["ref"]["third"], bad).sum())

    def rays():
        renderer.query_rays(to, td)

    def points():
        renderer.query_points(tpp, count_traversal=True)

    def sides_():
        got = renderer.query_sides(tps, count_traversal=True).cpu().numpy()
        assert np.array_equal(np.delete(got, bad), np.delete(b["ref"]["inside"], bad)) and (got[bad] == INVALID).all()

    for order in itertools.permutations((rays, points, sides_)):
        for q in order:
            q()
        rs, pst, ss = renderer.ray_query_stats(), renderer.point_query_stats(), renderer.side_query_stats()  # only now
        assert (rs["invalid_rays"], rs["rays"]) == (100, n), rs
        assert (pst["invalid_points"], pst["points"]) == (300, n) and pst["nodes_visited"] > 0, pst
        assert (ss["invalid_points"], ss["points"], ss["third_walks"], ss["walks"]) == (500, n, thirds, 2 * (n - 500) + thirds) and ss["nodes_visited"] > 0, ss
        assert rs["ms"] > 0 and pst["ms"] > 0 and ss["ms"] > 0


def test_rendering_and_sharing_are_undisturbed(renderer):
    b = set_batch(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 0.1, 4.0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r, **more):
        return pt_frame(r, **kw, **more)

    before, before_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert before[1][0] > 0 and before[1][3] == 0
    inside, crossings = sides(renderer, b["p"], want_crossings=True, tune_lds_stack=1)
    assert np.array_equal(inside, b["ref"]["inside"]) and np.array_equal(crossings, b["ref"]["brute"])
    renderer.query_signed_distance(tdev(b["p"]), tune_lds_stack=1)
    after, after_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before_spilling[0], after_spilling[0]) and before_spilling[1] == after_spilling[1]
    # a shared mesh stays shared: the queries only read it
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        assert np.array_equal(sides(other, b["p"]), b["ref"]["inside"])
        other.query_signed_distance(tdev(b["p"]))
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()
