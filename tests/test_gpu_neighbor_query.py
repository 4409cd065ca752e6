"""Neighbour queries on device tensors (Renderer.count_neighbors / list_neighbors, rt_count_neighbors_device / rt_fill_neighbors_device /
rt_list_neighbors_device) on the GPU.

The reference is tests/neighbor_exact.py's native brute force (tests/native/neighbor_query_ref.cpp: the arithmetic of csrc/point_tri.h
over all triangles, everything with d2 < rmax * rmax, sorted by (d2, index), no tree), which the kernel must match bit for bit in counts,
offsets and every list entry; its tree walk under the kernel's culling rule gives the nodes and triangles the kernel must count, exactly.
That reference in turn is held to its own walk, to the closest-point reference and to float64 on the CPU
(tests/test_neighbor_query_host.py).  The first tests run every family on its meshes under every radius; the others need ONE batch on
ONE mesh whose size they can cut, tile and plant points into: family b's 300 points on the terrain under the ten finite radius
variants, shuffled.  The listing protocol's tests are tests/gpu_listing.py's, on this batch."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_listing as L
import neighbor_exact as NX
import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
from gpu_query import RT_ERR_STATE, dev, pt_frame, ptr, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = NX.INF
INVALID = NX.INVALID


def check_lists(got, ref, what):
    """(offsets, dist, tri, counts) as tensors against a reference dict, bit for bit."""
    L.check_lists(L.NEIGHBORS, got, ref, what)


def check_case(renderer, p, rmax, ref, what, exact_work=False, **kw):
    """The three ways to ask against the reference of points p under radii rmax: count, list without a capacity (count + fill), list with
    one.  exact_work: the tree is the host-built single-level one, whose walk the reference has made: nodes and triangles agree exactly."""
    L.check_case(renderer, L.NEIGHBORS, (p, rmax), ref, what, exact_work=exact_work, **kw)


# ---- 1. every family, every radius, every tree ------------------------------------------------------------------------------------
# The +inf block of a part (neighbor_exact: its first eight points, on every mesh of at most 2 000 triangles - all but the doubled
# soup) is counted and listed like every other block, on every tree: lists as long as the mesh, the insertion at its longest.

@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, fam):
    """Under every radius variant (the blocks of the case), with the walk's work counted and compared."""
    for c in NX.family_case(fam):
        assert ("inf" in c["blocks"]) == (c["mesh"] != "soup_dup")
        set_mesh(renderer, c["verts"])
        check_case(renderer, c["p"], c["rmax"], c["ref"], (fam, c["mesh"]), exact_work=True)


@pytest.mark.parametrize("tree", ["two-level", "device build", "refit to moved vertices"])
@pytest.mark.parametrize("fam", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, fam, tree):
    for c in NX.family_case(fam, moved=tree.startswith("refit")):
        if tree == "two-level":
            renderer.set_mesh(*X._with_surface(c["verts"]), bvh_levels=2, blas_chunks=64)
        else:
            renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(PX.mesh(c["mesh"]))))
            if tree.startswith("refit"):
                assert c["ref"]["neighbors"] > 0 and not np.array_equal(c["verts"], PX.mesh(c["mesh"]))
                renderer.refit_mesh_device(tdev(c["verts"]))
        check_case(renderer, c["p"], c["rmax"], c["ref"], (fam, c["mesh"], tree))


def test_a_scalar_radius_is_an_array_of_it(renderer):
    """rmax_all with rmax_dev = NULL against an array filled with the same value, and against the reference."""
    import torch

    c = NX.family_case("b")[0]
    set_mesh(renderer, c["verts"])
    p = c["p"][:c["n"]]
    tp = tdev(p)
    for r in (float(np.median(NX.kth_dist(c["free"], 8))), 0.0, -1.0, float("inf"), 2.0 ** -76, float("nan")):
        ref = NX.reference(c["verts"], p, f32(r))
        arr = torch.full((len(p),), r, dtype=torch.float32, device=dev())
        one, many = renderer.list_neighbors(tp, r), renderer.list_neighbors(tp, arr)
        for x, y in zip(one, many):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), r
        check_lists(one, ref, r)
        assert torch.equal(renderer.count_neighbors(tp, r), renderer.count_neighbors(tp, arr))
        assert renderer.neighbor_query_stats()["invalid_points"] == (len(p) if r != r else 0)
    # with an array given, rmax_all is ignored
    prm = R.NeighborQueryParams()
    arr = tdev(c["rmax"][c["blocks"]["k8_above"]])
    cnt = torch.empty(len(p), dtype=torch.int32, device=dev())
    assert R.load().rt_count_neighbors_device(renderer._ctx, ptr(tp), ptr(arr), float("nan"), len(p), C.byref(prm), ptr(cnt), None) == 0
    renderer.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), NX.rows(c["ref"], c["blocks"]["k8_above"])["count"])


def test_pruning_happens(renderer):
    """Family b on the terrain with the k = 8 radius: mean triangles tested per point <= n_tris / 8 (brute force: n_tris), and exactly the
    reference walk's.  The cap is a condition, not a measurement: the CPU reference tests about 10 per point here
    (test_neighbor_query_host.py checks that it is within the cap)."""
    c = NX.family_case("b")[0]
    assert c["mesh"] == "terrain"
    set_mesh(renderer, c["verts"])
    block = c["blocks"]["k8_above"]
    ref = NX.rows(c["ref"], block)
    n, n_tris = c["n"], len(c["verts"])
    assert ref["tris_total"] / n <= n_tris / 8
    counts = renderer.count_neighbors(tdev(c["p"][block]), tdev(c["rmax"][block]), count_traversal=True)
    st = renderer.neighbor_query_stats()
    assert np.array_equal(counts.cpu().numpy(), ref["count"])
    print(f"terrain, family b, k = 8: {st['tris_tested'] / n:.2f} triangles and {st['nodes_visited'] / n:.2f} nodes per point, {st['neighbors'] / n:.2f} neighbours ({n_tris} triangles)")
    assert st["stack_overflow"] == 0 and (st["nodes_visited"], st["tris_tested"]) == (ref["nodes_total"], ref["tris_total"])
    assert 0 < st["tris_tested"] / n <= n_tris / 8
    renderer.count_neighbors(tdev(c["p"][block][:100]), tdev(c["rmax"][block][:100]))
    st = renderer.neighbor_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted


# ---- 2. one batch on the terrain ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    c = NX.family_case("b")[0]
    stop = c["blocks"]["inf"].start  # the finite radii
    perm = np.random.default_rng(13).permutation(stop)
    p, rmax = np.ascontiguousarray(c["p"][perm]), np.ascontiguousarray(c["rmax"][perm])
    ref = NX.rows(c["ref"], perm)
    above = np.nonzero((perm >= c["blocks"]["k1_above"].start) & (perm < c["blocks"]["k1_above"].stop))[0]
    assert ref["neighbors"] > 5 * len(p) and ref["invalid"] == 0 and ref["count"].max() <= NX.LONGEST
    return dict(v=c["verts"], p=p, rmax=rmax, ref=ref, n=len(p), reach=PX.reach_of(c["verts"]), k1_above=above)


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


def src(b):
    return b["p"], b["rmax"]


def first(b, n):
    return b["p"][:n], b["rmax"][:n], NX.rows(b["ref"], slice(0, n))


def test_against_query_points_on_the_same_arrays(renderer):
    """Entry 0 == query_points' answer (tri and dist bitwise); count > 0 == query_points finds a hit with that rmax."""
    b = set_batch(renderer)
    tp, tr = tdev(b["p"]), tdev(b["rmax"])
    offsets, dist, tri, counts = renderer.list_neighbors(tp, tr)
    pd, pt, _ = renderer.query_points(tp, tr, want_points=False)
    got = dict(count=counts.cpu().numpy(), offsets=offsets.cpu().numpy(), dist=dist.cpu().numpy(), tri=tri.cpu().numpy())
    first_dist, first_tri = NX.first_entries(got)
    assert NX.same_bits(first_dist, pd.cpu().numpy()) and np.array_equal(first_tri, pt.cpu().numpy())
    assert np.array_equal(got["count"] > 0, pt.cpu().numpy() >= 0) and 0.2 < (counts > 0).float().mean() < 0.9


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 1 000 points every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not."""
    b = set_batch(renderer)
    assert n <= b["n"]
    p, rmax, ref = first(b, n)
    for kw in TUNINGS:
        check_case(renderer, p, rmax, ref, (n, kw), exact_work=True, **kw)


def scattered(b, n, among=None):
    """n points drawn from the batch (or from its rows `among`) by a fixed scatter, and their reference."""
    idx = (np.arange(n, dtype=np.int64) * 2654435761) % (b["n"] if among is None else len(among))
    idx = idx if among is None else among[idx]
    return b["p"][idx], b["rmax"][idx], NX.rows(b["ref"], idx)


@pytest.mark.parametrize("n", [4094, 4095, 4096])
def test_the_scan_around_its_tile(renderer, n):
    """n + 1 = 4 095, 4 096, 4 097 offsets: around the scan's 4 096-element tile."""
    b = set_batch(renderer)
    p, rmax, ref = scattered(b, n)
    L.scan_around_its_tile(renderer, L.NEIGHBORS, (p, rmax), ref, n)


def test_more_points_than_lanes(renderer):
    """600 000 points with the radius one ulp above their nearest triangle."""
    b = set_batch(renderer)
    n = 600000
    assert n > 256 * 8 * 256
    p, rmax, ref = scattered(b, n, b["k1_above"])
    assert n // 8 < ref["neighbors"] < 4 * n  # (two thirds of the points lie on the surface: no radius is one ulp above 0)
    check_case(renderer, p, rmax, ref, n, exact_work=True)


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest in global memory; no overflow (check_case asserts it)."""
    b = set_batch(renderer)
    assert renderer.pt_stats()["bvh_depth"] > 2
    check_case(renderer, b["p"], b["rmax"], b["ref"], "one LDS entry", exact_work=True, tune_lds_stack=1)
    c = NX.family_case("f")[0]
    set_mesh(renderer, c["verts"])
    check_case(renderer, c["p"], c["rmax"], c["ref"], "one LDS entry, duplicated soup", exact_work=True, tune_lds_stack=1)


# ---- 3. capacity and offsets -----------------------------------------------------------------------------------------------------

def test_capacity(renderer):
    """Capacity at the total, one below it, half of it and 0: a slice that does not fit is not touched, every other one is complete, the
    offsets are the full sums."""
    b = set_batch(renderer)
    L.capacity(renderer, L.NEIGHBORS, src(b), b["ref"])


def test_foreign_offsets_are_safe(renderer):
    """The fill step on offsets it did not make: nothing outside [0, capacity) is written, a slice shorter than its point's list keeps the
    first entries, and slice_overflow counts the rest."""
    b = set_batch(renderer)
    L.foreign_offsets(renderer, L.NEIGHBORS, src(b), b["ref"])


def test_list_is_count_then_fill(renderer):
    b = set_batch(renderer)
    L.list_is_count_then_fill(renderer, L.NEIGHBORS, src(b), b["ref"])


# ---- 4. invalid points, bounds, refusals -------------------------------------------------------------------------------------------

def test_invalid_points(renderer):
    b = set_batch(renderer)
    reach, n = b["reach"], b["n"]
    rng = np.random.default_rng(43)
    where = rng.permutation(n)
    p, rmax = b["p"].copy(), b["rmax"].copy()
    invalid = np.zeros(n, bool)
    k = 0
    for comp in range(3):  # a NaN or an infinity in one component
        for bad in (np.nan, np.inf, -np.inf):
            p[where[k], comp] = bad
            invalid[where[k]] = True
            k += 1
    for comp in range(3):  # one step beyond the reach
        for sign in (1, -1):
            p[where[k], comp] = sign * np.nextafter(reach, INF)
            invalid[where[k]] = True
            k += 1
    rmax[where[k:k + 3]] = np.nan
    invalid[where[k:k + 3]] = True
    k += 3
    edge = where[k:k + 12]  # exactly at the reach: valid
    for j, i in enumerate(edge):
        p[i, j % 3] = (1 if j % 2 else -1) * reach
    rmax[edge[:6]] = INF  # and every triangle is within +inf of them
    k += 12
    nothing = where[k:k + 9]  # valid, and no neighbour: no radius
    rmax[nothing[:3]], rmax[nothing[3:6]], rmax[nothing[6:]] = 0.0, -INF, 2.0 ** -76
    exp = NX.reference(b["v"], p, rmax)
    assert np.array_equal(exp["count"] == INVALID, invalid) and (exp["count"][edge] >= 0).all() and (exp["count"][edge[:6]] == len(b["v"])).all()
    assert (exp["count"][nothing] == 0).all() and NX.walk_is_brute(exp)
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        check_case(renderer, p, rmax, exp, ("invalid points", kw), exact_work=True, **kw)
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive - 4 000 invalid points through one workgroup
    p_bad = np.tile(b["p"], (2, 1))[:4000].copy()
    p_bad[:, 1] = np.nan
    offsets, dist, tri, counts = renderer.list_neighbors(tdev(p_bad), 1.0, capacity=16, tune_max_blocks=1)
    st = renderer.neighbor_query_stats()
    assert (counts == INVALID).all() and (offsets == 0).all()
    assert (st["invalid_points"], st["neighbors"], st["neighbors_written"], st["points"]) == (4000, 0, 0, 4000)
    p_bad = b["p"].copy()
    p_bad[:1024, 2] = -np.inf
    exp = NX.reference(b["v"], p_bad, b["rmax"])
    assert (exp["count"][:1024] == INVALID).all() and exp["invalid"] == 1024
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        check_case(renderer, p_bad, b["rmax"], exp, ("1 024 invalid points in front", kw), exact_work=True, **kw)


def test_bounds_and_out_tensors(renderer):
    """Sentinels behind every output; the inputs are only read."""
    b = set_batch(renderer)
    L.bounds_and_out_tensors(renderer, L.NEIGHBORS, [(x[:2], x[2]) for x in (first(b, n) for n in (1, 65, b["n"]))])


def test_stream_order(renderer):
    """Points made by torch on a stream, the queries behind them on that stream without a host synchronisation, a torch reduction of the
    answers behind the queries; one synchronisation at the end.  (Halving and doubling is exact: the points are the batch's.)"""
    b = set_batch(renderer)
    L.stream_order(renderer, L.NEIGHBORS, src(b), b["ref"])


def test_errors_write_nothing(renderer):
    b = set_batch(renderer)
    n = 1000
    p, rmax, ref = first(b, n)
    e = L.Refusals(renderer, L.NEIGHBORS, (p, rmax), ref, short3=12)  # (one row short of n x 3)
    fresh = R.Renderer(0)
    try:
        e.every_entry(fresh._ctx, RT_ERR_STATE, "no mesh")
    finally:
        fresh.close()
    tp, tr = (ptr(x) for x in e.t)
    hp, short3, short1 = e.bp.hp, e.bp.short3, e.bp.short1
    e.tables([(None, tr, 0.0, n, None), (hp, tr, 0.0, n, None), (tp, hp, 0.0, n, None), (short3, tr, 0.0, n, None), (tp, short1, 0.0, n, None),
              (short3, None, 1.0, n, None), (tp, tr, 0.0, (1 << 30) + 1, None)] + [(tp, tr, 0.0, n, prm) for prm in e.bad_params])
    e.nothing_to_do((e.t[0][:0], 1.0), (e.t[0][:0], e.t[1][:0]))
    e.still_answers()


# ---- 5. what the rest of the process keeps ---------------------------------------------------------------------------------------

def test_the_five_kinds_of_stats_do_not_mix(renderer):
    """Each query kind keeps its own counters until somebody reads them: ray, point, side, hit and neighbour queries issued back to back,
    in several orders, each report their own."""
    import itertools

    b = set_batch(renderer)
    n, m = b["n"], 1200
    rng = np.random.default_rng(47)
    base = b["p"][:m]

    def spoiled(k, comp, bad):
        q = base.copy()
        q[rng.permutation(m)[:k], comp] = bad
        return tdev(q)

    to, tpp, tps, toh = spoiled(100, 0, np.nan), spoiled(300, 1, np.inf), spoiled(500, 2, np.nan), spoiled(700, 1, np.inf)
    td = tdev(np.broadcast_to(f32([0.0, -1.0, 0.0]), (m, 3)).copy())
    pn = b["p"].copy()
    pn[rng.permutation(n)[:900], 0] = -np.inf
    exp = NX.reference(b["v"], pn, b["rmax"])
    tpn, trn = tdev(pn), tdev(b["rmax"])

    def rays():
        renderer.query_rays(to, td)

    def points():
        renderer.query_points(tpp, count_traversal=True)

    def sides():
        renderer.query_sides(tps, count_traversal=True)

    def hits():
        renderer.count_ray_hits(toh, td, count_traversal=True)

    def neighbors():
        assert np.array_equal(renderer.count_neighbors(tpn, trn, count_traversal=True).cpu().numpy(), exp["count"])

    for order in list(itertools.permutations((rays, points, sides, hits, neighbors)))[::17]:
        for q in order:
            q()
        rs, pst, ss, hs, ns = (renderer.ray_query_stats(), renderer.point_query_stats(), renderer.side_query_stats(), renderer.hit_query_stats(),
                               renderer.neighbor_query_stats())  # only now
        assert (rs["invalid_rays"], rs["rays"]) == (100, m), rs
        assert (pst["invalid_points"], pst["points"]) == (300, m) and pst["nodes_visited"] > 0, pst
        assert (ss["invalid_points"], ss["points"]) == (500, m) and ss["nodes_visited"] > 0, ss
        assert (hs["invalid_rays"], hs["rays"], hs["launches"]) == (700, m, 1) and hs["nodes_visited"] > 0, hs
        assert (ns["invalid_points"], ns["points"], ns["neighbors"], ns["launches"]) == (900, n, exp["neighbors"], 1), ns
        assert (ns["nodes_visited"], ns["tris_tested"]) == (exp["nodes_total"], exp["tris_total"]), ns
        assert rs["ms"] > 0 and pst["ms"] > 0 and ss["ms"] > 0 and hs["ms"] > 0 and ns["ms"] > 0


def test_rendering_and_sharing_are_undisturbed(renderer):
    b = set_batch(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 30.0, 40.0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r, **more):
        return pt_frame(r, **kw, **more)

    before, before_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert before[1][0] > 0 and before[1][3] == 0
    check_case(renderer, b["p"], b["rmax"], b["ref"], "between frames", tune_lds_stack=1)
    after, after_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before_spilling[0], after_spilling[0]) and before_spilling[1] == after_spilling[1]
    # a shared mesh stays shared: the queries only read it
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        check_case(other, b["p"], b["rmax"], b["ref"], "the other context")
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()
