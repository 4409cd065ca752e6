"""All-hits ray queries on device tensors (Renderer.count_ray_hits / list_ray_hits, rt_count_ray_hits_device / rt_fill_ray_hits_device /
rt_list_ray_hits_device) on the GPU.

The reference is tests/hit_exact.py's native brute force (tests/native/hit_query_ref.cpp: the arithmetic of csrc/ray_parity.h over all
triangles, sorted by (t, index), no tree), which the kernel must match bit for bit in counts, offsets and every list entry; that
reference in turn is held to the oracle and to its own tree walk on the CPU (tests/test_hit_query_host.py).  The first tests run every
family on its meshes; the others need ONE batch on ONE mesh whose size they can cut, tile and plant rays into: the 10 800 rays of the
sphere's side case, shuffled, a third of them with a limit.  The listing protocol's tests are tests/gpu_listing.py's, on this batch."""
import functools

import numpy as np
import pytest

import gpu_listing as L
import hit_exact as H
import ray_exact as X
import sign_exact as SX
import raytracing_engine_amd as R
from gpu_query import RT_ERR_STATE, pt_frame, ptr, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
INVALID = H.INVALID
ALL = SX.CLOSED + SX.OPEN


def check_case(renderer, o, d, tmax, ref, what, **kw):
    """The three ways to ask against the reference of rays (o, d, tmax): count, list without a capacity (count + fill), list with one."""
    L.check_case(renderer, L.HITS, (o, d, tmax), ref, what, **kw)


# ---- 1. every family, every tree ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", X.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, fam):
    """With and without limits (at a hit's t, one ulp above it, half of it: the four blocks of the case)."""
    for p in H.family_case(fam):
        set_mesh(renderer, p["verts"])
        check_case(renderer, p["o"], p["d"], p["tmax"], p["ref"], (fam, p["mesh"]))


@pytest.mark.parametrize("name", ALL)
def test_the_meshes_of_the_side_query(renderer, name):
    """sign_exact's points along D[k]: the lists, and the counts against query_sides' crossings on the same device arrays."""
    c = H.side_case(name)
    set_mesh(renderer, c["verts"])
    check_case(renderer, c["o"], c["d"], None, c["ref"], name)
    n = c["n"]
    p = tdev(c["side"]["p"])
    _, crossings = renderer.query_sides(p, want_crossings=True)
    for k in range(3):
        dk = tdev(np.broadcast_to(SX.D[k], (n, 3)).copy())
        counts = renderer.count_ray_hits(p, dk)
        assert np.array_equal(counts.cpu().numpy(), crossings[:, k].cpu().numpy()), (name, k)


@functools.lru_cache(maxsize=None)
def moved_reference(fam, k):
    p = H.family_case(fam)[k]
    v = X.moved(p["verts"])
    return v, H.reference(v, p["o"], p["d"], p["tmax"])


@pytest.mark.parametrize("fam", ["a", "h"])
def test_two_level_device_built_and_refitted_trees(renderer, fam):
    for k, p in enumerate(H.family_case(fam)):
        v, a, e = X._with_surface(p["verts"])
        renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_case(renderer, p["o"], p["d"], p["tmax"], p["ref"], (fam, p["mesh"], "two-level"))
        renderer.set_mesh_device(tdev(v), tdev(a), tdev(e))
        check_case(renderer, p["o"], p["d"], p["tmax"], p["ref"], (fam, p["mesh"], "device build"))
        mv, mref = moved_reference(fam, k)
        assert mref["same"].all() and mref["hits"] > 0
        renderer.refit_mesh_device(tdev(mv))
        check_case(renderer, p["o"], p["d"], p["tmax"], mref, (fam, p["mesh"], "refit to moved vertices"))


def test_the_stack(renderer):
    """256 hits in one slice: the insertion at its longest, from the front and from behind."""
    s = H.stack()
    set_mesh(renderer, s["verts"])
    assert s["ref"]["count"][0] == H.STACK_QUADS and (np.diff(s["ref"]["t"][:H.STACK_QUADS]) > 0).all()
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_lds_stack=1)):
        check_case(renderer, s["o"], s["d"], s["tmax"], s["ref"], ("stack", kw), **kw)


def test_the_duplicates(renderer):
    """Equal t, ordered by index."""
    d = H.duplicates()
    set_mesh(renderer, d["verts"])
    t, tri = d["ref"]["t"].reshape(-1, 2), d["ref"]["tri"].reshape(-1, 2)
    assert H.same_bits(t[:, 0], t[:, 1]) and (tri[:, 0] < tri[:, 1]).all() and len(t) > 250
    check_case(renderer, d["o"], d["d"], None, d["ref"], "duplicates")
    renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(d["verts"])))
    check_case(renderer, d["o"], d["d"], None, d["ref"], "duplicates, device build")


# ---- 2. one batch on the sphere --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    c = H.side_case("sphere")
    rng = np.random.default_rng(13)
    perm = rng.permutation(len(c["o"]))
    o, d = np.ascontiguousarray(c["o"][perm]), np.ascontiguousarray(c["d"][perm])
    tmax = np.where(rng.random(len(o)) < 1 / 3, rng.uniform(0.3, 3.0, len(o)), np.inf).astype(f32)
    ref = H.reference(c["verts"], o, d, tmax)
    assert ref["same"].all() and ref["hits"] > len(o) // 2 and ref["invalid"] == 0
    return dict(v=c["verts"], o=o, d=d, tmax=tmax, ref=ref, n=len(o), reach=SX.PX.reach_of(c["verts"]))


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


def src(b):
    return b["o"], b["d"], b["tmax"]


def first(b, n):
    return b["o"][:n], b["d"][:n], b["tmax"][:n], H.rows(b["ref"], slice(0, n))


def test_against_the_other_kinds_on_the_same_arrays(renderer):
    """First entry == query_rays' closest hit; count > 0 == query_rays(any_hit=True) with the same tmax."""
    b = set_batch(renderer)
    to, td, tt = tdev(b["o"]), tdev(b["d"]), tdev(b["tmax"])
    offsets, t, tri, counts = renderer.list_ray_hits(to, td, tt)
    ct, ctri = renderer.query_rays(to, td, tt)
    occluded = renderer.query_rays(to, td, tt, any_hit=True)
    first_t, first_tri = H.first_hits(dict(count=counts.cpu().numpy(), offsets=offsets.cpu().numpy(), t=t.cpu().numpy(), tri=tri.cpu().numpy()))
    assert H.same_bits(first_t, ct.cpu().numpy()) and np.array_equal(first_tri, ctri.cpu().numpy())
    assert np.array_equal(counts.cpu().numpy() > 0, occluded.cpu().numpy() == 1) and 0.2 < (counts > 0).float().mean() < 0.9


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 1 000 rays every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not."""
    b = set_batch(renderer)
    assert n <= b["n"]
    o, d, tmax, ref = first(b, n)
    for kw in TUNINGS:
        check_case(renderer, o, d, tmax, ref, (n, kw), **kw)


def scattered(b, n):
    """n rays drawn from the batch by a fixed scatter, and their reference."""
    idx = (np.arange(n, dtype=np.int64) * 2654435761) % b["n"]
    return b["o"][idx], b["d"][idx], b["tmax"][idx], H.rows(b["ref"], idx)


@pytest.mark.parametrize("n", [4094, 4095, 4096, 70000])
def test_the_scan_around_its_tile(renderer, n):
    """n + 1 offsets around the scan's 4 096-element tile, and several tiles."""
    b = set_batch(renderer)
    o, d, tmax, ref = scattered(b, n)
    L.scan_around_its_tile(renderer, L.HITS, (o, d, tmax), ref, n)


def test_more_rays_than_lanes(renderer):
    b = set_batch(renderer)
    n = 600000
    assert n > 256 * 8 * 256
    o, d, tmax, ref = scattered(b, n)
    check_case(renderer, o, d, tmax, ref, n)


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest in global memory."""
    for name in ("sphere", "soup"):
        c = H.side_case(name)
        set_mesh(renderer, c["verts"])
        assert renderer.pt_stats()["bvh_depth"] > 1
        check_case(renderer, c["o"], c["d"], None, c["ref"], (name, "one LDS entry"), tune_lds_stack=1)


# ---- 3. capacity and offsets -----------------------------------------------------------------------------------------------------

def test_capacity(renderer):
    """Capacity at the total, one below it, half of it and 0: a slice that does not fit is not touched, every other one is complete, the
    offsets are the full sums."""
    b = set_batch(renderer)
    L.capacity(renderer, L.HITS, src(b), b["ref"])


def test_foreign_offsets_are_safe(renderer):
    """The fill step on offsets it did not make: nothing outside [0, capacity) is written, a slice shorter than its ray's hits keeps the
    first of them, and slice_overflow counts the rest."""
    b = set_batch(renderer)
    L.foreign_offsets(renderer, L.HITS, src(b), b["ref"])


def test_list_is_count_then_fill(renderer):
    b = set_batch(renderer)
    L.list_is_count_then_fill(renderer, L.HITS, src(b), b["ref"])


# ---- 4. invalid rays, bounds, refusals -------------------------------------------------------------------------------------------

def test_invalid_rays(renderer):
    b = set_batch(renderer)
    reach, n = b["reach"], b["n"]
    rng = np.random.default_rng(43)
    where = rng.permutation(n)
    o, d, tmax = b["o"].copy(), b["d"].copy(), b["tmax"].copy()
    invalid = np.zeros(n, bool)
    k = 0
    for arr in (o, d):  # a NaN or an infinity in one component of the origin or of the direction
        for comp in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                arr[where[k], comp] = bad
                invalid[where[k]] = True
                k += 1
    for comp in range(3):  # one step beyond the reach
        for sign in (1, -1):
            o[where[k], comp] = sign * np.nextafter(reach, INF)
            invalid[where[k]] = True
            k += 1
    tmax[where[k:k + 3]] = np.nan
    invalid[where[k:k + 3]] = True
    k += 3
    edge = where[k:k + 12]  # exactly at the reach: valid
    for j, i in enumerate(edge):
        o[i, j % 3] = (1 if j % 2 else -1) * reach
    k += 12
    nothing = where[k:k + 9]  # valid, and no hit: tmax <= 0, a zero direction
    tmax[nothing[:3]], tmax[nothing[3:6]] = 0.0, -INF
    d[nothing[6:]] = [0.0, -0.0, 0.0]
    exp = H.reference(b["v"], o, d, tmax)
    assert np.array_equal(exp["count"] == INVALID, invalid) and (exp["count"][edge] >= 0).all() and (exp["count"][nothing] == 0).all() and exp["same"].all()
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        check_case(renderer, o, d, tmax, exp, ("invalid rays", kw), **kw)
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive - 4 000 invalid rays through one workgroup
    o_bad = np.tile(b["o"], (2, 1))[:4000].copy()
    o_bad[:, 1] = np.nan
    d_bad = np.tile(b["d"], (2, 1))[:4000]
    offsets, t, tri, counts = renderer.list_ray_hits(tdev(o_bad), tdev(d_bad), capacity=16, tune_max_blocks=1)
    st = renderer.hit_query_stats()
    assert (counts == INVALID).all() and (offsets == 0).all()
    assert (st["invalid_rays"], st["hits"], st["hits_written"], st["rays"]) == (4000, 0, 0, 4000)
    d_bad = b["d"].copy()
    d_bad[:1024, 2] = -np.inf
    exp = H.reference(b["v"], b["o"], d_bad, b["tmax"])
    assert (exp["count"][:1024] == INVALID).all() and exp["invalid"] == 1024
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        check_case(renderer, b["o"], d_bad, b["tmax"], exp, ("1 024 invalid rays in front", kw), **kw)


def test_bounds_and_out_tensors(renderer):
    """Sentinels behind every output; the inputs are only read."""
    b = set_batch(renderer)
    L.bounds_and_out_tensors(renderer, L.HITS, [(x[:3], x[3]) for x in (first(b, n) for n in (1, 65, b["n"]))])


def test_stream_order(renderer):
    """Rays made by torch on a stream, the queries behind them on that stream without a host synchronisation, a torch reduction of the
    answers behind the queries; one synchronisation at the end.  (Halving and doubling is exact: the rays are the batch's.)"""
    b = set_batch(renderer)
    L.stream_order(renderer, L.HITS, src(b), b["ref"])


def test_errors_write_nothing(renderer):
    b = set_batch(renderer)
    n = 1000
    o, d, tmax, ref = first(b, n)
    e = L.Refusals(renderer, L.HITS, (o, d, tmax), ref, short3=12)  # (one row short of n x 3)
    fresh = R.Renderer(0)
    try:
        e.every_entry(fresh._ctx, RT_ERR_STATE, "no mesh")
    finally:
        fresh.close()
    to, td, tt = (ptr(x) for x in e.t)
    hp, short3, short1 = e.bp.hp, e.bp.short3, e.bp.short1
    e.tables([(None, td, tt, n, None), (to, None, tt, n, None), (hp, td, tt, n, None), (to, hp, tt, n, None), (to, td, hp, n, None), (short3, td, tt, n, None),
              (to, short3, tt, n, None), (to, td, short1, n, None), (to, td, tt, (1 << 30) + 1, None)] + [(to, td, tt, n, prm) for prm in e.bad_params])
    e.nothing_to_do((e.t[0][:0], e.t[1][:0]), (e.t[0][:0], e.t[1][:0]))
    e.still_answers()


# ---- 5. what the rest of the process keeps ---------------------------------------------------------------------------------------

def test_the_four_kinds_of_stats_do_not_mix(renderer):
    """Each query kind keeps its own counters until somebody reads them: ray, point, side and hit queries issued back to back, in
    several orders, each report their own."""
    import itertools

    b = set_batch(renderer)
    n, ref = b["n"], b["ref"]
    rng = np.random.default_rng(47)
    p = H.side_case("sphere")["side"]["p"]
    m = len(p)
    o = p.copy()
    o[rng.permutation(m)[:100], 0] = np.nan
    pp = p.copy()
    pp[rng.permutation(m)[:300], 1] = np.inf
    ps = p.copy()
    ps[rng.permutation(m)[:500], 2] = np.nan
    oh = b["o"].copy()
    bad = rng.permutation(n)[:700]
    oh[bad, 1] = np.inf
    exp = H.reference(b["v"], oh, b["d"], b["tmax"])
    to, td, tpp, tps = tdev(o), tdev(np.broadcast_to(SX.D[0], o.shape).copy()), tdev(pp), tdev(ps)
    toh, tdh, tth = tdev(oh), tdev(b["d"]), tdev(b["tmax"])

    def rays():
        renderer.query_rays(to, td)

    def points():
        renderer.query_points(tpp, count_traversal=True)

    def sides():
        renderer.query_sides(tps, count_traversal=True)

    def hits():
        assert np.array_equal(renderer.count_ray_hits(toh, tdh, tth, count_traversal=True).cpu().numpy(), exp["count"])

    for order in list(itertools.permutations((rays, points, sides, hits)))[::5]:
        for q in order:
            q()
        rs, pst, ss, hs = renderer.ray_query_stats(), renderer.point_query_stats(), renderer.side_query_stats(), renderer.hit_query_stats()  # only now
        assert (rs["invalid_rays"], rs["rays"]) == (100, m), rs
        assert (pst["invalid_points"], pst["points"]) == (300, m) and pst["nodes_visited"] > 0, pst
        assert (ss["invalid_points"], ss["points"]) == (500, m) and ss["nodes_visited"] > 0, ss
        assert (hs["invalid_rays"], hs["rays"], hs["hits"], hs["launches"]) == (700, n, exp["hits"], 1) and hs["nodes_visited"] > 0, hs
        assert rs["ms"] > 0 and pst["ms"] > 0 and ss["ms"] > 0 and hs["ms"] > 0


def test_rendering_and_sharing_are_undisturbed(renderer):
    b = set_batch(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 0.1, 4.0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r, **more):
        return pt_frame(r, **kw, **more)

    before, before_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert before[1][0] > 0 and before[1][3] == 0
    check_case(renderer, b["o"], b["d"], b["tmax"], b["ref"], "between frames", tune_lds_stack=1)
    after, after_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before_spilling[0], after_spilling[0]) and before_spilling[1] == after_spilling[1]
    # a shared mesh stays shared: the queries only read it
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        check_case(other, b["o"], b["d"], b["tmax"], b["ref"], "the other context")
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()


def test_pruning_happens(renderer):
    """Family a of the 960-triangle sphere: mean triangles tested per ray <= n_tris / 8 (brute force: n_tris).  The cap is a condition,
    not a measurement: the CPU reference walk tests about 4 per walk on this input (test_hit_query_host.py)."""
    c = H.side_case("sphere")
    set_mesh(renderer, c["verts"])
    n_tris = len(c["verts"])
    assert n_tris == 960
    a = c["side"]["rows"]["a"]
    sel = np.r_[tuple(np.arange(c["n"])[a] + k * c["n"] for k in range(3))]
    ref = H.rows(c["ref"], sel)
    counts = renderer.count_ray_hits(tdev(c["o"][sel]), tdev(c["d"][sel]), count_traversal=True)
    st = renderer.hit_query_stats()
    assert np.array_equal(counts.cpu().numpy(), ref["count"])
    print(f"sphere, family a: {st['tris_tested'] / len(sel):.2f} triangles and {st['nodes_visited'] / len(sel):.2f} nodes per ray, {st['hits'] / len(sel):.2f} hits ({n_tris} triangles)")
    assert st["stack_overflow"] == 0 and st["nodes_visited"] >= len(sel)
    assert 0 < st["tris_tested"] / len(sel) <= n_tris / 8
    renderer.count_ray_hits(tdev(c["o"][sel][:100]), tdev(c["d"][sel][:100]))
    st = renderer.hit_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted
