"""CPU tests of the all-hits ray queries (rt_count_ray_hits_device / rt_fill_ray_hits_device / rt_list_ray_hits_device,
Renderer.count_ray_hits / list_ray_hits): the boundary (exports, bindings, NULL contexts, struct layouts,
defaults, the wrappers' refusals), and the answer itself through the native reference tests/native/hit_query_ref.cpp - clean under
ASan + UBSan; its BVH8 walk with the kernels' slab test lists, entry for entry and bit for bit, what its brute force over all triangles
lists, on every family of tests/ray_exact.py with and without limits and on every mesh of tests/sign_exact.py (tree independence: no
GPU needed); a limited list is the unlimited one cut strictly below the limit; the first entry is the oracle's brute-force closest hit;
the counts along D[k] are the side reference's crossings.  The kernel itself is tested on the GPU (tests/test_gpu_hit_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import hit_exact as H
import ray_exact as RX
import sign_exact as SX
import raytracing_engine_amd as R

FUNCTIONS = ("rt_default_hit_query_params", "rt_count_ray_hits_device", "rt_fill_ray_hits_device", "rt_list_ray_hits_device", "rt_get_hit_query_stats")
V = C.c_void_p(16)
P = C.byref(R.HitQueryParams())
KIND = AB.Kind(functions=FUNCTIONS, methods=("count_ray_hits", "list_ray_hits", "hit_query_stats"), params="HitQueryParams", stats="HitQueryStats",
               params_c="rt_hit_query_params", stats_c="rt_hit_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["rays", "invalid_rays", "hits", "hits_written", "incomplete_rays", "slice_overflow", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
               default="rt_default_hit_query_params",
               null_calls=(("rt_count_ray_hits_device", (None, None, None, 0, None, None, None)), ("rt_count_ray_hits_device", (V, V, V, 1, P, V, V)),
                           ("rt_fill_ray_hits_device", (None, None, None, 0, None, None, 0, None, None)), ("rt_fill_ray_hits_device", (V, V, V, 1, P, V, 1, V, V)),
                           ("rt_list_ray_hits_device", (None, None, None, 0, None, None, None, 0, None, None)), ("rt_list_ray_hits_device", (V, V, V, 1, P, V, V, 1, V, V)),
                           ("rt_get_hit_query_stats", (C.byref(R.HitQueryStats()),)), ("rt_default_hit_query_params", ())))
ALL = SX.CLOSED + SX.OPEN
f32 = np.float32


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    AB.struct_layout(KIND, tmp_path)


def test_default_params_are_zeros():
    AB.default_params(KIND)


def test_the_wrappers_check_their_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    for bad in (a, good, good.double(), torch.zeros(3, 4).t(), torch.zeros(4, 4)):
        for call in (r.count_ray_hits, r.list_ray_hits, lambda x, y: r.list_ray_hits(x, y, capacity=8)):
            with pytest.raises(ValueError):
                call(bad, bad)


def test_the_wrappers_compare_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    o, d = torch.zeros(4, 3), torch.zeros(4, 3)
    cnt, off = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    t, tri = torch.zeros(8), torch.zeros(8, dtype=torch.int32)
    for call in (r.count_ray_hits, r.list_ray_hits, lambda *a, **k: r.list_ray_hits(*a, capacity=8, **k)):
        with pytest.raises(ValueError, match="origins"):
            call(torch.zeros(4, 4), d)
        with pytest.raises(ValueError, match="disagree"):
            call(o, torch.zeros(5, 3))
        for bad_tmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1)):
            with pytest.raises(ValueError, match="tmax"):
                call(o, d, tmax=bad_tmax)
    with pytest.raises(ValueError, match="counts"):
        r.count_ray_hits(o, d, out=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="counts"):
        r.count_ray_hits(o, d, out=torch.zeros(4))  # float32 where int32 is due
    with pytest.raises(TypeError, match="count_ray_hits"):
        r.count_ray_hits(o, d, tune_nothing=1)
    with pytest.raises(TypeError, match="list_ray_hits"):
        r.list_ray_hits(o, d, tune_nothing=1)
    with pytest.raises(TypeError, match="list_ray_hits"):
        r.list_ray_hits(o, d, capacity=8, count_traversal=True)  # the wrapper exposes the tuning only
    with pytest.raises(ValueError, match="capacity"):
        r.list_ray_hits(o, d, out=(off, t, tri, cnt))  # out without a capacity
    with pytest.raises(ValueError, match="capacity"):
        r.list_ray_hits(o, d, capacity=-1)
    with pytest.raises(ValueError, match="out"):
        r.list_ray_hits(o, d, capacity=8, out=(off, t, tri))
    with pytest.raises(ValueError, match="offsets"):
        r.list_ray_hits(o, d, capacity=8, out=(torch.zeros(4, dtype=torch.int64), t, tri, cnt))  # n where n + 1 is due
    with pytest.raises(ValueError, match="offsets"):
        r.list_ray_hits(o, d, capacity=8, out=(torch.zeros(5, dtype=torch.int32), t, tri, cnt))
    with pytest.raises(ValueError, match="out t"):
        r.list_ray_hits(o, d, capacity=8, out=(off, torch.zeros(7), tri, cnt))
    with pytest.raises(ValueError, match="out tri"):
        r.list_ray_hits(o, d, capacity=8, out=(off, t, torch.zeros(8), cnt))
    with pytest.raises(ValueError, match="counts"):
        r.list_ray_hits(o, d, capacity=8, out=(off, t, tri, torch.zeros(5, dtype=torch.int32)))
    # the old methods accept and refuse what they did
    with pytest.raises(TypeError, match=r"query_rays\(\) got an unexpected keyword argument 'tune_nothing'"):
        r.query_rays(o, d, tune_nothing=1)


# ---- the native reference ------------------------------------------------------------------------------------------------------
def check_reference(ref, what):
    """What every answer of the reference satisfies by itself: walk == brute force, the offsets are the counts' sums, every list
    ascends strictly in (t, tri), every t is positive."""
    count = ref["count"]
    assert ref["same"].all(), (what, np.nonzero(ref["same"] == 0)[0][:8])
    assert np.array_equal(ref["walk_count"], np.maximum(count, 0)), what
    assert np.array_equal(np.diff(ref["offsets"]), np.maximum(count, 0)) and ref["offsets"][0] == 0 and ref["offsets"][-1] == ref["hits"], what
    assert ref["invalid"] == int((count == H.INVALID).sum()) and (count >= H.INVALID).all() and (count != -1).all(), what
    t, tri = ref["t"].astype(np.float64), ref["tri"].astype(np.int64)
    assert (t > 0).all() and np.isfinite(t).all(), what
    inner = np.ones(len(t), bool)
    inner[ref["offsets"][:-1][ref["offsets"][:-1] < len(t)]] = False  # a list's first entry has no predecessor
    later = (t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (tri[1:] > tri[:-1]))
    assert later[inner[1:]].all(), what


def test_the_reference_is_clean_under_sanitizers():
    """ASan + UBSan build of the stand-alone program on a slice of every batch - limits, invalid rays, zero directions, empty intervals
    and an empty batch included; its answers are the plain build's."""
    batches = [(p["verts"], p["o"][k::7], p["d"][k::7], p["tmax"][k::7]) for k, fam in enumerate(RX.FAMILIES) for p in H.family_case(fam)]
    batches += [(c["verts"], c["o"][::29], c["d"][::29], None) for c in (H.side_case(name) for name in ALL)]
    s, dup = H.stack(), H.duplicates()
    batches += [(s["verts"], s["o"], s["d"], s["tmax"]), (dup["verts"], dup["o"][::5], dup["d"][::5], None)]
    v, o, d, tmax = batches[0]
    o, d, tmax = o.copy(), d.copy(), tmax.copy()
    o[0, 1], o[1, 2], d[2, 0], d[3, 1], tmax[4] = np.nan, np.inf, np.nan, -np.inf, np.nan
    o[5, 0] = np.nextafter(f32(32.0) * max(f32(1.0), np.abs(v).max()), f32(np.inf))
    d[6] = 0.0
    tmax[7], tmax[8], tmax[9] = 0.0, -1.0, -np.inf
    batches[0] = (v, o, d, tmax)
    batches.append((v, o[:0], d[:0], tmax[:0]))
    for k, (v, o, d, tmax) in enumerate(batches):
        plain = H.reference(v, o, d, tmax)
        checked = H.reference(v, o, d, tmax, sanitized=True)
        for key in ("count", "walk_count", "same", "offsets", "t", "tri"):
            assert H.same_bits(plain[key], checked[key]), (k, key)
        assert (plain["nodes"], plain["tris"], plain["invalid"], plain["hits"]) == (checked["nodes"], checked["tris"], checked["invalid"], checked["hits"])
        check_reference(plain, k)
        if k == 0:
            assert plain["count"][:10].tolist() == [H.INVALID] * 6 + [0] * 4 and plain["invalid"] == 6 and (plain["count"][10:] >= 0).all()


@pytest.mark.parametrize("fam", RX.FAMILIES)
def test_the_walk_lists_what_brute_force_lists_with_and_without_limits(fam):
    """Tree independence on every family of tests/ray_exact.py: the BVH8 walk with the kernels' slab test and tmax = +inf finds, under the
    boxes it enters, exactly the hits that the brute force finds over all triangles - without a limit, with the limit at the t of one of
    the ray's own hits, one ulp above it and at half of it.  And the limit means what it says: the limited list is the unlimited one cut
    strictly below the limit, so the hit AT the limit is out and is in again one ulp later."""
    hits = 0
    for p in H.family_case(fam):
        ref, n = p["ref"], p["n"]
        what = (fam, p["mesh"])
        check_reference(ref, what)
        assert ref["invalid"] == 0
        free = H.rows(ref, slice(0, n))
        for v, name in enumerate(H.VARIANTS):
            got = H.rows(ref, slice(v * n, (v + 1) * n))
            lim = p["tmax"][v * n:(v + 1) * n]
            keep = free["t"] < np.repeat(lim, np.diff(free["offsets"]))  # fp32 against fp32, strict
            kept = np.bincount(np.repeat(np.arange(n), np.diff(free["offsets"]))[keep], minlength=n)
            assert np.array_equal(got["count"], kept), (what, name)
            assert H.same_bits(got["t"], free["t"][keep]) and np.array_equal(got["tri"], free["tri"][keep]), (what, name)
        has = p["picked"] >= 0
        at, above = ref["count"][n:2 * n], ref["count"][2 * n:3 * n]
        # ties aside, `at` keeps the hits in front of the picked one and `above` takes the picked one in as well
        assert (at[has] <= p["picked"][has]).all() and (above[has] >= p["picked"][has] + 1).all() and (above[has] > at[has]).all(), what
        assert (ref["count"][3 * n:][has] <= at[has]).all() and (ref["count"][n:][np.tile(~has, 3)] == 0).all(), what
        hits += free["hits"]
        print(f"{fam} {p['mesh']}: {free['hits'] / n:.2f} hits per ray (most {free['count'].max()}), {ref['tris'] / (4 * n):.2f} triangles and "
              f"{ref['nodes'] / (4 * n):.2f} nodes per walk; brute force {len(p['verts'])}")
    assert hits > 250


@pytest.mark.parametrize("fam", RX.FAMILIES)
def test_the_first_entry_is_the_oracles_closest_hit(fam):
    """The first list entry equals the oracle's brute-force closest hit (t, tri) bit for bit, and an empty list is its miss."""
    for p in H.family_case(fam):
        want = RX.part_reference(p["part"])
        t, tri = H.first_hits(H.rows(p["ref"], slice(0, p["n"])))
        assert H.same_bits(t, want["t"]) and np.array_equal(tri, want["tri"]), (fam, p["mesh"])
        assert np.array_equal(tri < 0, p["ref"]["count"][:p["n"]] == 0)


@pytest.mark.parametrize("name", ALL)
def test_the_meshes_of_the_side_query(name):
    """On every mesh of tests/sign_exact.py, every family of its points along each D[k], no limit: walk == brute force, the count is the
    side reference's crossings, the first entry is the closest accepted triangle that reference holds to the oracle - and, on family a,
    the oracle's own brute-force closest hit; the walk prunes."""
    import oracle as O

    c = H.side_case(name)
    ref, n, side = c["ref"], c["n"], c["side"]
    check_reference(ref, name)
    assert ref["invalid"] == 0
    t, tri = H.first_hits(ref)
    sc = O.TriScene(*RX._with_surface(c["verts"]))
    a = side["rows"]["a"]
    for k in range(3):
        block = slice(k * n, (k + 1) * n)
        assert np.array_equal(ref["count"][block], side["ref"]["brute"][:, k]), (name, k)
        assert H.same_bits(t[block], side["ref"]["t"][:, k]) and np.array_equal(tri[block], side["ref"]["tri"][:, k]), (name, k)
        ot, otri, _ = RX.oracle_answers(sc, side["p"][a], np.broadcast_to(SX.D[k], side["p"][a].shape), None, use_bvh=False)
        assert H.same_bits(t[block][a], ot) and np.array_equal(tri[block][a], otri), (name, k)
    per_walk = ref["tris"] / (3 * n)
    print(f"{name}: {ref['hits'] / (3 * n):.2f} hits per ray (most {ref['count'].max()}), {per_walk:.2f} triangles and {ref['nodes'] / (3 * n):.2f} nodes per walk")
    assert per_walk < len(c["verts"]) / 8


def test_the_stack():
    """256 parallel quads: the axis-offset ray passes through all of them, in strictly ascending t; rays from behind list the same quads
    the other way round; limits inside the stack cut it."""
    s = H.stack()
    ref = s["ref"]
    check_reference(ref, "stack")
    assert len(s["verts"]) == 2 * H.STACK_QUADS and ref["count"][0] == H.STACK_QUADS
    t0, tri0 = ref["t"][:H.STACK_QUADS], ref["tri"][:H.STACK_QUADS]
    assert (np.diff(t0) > 0).all() and np.array_equal(tri0 // 2, np.arange(H.STACK_QUADS))  # one triangle of every quad, front to back
    back = s["n"] // 3
    lo, hi = ref["offsets"][back], ref["offsets"][back + 1]
    assert hi - lo == H.STACK_QUADS and np.array_equal(ref["tri"][lo:hi] // 2, np.arange(H.STACK_QUADS)[::-1])
    assert ref["count"][5] == 0 and ref["count"][6] == 0  # beside the stack
    limited = np.isfinite(s["tmax"])
    assert limited.sum() >= 8 and ((ref["count"][limited] > 0) & (ref["count"][limited] < H.STACK_QUADS)).all()
    assert set(ref["count"][~limited].tolist()) >= {0, H.STACK_QUADS}


def test_the_duplicates():
    """Every triangle twice: every t comes twice in a row, and the lower index comes first."""
    d = H.duplicates()
    ref = d["ref"]
    check_reference(ref, "duplicates")
    assert ref["hits"] > 500 and (ref["count"] % 2 == 0).all()
    t, tri = ref["t"].reshape(-1, 2), ref["tri"].reshape(-1, 2)
    assert H.same_bits(t[:, 0], t[:, 1]) and np.array_equal(tri[:, 0] + d["half"], tri[:, 1])
    # and it is the sphere's own list, doubled
    c = H.side_case("sphere")
    a = c["side"]["rows"]["a"]
    single = H.rows(c["ref"], np.r_[np.arange(c["n"])[a], c["n"] + np.arange(c["n"])[a]])
    assert np.array_equal(2 * single["count"], ref["count"]) and H.same_bits(single["t"], t[:, 0]) and np.array_equal(single["tri"], tri[:, 0])
