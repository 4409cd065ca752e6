"""CPU tests of the neighbour queries (rt_count_neighbors_device / rt_fill_neighbors_device / rt_list_neighbors_device,
Renderer.count_neighbors / list_neighbors): the boundary (exports, bindings, NULL contexts, struct layouts,
defaults, the wrappers' refusals), and the answer itself through the native reference tests/native/neighbor_query_ref.cpp - clean under
ASan + UBSan; its BVH8 walk under the kernel's culling rule (skip exactly when child_lb2 >= limit2) lists, entry for entry and bit for
bit, what its brute force over all triangles lists, on every family of tests/point_exact.py under every radius of
tests/neighbor_exact.py (tree independence: no GPU needed); entry 0 is the closest-point reference's answer; a limited list is the
unlimited one cut strictly below the limit; ties come lower index first; the float64 contract holds and rejects a withheld neighbour.
The kernel itself is tested on the GPU (tests/test_gpu_neighbor_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import neighbor_exact as NX
import point_exact as PX
import raytracing_engine_amd as R

FUNCTIONS = ("rt_default_neighbor_query_params", "rt_count_neighbors_device", "rt_fill_neighbors_device", "rt_list_neighbors_device", "rt_get_neighbor_query_stats")
V = C.c_void_p(16)
P = C.byref(R.NeighborQueryParams())
KIND = AB.Kind(functions=FUNCTIONS, methods=("count_neighbors", "list_neighbors", "neighbor_query_stats"), params="NeighborQueryParams", stats="NeighborQueryStats",
               params_c="rt_neighbor_query_params", stats_c="rt_neighbor_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["points", "invalid_points", "neighbors", "neighbors_written", "incomplete_points", "slice_overflow", "nodes_visited", "tris_tested",
                             "stack_overflow", "launches", "ms"],
               default="rt_default_neighbor_query_params",
               null_calls=(("rt_count_neighbors_device", (None, None, 1.0, 0, None, None, None)), ("rt_count_neighbors_device", (V, V, 1.0, 1, P, V, V)),
                           ("rt_fill_neighbors_device", (None, None, 1.0, 0, None, None, 0, None, None)), ("rt_fill_neighbors_device", (V, V, 1.0, 1, P, V, 1, V, V)),
                           ("rt_list_neighbors_device", (None, None, 1.0, 0, None, None, None, 0, None, None)), ("rt_list_neighbors_device", (V, V, 1.0, 1, P, V, V, 1, V, V)),
                           ("rt_get_neighbor_query_stats", (C.byref(R.NeighborQueryStats()),)), ("rt_default_neighbor_query_params", ())))
f32 = np.float32
INF = NX.INF


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
        for call in (r.count_neighbors, r.list_neighbors, lambda x, y: r.list_neighbors(x, y, capacity=8)):
            with pytest.raises(ValueError):
                call(bad, 1.0)
    with pytest.raises(TypeError):
        r.count_neighbors(good)  # a radius is required


def test_the_wrappers_compare_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    p = torch.zeros(4, 3)
    cnt, off = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    dist, tri = torch.zeros(8), torch.zeros(8, dtype=torch.int32)
    for call in (r.count_neighbors, r.list_neighbors, lambda *a, **k: r.list_neighbors(*a, capacity=8, **k)):
        with pytest.raises(ValueError, match="points"):
            call(torch.zeros(4, 4), 1.0)
        for bad_rmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1), torch.zeros(4, dtype=torch.float64), None, "1", True, np.zeros(4, f32)):
            with pytest.raises(ValueError, match="rmax"):
                call(p, bad_rmax)
    with pytest.raises(ValueError, match="counts"):
        r.count_neighbors(p, 1.0, out=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="counts"):
        r.count_neighbors(p, 1.0, out=torch.zeros(4))  # float32 where int32 is due
    with pytest.raises(TypeError, match="count_neighbors"):
        r.count_neighbors(p, 1.0, tune_nothing=1)
    with pytest.raises(TypeError, match="list_neighbors"):
        r.list_neighbors(p, 1.0, tune_nothing=1)
    with pytest.raises(TypeError, match="list_neighbors"):
        r.list_neighbors(p, 1.0, capacity=8, count_traversal=True)  # the wrapper exposes the tuning only
    with pytest.raises(ValueError, match="capacity"):
        r.list_neighbors(p, 1.0, out=(off, dist, tri, cnt))  # out without a capacity
    with pytest.raises(ValueError, match="capacity"):
        r.list_neighbors(p, 1.0, capacity=-1)
    with pytest.raises(ValueError, match="out"):
        r.list_neighbors(p, 1.0, capacity=8, out=(off, dist, tri))
    for bad_out in ((torch.zeros(4, dtype=torch.int64), dist, tri, cnt), (off, torch.zeros(7), tri, cnt), (off, dist, torch.zeros(8), cnt),
                    (off, dist, tri, torch.zeros(5, dtype=torch.int32)), (off.int(), dist, tri, cnt)):
        with pytest.raises(ValueError):
            r.list_neighbors(p, 1.0, capacity=8, out=bad_out)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_is_clean_under_asan_and_ubsan():
    """Every radius variant (the +inf block included) on the needle mesh and on the terrain, through the sanitised build run as a program."""
    for name, n in (("g", 40), ("b", 24)):
        part = PX.family(name, n)[0]
        free = NX.reference(part["verts"], part["p"], INF, sanitized=True)
        rmax = np.concatenate([NX.radii(free, v) for v in NX.VARIANTS] + [np.full(len(part["p"]), INF, f32)])
        p = np.tile(part["p"], (len(NX.VARIANTS) + 1, 1))
        p[3], rmax[5] = np.nan, np.nan  # invalid points go the same way
        clean = NX.reference(part["verts"], p, rmax, sanitized=True)
        plain = NX.reference(part["verts"], p, rmax)
        for key in ("count", "offsets", "tri", "nodes", "tris"):
            assert np.array_equal(clean[key], plain[key]), key
        assert NX.same_bits(clean["dist"], plain["dist"]) and clean["invalid"] == 2 and (clean["count"][[3, 5]] == NX.INVALID).all()


@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_the_walk_lists_what_the_brute_force_lists(fam):
    """Tree independence, and what follows from the definition: sorted lists, entry 0 = the closest-point answer, a limited list = the
    unlimited one cut strictly below limit2, empty lists where nothing can be listed."""
    probed = dict(above=0, at=0)
    for c in NX.family_case(fam):
        ref, free, n, what = c["ref"], c["free"], c["n"], (fam, c["mesh"])
        assert NX.walk_is_brute(ref) and NX.walk_is_brute(free), what
        assert ref["invalid"] == 0 and free["invalid"] == 0
        # the runtime guard: if a family exceeds it, lower its k in neighbor_exact.KS and say so there
        assert NX.longest_limited(c) <= NX.LONGEST, (what, NX.longest_limited(c))
        assert ("inf" in c["blocks"]) == (len(c["verts"]) <= NX.INF_MAX_TRIS)
        count, off = ref["count"].astype(np.int64), ref["offsets"]
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(count)])) and off[-1] == ref["neighbors"]
        # ascending by (d2, index) inside every slice; dist = sqrt(d2), so non-decreasing
        owner = np.repeat(np.arange(len(count)), count)
        inner = owner[1:] == owner[:-1]
        d2, tri = ref["d2"], ref["tri"]
        assert ((d2[1:] > d2[:-1]) | ((d2[1:] == d2[:-1]) & (tri[1:] > tri[:-1])))[inner].all(), what
        assert (ref["dist"][1:] >= ref["dist"][:-1])[inner].all() and NX.same_bits(ref["dist"], np.sqrt(d2))
        # entry 0 is rt_query_points_device's answer for the same rmax; an empty list is its miss
        near = PX.reference(c["verts"], c["p"], c["rmax"])["brute"]
        first_dist, first_tri = NX.first_entries(ref)
        assert np.array_equal(first_tri, near["tri"]) and NX.same_bits(first_dist, near["dist"]), what
        # limited = unlimited, cut strictly below limit2 = fp32(rmax * rmax)
        limit2 = (c["rmax"] * c["rmax"]).astype(f32)
        for v, block in c["blocks"].items():
            k = block.stop - block.start
            cut = NX.rows(ref, block)
            assert len(free["d2"]) == n * len(c["verts"])  # the unlimited list holds every triangle
            keep = (free["d2"].reshape(n, -1)[:k] < limit2[block][:, None]) & (c["rmax"][block] > 0)[:, None]
            assert np.array_equal(cut["count"], keep.sum(1)), (what, v)
            assert NX.same_bits(cut["d2"], free["d2"].reshape(n, -1)[:k][keep]) and np.array_equal(cut["tri"], free["tri"].reshape(n, -1)[:k][keep]), (what, v)
            if v in ("half", "zero", "negative", "underflow"):
                walked = (c["rmax"][block] > 0) & (limit2[block] > 0)  # (half of a distance 0 is no radius)
                assert (cut["count"] == 0).all() and np.array_equal(cut["nodes"] > 0, walked) and (walked.any() == (v == "half")), (what, v)
            elif v == "inf":
                assert (cut["count"] == len(c["verts"])).all(), what
            elif v.endswith("above"):  # the k-th nearest and everything before it is in (a distance 0 has no ulp above it that squares to more)
                kk = min(int(v[1:].split("_")[0]), len(c["verts"]))
                reached = limit2[block] > free["d2"].reshape(n, -1)[:, kk - 1]
                assert (cut["count"][reached] >= kk).all(), (what, v)
                probed["above"] += int(reached.sum())
            else:  # strict: where the radius squares to no more than the k-th d2, that entry and its ties are out
                kk = min(int(v[1:].split("_")[0]), len(c["verts"]))
                d2k = free["d2"].reshape(n, -1)[:, kk - 1]
                exact = limit2[block] <= d2k
                assert (cut["count"][exact] < kk).all(), (what, v)
                probed["at"] += int(exact.sum())
    assert probed["above"] > 100 and probed["at"] > 100, probed  # (points on the surface have a nearest distance 0: no radius excludes or includes it)


def test_exact_ties_come_lower_index_first():
    """Family e: points above vertices and edge midpoints of the flat grid."""
    (c,) = NX.family_case("e")
    ref = c["ref"]
    count = ref["count"].astype(np.int64)
    owner = np.repeat(np.arange(len(count)), count)
    tie = (owner[1:] == owner[:-1]) & (ref["d2"][1:] == ref["d2"][:-1])
    assert tie.sum() > 1000 and (ref["tri"][1:][tie] > ref["tri"][:-1][tie]).all()


def test_duplicated_triangles_are_listed_twice():
    """Family f: the soup with every triangle again as i + n."""
    (c,) = NX.family_case("f")
    half = len(c["verts"]) // 2
    for v in ("k8_above", "k40_above"):
        cut = NX.rows(c["ref"], c["blocks"][v])
        assert (cut["count"] % 2 == 0).all() and cut["neighbors"] > 0
        owner = np.repeat(np.arange(len(cut["count"])), cut["count"])
        order = np.lexsort((np.arange(len(owner)), cut["tri"] % half, owner))  # by point, then by triangle modulo the copy, then by place in the list
        d2, tri, who = cut["d2"][order].reshape(-1, 2), cut["tri"][order].reshape(-1, 2), owner[order].reshape(-1, 2)
        assert NX.same_bits(d2[:, 0], d2[:, 1]) and np.array_equal(tri[:, 0] + half, tri[:, 1]) and np.array_equal(who[:, 0], who[:, 1])


@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_the_float64_contract(fam):
    """Kp = 16 and unit of tests/point_exact.py: required inside rmax - Kp unit, forbidden beyond rmax + Kp unit, every dist within Kp unit.
    A constructed wrong answer - one neighbour withheld that lies more than the band inside - is rejected."""
    rejected = 0
    for c in NX.family_case(fam, 120):
        em = PX.ExactTris(c["verts"])
        ref, p, rmax = c["ref"], c["p"], c["rmax"]
        D = em.all_dists(p)
        ok = NX.contract(em, p, rmax, ref["count"], ref["offsets"], ref["dist"], ref["tri"], D)
        assert ok.all(), (fam, c["mesh"], np.nonzero(~ok)[0][:8])
        # withhold, per point, the listed neighbour that lies deepest inside - where that is more than the band
        count, off = ref["count"].astype(np.int64), ref["offsets"]
        band = PX.KP * PX.unit_of(p, em)
        has = count > 0
        inside = has & (D[np.arange(len(p)), ref["tri"][np.where(has, off[:-1], 0)]] < rmax.astype(np.float64) - 4 * band)
        take = np.ones(len(ref["tri"]), bool)
        take[off[:-1][inside]] = False
        less = count - inside
        wrong = NX.contract(em, p, rmax, less, np.concatenate([[0], np.cumsum(less)]), ref["dist"][take], ref["tri"][take], D)
        assert not wrong[inside].any() and wrong[~inside].all(), (fam, c["mesh"])
        rejected += int(inside.sum())
    assert rejected > 100, rejected


def test_the_terrain_is_pruned():
    """What tests/test_gpu_neighbor_query.py relies on: family b on the terrain with the k = 8 radius tests at most n_tris / 8 triangles a point."""
    c = NX.family_case("b")[0]
    assert c["mesh"] == "terrain"
    cut = NX.rows(c["ref"], c["blocks"]["k8_above"])
    print(f"terrain, family b, k = 8: {cut['tris_total'] / c['n']:.2f} triangles and {cut['nodes_total'] / c['n']:.2f} nodes per point, {cut['neighbors'] / c['n']:.2f} neighbours")
    assert 0 < cut["tris_total"] / c["n"] <= len(c["verts"]) / 8
