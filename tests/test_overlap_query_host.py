"""CPU tests of the overlap queries (rt_count_overlaps_device / rt_fill_overlaps_device / rt_list_overlaps_device,
Renderer.count_overlaps / list_overlaps): the boundary (exports, bindings, NULL contexts, struct layouts,
defaults, the wrappers' refusals), and the answer itself through the native reference tests/native/overlap_query_ref.cpp - clean under
ASan + UBSan; its BVH8 walk under the kernel's culling rule (skip exactly when the decoded child box does not overlap the query's box)
lists, entry for entry, what its brute force over all pairs lists, on every family of tests/overlap_exact.py (tree independence: no GPU
needed); answers computed by hand; bits 0-2 against the all-hits reference of tests/hit_exact.py; the float64 contract.
The kernel itself is tested on the GPU (tests/test_gpu_overlap_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import hit_exact as HX
import overlap_exact as OX
import point_exact as PX
import raytracing_engine_amd as R

FUNCTIONS = ("rt_default_overlap_query_params", "rt_count_overlaps_device", "rt_fill_overlaps_device", "rt_list_overlaps_device", "rt_get_overlap_query_stats")
V = C.c_void_p(16)
P = C.byref(R.OverlapQueryParams())
KIND = AB.Kind(functions=FUNCTIONS, methods=("count_overlaps", "list_overlaps", "overlap_query_stats"), params="OverlapQueryParams", stats="OverlapQueryStats",
               params_c="rt_overlap_query_params", stats_c="rt_overlap_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["triangles", "invalid_triangles", "overlaps", "overlaps_written", "incomplete_triangles", "slice_overflow", "nodes_visited", "tris_tested",
                             "stack_overflow", "launches", "ms"],
               default="rt_default_overlap_query_params",
               null_calls=(("rt_count_overlaps_device", (None, 0, None, None, None)), ("rt_count_overlaps_device", (V, 1, P, V, V)),
                           ("rt_fill_overlaps_device", (None, 0, None, None, 0, None, None)), ("rt_fill_overlaps_device", (V, 1, P, V, 1, V, V)),
                           ("rt_list_overlaps_device", (None, 0, None, None, None, 0, None, None)), ("rt_list_overlaps_device", (V, 1, P, V, V, 1, V, V)),
                           ("rt_get_overlap_query_stats", (C.byref(R.OverlapQueryStats()),)), ("rt_default_overlap_query_params", ())))
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
    a = np.zeros((4, 9), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    for bad in (a, good, good.view(4, 3, 3), good.double(), torch.zeros(9, 4).t(), torch.zeros(4, 8), None):
        for call in (r.count_overlaps, r.list_overlaps, lambda x: r.list_overlaps(x, capacity=8)):
            with pytest.raises(ValueError):
                call(bad)


def test_the_wrappers_compare_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    q = torch.zeros(4, 9)
    cnt, off = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    tri, edges = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    for call in (r.count_overlaps, r.list_overlaps, lambda *a, **k: r.list_overlaps(*a, capacity=8, **k)):
        for bad in (torch.zeros(4, 8), torch.zeros(4, 3, 2), torch.zeros(10)):
            with pytest.raises(ValueError, match="tris"):
                call(bad)
    assert r._tri_rows(torch.zeros(4, 3, 3))[1] == 4 and r._tri_rows(torch.zeros(36))[1] == 4 and r._tri_rows(q)[1] == 4
    with pytest.raises(ValueError, match="counts"):
        r.count_overlaps(q, out=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(TypeError, match="count_overlaps"):
        r.count_overlaps(q, tune_nothing=1)
    with pytest.raises(TypeError, match="list_overlaps"):
        r.list_overlaps(q, capacity=8, count_traversal=True)  # the wrapper exposes the tuning only
    with pytest.raises(ValueError, match="capacity"):
        r.list_overlaps(q, out=(off, tri, edges, cnt))  # out without a capacity
    with pytest.raises(ValueError, match="capacity"):
        r.list_overlaps(q, capacity=-1)
    with pytest.raises(ValueError, match="edges"):
        r.list_overlaps(q, capacity=8, out=(off, tri, edges))
    for bad_out in ((torch.zeros(4, dtype=torch.int64), tri, edges, cnt), (off, torch.zeros(7, dtype=torch.int32), edges, cnt), (off, tri, torch.zeros(8), cnt),
                    (off, tri, edges, torch.zeros(5, dtype=torch.int32)), (off.int(), tri, edges, cnt)):
        with pytest.raises(ValueError):
            r.list_overlaps(q, capacity=8, out=bad_out)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_is_clean_under_asan_and_ubsan():
    """Family e on the grid (coplanar, degenerate, far, invalid queries) and family d on the needle mesh, through the sanitised build
    run as a program of its own."""
    for c in (OX.family_case("e")[0], OX.family_case("d")[0]):
        clean = OX.reference(c["verts"], c["q"], sanitized=True)
        for key in ("count", "offsets", "tri", "edges", "nodes", "tris", "pair_mask"):
            assert np.array_equal(clean[key], c["ref"][key]), key


T0 = [0, 0, 0, 4, 0, 0, 0, 4, 0]  # the mesh of the hand-computed answers: one triangle in the plane z = 0


def test_answers_computed_by_hand():
    """Against the one triangle T0.  (1) edge A0A1 pierces T0 at (1, 1, 0), T0's edge v0v1 pierces the query (plane x = 1) at (1, 0, 0),
    edge A2A0 and T0's edge v0v2 run parallel to the other's plane (det == 0), the other two cross the planes outside: bits 0 and 3.
    (2) a query that straddles T0 well inside: its edges A0A1 and A2A0 pierce at (1, 1.5, 0) and (1.5, 1, 0), A1A2 runs below and
    parallel, no edge of T0 comes near: bits 0 and 2.  (3) the boxes meet, edge A0A1 crosses the plane at (3.5, 3.5, 0) beyond the
    hypotenuse: cand, mask 0, not listed.  (4) boxes apart: no cand.  (5) coplanar and overlapping: cand, every det == 0, mask 0."""
    q = f32([[1, 1, -1, 1, 1, 1, 1, -3, -1],
             [1, 1, 1, 1, 2, -1, 2, 1, -1],
             [3.5, 3.5, -1, 3.5, 3.5, 1, 3.9, 3.9, 0],
             [10, 10, 1, 11, 10, 1, 10, 11, 1],
             [1, 1, 0, 2, 1, 0, 1, 2, 0]])
    ref = OX.reference(f32([T0]), q)
    assert ref["count"].tolist() == [1, 1, 0, 0, 0] and ref["tri"].tolist() == [0, 0] and ref["edges"].tolist() == [0b001001, 0b000101]
    assert ref["offsets"].tolist() == [0, 1, 2, 2, 2, 2] and OX.walk_is_brute(ref) and ref["invalid"] == 0
    assert ref["pair_q"].tolist() == [0, 1, 2, 4] and ref["pair_mask"].tolist() == [9, 5, 0, 0]  # cand without a piercing edge: masks 0
    assert np.array_equal(OX.cand_numpy(f32([T0]), q)[:, 0], [True, True, True, False, True])


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("fam", OX.FAMILIES)
def test_the_walk_lists_what_the_brute_force_lists(fam, moved):
    """Tree independence on every family and mesh (and on the moved vertices the refit tests use), and what follows from the definition."""
    for c in OX.family_case(fam, moved):
        ref, what = c["ref"], (fam, c["mesh"], moved)
        assert OX.walk_is_brute(ref), what
        count = np.maximum(ref["count"], 0).astype(np.int64)
        assert np.array_equal(ref["offsets"], np.concatenate([[0], np.cumsum(count)])) and ref["offsets"][-1] == ref["overlaps"]
        owner = np.repeat(np.arange(len(count)), count)
        assert (ref["tri"][1:] > ref["tri"][:-1])[owner[1:] == owner[:-1]].all(), what  # ascending by index, no triangle twice
        assert ((ref["edges"] > 0) & (ref["edges"] < 64)).all()
        # the lists are the cand pairs with a mask, and cand is the numpy one
        listed = ref["pair_mask"] != 0
        assert np.array_equal(ref["pair_q"][listed], owner) and np.array_equal(ref["pair_t"][listed], ref["tri"]) and np.array_equal(ref["pair_mask"][listed], ref["edges"])
        valid = ref["count"] >= 0
        cand = OX.cand_numpy(c["verts"], c["q"]) & valid[:, None]
        assert np.array_equal(np.stack(np.nonzero(cand)), np.stack([ref["pair_q"], ref["pair_t"]])), what
        if fam != "d":  # the runtime guard of the O(k^2) insertion
            assert ref["count"].max() <= OX.LONGEST, (what, int(ref["count"].max()))
        if fam == "c" and not moved:
            assert (ref["count"] >= 1).all() and ((ref["edges"] & 1).astype(bool).sum() >= len(count)), what  # the planted edge pierces
        if fam == "d":
            assert (ref["tris"] == len(c["verts"])).all() and ref["overlaps"] > 0, what  # the box spans the mesh: every record is fetched
        if fam == "e":
            kinds = c["kinds"]
            assert np.array_equal(ref["count"] == OX.INVALID, kinds == "invalid") and ref["invalid"] == int((kinds == "invalid").sum()) == 12
            assert (ref["count"][kinds == "far"] == 0).all(), what
            assert moved or (ref["count"][kinds == "coplanar"] == 0).all(), what  # (the moved grid is no plane any more)
            assert (ref["nodes"][kinds == "invalid"] == 0).all() and (ref["nodes"][kinds != "invalid"] >= 1).all()
            if c["mesh"] == "grid":  # cand holds for the coplanar queries, and every det is 0
                assert (kinds == "coplanar").sum() == 24 and np.isin(np.nonzero(kinds == "coplanar")[0], ref["pair_q"]).all()
            seg = ref["edges"][np.isin(owner, np.nonzero(kinds == "segment")[0])]
            assert len(seg) > 0 and (seg & 0b111000 == 0).all() and (ref["count"][kinds == "point"] == 0).all()  # no area: bits 0-2 only


def test_terrain_and_grid_asked_with_their_own_triangles():
    """What the definition gives for pairs that share vertices and edges, deterministically: 3 199 pairs on the 1 154-triangle terrain
    (1 770 of them with a query edge through the mesh triangle), none on the 512-triangle grid (coplanar neighbours)."""
    for mesh, n_tris, pairs, by_query_edge in (("terrain", 1154, 3199, 1770), ("grid", 512, 0, 0)):
        v = PX.mesh(mesh)
        parts = [OX.reference(v, v[a:a + 600]) for a in range(0, len(v), 600)]
        assert len(v) == n_tris and sum(p["overlaps"] for p in parts) == pairs and all(OX.walk_is_brute(p) for p in parts)
        assert sum(int((p["edges"] & 7 != 0).sum()) for p in parts) == by_query_edge


def test_bits_0_to_2_are_the_all_hits_reference_under_cand():
    """The 3 n edge segments (o, d, tmax = 1) through tests/hit_exact.py's reference, cut to cand in numpy fp32: exactly bits 0-2.  The
    hits that cand removes are counted: on these inputs there are none."""
    removed = kept = 0
    for fam in ("a", "b", "c", "d"):
        for c in OX.family_case(fam):
            ref, q = c["ref"], c["q"]
            o, d = OX.edge_segments(q)
            hits = HX.reference(c["verts"], o, d, np.ones(len(o), f32))
            assert hits["invalid"] == 0
            ray = np.repeat(np.arange(len(o)), hits["count"])
            cand = OX.cand_numpy(c["verts"], q)[ray // 3, hits["tri"]]
            removed += int((~cand).sum())
            got = set(zip((ray // 3)[cand].tolist(), (ray % 3)[cand].tolist(), hits["tri"][cand].tolist()))
            owner = np.repeat(np.arange(len(q)), np.maximum(ref["count"], 0))
            want = {(int(i), k, int(t)) for i, t, m in zip(owner, ref["tri"], ref["edges"]) for k in range(3) if (m >> k) & 1}
            assert got == want, (fam, c["mesh"], len(got), len(want))
            kept += len(want)
    print(f"bits 0-2: {kept} hits kept, {removed} removed by cand")
    assert kept > 1000 and removed == 0


def test_the_float64_contract():
    """overlap_exact.contract under M = 2^-21 (16 x the measured 1.97e-8): no (test, pair) case of any family breaks it, and at least
    90 % of the set bits of families a and c lie in the "must be set" class.  A bit withheld from that class is seen."""
    set_bits = must = 0
    for fam in OX.FAMILIES:
        for c in OX.family_case(fam):
            ref = c["ref"]
            lows = OX.pair_lows(c["verts"], c["q"], ref["pair_q"], ref["pair_t"])
            bad, must_set = OX.contract(lows, ref["pair_mask"])
            assert bad == 0, (fam, c["mesh"], bad)
            if fam in ("a", "c"):
                set_bits += sum(int(((ref["pair_mask"] >> k) & 1).sum()) for k in range(6))
                must += int(must_set.sum())
                if must_set.any():  # (the grid's displaced own triangles meet nothing)
                    i, k = np.argwhere(must_set)[0]
                    wrong = ref["pair_mask"].copy()
                    wrong[i] &= ~(1 << k)
                    assert OX.contract(lows, wrong)[0] == 1
    print(f"families a and c: {must} of {set_bits} set bits must be set under M = {OX.M:.3g}")
    assert set_bits > 1000 and must >= 0.9 * set_bits
    assert OX.M == 2.0 ** -21 and 16 * OX.M_MEASURED <= OX.M < 32 * OX.M_MEASURED


@pytest.mark.parametrize("k", [-16, 14])
def test_the_reference_is_covariant_under_scale(k):
    """Every length x 2^k: the same counts, indices and masks (what tests/test_gpu_overlap_query.py asks of the kernel)."""
    for fam in ("a", "b", "c"):
        for c in OX.family_case(fam):
            if c["mesh"] not in ("soup", "grid", "terrain", "needle"):
                continue
            ref = OX.reference(np.ldexp(c["verts"], k).astype(f32), np.ldexp(c["q"], k).astype(f32))
            for key in ("count", "offsets", "tri", "edges", "pair_mask"):
                assert np.array_equal(ref[key], c["ref"][key]), (fam, c["mesh"], key)
