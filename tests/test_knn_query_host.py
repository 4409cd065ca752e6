"""CPU tests of the k-nearest queries (rt_query_knn_device, Renderer.query_knn): the boundary (exports, bindings,
NULL contexts, struct layouts, defaults, the wrapper's refusals), and the answer itself through the native reference
tests/native/knn_query_ref.cpp - clean under ASan + UBSan; its BVH8 walk under the kernel's culling rule (a bound that shrinks to the
k-th best, a box skipped only when lb2 > bound) returns, entry for entry and bit for bit, what its brute force over all triangles
returns, on every family of tests/point_exact.py under every k and radius of tests/knn_exact.py (tree independence: no GPU needed); the
brute force is the radius query's reference list cut at k (so the new reference does not only agree with itself); k = 1 is the
closest-point reference's answer; ties come lower index first and a cut inside a duplicate pair keeps the first copy; the float64
contract holds and rejects a withheld k-th neighbour; the walk prunes.  The kernel itself is tested on the GPU
(tests/test_gpu_knn_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import knn_exact as KX
import neighbor_exact as NX
import point_exact as PX
import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

FUNCTIONS = ("rt_default_knn_query_params", "rt_query_knn_device", "rt_get_knn_query_stats")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS, methods=("query_knn", "knn_query_stats"), params="KnnQueryParams", stats="KnnQueryStats",
               params_c="rt_knn_query_params", stats_c="rt_knn_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["points", "invalid_points", "neighbors", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
               constants={"RT_KNN_MAX_K": _lib.KNN_MAX_K}, default="rt_default_knn_query_params",
               null_calls=(("rt_query_knn_device", (None, None, 0, 1, None, None, None, None)),
                           ("rt_query_knn_device", (V, V, 1, 8, C.byref(R.KnnQueryParams()), V, V, V)),
                           ("rt_get_knn_query_stats", (C.byref(R.KnnQueryStats()),)), ("rt_default_knn_query_params", ())))
f32 = np.float32
INF = NX.INF


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)
    assert R.Renderer.KNN_MAX_K == _lib.KNN_MAX_K == KX.BIG_K == 1024


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    AB.struct_layout(KIND, tmp_path)


def test_default_params_are_zeros():
    AB.default_params(KIND)


def test_the_wrapper_checks_its_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    for bad in (a, good, good.double(), torch.zeros(3, 4).t(), torch.zeros(4, 4)):
        with pytest.raises(ValueError):
            r.query_knn(bad, 8)
    with pytest.raises(TypeError):
        r.query_knn(good)  # a k is required


def test_the_wrapper_refuses_k_shapes_and_types():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    p = torch.zeros(4, 3)
    for bad_k in (0, 1025, -1, 2 ** 32, 1.0, "8", None, True):
        with pytest.raises(ValueError, match="k must"):
            r.query_knn(p, bad_k)
    with pytest.raises(ValueError, match="points"):
        r.query_knn(torch.zeros(4, 4), 8)
    for bad_rmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1), torch.zeros(4, dtype=torch.float64), "1", True, np.zeros(4, f32)):
        with pytest.raises(ValueError, match="rmax"):
            r.query_knn(p, 8, rmax=bad_rmax)
    dist, tri, cnt = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="out must"):
        r.query_knn(p, 8, out=(dist, tri))
    with pytest.raises(ValueError, match="out must"):
        r.query_knn(p, 8, out=dist)
    for bad_dist in (torch.zeros(4, 7), torch.zeros(5, 8), torch.zeros(32), torch.zeros(8, 4).t(), torch.zeros(4, 8, dtype=torch.float64), np.zeros((4, 8), f32)):
        with pytest.raises(ValueError, match="out dist"):
            r.query_knn(p, 8, out=(bad_dist, tri, cnt))
    for bad_tri in (torch.zeros(4, 7, dtype=torch.int32), torch.zeros(32, dtype=torch.int32), torch.zeros(4, 8), torch.zeros(8, 4, dtype=torch.int32).t(),
                    torch.zeros(4, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="out tri"):
            r.query_knn(p, 8, out=(dist, bad_tri, cnt))
    for bad_cnt in (torch.zeros(5, dtype=torch.int32), torch.zeros(4), torch.zeros(4, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="counts"):
            r.query_knn(p, 8, out=(dist, tri, bad_cnt))
    with pytest.raises(TypeError, match="query_knn"):
        r.query_knn(p, 8, tune_nothing=1)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_is_clean_under_asan_and_ubsan():
    """Every radius variant and no radius, under every k (rows as long as the mesh, short rows and 1024 among them) on the needle mesh
    and on the terrain, through the sanitised build run as a program."""
    for name, n in (("g", 40), ("b", 24)):
        part = PX.family(name, n)[0]
        free = NX.reference(part["verts"], part["p"], INF, sanitized=True)
        rmax = np.concatenate([NX.radii(free, v) for v in NX.VARIANTS] + [np.full(len(part["p"]), INF, f32)])
        p = np.tile(part["p"], (len(NX.VARIANTS) + 1, 1))
        p[3], rmax[5] = np.nan, np.nan  # invalid points go the same way
        ks = KX.ks_of(part["verts"]) + (KX.BIG_K,)
        k = np.repeat(np.asarray(ks, np.uint32), len(p))
        p, rmax = np.tile(p, (len(ks), 1)), np.tile(rmax, len(ks))
        clean = KX.reference(part["verts"], p, k, rmax, sanitized=True)
        plain = KX.reference(part["verts"], p, k, rmax)
        for key in ("count", "tri", "walk_tri", "nodes", "tris"):
            assert np.array_equal(clean[key], plain[key]), key
        assert KX.same_bits(clean["dist"], plain["dist"]) and clean["invalid"] == 2 * len(ks) and (clean["count"][[3, 5]] == KX.INVALID).all()
        assert KX.walk_is_brute(clean)


@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_the_walk_returns_what_the_brute_force_returns(fam):
    """Tree independence under a shrinking bound, and what follows from the definition: well-formed rows; every row the first
    min(k, length) entries of the radius query's list for the same rmax (tests/neighbor_exact.py's reference, another program); k = 1 the
    closest-point reference's answer; rows under a smaller k prefixes of rows under a larger one."""
    short = full = 0
    for c in KX.family_case(fam):
        what = (fam, c["mesh"])
        assert KX.walk_is_brute(c["walk"]) and c["walk"]["invalid"] == 0, what
        n_tris, n_nx = len(c["verts"]), len(c["nx"]["p"])
        assert c["ks"][:5] == (1, 2, 7, 8, 40) and ((n_tris, n_tris + 4) == c["ks"][5:] if c["mesh"] == "needle" else len(c["ks"]) == 5)
        free = NX.rows(c["nx"]["free"], slice(0, c["n"]))  # the unlimited lists of the part's points: the block "none"
        for k in c["ks"]:
            row = c["ref"][k]
            assert row["k"] == k and row["dist"].shape == (len(c["p"]), k)
            assert KX.expected(row["count"], row["dist"], row["tri"]) and KX.same_bits(row["dist"], np.sqrt(row["d2"])), (what, k)
            head = {key: (val[:n_nx] if isinstance(val, np.ndarray) else val) for key, val in row.items()}
            tail = {key: (val[n_nx:] if isinstance(val, np.ndarray) else val) for key, val in row.items()}
            assert KX.prefix_of_list(c["nx"]["ref"], head), (what, k)
            assert KX.prefix_of_list(free, tail) and (tail["count"] == min(k, n_tris)).all(), (what, k)
            short += int(((row["count"] >= 0) & (row["count"] < min(k, n_tris))).sum())
            full += int((row["count"] == k).sum())
            for v in ("zero", "negative", "underflow"):
                assert (row["count"][c["blocks"][v]] == 0).all() and (row["nodes"][c["blocks"][v]] == 0).all(), (what, k, v)
        # k = 1 is rt_query_points_device's answer for the same rmax
        near = PX.reference(c["verts"], c["p"], c["rmax"])["brute"]
        one = c["ref"][1]
        assert np.array_equal(one["tri"][:, 0], near["tri"]) and KX.same_bits(one["dist"][:, 0], near["dist"]), what
        assert np.array_equal(one["count"], (near["tri"] >= 0).astype(np.int32))
        for small, large in zip(c["ks"][:-1], c["ks"][1:]):
            a, b = c["ref"][min(small, large)], c["ref"][max(small, large)]
            assert KX.same_bits(a["dist"], b["dist"][:, :a["k"]]) and np.array_equal(a["tri"], b["tri"][:, :a["k"]]), (what, small, large)
        # RT_KNN_MAX_K on the first points: on these meshes of at most 4 000 triangles the first 1 024 of the whole sorted mesh
        big = c["big"]["ref"]
        assert big["dist"].shape == (min(c["n"], KX.BIG_POINTS), KX.BIG_K) and (big["count"] == min(KX.BIG_K, n_tris)).all(), what
        assert KX.prefix_of_list(NX.rows(c["nx"]["free"], slice(0, len(big["count"]))), big), what
    assert short > 100 and full > 100, (short, full)


def test_exact_ties_come_lower_index_first():
    """Family e: points above vertices and edge midpoints of the flat grid."""
    (c,) = KX.family_case("e")
    ties = 0
    for k in (2, 7, 8, 40):
        row = c["ref"][k]
        inside = np.arange(k)[None, 1:] < row["count"][:, None]
        tie = inside & (row["d2"][:, 1:] == row["d2"][:, :-1])
        assert (row["tri"][:, 1:] > row["tri"][:, :-1])[tie].all()
        ties += int(tie.sum())
    assert ties > 1000, ties


def test_a_cut_inside_a_duplicate_pair_keeps_the_first_copy():
    """Family f: the soup with every triangle again as i + n, so a sorted list goes in pairs (t, t + n) of equal d2 (where no third
    triangle ties with them).  Under an odd k the cut falls inside a pair: seen from the row under k + 1, whose entries k - 1 and k tie,
    the row under k ends with the lower index of the two, and that is the first copy."""
    (c,) = KX.family_case("f")
    half = len(c["verts"]) // 2
    pairs = 0
    for k in (1, 7):
        a, b = c["ref"][k], c["ref"][k + 1]
        tie = (b["count"] == k + 1) & (b["d2"][:, k - 1] == b["d2"][:, k])
        assert np.array_equal(a["tri"][tie, k - 1], b["tri"][tie, k - 1]) and (b["tri"][tie, k - 1] < b["tri"][tie, k]).all()
        assert not (a["tri"][tie] == b["tri"][tie, k][:, None]).any()  # the higher index of the tie is not in the row under k
        pair = tie & (b["tri"][:, k - 1] + half == b["tri"][:, k])
        assert (a["tri"][pair, k - 1] < half).all()
        pairs += int(pair.sum())
    assert pairs > 1000, pairs


@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_the_float64_contract(fam):
    """Kp = 16 and unit of tests/point_exact.py: every listed dist within Kp unit of its triangle's D, no unlisted triangle with D below the
    row's last D - 2 Kp unit, short rows complete within rmax - Kp unit.  A constructed wrong answer - the float64 k nearest with the
    true k-th withheld (the k + 1-th in its place) - is rejected wherever the two are more than the band apart."""
    rejected = 0
    for c in KX.family_case(fam, 120):
        em = PX.ExactTris(c["verts"])
        p, rmax = c["p"], c["rmax"]
        D = em.all_dists(p)
        band = PX.KP * PX.unit_of(p, em)
        order = np.argsort(D, axis=1, kind="stable")
        Ds = np.take_along_axis(D, order, 1)
        for k in c["ks"]:
            row = c["ref"][k]
            ok = KX.contract(em, p, rmax, k, row["count"], row["dist"], row["tri"], D)
            assert ok.all(), (fam, c["mesh"], k, np.nonzero(~ok)[0][:8])
            if k >= len(c["verts"]):
                continue
            # the float64 answer without a limit is right; with its k-th entry replaced by the k + 1-th it is wrong where the gap is clear
            none = c["blocks"]["none"]
            kk = np.full(none.stop - none.start, k, np.int32)
            right_t, right_d = order[none, :k].astype(np.int32), Ds[none, :k]
            assert KX.contract(em, p[none], None, k, kk, right_d, right_t, D[none]).all()
            wrong_t, wrong_d = right_t.copy(), right_d.copy()
            wrong_t[:, k - 1], wrong_d[:, k - 1] = order[none, k], Ds[none, k]
            clear = Ds[none, k] - Ds[none, k - 1] > 4 * band[none]
            wrong = KX.contract(em, p[none], None, k, kk, wrong_d, wrong_t, D[none])
            assert not wrong[clear].any(), (fam, c["mesh"], k)
            rejected += int(clear.sum())
    assert rejected > 100, rejected


def test_the_terrain_is_pruned():
    """What tests/test_gpu_knn_query.py relies on: family b on the terrain (1 154 triangles) with k = 8 and no rmax tests at most
    n_tris / 8 = 144 triangles a point.  A condition, not a measurement: query_points tests 6.8 there, the k = 8 radius walk 9.8.
    The reference walk gives 19.81 triangles and 7.56 nodes per point."""
    c = KX.family_case("b")[0]
    assert c["mesh"] == "terrain" and len(c["verts"]) == 1154
    row = c["ref"][8]
    none = c["blocks"]["none"]
    tris, nodes = row["tris"][none].mean(), row["nodes"][none].mean()
    print(f"terrain, family b, k = 8, no rmax: {tris:.2f} triangles and {nodes:.2f} nodes per point")
    assert (row["count"][none] == 8).all() and 0 < tris <= len(c["verts"]) / 8
