"""CPU tests of the sphere-cast query (rt_query_sweeps_device / Renderer.query_sweeps): the boundary (exports,
bindings, NULL contexts, struct layouts, defaults, the wrapper's refusals), and the arithmetic of csrc/sweep_tri.h through the native
reference tests/native/sweep_query_ref.cpp - clean under ASan + UBSan as a program of its own; its BVH8 walk with the culling rule
equals its brute force bit for bit on every family (the test of the bound's derivation: no GPU needed); the brute force satisfies
the float64 contract of tests/sweep_exact.py with the committed K, agrees with closed forms and with the closest-point and ray
references; and that contract rejects mutated answers.  The kernel itself is tested on the GPU (tests/test_gpu_sweep_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import raytracing_engine_amd as R
import sweep_exact as SX

PX, RX = SX.PX, SX.RX
FUNCTIONS = ("rt_default_sweep_query_params", "rt_query_sweeps_device", "rt_get_sweep_query_stats")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS, methods=("query_sweeps", "sweep_query_stats"), params="SweepQueryParams", stats="SweepQueryStats",
               params_c="rt_sweep_query_params", stats_c="rt_sweep_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["sweeps", "invalid_sweeps", "hits", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
               default="rt_default_sweep_query_params",
               null_calls=(("rt_query_sweeps_device", (None, None, None, None, 0, None, None, None, None)),
                           ("rt_query_sweeps_device", (V, V, V, None, 1, C.byref(R.SweepQueryParams()), V, V, V)),
                           ("rt_get_sweep_query_stats", (C.byref(R.SweepQueryStats()),)), ("rt_default_sweep_query_params", ())))
f32 = np.float32
N_CONTRACT = 480  # items per family where float64 distances are evaluated


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


def test_the_wrapper_checks_its_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    for bad in (a, good, good.double(), torch.zeros(3, 4).t(), torch.zeros(4, 2)):
        with pytest.raises(ValueError):
            r.query_sweeps(bad, bad, 0.5)
        with pytest.raises(ValueError):
            r.query_sweeps(bad, bad, 0.5, want_points=False)


def test_the_wrapper_compares_lengths_shapes_and_radius_forms():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    t, tri, pt = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="disagree"):
        r.query_sweeps(o, torch.ones(5, 3), 0.5)
    for bad_tmax in (torch.zeros(3), torch.zeros(4, 1)):
        with pytest.raises(ValueError, match="tmax"):
            r.query_sweeps(o, d, 0.5, tmax=bad_tmax)
    for bad_radius in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1), torch.zeros(4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="radius"):
            r.query_sweeps(o, d, bad_radius)
    for bad_radius in (-0.5, float("nan"), float("inf"), True, "1", None, np.zeros(4, np.float32), [0.5] * 4):
        with pytest.raises(ValueError, match="radius"):
            r.query_sweeps(o, d, bad_radius)
    with pytest.raises(ValueError, match="out"):
        r.query_sweeps(o, d, 0.5, out=(t, tri))  # want_points=True fills three
    with pytest.raises(ValueError, match="out"):
        r.query_sweeps(o, d, 0.5, out=(t, tri, pt), want_points=False)
    with pytest.raises(ValueError, match="out"):
        r.query_sweeps(o, d, 0.5, out=t)
    with pytest.raises(ValueError, match="out t"):
        r.query_sweeps(o, d, 0.5, out=(torch.zeros(5), tri, pt))
    with pytest.raises(ValueError, match="tri"):
        r.query_sweeps(o, d, 0.5, out=(t, torch.zeros(4), pt))  # float32 where int32 is due
    with pytest.raises(ValueError, match="point"):
        r.query_sweeps(o, d, 0.5, out=(t, tri, torch.zeros(5, 3)))
    with pytest.raises(TypeError):
        r.query_sweeps(o, d, 0.5, tune_nothing=1)
    # what passes every check of the wrapper reaches the library, which this renderer does not have
    for radius in (0.5, 0, np.float32(0.25), torch.full((4,), 0.5)):
        with pytest.raises(AttributeError):
            r.query_sweeps(o, d, radius, sync=False)


# ---- the native reference ------------------------------------------------------------------------------------------------------
def test_the_reference_is_clean_under_sanitizers():
    """ASan + UBSan build of the stand-alone program, run as a program of its own, on a slice of one family with limits, pairs and
    invalid items; its answers are the plain build's."""
    for c in SX.family_case("d") + SX.family_case("h"):
        k = min(48, len(c["r"]))
        o, d, r = c["o"][-k:].copy(), c["d"][-k:].copy(), c["r"][-k:].copy()
        tmax = np.full(k, np.inf, f32) if "tmax" not in c else c["tmax"][-k:].copy()
        o[0, 1], r[1], tmax[2] = np.nan, -1.0, np.nan
        pairs = np.stack([np.arange(3, k), np.arange(3, k) % len(c["verts"])], 1)
        plain = SX.reference(c["verts"], o, d, r, tmax, pairs=pairs)
        checked = SX.reference(c["verts"], o, d, r, tmax, pairs=pairs, sanitized=True)
        for col in ("brute", "walk"):
            for key in ("t", "tri", "point"):
                assert SX.NR.same_bits(plain[col][key], checked[col][key]), (c["mesh"], col, key)
        assert SX.NR.same_bits(plain["pair_t"], checked["pair_t"])
        assert plain["brute"]["tri"][:3].tolist() == [-2, -2, -2]


@pytest.mark.parametrize("moved", (False, True))
@pytest.mark.parametrize("name", SX.FAMILIES + ("h",))
def test_the_walk_with_the_culling_rule_equals_brute_force(name, moved):
    """Tree independence: (b), the BVH8 walk that skips a box only when its entry time > best t, returns (a), the minimum over all
    triangles with every candidate evaluated, bit for bit in t, tri and point."""
    hits = 0
    for c in SX.family_case(name, 2400, moved):
        assert SX.walk_is_brute(c["ref"]), (name, c["mesh"])
        hits += int((c["ref"]["brute"]["tri"] >= 0).sum())
    assert hits >= (10 if name == "h" else 30), (name, hits)


def test_the_walk_visits_fewer_nodes_than_the_tree_has():
    """Families a and d on the soup and the terrain: the bound prunes.  Recorded in DESIGN.md section 6.24."""
    for name in ("a", "d"):
        for c in SX.family_case(name):
            if c["mesh"] not in ("soup_small", "terrain"):
                continue
            n = len(c["r"])
            per_item, tree = c["ref"]["nodes_total"] / n, c["ref"]["tree_nodes"]
            print(f"family {name} {c['mesh']}: {per_item:.2f} of {tree} nodes, {c['ref']['tris_total'] / n:.2f} of {len(c['verts'])} records per item")
            assert tree > 100 and per_item < tree / 8 and c["ref"]["tris_total"] / n < len(c["verts"]) / 8
            assert int(c["ref"]["nodes"].max()) < tree


def test_invalid_items_are_refused_and_the_rest_answered():
    for c in SX.family_case("h"):
        a = c["ref"]["brute"]
        bad = ~c["valid"]
        assert (a["tri"][bad] == SX.INVALID).all() and (a["tri"][~bad] >= SX.MISS).all()
        assert np.isnan(a["t"][bad]).all() and np.isnan(a["point"][bad]).all() and not np.isnan(a["t"][~bad]).any()
        assert bad.sum() == 18 + 6 + 1 + 3 and (a["tri"][~(c["tmax"] > 0) & ~bad] == SX.MISS).all()


def test_limits_are_strict_and_a_limit_at_or_below_zero_misses():
    """(d): tmax at the unlimited answer misses or finds nothing nearer (strictly), one ulp above keeps it, half of it, 0 and a
    negative limit miss, +inf is the unlimited answer."""
    for c in SX.family_case("d"):
        a = c["ref"]["brute"]
        full = SX.reference(c["verts"], c["o"], c["d"], c["r"])["brute"]
        kind = np.arange(len(a["t"])) % 6
        hit = full["tri"] >= 0
        assert hit.sum() > 100
        for k in (1, 3):
            assert SX.NR.same_bits(a["t"][kind == k], full["t"][kind == k]) and (a["tri"][kind == k] == full["tri"][kind == k]).all()
        assert (a["tri"][(kind == 0) | (kind == 4) | (kind == 5)] == SX.MISS).all()
        assert (a["tri"][(kind == 2) & (full["t"] > 0)] == SX.MISS).all()


# ---- the contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SX.FAMILIES)
def test_the_reference_satisfies_the_contract(name):
    for c in SX.family_case(name, N_CONTRACT):
        a = c["ref"]["brute"]
        assert (a["tri"] >= SX.MISS).all(), (name, c["mesh"])
        need = SX.needs(SX.items_of(c), a["t"], a["tri"], a["point"])
        print(f"family {name} {c['mesh']}: K needed {need.max():.3f}")
        assert (need <= SX.K).all(), (name, c["mesh"], int((need > SX.K).sum()), float(need.max()))
        assert (need.max() <= 16 * SX.K_MEASURED), "a family that needs 16 times the others has picked a wrong feature"


def test_the_constant_is_four_times_the_measurement():
    assert SX.K == RX.pow2_margin(SX.K_MEASURED) and SX.K_MEASURED == max(SX.K_FAMILY.values())
    assert max(SX.K_FAMILY.values()) <= 16 * sorted(SX.K_FAMILY.values())[len(SX.K_FAMILY) // 2]  # no family far above the median


def _differs(a, b, rel=1e-3):
    """Items whose answers differ: hit against miss, or times apart by more than rel of the larger."""
    ha, hb = a["tri"] >= 0, b["tri"] >= 0
    ta, tb = np.where(ha, a["t"], 0.0).astype(np.float64), np.where(hb, b["t"], 0.0).astype(np.float64)
    return (ha != hb) | (ha & hb & (np.abs(ta - tb) > rel * np.maximum(ta, tb)))


@pytest.mark.parametrize("mode,family", (("noedges", "m"), ("novertices", "m"), ("faceunchecked", "e"), ("faceunchecked", "a"), ("withhold", "c"), ("withhold", "m")))
def test_the_contract_rejects_mutated_references(mode, family):
    """The margin costs no power: the reference with the edge cylinders withheld, with the vertex spheres withheld, with the face
    accepted without its inside test, and with the winning triangle withheld answers differently on many items, and nearly every
    one of those answers is rejected (a withheld feature next to a grazing path changes the time by much and the distance by little)."""
    differing = rejected = 0
    for c in SX.family_case(family, N_CONTRACT):
        if family == "c" and c["mesh"] == "grid":
            continue  # its starts are exactly at r: with the touched triangle withheld a miss is as right
        good = c["ref"]["brute"]
        bad = SX.reference(c["verts"], c["o"], c["d"], c["r"], c.get("tmax"), mode=mode)["brute"]
        diff = _differs(good, bad)
        ok = SX.check(SX.items_of(c), bad["t"], bad["tri"], bad["point"])
        differing += int(diff.sum())
        rejected += int((diff & ~ok).sum())
    print(f"{mode} on family {family}: {differing} answers differ, {rejected} rejected")
    assert differing >= 20 and rejected >= 0.9 * differing, (mode, family, differing, rejected)


def test_the_contract_rejects_a_vertex_moved_by_64_K_units():
    """Answers computed on a mesh whose every triangle has vertex 0 moved by 64 K units along its normal, held to the contract of the
    unmoved mesh: rejected wherever the contact lies in the face with a weight of at least a quarter on that vertex."""
    seen = 0
    for m in ("terrain", "tetra"):
        v = SX.mesh(m)
        rng = np.random.default_rng(5)
        o, d = SX._aimed(rng, v, 300, "i")
        r = SX.edge_length(v) * rng.uniform(0.05, 0.5, 300)
        part = dict(verts=v, o=np.ascontiguousarray(o, f32), d=np.ascontiguousarray(d, f32), r=np.ascontiguousarray(r, f32))
        it = SX.items_of(part)
        good = SX.reference(v, part["o"], part["d"], part["r"])["brute"]
        assert SX.check(it, good["t"], good["tri"], good["point"]).all()
        S = max(float(np.abs(part["o"]).max()), float(np.abs(v).max()), float(part["r"].max()))
        tri64 = v.reshape(-1, 3, 3).astype(np.float64)
        moved = tri64.copy()
        moved[:, 0] += PX._normals(v, np.arange(len(tri64))) * 64 * SX.K * SX.U * S
        bad = SX.reference(moved.astype(f32).reshape(-1, 9), part["o"], part["d"], part["r"])["brute"]
        same = (bad["tri"] == good["tri"]) & (good["tri"] >= 0) & (good["t"] > 0)
        T = tri64[np.where(same, good["tri"], 0)]
        e1, e2, ap = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], good["point"].astype(np.float64) - T[:, 0]
        n = np.cross(e1, e2)
        u, w = (np.cross(ap, e2) * n).sum(1) / (n * n).sum(1), (np.cross(e1, ap) * n).sum(1) / (n * n).sum(1)
        in_face = same & (u > 0.05) & (w > 0.05) & (1 - u - w >= 0.25)
        assert in_face.sum() >= 20, (m, int(in_face.sum()))
        assert not SX.check(it, bad["t"], bad["tri"], bad["point"])[in_face].any(), m
        seen += int(in_face.sum())
    assert seen >= 60


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
BIG = np.array([[-4.0, 0.0, -4.0, 4.0, 0.0, -4.0, 0.0, 0.0, 6.0]], f32)  # one large triangle in the plane y = 0


def _closed(o, d, r, t64):
    """The reference's answer on BIG and the float64 closed form t64, both held to the contract; returns the two times."""
    o, d, r = np.asarray([o], f32), np.asarray([d], f32), np.asarray([r], f32)
    ref = SX.reference(BIG, o, d, r)
    assert SX.walk_is_brute(ref)
    a = ref["brute"]
    it = SX.Items(BIG, o, d, r)
    assert a["tri"][0] == 0 and SX.check(it, a["t"], a["tri"], a["point"]).all(), (a, SX.needs(it, a["t"], a["tri"], a["point"]))
    assert SX.check(it, np.array([t64]), np.array([0])).all()
    assert abs(float(a["t"][0]) - t64) <= 1e-5 * t64, (a["t"], t64)
    return float(a["t"][0]), t64


def _entry(m, d, r):
    """Smallest root of |m + t d| = r, float64."""
    A, B, Cc = float(d @ d), float(m @ d), float(m @ m) - r * r
    return (-B - np.sqrt(B * B - A * Cc)) / A


def test_closed_forms_on_one_large_triangle():
    """A face hit at t = (h - r) / |d_n|, an edge hit from the cylinder's quadratic, a vertex hit from the sphere's."""
    for h, r, d in ((3.0, 0.5, (0.1, -1.0, 0.05)), (2.5, 0.0, (0.3, -0.7, -0.2)), (-1.75, 0.625, (0.0, 2.0, 0.25))):
        dd = np.asarray(d, f32).astype(np.float64)
        _closed((0.3, h, 0.2), d, r, (abs(h) - float(f32(r))) / abs(dd[1]))
    # the edge from (-4, 0, -4) to (4, 0, -4), met from outside the triangle: the components across the edge (y, z) decide
    for o, d, r in (((0.5, 2.0, -7.0), (0.0, -0.5, 1.0), 0.75), ((-1.0, -1.0, -6.5), (0.4, 0.25, 0.5), 0.3), ((2.0, 0.5, -9.0), (-0.2, -0.1, 2.0), 1.5)):
        o64, d64 = np.asarray(o, f32).astype(np.float64), np.asarray(d, f32).astype(np.float64)
        m = o64 - [0.0, 0.0, -4.0]
        _closed(o, d, r, _entry(m[1:], d64[1:], float(f32(r))))
    # the vertex (0, 0, 6), met from beyond it
    for o, d, r in (((0.5, 1.5, 10.0), (-0.1, -0.3, -1.0), 0.5), ((0.0, -0.25, 9.0), (0.0, 0.0625, -0.5), 1.25), ((-1.0, 0.5, 12.0), (0.2, -0.1, -1.5), 0.5)):
        o64, d64 = np.asarray(o, f32).astype(np.float64), np.asarray(d, f32).astype(np.float64)
        _closed(o, d, r, _entry(o64 - [0.0, 0.0, 6.0], d64, float(f32(r))))


def test_degenerate_items_on_one_large_triangle():
    """A zero direction touches only at t = 0; a path that moves away misses; a start in contact is t = 0 whatever the direction."""
    o = np.array([[0.3, 1.0, 0.2]] * 4, f32)
    d = np.array([[0, 0, 0], [0, 0, 0], [0.1, 1.0, 0.0], [0.1, 1.0, 0.0]], f32)
    r = np.array([0.5, 1.0, 0.5, 1.5], f32)
    a = SX.reference(BIG, o, d, r)["brute"]
    assert a["tri"].tolist() == [-1, 0, -1, 0] and a["t"].tolist() == [np.inf, 0.0, np.inf, 0.0]
    assert np.abs(a["point"][1] - [0.3, 0.0, 0.2]).max() < 1e-6 and a["point"][1, 1] == 0 and np.isnan(a["point"][0]).all()


# ---- cross-checks against the references that exist ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "c"))
def test_the_start_touches_exactly_where_the_closest_point_reference_says(name):
    """t == 0 exactly where closest_on_tri's smallest d2 <= r * r (one fp32 product), and then the lowest such index is answered."""
    zero = 0
    for c in SX.family_case(name):
        a = c["ref"]["brute"]
        d2 = PX.reference(c["verts"], c["o"])["brute"]["d2"]
        touching = d2 <= c["r"] * c["r"]
        assert ((a["t"] == 0) == touching).all() and (a["tri"][touching] >= 0).all(), (name, c["mesh"])
        zero += int(touching.sum())
        k = np.nonzero(touching)[0][:40]  # the lowest index among the triangles the start touches
        if len(k):
            nt = len(c["verts"])
            pairs = np.stack([np.repeat(k, nt), np.tile(np.arange(nt), len(k))], 1)
            t = SX.reference(c["verts"], c["o"], c["d"], c["r"], pairs=pairs)["pair_t"].reshape(len(k), nt)
            assert (a["tri"][k] == (t == 0).argmax(1)).all(), (name, c["mesh"])
    assert zero >= 200


def test_a_sweep_of_radius_zero_is_the_ray_reference_on_face_interior_hits():
    """(e), r = 0: where the float64 ray reference finds no triangle's edge within 256 units of the ray, tri is its triangle and t
    agrees with its t within K units along the ray."""
    seen = 0
    for c in SX.family_case("e", N_CONTRACT * 2):
        a = c["ref"]["brute"]
        em = RX.ExactMesh(c["verts"])
        if not np.isfinite(em.n).all():
            continue
        cand = RX.Candidates(c["o"], c["d"], em)
        tri64, t64 = RX.exact_closest(cand)
        clear = ~cand._any((cand.t > 0) & (np.abs(cand.du) < 256)) & (tri64 >= 0)
        assert clear.sum() >= 50, c["mesh"]
        assert (a["tri"][clear] == tri64[clear]).all(), c["mesh"]
        _, _, tunit = RX.exact_pairs(c["o"][clear], c["d"][clear], em, tri64[clear])
        assert (np.abs(a["t"][clear].astype(np.float64) - t64[clear]) <= SX.K * tunit).all(), c["mesh"]
        seen += int(clear.sum())
    assert seen >= 300


def test_ties_on_the_grid_go_to_the_lower_index():
    """(f): straight down onto a shared vertex or a shared edge.  Wherever several triangles' own toi - looked at pair by pair - are
    bit-equal to the answer's, the answer is the lowest index among them."""
    c, = SX.family_case("f")
    a = c["ref"]["brute"]
    n, nt = len(c["r"]), len(c["verts"])
    assert (a["tri"] >= 0).all() and (a["t"] > 0).all()
    k = np.arange(0, n, 4)
    pairs = np.stack([np.repeat(k, nt), np.tile(np.arange(nt), len(k))], 1)
    t = SX.reference(c["verts"], c["o"], c["d"], c["r"], pairs=pairs)["pair_t"].reshape(len(k), nt)
    at_best = t.view(np.uint32) == a["t"][k].view(np.uint32)[:, None]
    assert (t >= a["t"][k][:, None]).all()
    assert (at_best.sum(1) >= 2).mean() > 0.5, float((at_best.sum(1) >= 2).mean())
    assert (a["tri"][k] == at_best.argmax(1)).all()
