"""CPU tests of the closest-point query (rt_query_points_device / Renderer.query_points): the boundary (exports,
bindings, NULL contexts, struct layouts, defaults, the wrapper's refusals), and the arithmetic of csrc/point_tri.h through the native
reference tests/native/point_query_ref.cpp - clean under ASan + UBSan; its BVH8 walk with the culling rule equals its brute force bit
for bit on every family (the test of the culling argument: no GPU needed); the brute force satisfies the float64 contract of
tests/point_exact.py with the committed Kp; and that contract rejects wrong answers.  The kernel itself is tested on the GPU
(tests/test_gpu_point_query.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_boundary as AB
import point_exact as PX
import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

FUNCTIONS = ("rt_default_point_query_params", "rt_query_points_device", "rt_get_point_query_stats")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS, params="PointQueryParams", stats="PointQueryStats", params_c="rt_point_query_params", stats_c="rt_point_query_stats",
               params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"], stats_fields=["points", "invalid_points", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
               constants={"RT_POINT_MISS": _lib.POINT_MISS, "RT_POINT_INVALID": _lib.POINT_INVALID}, default="rt_default_point_query_params",
               null_calls=(("rt_query_points_device", (None, None, 0, None, None, None, None)),
                           ("rt_query_points_device", (V, None, 1, C.byref(R.PointQueryParams()), V, V, V)),
                           ("rt_get_point_query_stats", (C.byref(R.PointQueryStats()),)), ("rt_default_point_query_params", ())))
N = 4000


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    AB.struct_layout(KIND, tmp_path)
    assert (R.Renderer.POINT_MISS, R.Renderer.POINT_INVALID) == (-1, -2)


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
            r.query_points(bad)
        with pytest.raises(ValueError):
            r.query_points(bad, want_points=False)


def test_the_wrapper_compares_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    p = torch.zeros(4, 3)
    d, t, c = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="points"):
        r.query_points(torch.zeros(4, 4))
    for bad_rmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1)):
        with pytest.raises(ValueError, match="rmax"):
            r.query_points(p, rmax=bad_rmax)
    with pytest.raises(ValueError, match="rmax"):
        r.query_points(p, rmax=np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="out"):
        r.query_points(p, out=(d, t))  # want_points=True fills three
    with pytest.raises(ValueError, match="out"):
        r.query_points(p, out=(d, t, c), want_points=False)
    with pytest.raises(ValueError, match="out"):
        r.query_points(p, out=d)
    with pytest.raises(ValueError, match="dist"):
        r.query_points(p, out=(torch.zeros(5), t, c))
    with pytest.raises(ValueError, match="tri"):
        r.query_points(p, out=(d, torch.zeros(4), c))  # float32 where int32 is due
    with pytest.raises(ValueError, match="point"):
        r.query_points(p, out=(d, t, torch.zeros(5, 3)))
    with pytest.raises(TypeError):
        r.query_points(p, tune_nothing=1)


# ---- the native reference ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_reference(name):
    """[(part, reference answers)] of one family, computed once for the tests below and left unchanged."""
    return [(part, PX.reference(part["verts"], part["p"])) for part in PX.family(name, N)]


def same_bits(a, b):
    return a.view(np.uint32).tolist() == b.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist() == b.tolist()


def test_the_reference_is_clean_under_sanitizers():
    """ASan + UBSan build of the stand-alone program on a slice of every family, limits and invalid points included; its answers
    are the plain build's."""
    for name in PX.FAMILIES:
        for part, ref in family_reference(name):
            k = min(150, len(part["p"]))
            p = part["p"][-k:].copy()  # the tail: family d's points at the reach
            rmax = np.where(np.arange(k) % 3 == 0, np.float32(np.inf), ref["brute"]["dist"][-k:]).astype(np.float32)
            p[0, 1] = np.nan
            rmax[1:4] = [np.nan, 0.0, -1.0]
            plain = PX.reference(part["verts"], p, rmax)
            checked = PX.reference(part["verts"], p, rmax, sanitized=True)
            for col in ("brute", "walk"):
                for key in ("tri", "d2", "u", "v", "dist", "c"):
                    assert same_bits(plain[col][key].ravel(), checked[col][key].ravel()), (name, part["mesh"], col, key)
            assert plain["brute"]["tri"][:4].tolist() == [-2, -2, -1, -1]


@pytest.mark.parametrize("name", PX.FAMILIES)
def test_the_walk_with_the_culling_rule_equals_brute_force(name):
    """Tree independence: (b), the BVH8 walk that skips a box only when lb2 > best d2, returns (a), the minimum over all triangles,
    bit for bit - family d's points at the reach limit too - and does prune."""
    for part, ref in family_reference(name):
        a, b = ref["brute"], ref["walk"]
        assert (a["tri"] >= 0).all(), (name, part["mesh"])
        for key in ("tri", "d2", "u", "v", "dist", "c"):
            assert same_bits(a[key].ravel(), b[key].ravel()), (name, part["mesh"], key)
        n_tris = len(part["verts"])
        if n_tris > 100 and name != "d":
            assert ref["tris"] / len(part["p"]) < n_tris / 8, (name, part["mesh"], ref["tris"] / len(part["p"]))


def test_the_walk_equals_brute_force_under_limits():
    for name in ("a", "c", "g"):
        for part, ref in family_reference(name):
            d = ref["brute"]["dist"]
            n = len(d)
            rmax = np.choose(np.arange(n) % 5, [d, np.nextafter(d, np.float32(np.inf)), d * np.float32(0.5), np.full(n, np.inf, np.float32),
                                                 np.full(n, 1e-30, np.float32)]).astype(np.float32)
            lim = PX.reference(part["verts"], part["p"], rmax)
            a, b = lim["brute"], lim["walk"]
            for key in ("tri", "d2", "u", "v", "dist", "c"):
                assert same_bits(a[key].ravel(), b[key].ravel()), (name, part["mesh"], key)
            # the limited answer is the unlimited one where its d2 < rmax * rmax (one fp32 product), else a miss
            keep = ref["brute"]["d2"] < rmax * rmax
            assert a["tri"].tolist() == np.where(keep, ref["brute"]["tri"], -1).tolist()
            assert same_bits(a["dist"], np.where(keep, d, np.float32(np.inf)).astype(np.float32))
            # (rmax = dist: hit or miss as dist * dist rounds above d2 or not; both occur)  an rmax whose square is 0 admits nothing
            assert 0 < keep[np.arange(n) % 5 == 0].sum() < n // 5 or n < 100
            assert (a["tri"][np.arange(n) % 5 == 4] == -1).all() and keep[np.arange(n) % 5 == 3].all()


@pytest.mark.parametrize("name", PX.FAMILIES)
def test_the_reference_satisfies_the_contract(name):
    for part, ref in family_reference(name):
        em = PX.ExactTris(part["verts"])
        a = ref["brute"]
        ok = PX.check(em, part["p"], a["tri"], a["dist"], a["c"])
        assert ok.all(), (name, part["mesh"], int((~ok).sum()), float(PX.needs(em, part["p"], a["tri"], a["dist"], a["c"]).max()))
        # (u, v) lies in the closed triangle, up to one rounding of the sum
        assert (a["u"] >= 0).all() and (a["v"] >= 0).all() and (a["u"].astype(np.float64) + a["v"] <= 1 + 2.0 ** -23).all()
        assert np.isfinite(a["d2"]).all()


def test_exact_ties_go_to_the_lower_index():
    """(e): above vertices and edge midpoints of the grid several triangles are at the same exact distance.  Wherever the reference's
    own d2 of those triangles are bit-equal - looked at pair by pair - the answer is the lowest index among them.  (f): every triangle
    of the soup twice: the first copy wins."""
    (part, ref), = family_reference("e")
    em = PX.ExactTris(part["verts"])
    D = em.all_dists(part["p"])
    tied = D == D.min(1, keepdims=True)  # exactly, in float64
    assert (tied.sum(1) >= 2).mean() > 0.5  # (the float64 evaluation itself rounds: not every geometric tie is an equality)
    i, t = np.nonzero(tied)
    d2 = PX.reference(part["verts"], part["p"], pairs=np.stack([i, t], 1))["pair_d2"]
    best = ref["brute"]
    at_best = d2.view(np.uint32) == best["d2"].view(np.uint32)[i]
    lowest = np.full(len(part["p"]), np.iinfo(np.int64).max)
    np.minimum.at(lowest, i[at_best], t[at_best])
    has = lowest < np.iinfo(np.int64).max
    assert has.mean() > 0.9  # the winner is nearly always one of the exactly tied triangles
    assert (best["tri"][has] <= lowest[has]).all()
    several = np.bincount(i[at_best], minlength=len(has)) >= 2
    assert several.mean() > 0.5 and (best["tri"][several] == lowest[several]).all()
    (part, ref), = family_reference("f")
    assert (ref["brute"]["tri"] < len(part["verts"]) // 2).all()


def test_degenerate_triangles_are_the_segment_or_point_they_are():
    (part, ref), = family_reference("g")
    a = ref["brute"]
    assert set(a["tri"].tolist()) >= {3, 6, 9}  # the needle, the collinear one and the point are all somebody's nearest
    assert np.isfinite(a["dist"]).all() and np.isfinite(a["c"]).all()


def test_the_contract_rejects_wrong_answers():
    """The margin costs no power: float64 answers from geometry with one vertex of the nearest triangle moved by 64 Kp units, and
    float64 answers with the nearest triangle withheld (for points whose two nearest triangles differ by more than the band), are
    all rejected; the unaltered float64 answers pass."""
    for part in PX.family("c", 900):
        em = PX.ExactTris(part["verts"])
        p = part["p"]
        D = em.all_dists(p)
        unit = PX.unit_of(p, em)
        tri, dist, c = PX.exact_answer(em, p, D)
        assert PX.check(em, p, tri, dist, c, D=D).all()
        # one vertex moved: the one that weighs most at the nearest point, along the line from that point to p
        idx = np.arange(len(p))
        uv = _weights(em, tri, c)
        w = np.stack([1 - uv.sum(1), uv[:, 0], uv[:, 1]], 1)
        k = w.argmax(1)
        direction = p.astype(np.float64) - c
        off = np.linalg.norm(direction, axis=1) > 1e-9
        direction = direction / np.where(off, np.linalg.norm(direction, axis=1), 1.0)[:, None]
        alt = PX.ExactTris(part["verts"][:1])
        alt.v = em.v[tri].copy()
        alt.v[idx, k] += direction * (64 * PX.KP * unit)[:, None]
        d_alt = alt.dist(p, idx)
        c_alt = PX.closest_point64(alt, p, idx)
        rejected = ~PX.check(em, p, tri, d_alt, c_alt, D=D)
        assert off.mean() > 0.9 and rejected[off].all(), int((~rejected[off]).sum())
        # the nearest triangle withheld
        tri2, dist2, c2 = PX.exact_answer(em, p, D, withhold_nearest=True)
        apart = dist2 - dist > PX.KP * unit
        assert apart.mean() > 0.5 and not PX.check(em, p, tri2, dist2, c2, D=D)[apart].any()


def _weights(em, tri, c):
    """(u, v) of the points c in their triangles, least squares in float64."""
    A, B, Cc = em.v[tri, 0], em.v[tri, 1], em.v[tri, 2]
    ab, ac, ap = B - A, Cc - A, c - A
    d11, d12, d22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    r1, r2 = (ap * ab).sum(1), (ap * ac).sum(1)
    det = d11 * d22 - d12 * d12
    return np.stack([(r1 * d22 - r2 * d12) / det, (r2 * d11 - r1 * d12) / det], 1)


def test_pruning_on_the_terrain():
    """What the GPU test's cap (mean triangles tested per point <= n_tris / 8 on family b of the terrain) is worth: the reference walk
    stays far below it.  Recorded in DESIGN.md section 6.14."""
    part, ref = family_reference("b")[0]
    assert part["mesh"] == "terrain"
    n_tris = len(part["verts"])
    per_point = ref["tris"] / len(part["p"])
    print(f"terrain, family b: {per_point:.2f} triangles and {ref['nodes'] / len(part['p']):.2f} nodes per point; cap {n_tris / 8:.1f}; brute force {n_tris}")
    assert per_point < n_tris / 8 / 4
