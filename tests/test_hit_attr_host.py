"""CPU tests of the hit attributes (rt_query_rays_attr_device / rt_query_points_attr_device, Renderer.query_rays / query_points with
attributes=True, Renderer.interpolate): the boundary (exports, bindings, NULL contexts, the wrapper's refusals),
and the arithmetic of csrc/hit_attr.h through the native reference tests/native/hit_attr_ref.cpp - clean under ASan + UBSan; its
brute-force winner and t are the oracle's bit for bit on all ten ray families, and the header's u, v, det pass the accept test for it;
the invariants the header's comment proves hold on every hit; the reference satisfies the float64 contract of tests/attr_exact.py with
the committed constants; that contract rejects wrong answers; interpolate() reproduces the hit point; degenerate triangles have zero
normals.  The kernels themselves are tested on the GPU (tests/test_gpu_hit_attr.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_boundary as AB
import attr_exact as AX
import point_exact as PX
import ray_exact as RX
import raytracing_engine_amd as R
from raytracing_engine_amd import _lib
from test_ray_contract import family_data as oracle_data  # the oracle's brute-force answers per family, computed once for both modules

f32 = np.float32
FUNCTIONS = ("rt_query_rays_attr_device", "rt_query_points_attr_device")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS,  # no structs of its own: the ray and point queries' parameters
               null_calls=(("rt_query_rays_attr_device", (None, None, None, 0, None, None, None, None, None)),
                           ("rt_query_rays_attr_device", (V, V, None, 1, C.byref(R.RayQueryParams()), V, V, V, V)),
                           ("rt_query_points_attr_device", (None, None, 0, None, None, None, None, None, None)),
                           ("rt_query_points_attr_device", (V, None, 1, C.byref(R.PointQueryParams()), V, V, V, V, V))))


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)
    assert len(_lib.PROTOTYPES["rt_query_rays_attr_device"][1]) == 10 and len(_lib.PROTOTYPES["rt_query_points_attr_device"][1]) == 10


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_the_wrapper_refuses_before_the_library_is_called():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context and no library: whatever gets past the wrapper's checks fails on None
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), f32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    with pytest.raises(ValueError, match="attributes"):
        r.query_rays(good, good, any_hit=True, attributes=True)
    for bad in (a, good, good.double(), torch.zeros(3, 4).t(), torch.zeros(4, 4)):
        with pytest.raises(ValueError):
            r.query_rays(bad, good, attributes=True)
        with pytest.raises(ValueError):
            r.query_rays(good, bad, attributes=True)
        with pytest.raises(ValueError):
            r.query_points(bad, attributes=True)
        with pytest.raises(ValueError):
            r.query_points(bad, attributes=True, want_points=False)


def test_the_wrapper_checks_the_arity_and_shapes_of_out():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's, as in test_point_query_host.py)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    o = torch.zeros(4, 3)
    t, tri, c, uv, nrm = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(4, 3)
    for bad in ((t, tri), (t, tri, uv), (t, tri, uv, nrm, nrm), t):
        with pytest.raises(ValueError, match="out"):
            r.query_rays(o, o, attributes=True, out=bad)
    with pytest.raises(ValueError, match="out"):
        r.query_rays(o, o, out=(t, tri, uv, nrm))  # the plain query fills two
    with pytest.raises(ValueError, match="uv"):
        r.query_rays(o, o, attributes=True, out=(t, tri, torch.zeros(4, 3), nrm))
    with pytest.raises(ValueError, match="normal"):
        r.query_rays(o, o, attributes=True, out=(t, tri, uv, torch.zeros(5, 3)))
    for bad in ((t, tri, c), (t, tri, c, uv), (t, tri, uv, nrm), t):
        with pytest.raises(ValueError, match="out"):
            r.query_points(o, attributes=True, out=bad)
    with pytest.raises(ValueError, match="out"):
        r.query_points(o, attributes=True, want_points=False, out=(t, tri, c, uv, nrm))
    with pytest.raises(ValueError, match="uv"):
        r.query_points(o, attributes=True, out=(t, tri, c, torch.zeros(4), nrm))
    with pytest.raises(ValueError, match="normal"):
        r.query_points(o, attributes=True, want_points=False, out=(t, tri, uv, torch.zeros(4, 2)))
    with pytest.raises(TypeError):
        r.query_rays(o, o, attributes=True, tune_nothing=1)


# ---- the native reference ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_reference(name):
    """[(part, oracle brute force, ExactMesh, reference answers)] of one ray family, computed once for the tests below and left unchanged."""
    return [(p["part"], p["brute"], p["em"], AX.reference(RX.mesh(p["part"]["mesh"])[0], p["part"]["o"], p["part"]["d"])) for p in oracle_data(name)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_reference_is_clean_under_sanitizers():
    """ASan + UBSan build of the stand-alone program on a slice of every family, limits, invalid rays and the normals-only list
    included; its answers are the plain build's."""
    for name in RX.FAMILIES:
        for part, _, _, ref in family_reference(name):
            k = min(120, len(part["o"]))
            o, d = part["o"][:k].copy(), part["d"][:k].copy()
            tmax = np.where(np.arange(k) % 3 == 0, f32(np.inf), ref["t"][:k]).astype(f32)
            o[0, 1], d[1, 2] = np.nan, np.inf
            tmax[2:5] = [np.nan, 0.0, -1.0]
            tris = np.array([0, -1, len(RX.mesh(part["mesh"])[0]) - 1], np.int32)
            plain = AX.reference(RX.mesh(part["mesh"])[0], o, d, tmax, tris)
            checked = AX.reference(RX.mesh(part["mesh"])[0], o, d, tmax, tris, sanitized=True)
            for key in ("t", "ub", "vb", "uvd", "normal", "tri_normals"):
                assert np.array_equal(bits(plain[key]), bits(checked[key])), (name, part["mesh"], key)
            assert np.array_equal(plain["tri"], checked["tri"]) and plain["tri"][:5].tolist() == [-2, -2, -2, -1, -1]
            assert np.isnan(plain["ub"][:5]).all() and np.isnan(plain["normal"][:5]).all() and np.isnan(plain["tri_normals"][1]).all()


@pytest.mark.parametrize("name", RX.FAMILIES)
def test_the_winner_is_the_oracles_and_passes_the_accept_test(name):
    """Same arithmetic as the walk: the reference's winner and t are the oracle's brute-force answers bit for bit, and the header's
    u, v, det of that winner are values the accept test of tri_test passes."""
    hits = 0
    for part, brute, _, ref in family_reference(name):
        assert np.array_equal(ref["tri"], brute["tri"]), (name, part["mesh"], np.nonzero(ref["tri"] != brute["tri"])[0][:8])
        assert np.array_equal(bits(ref["t"]), bits(brute["t"])), (name, part["mesh"])
        hit = ref["tri"] >= 0
        u, v, det = (ref["uvd"][hit, k] for k in range(3))
        s = (u + v).astype(f32)  # the fp32 sum the test forms
        pos = det > 0
        assert (det != 0).all()
        assert (np.where(pos, (u >= 0) & (v >= 0) & (s <= det), (u <= 0) & (v <= 0) & (s >= det))).all(), (name, part["mesh"])
        assert np.array_equal(bits(ref["ub"][hit]), bits(u / det)) and np.array_equal(bits(ref["vb"][hit]), bits(v / det))  # numpy's fp32 quotient is correctly rounded too
        assert np.isnan(ref["ub"][~hit]).all() and np.isnan(ref["vb"][~hit]).all() and np.isnan(ref["normal"][~hit]).all()
        hits += int(hit.sum())
    assert hits > 1000


@pytest.mark.parametrize("name", RX.FAMILIES)
def test_invariants_on_every_hit(name):
    for part, _, _, ref in family_reference(name):
        hit = ref["tri"] >= 0
        ub, vb = ref["ub"][hit], ref["vb"][hit]
        assert (ub >= 0).all() and (vb >= 0).all()  # as comparisons: -0.0 passes
        assert (ub.astype(np.float64) + vb.astype(np.float64) <= 1 + 2.0 ** -22).all(), (name, part["mesh"])
        n2 = (ref["normal"][hit].astype(np.float64) ** 2).sum(1)
        zero = (ref["normal"][hit] == 0).all(1)
        assert (zero | (np.abs(n2 - 1) <= 2.0 ** -21)).all(), (name, part["mesh"], float(np.abs(n2 - 1)[~zero].max()))
        if name in RX.CLOSEST_FAMILIES:
            assert not zero.any()


# ---- the float64 contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RX.FAMILIES)
def test_the_reference_satisfies_the_contract(name, capsys):
    k_uv = k_n = 0.0
    excluded = 0
    for part, _, em, ref in family_reference(name):
        need = AX.uv_needs(em, part["o"], part["d"], ref["tri"], ref["ub"], ref["vb"])
        assert (need <= AX.KUV).all(), (name, part["mesh"], int((need > AX.KUV).sum()), float(need.max()))
        need_n, ex = AX.normal_needs(em, ref["tri"], ref["normal"])
        assert (need_n <= AX.KN).all(), (name, part["mesh"], int((need_n > AX.KN).sum()), float(need_n.max()))
        k_uv, k_n, excluded = max(k_uv, float(need.max())), max(k_n, float(need_n.max())), excluded + ex
    with capsys.disabled():
        print(f"\n  [hit attributes] family {name}: Kuv needed {k_uv:.3f} of {AX.KUV:g}, Kn needed {k_n:.3f} of {AX.KN:g}, excluded from Kn {excluded}", end="")
    if name in RX.CLOSEST_FAMILIES:
        assert excluded == 0


def test_the_contract_rejects_wrong_answers():
    """Power.  Kuv is set by the grazing rays of family (g) - the quotient by det loses 1 / |cos| of its digits - so in units of 2^-24 S
    it is wide for the rays of family (a): Kuv units are S / 64, a fraction of a triangle for an origin a few triangles away.  The
    contract rejects every altered answer that is off by more than twice the band, perpendicular to the ray: (ub, vb) swapped (the
    point moves by |ub - vb| |V1 - V2|: beyond twice the band for 14 % of the hits on the soup and on the terrain, hundreds of rays,
    and for next to none on the flat grid, whose cells are 0.37 wide at S > 5.3), barycentrics applied to the neighbouring triangle
    (the next index - a soup triangle elsewhere, the quad's other half or the next quad on the grids: 99 %, 99 %, 52 %), and a
    normal with one sign flipped (all of them)."""
    shares, counts = [], []
    for part, _, em, ref in family_reference("a"):
        hit = ref["tri"] >= 0
        o, d, tri, ub, vb = part["o"][hit], part["d"][hit], ref["tri"][hit], ref["ub"][hit], ref["vb"][hit]
        assert AX.check_uv(em, o, d, tri, ub, vb).all()
        d64 = d.astype(np.float64)
        dh = d64 / np.linalg.norm(d64, axis=1, keepdims=True)
        S = np.maximum(np.maximum(np.abs(o.astype(np.float64)).max(1), em.vmax[tri]), np.abs(AX.bary_point(em, tri, ub, vb)).max(1))

        def apart(P):  # distance of P from the unaltered point, perpendicular to the ray, in units
            diff = P - AX.bary_point(em, tri, ub, vb)
            return np.linalg.norm(diff - (diff * dh).sum(1, keepdims=True) * dh, axis=1) / (AX.U * S)

        far = apart(AX.bary_point(em, tri, vb, ub)) > 2 * AX.KUV
        assert not AX.check_uv(em, o, d, tri, vb, ub)[far].any()
        other = (tri + 1) % em.n_tris
        moved = AX.bary_point(em, other, ub, vb)
        far2 = apart(moved) > 2 * AX.KUV
        assert not AX.check_uv(em, o, d, tri, ub, vb, point=moved)[far2].any()
        shares.append((part["mesh"], float(far.mean()), float(far2.mean())))
        counts.append((part["mesh"], int(far.sum()), int(far2.sum())))
        nrm = ref["normal"][hit].copy()
        assert AX.check_normal(em, tri, nrm).all()
        k = np.abs(nrm).argmax(1)
        nrm[np.arange(len(nrm)), k] *= -1
        assert not AX.check_normal(em, tri, nrm).any()
    print("shares of the altered answers beyond twice the band (swapped, neighbour):", shares)
    # at least a hundred rays per mesh on which the alteration is visible at all (the grid's swapped points excepted, see above)
    assert all(n_far >= 100 for m, n_far, _ in counts if m != "grid") and all(n_far2 >= 100 for _, _, n_far2 in counts), counts


# ---- interpolate -----------------------------------------------------------------------------------------------------------------
def test_interpolate_reproduces_the_hit_point():
    """On CPU tensors: the vertex positions interpolated at the reference's (tri, ub, vb) are o + t d within the contract (float64
    tensors, so that the evaluation adds nothing), in float32 too up to its own rounding; miss rows are NaN."""
    torch = pytest.importorskip("torch")
    misses = 0
    for part, _, em, ref in family_reference("a") + family_reference("g"):
        verts = RX.mesh(part["mesh"])[0].reshape(-1, 3, 3)
        tri, uv = torch.from_numpy(ref["tri"]), torch.from_numpy(np.stack([ref["ub"], ref["vb"]], 1))
        P = R.Renderer.interpolate(tri, uv.double(), torch.from_numpy(verts).double()).numpy()
        hit = ref["tri"] >= 0
        assert P.shape == (len(hit), 3) and np.isnan(P[~hit]).all() and np.isfinite(P[hit]).all()
        misses += int((~hit).sum())
        assert AX.check_uv(em, part["o"], part["d"], ref["tri"], ref["ub"], ref["vb"], point=np.where(hit[:, None], P, 0.0)).all()
        assert np.array_equal(P[hit], AX.bary_point(em, ref["tri"][hit], ref["ub"][hit], ref["vb"][hit]))
        P32 = R.Renderer.interpolate(tri, uv, torch.from_numpy(verts))
        assert P32.dtype == torch.float32 and np.isnan(P32.numpy()[~hit]).all()
        assert np.abs(P32.numpy()[hit] - P[hit]).max() <= 8 * 2.0 ** -24 * np.abs(verts).max()
        # a (n_tris, 3, C) attribute of another width, int64 indices
        w = R.Renderer.interpolate(tri.long(), uv, torch.ones(len(verts), 3, 5))
        assert w.shape == (len(hit), 5) and np.allclose(w.numpy()[hit], 1.0, atol=1e-6) and np.isnan(w.numpy()[~hit]).all()
    assert misses > 0  # there were miss rows to look at
    with pytest.raises(ValueError):
        R.Renderer.interpolate(tri, uv, torch.ones(len(verts), 3))
    with pytest.raises(ValueError):
        R.Renderer.interpolate(tri, uv[:-1], torch.ones(len(verts), 3, 1))


# ---- degenerate records ----------------------------------------------------------------------------------------------------------
def test_degenerate_winners_have_zero_normals_and_finite_uv():
    """Closest-point winners without a normal: the collinear triangle and the point of point_exact's needle mesh (zero area), and
    triangles of size ~1e-25, whose |n|^2 underflows.  Their (u, v) - point_tri.h's - are finite, their normals three zeros; the
    needle of aspect 1e6 beside them has a unit normal."""
    v = PX.needle_mesh().reshape(-1, 3, 3)
    tiny = (np.array([[1.5, -0.5, 0.25]], f32) + np.array([[0, 0, 0], [1e-25, 0, 0], [0, 1e-25, 0]], f32)).astype(f32)  # collapses to a point at this offset
    tiny0 = np.array([[0, 0, 0], [1e-25, 0, 0], [0, 1e-25, 0]], f32)  # at the origin it keeps its shape: area 5e-51
    verts = np.concatenate([v, tiny[None], tiny0[None]]).reshape(-1, 9)
    pts = np.array([v[6, 0], (v[6, 0] + v[6, 1]) / 2, v[9, 0], tiny[0], tiny0[0], [3e-26, 3e-26, 0], v[3, 0]], f32)
    ref = PX.reference(verts, pts)["brute"]
    assert ref["tri"].tolist() == [6, 6, 9, 12, 13, 13, 3]
    assert np.isfinite(ref["u"]).all() and np.isfinite(ref["v"]).all() and (ref["u"] >= 0).all() and (ref["v"] >= 0).all()
    normals = AX.reference(verts, np.zeros((0, 3), f32), np.zeros((0, 3), f32), tris=ref["tri"])["tri_normals"]
    assert (normals[:6] == 0).all() and not np.signbit(normals[:6]).any()
    assert abs(float((normals[6].astype(np.float64) ** 2).sum()) - 1) <= 2.0 ** -21
