"""Oracle B's ray queries against exact geometry (CPU only).

Every other path B test compares the kernels with oracle B, which shares their arithmetic: tri_test, SHADOW_TMAX and the box padding
are restated there, so an error common to both is invisible.  Here the oracle's answers - by brute force and through its own BVH -
are held to a float64 evaluation of the same rays and triangles (tests/ray_exact.py: the reference, the contract with its band K
and distance tolerance Kt, the ray families (a)-(j) and how the two constants were measured).  tests/test_gpu_ray_contract.py
holds the kernels to the same contract.  Measured figures are printed (they show without -s)."""
import functools

import numpy as np
import pytest

import ray_exact as X

f32 = np.float32


def say(capsys, text):
    with capsys.disabled():
        print("\n  [ray contract] " + text, end="")


@functools.lru_cache(maxsize=None)
def family_data(name):
    """Per part of the family: the oracle's answers by brute force and through its BVH, and the float64 candidates."""
    out = []
    for part in X.family(name):
        cc, co = X.part_candidates(part)
        out.append(dict(part=part, brute=X.part_reference(part), bvh=X.part_reference(part, use_bvh=True), cc=cc, co=co,
                        em=X.ExactMesh(X.mesh(part["mesh"])[0])))
    return out


@pytest.mark.parametrize("name", X.FAMILIES)
def test_oracle_answers_satisfy_the_exact_contract(name, capsys):
    closest = name in X.CLOSEST_FAMILIES
    n = hits = in_band = determined = 0
    k_need = kt_need = 0.0
    for p in family_data(name):
        part, cc, co = p["part"], p["cc"], p["co"]
        for how in ("brute", "bvh"):
            r = p[how]
            if closest:
                ok = cc.check_closest(r["tri"], r["t"])
                assert ok.all(), (name, part["mesh"], how, "closest hit", np.nonzero(~ok)[0][:8])
            ok = co.check_occluded(r["occ"])
            assert ok.all(), (name, part["mesh"], how, "occlusion", np.nonzero(~ok)[0][:8])
        b = p["brute"]
        assert np.array_equal(b["tri"], p["bvh"]["tri"]) and np.array_equal(b["t"], p["bvh"]["t"]) and np.array_equal(b["occ"], p["bvh"]["occ"])
        band, sure = cc.band()
        n += len(part["o"])
        hits += int((b["tri"] >= 0).sum())
        in_band += int(band.sum())
        determined += int((~band).sum())
        if closest:
            kt, k = cc.needs_closest(part["o"], part["d"], p["em"], b["tri"], b["t"], X.KT_DIST)
            k_need, kt_need = max(k_need, float(k.max())), max(kt_need, float(kt.max()))
        k_need = max(k_need, float(co.needs_occluded(b["occ"], X.KT_DIST).max()))
        assert 0.02 < b["occ"].mean() < 0.98, (name, part["mesh"], b["occ"].mean())  # both occlusion answers occur
        zeros = (part["d"] == 0).any(1)
        assert zeros.sum() >= 20 and (np.signbit(part["d"]) & (part["d"] == 0)).any(), "zero and -0.0 direction components"
    say(capsys, f"family {name}: {n} rays, K needed {k_need:.3f} of {X.K_BAND:g}, Kt needed {kt_need:.3f} of {X.KT_DIST:g}, "
                f"hit {hits / n:.1%}, a triangle in the band {in_band / n:.1%}")
    # the conditions that keep the family from being vacuous
    if closest:
        assert hits >= n / 2, hits / n
    if name in ("a", "g"):
        assert determined >= 0.99 * n, determined / n
    if name in ("b", "c", "d", "f"):
        assert in_band >= 0.05 * n, in_band / n


def test_grazing_families_graze():
    for name in ("g", "h"):
        for p in family_data(name):
            part, em = p["part"], p["em"]
            d = part["d"].astype(np.float64)
            cos = np.abs((d * em.n[part["target"]]).sum(1)) / np.linalg.norm(d, axis=1)  # to the triangle each ray is aimed at
            assert 0.5e-5 < cos.min() < 1e-4 and 0.9e-2 < cos.max() < 1.1e-2
    part = family_data("h")[0]["part"]
    M = np.abs(X.mesh("grid")[0]).max()
    far = np.abs(part["o"]).max(1)
    assert far.max() <= 32 * M and (far > 16 * M).mean() > 0.3
    part = family_data("d")[0]["part"]
    M = np.abs(X.mesh("soup")[0]).max()
    far = np.abs(part["o"]).max(1)
    assert far.max() <= 32 * M and (far > 16 * M).mean() > 0.15


# ---- the power of the checker: float64 only, no oracle, no kernels ------------------------------------------------------------
def _beside_edges(n=2000, seed=7):
    """Rays onto the terrain that pass BESIDE the two y-running edges of one vertex V, 12 to 40 units (2^-24 S) from them on their
    +x side and within a quarter of the edge's length of V: outside the band (inside it the contract accepts either neighbour, and
    a miss, by construction), inside the strip those edges sweep when V moves 64 units along +x.  Returns (vertices, the same
    with V moved, origins, directions, segments ending 0.03 to 0.07 % behind the surface)."""
    rng = np.random.default_rng(seed)
    verts = X.mesh("terrain")[0]
    v3 = verts.reshape(-1, 3)
    xs, ys = np.unique(v3[:-6, 0]), np.unique(v3[:-6, 1])
    vx, vy = xs[len(xs) // 2], ys[len(ys) // 5]  # a vertex inside the field, a dozen units in front of the origins
    at = lambda x, y: v3[(v3[:, 0] == x) & (v3[:, 1] == y)][0].astype(np.float64)
    V = at(vx, vy)
    W = np.stack([at(vx, ys[len(ys) // 5 + 1]), at(vx, ys[len(ys) // 5 - 1])])
    S = max(float(np.abs(W).max()), float(np.abs(V).max()), 30.0)
    unit = X.U * S
    moved = v3.copy()
    moved[(v3 == V.astype(f32)).all(1)] += np.array([64 * unit, 0, 0])
    moved = moved.astype(f32)
    assert (moved != v3).any(1).sum() == 6  # V is a corner of six triangles
    s = rng.uniform(0.02, 0.25, (n, 1))
    on_edge = V + s * (W[rng.integers(0, 2, n)] - V)
    o = rng.uniform([-5, -2, 8], [5, 2, 30], (n, 3)).astype(f32).astype(np.float64)
    # how many units of delta one unit along +x is worth for each ray (the incidence and the surface's slope decide)
    em = X.ExactMesh(verts)
    probe = X.exact_pairs(o[:, None, :], (on_edge + np.array([100 * unit, 0, 0]) - o)[:, None, :], em, np.arange(em.n_tris)[None, :])
    slope = np.where(probe[0] > 0, probe[1], -np.inf).max(1, keepdims=True) / 100
    assert (slope > 0.4).all()
    # delta between 12 units and nine tenths of what the moved edge sweeps at s <= 1/4 (48 units along x)
    aim = on_edge + np.array([1.0, 0, 0]) * unit * rng.uniform(12 / slope, 0.9 * 48, (n, 1))
    o = o.astype(f32)
    d = (aim - o).astype(f32)
    seg = ((aim - o) / rng.uniform(0.9993, 0.9997, (n, 1))).astype(f32)
    return verts, moved.reshape(-1, 9), o, d, seg


def test_the_contract_would_catch_wrong_geometry(capsys):
    """In the manner of test_the_irradiance_test_would_catch_...: the checker, fed answers computed in float64 from slightly wrong
    geometry, must reject them.  Measured shares of the rays rejected (this seed): moved vertex 100 %, inverted edge sign 100 %,
    0.999 -> 1.0 100 %; half of each is asserted, and the unaltered float64 answers must pass for every ray."""
    verts, moved, o, d, seg = _beside_edges()
    em = X.ExactMesh(verts)
    cc, co = X.Candidates(o, d, em), X.Candidates(seg * 0 + o, seg, em)
    band, sure = cc.band()
    assert not band.any() and sure.all(), "every ray is outside the band and surely hits"
    tri, t = X.exact_closest(cc)
    assert cc.check_closest(tri, t).all()
    truly_hidden = co._any((co.du >= 0) & (co.t > 0) & (co.t < X.T_SHADOW))
    assert co.check_occluded(truly_hidden).all()

    # one vertex moved by 64 units
    alt = X.Candidates(o, d, X.ExactMesh(moved))
    rej_moved = 1 - cc.check_closest(*X.exact_closest(alt)).mean()

    # the sign of one edge test inverted: edge 0 (v0 -> v1) accepts its outer side
    t_all, du_all, _ = X.exact_pairs(o[:, None, :], d[:, None, :], em, np.arange(em.n_tris)[None, :], flip_edge=0)
    best = np.where((t_all > 0) & (du_all >= 0), t_all, np.inf)
    wrong_tri = np.where(np.isfinite(best.min(1)), best.argmin(1), -1)
    rej_sign = 1 - cc.check_closest(wrong_tri, best.min(1)).mean()

    # 0.999 replaced by 1.0
    wrong_occ = co._any((co.du >= 0) & (co.t > 0) & (co.t < 1.0))
    rej_tmax = 1 - co.check_occluded(wrong_occ).mean()

    say(capsys, f"altered float64 answers rejected: vertex moved 64 units {rej_moved:.1%}, edge sign inverted {rej_sign:.1%}, "
                f"0.999 -> 1.0 {rej_tmax:.1%}")
    assert rej_moved >= 0.5 * MEASURED_REJECTED["moved"] > 0.25
    assert rej_sign >= 0.5 * MEASURED_REJECTED["sign"] > 0.25
    assert rej_tmax >= 0.5 * MEASURED_REJECTED["tmax"] > 0.25


MEASURED_REJECTED = dict(moved=1.0, sign=1.0, tmax=1.0)


# ---- the closed surface --------------------------------------------------------------------------------------------------------
def test_closed_surface_random_rays_all_hit(capsys):
    """200 000 rays from above the height field's footprint, each aimed down (up to 23 degrees off the vertical) at a uniformly
    random point of it: a surface without holes stops every one.  The intersection is NOT watertight along shared edges (below),
    but a random ray meets the band with a probability of the order of 2^-24 x (edge length per area) x S, about 1e-5 here, and so
    far none of these did.  Measured: 0 of 200 000 pass through.  Any that do must lie inside the band (the contract)."""
    import oracle as O

    rng = np.random.default_rng(31)
    n = 200000
    v, a, e = X.mesh("terrain")
    target = np.concatenate([rng.uniform([-27, 5], [27, 59], (n, 2)), np.full((n, 1), -5.0)], 1)
    d = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), -1.0)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (target - d * (17.0 / -d[:, 2:3])).astype(f32)  # origins at z = 12: above every hill, below the light
    d = d.astype(f32)
    t, tri, _ = X.oracle_answers(O.TriScene(v, a, e), o, d, None, use_bvh=True)
    leak = np.nonzero(tri < 0)[0]
    say(capsys, f"closed surface, random rays: {len(leak)} of {n} pass through")
    if len(leak):
        cc = X.Candidates(o[leak], d[leak], X.ExactMesh(v))
        assert cc.check_closest(tri[leak], t[leak]).all(), "a ray passes through the surface outside the band"
    assert len(leak) == 0  # measured; a leak inside the band would be no error of the oracle, but it would be news


def test_closed_surface_edge_aimed_rays_leak_only_inside_the_band(capsys):
    """Rays aimed at points ON the height field's shared edges (family (b)'s terrain part, plus as many again).  The fp32 test
    evaluates a shared edge differently for its two triangles and may reject both: such a ray passes through the closed surface
    (no hit, or a hit on whatever lies behind).  Every such ray must lie inside the band of its exact first triangle; the rate is
    printed.  Measured: see DESIGN.md section 6.3."""
    rng = np.random.default_rng(41)
    part = X._aimed(rng, "terrain", 8000, "e")
    ref = X.part_reference(part)
    cc, _ = X.part_candidates(part)
    tri64, t64 = X.exact_closest(cc)
    inner = tri64 >= 0  # the rest are aimed at the field's outer edges (or the light's) and pass beside them
    assert inner.mean() > 0.9
    te, due, tue = X.exact_pairs(part["o"], part["d"], X.ExactMesh(X.mesh("terrain")[0]), np.where(inner, tri64, 0))
    t = np.where(ref["tri"] >= 0, ref["t"].astype(np.float64), np.inf)
    with np.errstate(invalid="ignore"):
        leak = inner & (t - t64 > X.KT_DIST * tue)
    through = inner & (ref["tri"] < 0)
    n_in = inner.sum()
    say(capsys, f"closed surface, edge-aimed rays: {leak.sum() / n_in:.1%} of {n_in} leak ({through.sum() / n_in:.1%} hit nothing at all, "
                f"{(leak & ~through).sum() / n_in:.1%} hit a later surface); largest distance of a leaking ray from its edge {np.abs(due[leak]).max():.2f} units")
    assert leak.any(), "edge-aimed rays are expected to find the leaks"
    assert (np.abs(due[leak]) < X.K_BAND).all()
    assert cc.check_closest(ref["tri"], ref["t"]).all()
