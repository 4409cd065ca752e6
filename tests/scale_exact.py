"""Path B across coordinate scale: the problem scaled by 2^k, what each answer must then be, and how far that holds.

Test helper (imported by tests/test_scale_host.py and tests/test_gpu_scale.py); a sibling of tests/ray_exact.py, tests/point_exact.py,
tests/hit_exact.py, tests/neighbor_exact.py, tests/sign_exact.py and tests/attr_exact.py, whose meshes, families and native references
it uses; not a conftest, no fixtures.

THE IDEA.  Multiplying every LENGTH of a problem - vertices, origins, points, tmax, rmax, occlusion segments, ray_eps, the camera's
position - by 2^k changes no fp32 mantissa, so every fp32 operation of path B rounds as before until an intermediate leaves the
normal range.  Directions, albedo, emission and the sky are not lengths and stay.  The answers of the scaled problem are then the
k = 0 answers, transformed: indices, counts, offsets, sides, crossings, barycentrics, unit normals and frames unchanged; t (directions
unscaled), dist, signed distance, closest points and listed t / dist times 2^k.  That is a test without a tolerance.

THE RANGES.  measure() (python tests/scale_exact.py) finds, on the CPU references - never on the kernels -, for each family of answers
the contiguous range of k about 0 over which ALL answers of the case are bit for bit the transformed k = 0 answers.  RANGES holds
what it found: (k_lo, k_hi) inclusive; k_lo - 1 and k_hi + 1 are the first scales at which an answer differs.  The cases: 4 096 rays
(ray_exact's families on its soup of 2 000 triangles and its flat grid), 4 096 points (point_exact's families on the soup, the grid and
the needle mesh), 4 096 points of sign_exact's families on its sphere and on the soup, and 48 x 32 frames, 2 samples, 3 bounces, of the
Cornell box and of soup_scene(2000), Lambert and with mirrors and glass.  m0(family) is the largest |coordinate| of the family's
smallest mesh at k = 0: a range's upper end k_hi has been seen to hold up to M = m0 * 2^k_hi on every mesh of the family.

THE CONTRACTS.  contract_failures(family, k) holds answers at scale k to the float64 contracts of the sibling modules on the scaled
problem, constants unchanged: their units are relative to the largest coordinate, so they are as strict at 2^-30 as at 1.

THE LIMIT.  COORD_LIMIT_LOG2 is the library's RT_PT_MAX_COORD_LOG2 (derived in DESIGN.md section 6.3, it must lie inside every measured
range); gpu_scales(family) are the scales the GPU tests use: up to the limit at the top, down to the measured end at the bottom.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attr_exact as AX  # noqa: E402
import hit_exact as HX  # noqa: E402
import native_ref as NR  # noqa: E402
import neighbor_exact as NX  # noqa: E402
import point_exact as PX  # noqa: E402
import ray_exact as RX  # noqa: E402
import sign_exact as SX  # noqa: E402

ROOT = PX.ROOT
f32 = np.float32
INF = f32(np.inf)
N = 4096
FRAME = dict(width=48, height=32, spp=2, bounces=3)

# The library's limit (include/rt_abi.h RT_PT_MAX_COORD_LOG2): meshes with max(1, M) above 2^COORD_LIMIT_LOG2
# are refused by every path B render and query entry.
COORD_LIMIT_LOG2 = 20
# The smallest feature (edge, surface-to-light distance, ray_eps) above which answers are scale-covariant: 2^FEATURE_MIN_LOG2
FEATURE_MIN_LOG2 = -24

LENGTHS = ("verts", "o", "p", "tmax", "rmax", "seg", "ray_eps", "pos")  # multiplied by 2^k
FIXED = ("d", "albedo", "emission", "sky", "rot", "kind", "ior")           # not lengths


# ---- scaling -------------------------------------------------------------------------------------------------------------------
SCALE = np.ldexp  # (x, k) -> x * 2^k.  tests/test_scale_host.py puts a factor that is no power of two here to show that the self-check sees it


def scaled(x, k, scale=None):
    """x * 2^k in fp32 (None stays None)."""
    if x is None:
        return None
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray((scale or SCALE)(np.asarray(x, f32), k), f32)


def exactly_scaled(x, y):
    """y is x times a power of two with nothing lost: the same mantissas and signs, zeros, infinities and NaNs where they were."""
    if x is None:
        return y is None
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    mx, _ = np.frexp(x)
    my, _ = np.frexp(y)
    return x.shape == y.shape and bool(np.array_equal(mx, my, equal_nan=True)) and bool(np.array_equal(np.signbit(x), np.signbit(y)))


def scaled_problem(k, scale=None, check=True, **q):
    """The problem q (keys of LENGTHS and FIXED) with every length times 2^k.  The self-check: every scaled array kept its mantissas
    (check=False returns the problem with "exact" False instead of raising - a scan past the ends of the number format wants that)."""
    out, exact = {}, True
    for key, x in q.items():
        if key in LENGTHS:
            out[key] = scaled(x, k, scale)
            exact = exact and exactly_scaled(x, out[key])
        elif key in FIXED:
            out[key] = x
        else:
            raise KeyError(f"{key}: neither a length nor a fixed quantity")
    if check:
        assert exact, f"scaling by 2^{k} is not exact: a mantissa changed (not a power of two, or the number format ran out)"
    out["exact"] = exact
    return out


bits_equal = functools.partial(NR.same_bits, same_dtype=True)  # bit-equal arrays of one dtype and shape (NaN equals the same NaN, -0.0 is not 0.0)


def transformed(answers, k):
    """The k = 0 answers as the problem scaled by 2^k must give them: keys that end in "*" are lengths, the others stay."""
    return {key: (scaled(x, k) if key.endswith("*") else x) for key, x in answers.items()}


def differing(got, want):
    """Names of the answers that are not bit-equal (a missing or extra key counts)."""
    return sorted(key for key in set(got) | set(want) if key not in got or key not in want or not bits_equal(got[key], want[key]))


# ---- the cases: inputs at k = 0 ------------------------------------------------------------------------------------------------
RAY_MESHES = ("soup", "grid")
POINT_MESHES = ("soup", "grid", "needle")


def _gather(parts, meshes, keys, total):
    """The parts on `meshes`, concatenated per mesh and thinned evenly (every family stays in) so that all meshes together hold `total` rows."""
    by = {}
    for part in parts:
        if part["mesh"] in meshes:
            by.setdefault(part["mesh"], []).append(part)
    out, left = [], total
    for i, m in enumerate(meshes):
        take = left // (len(meshes) - i)
        have = sum(len(p[keys[0]]) for p in by[m])
        assert have >= take, (m, have, take)
        pick = np.round(np.linspace(0, have - 1, take)).astype(np.int64)
        rows = {key: np.ascontiguousarray(np.concatenate([p[key] for p in by[m]])[pick], f32) for key in keys}
        assert len(np.unique(pick)) == take, (m, take)
        left -= take
        out.append(dict(mesh=m, **rows))
    return out


@functools.lru_cache(maxsize=None)
def ray_cases():
    """[dict(mesh, verts, o, d, seg, tmax)]: N rays of ray_exact's families on the soup and the grid.  tmax in turn: none, one ulp
    above the k = 0 closest hit's t (the hit stays), half of it (it goes)."""
    parts = [p for name in RX.FAMILIES for p in RX.family(name, 1200)]
    out = []
    for c in _gather(parts, RAY_MESHES, ("o", "d", "seg"), N):
        c["verts"] = RX.mesh(c["mesh"])[0]
        t = AX.reference(c["verts"], c["o"], c["d"])["t"]
        i = np.arange(len(t))
        t1 = np.where(np.isfinite(t), t, f32(1))
        c["tmax"] = np.select([i % 3 == 0, i % 3 == 1], [np.full(len(t), INF), np.nextafter(t1, INF)], f32(0.5) * t1).astype(f32)
        out.append(c)
    assert sum(len(c["o"]) for c in out) == N
    return out


@functools.lru_cache(maxsize=None)
def point_cases():
    """[dict(mesh, verts, p, rmax)]: N points of point_exact's families on the soup, the grid and the needle mesh.  rmax: twice the
    k = 0 distance plus 0.1, at most the distance plus 0.5 (ten neighbours a point on average, up to 364); every fourth point without a limit for the closest-point query (rmax_point)."""
    parts = [p for name in PX.FAMILIES for p in PX.family(name, 2400)]
    out = []
    for c in _gather(parts, POINT_MESHES, ("p",), N):
        c["verts"] = PX.mesh(c["mesh"])
        dist = PX.reference(c["verts"], c["p"])["brute"]["dist"]
        c["rmax"] = np.minimum(f32(2) * dist + f32(0.1), dist + f32(0.5)).astype(f32)
        c["rmax_point"] = np.where(np.arange(len(dist)) % 4 == 0, INF, c["rmax"]).astype(f32)
        out.append(c)
    assert sum(len(c["p"]) for c in out) == N
    return out


@functools.lru_cache(maxsize=None)
def side_cases():
    """[dict(mesh, verts, p)]: N points of sign_exact's nine families, half on its sphere and half on the open soup."""
    out = []
    for m in ("sphere", "soup"):
        verts = SX.mesh(m)
        p = np.concatenate([SX.family(f, verts, 228) for f in SX.FAMILIES])
        out.append(dict(mesh=m, verts=verts, p=np.ascontiguousarray(p[np.round(np.linspace(0, len(p) - 1, N // 2)).astype(np.int64)], f32)))
    return out


@functools.lru_cache(maxsize=None)
def frame_scenes():
    """{name: dict(mesh, view[, kind, ior])}: the Cornell box and the 2 000-triangle soup, Lambert and with mirrors and glass."""
    from raytracing_engine_amd import scenes

    cv, ca, ce, kind, ior = scenes.cornell_surfaces_scene()
    soup = scenes.soup_scene(2000, seed=2)
    rng = np.random.default_rng(7)
    skind = rng.choice(np.array([scenes.SURFACE_LAMBERT, scenes.SURFACE_MIRROR, scenes.SURFACE_GLASS], np.uint32), len(soup[0]), p=[0.6, 0.2, 0.2]).astype(np.uint32)
    skind[(soup[2] > 0).any(1)] = scenes.SURFACE_LAMBERT
    sior = np.where(skind == scenes.SURFACE_GLASS, f32(1.5), f32(1)).astype(f32)
    cview = dict(pos=(0.0, 1.0, 0.0), sky=(0.0, 0.0, 0.0), ray_eps=1e-3, seed=3)
    sview = dict(pos=(0.0, 0.0, 0.0), sky=(0.2, 0.2, 0.25), ray_eps=1e-3, seed=5)
    return {
        "cornell": dict(mesh=scenes.cornell_tri_scene(), view=cview),
        "soup": dict(mesh=soup, view=sview),
        "cornell_surfaces": dict(mesh=(cv, ca, ce), view=cview, kind=kind, ior=ior),
        "soup_surfaces": dict(mesh=soup, view=sview, kind=skind, ior=sior),
    }


def scaled_view(view, k, **kw):
    """Keyword arguments of a render() (oracle, SurfRef or Renderer.render_pt) at scale k: pos and ray_eps are lengths."""
    q = scaled_problem(k, pos=np.asarray(view["pos"], f32), ray_eps=np.asarray(view["ray_eps"], f32), **kw)
    return dict(pos=tuple(float(x) for x in q["pos"]), ray_eps=float(q["ray_eps"]), sky=view["sky"], seed=view["seed"], spp=FRAME["spp"], bounces=FRAME["bounces"]), q["exact"]


def _meshes(family):
    if family in FRAME_FAMILIES:
        return [s["mesh"][0] for s in frame_scenes().values()]
    cases = ray_cases() if family in RAY_FAMILIES else side_cases() if family in SIDE_FAMILIES else point_cases()
    return [c["verts"] for c in cases]


def m0(family, largest=False):
    """The largest |coordinate| of the family's mesh with the smallest one at k = 0 (largest=True: with the largest one): the range's
    upper end k_hi has been seen on EVERY mesh of the family, so what it vouches for is the smallest M0 * 2^k_hi."""
    ms = [float(np.abs(v).max()) for v in _meshes(family)]
    return max(ms) if largest else min(ms)


def k_limit(family):
    """The largest k at which every mesh of the family is within the library's limit: max(1, M0 * 2^k) <= 2^COORD_LIMIT_LOG2."""
    return int(np.floor(COORD_LIMIT_LOG2 - np.log2(m0(family, largest=True))))


def feature0(family):
    """The smallest feature of the family's cases at k = 0: ray_eps for frames; else the shortest triangle edge that is not zero, and
    for the families on points the smallest distance of a point from the surface that is not zero."""
    if family in FRAME_FAMILIES:
        return min(float(s["view"]["ray_eps"]) for s in frame_scenes().values())
    f = np.inf
    for v in _meshes(family):
        t = np.asarray(v, np.float64).reshape(-1, 3, 3)
        e = np.concatenate([np.linalg.norm(t[:, (i + 1) % 3] - t[:, i], axis=1) for i in range(3)])
        f = min(f, float(e[e > 0].min()))
    if family in POINT_FAMILIES + SIDE_FAMILIES:
        d = answers("closest_point" if family in POINT_FAMILIES else "sides", 0)
        d = np.abs(d["dist*" if family in POINT_FAMILIES else "sdist*"].astype(np.float64))
        f = min(f, float(d[(d > 0) & np.isfinite(d)].min()))
    return f


def host_scales(family):
    """The scales at which tests/test_scale_host.py holds the references' answers to the float64 contracts: k = 0, +-1, +-12, both ends of
    the measured range and one step inside, and the GPU tests' scales."""
    lo, hi = RANGES[family]
    return sorted({0, 1, -1, 12, -12, lo, lo + 1, hi, hi - 1} | set(gpu_scales(family)))


def gpu_scales(family):
    """The scales of tests/test_gpu_scale.py: k = 0, +-1, +-12, the innermost edge on each side of the range that applies to the library
    - the measured one, cut at the coordinate limit - and one step inside it."""
    lo, hi = RANGES[family][0], min(RANGES[family][1], k_limit(family))
    return sorted({0, 1, -1, 12, -12, lo, lo + 1, hi, hi - 1})


# ---- the families: the references' answers at scale k, lengths marked with "*" ---------------------------------------------------
def _cat(rows):
    return {key: np.concatenate([r[key] for r in rows]) for key in rows[0]}


def _rays_at(k, check):
    out = []
    for c in ray_cases():
        q = scaled_problem(k, check=check, verts=c["verts"], o=c["o"], d=c["d"], seg=c["seg"], tmax=c["tmax"])
        q["mesh"] = c["mesh"]
        out.append(q)
    return out


def _points_at(k, check, cases=None, rmax="rmax"):
    out = []
    for c in cases or point_cases():
        q = scaled_problem(k, check=check, verts=c["verts"], p=c["p"], rmax=c.get(rmax))
        q["mesh"] = c["mesh"]
        out.append(q)
    return out


def closest_hit(k, check=True):
    """Closest hit without a limit (the oracle has none): oracle B's brute force."""
    import oracle as O

    rows = []
    for q in _rays_at(k, check):
        a, e = PX.surface(q["verts"])
        t, tri, _ = RX.oracle_answers(O.TriScene(q["verts"], a, e), q["o"], q["d"], None, False)
        rows.append({"tri": tri, "t*": t, "exact": np.array([q["exact"]])})
    return _cat(rows)


def hit_attr(k, check=True):
    """Closest hit under tmax with its barycentrics and normal: hit_attr_ref's brute force."""
    rows = []
    for q in _rays_at(k, check):
        r = AX.reference(q["verts"], q["o"], q["d"], q["tmax"])
        rows.append({"tri": r["tri"], "t*": r["t"], "ub": r["ub"], "vb": r["vb"], "normal": r["normal"], "exact": np.array([q["exact"]])})
    return _cat(rows)


def occlusion(k, check=True):
    import oracle as O

    rows = []
    for q in _rays_at(k, check):
        a, e = PX.surface(q["verts"])
        _, _, occ = RX.oracle_answers(O.TriScene(q["verts"], a, e), q["o"], q["d"], q["seg"], False)
        rows.append({"occluded": occ, "exact": np.array([q["exact"]])})
    return _cat(rows)


def all_hits(k, check=True):
    rows = []
    for q in _rays_at(k, check):
        r = HX.reference(q["verts"], q["o"], q["d"], q["tmax"])
        assert r["same"].all()  # tree independence at this scale too
        rows.append({"count": r["count"], "offsets": r["offsets"], "tri": r["tri"], "t*": r["t"], "exact": np.array([q["exact"]])})
    return _cat(rows)


def closest_point(k, check=True):
    """Closest point and its attributes: point_query_ref's brute force, the winners' normals from hit_attr_ref."""
    rows = []
    for q in _points_at(k, check, rmax="rmax_point"):
        b = PX.reference(q["verts"], q["p"], q["rmax"])["brute"]
        nrm = AX.reference(q["verts"], np.zeros((0, 3), f32), np.zeros((0, 3), f32), tris=b["tri"])["tri_normals"]
        rows.append({"tri": b["tri"], "dist*": b["dist"], "c*": b["c"], "u": b["u"], "v": b["v"], "normal": nrm, "exact": np.array([q["exact"]])})
    return _cat(rows)


def neighbors(k, check=True):
    rows = []
    for q in _points_at(k, check):
        r = NX.reference(q["verts"], q["p"], q["rmax"])
        rows.append({"count": r["count"], "offsets": r["offsets"], "tri": r["tri"], "dist*": r["dist"], "exact": np.array([q["exact"]])})
    return _cat(rows)


def sides(k, check=True):
    """Sides, crossings and the signed distance (point_query_ref's distance with side_query_ref's side)."""
    rows = []
    for q in _points_at(k, check, side_cases()):
        r = SX.reference(q["verts"], q["p"])
        dist = PX.reference(q["verts"], q["p"])["brute"]["dist"]
        sd = np.where(r["inside"] == 1, -dist, dist).astype(f32)
        rows.append({"inside": r["inside"], "crossings": r["brute"],"sdist*": sd, "exact": np.array([q["exact"]])})
    return _cat(rows)


def _frames(k, check, names):
    import oracle as O

    out, exact = {}, True
    for name in names:
        s = frame_scenes()[name]
        v, a, e = s["mesh"]
        vk = scaled_problem(k, check=check, verts=v)
        kw, ex = scaled_view(s["view"], k, check=check)
        exact = exact and ex and vk["exact"]
        if "kind" in s:
            from test_pt_surfaces_ref import SurfRef

            ref = SurfRef(vk["verts"], a, e, s["kind"], s["ior"])
        else:
            ref = O.TriScene(vk["verts"], a, e)
        out[name] = ref.render(FRAME["width"], FRAME["height"], **kw)[0]
    out["exact"] = np.array([exact])
    return out


def frames_lambert(k, check=True):
    return _frames(k, check, ("cornell", "soup"))


def frames_surfaces(k, check=True):
    return _frames(k, check, ("cornell_surfaces", "soup_surfaces"))


RAY_FAMILIES = ("closest_hit", "hit_attr", "occlusion", "all_hits")
POINT_FAMILIES = ("closest_point", "neighbors")
SIDE_FAMILIES = ("sides",)
FRAME_FAMILIES = ("frames_lambert", "frames_surfaces")
FAMILIES = {f.__name__: f for f in (closest_hit, hit_attr, occlusion, all_hits, closest_point, neighbors, sides, frames_lambert, frames_surfaces)}


@functools.lru_cache(maxsize=None)
def _answers(family, k):
    return FAMILIES[family](k, False)


def answers(family, k, check=True):
    """The family's answers at scale k, computed once; check: the scaling itself must have been exact (the "exact" entry)."""
    a = _answers(family, k)
    assert not check or a["exact"].all(), f"{family}: scaling by 2^{k} is not exact: a mantissa changed (not a power of two, or the number format ran out)"
    return a


def holds_at(family, k):
    """(every answer of the family at scale k is the transformed k = 0 answer, the names of those that are not)."""
    got = answers(family, k, False)
    bad = differing(got, transformed(answers(family, 0), k))
    return not bad and bool(got["exact"].all()), bad


# ---- the float64 contracts at scale k, constants unchanged (their units are relative to the largest coordinate) -------------------
def _split(ans, cases, key, listed=()):
    """The family's answers cut back into its cases (rows of cases[i][key] each; `listed` answers follow the lists' lengths)."""
    out, at, lat = [], 0, 0
    for c in cases:
        n = len(c[key])
        part = {name: x[at:at + n] for name, x in ans.items() if name not in listed and name not in ("exact", "offsets")}
        if listed:
            offsets = ans["offsets"][at + len(out):at + len(out) + n + 1]  # every case brought its own n + 1 offsets
            total = int(offsets[-1])
            part["offsets"] = offsets
            for name in listed:
                part[name] = ans[name][lat:lat + total]
            lat += total
        out.append(part)
        at += n
    return out


def contract_failures(family, k, ans=None):
    """How many answers `ans` (default: the references' own) of the family at scale k miss the family's float64 contract on the scaled
    problem: ray_exact's K and Kt, attr_exact's Kuv and Kn, point_exact's and neighbor_exact's Kp, sign_exact's rule; for all_hits
    (bit-for-bit against a definition: there is no tolerance to hold) the tree walk's list being the brute force's, which the
    evaluator asserts."""
    ans = answers(family, k) if ans is None else ans
    bad = 0
    if family in RAY_FAMILIES:
        qs = _rays_at(k, True)
        if family == "all_hits":
            return 0
        for q, a in zip(qs, _split(ans, qs, "o")):
            em = RX.ExactMesh(q["verts"])
            if family == "closest_hit":
                bad += int((~RX.Candidates(q["o"], q["d"], em).check_closest(a["tri"], a["t*"])).sum())
            elif family == "occlusion":
                bad += int((~RX.Candidates(q["o"], q["seg"], em).check_occluded(a["occluded"])).sum())
            else:
                bad += int((~AX.check_uv(em, q["o"], q["d"], a["tri"], a["ub"], a["vb"])).sum()) + int((~AX.check_normal(em, a["tri"], a["normal"])).sum())
    elif family == "closest_point":
        qs = _points_at(k, True, rmax="rmax_point")
        for q, a in zip(qs, _split(ans, qs, "p")):
            et = PX.ExactTris(q["verts"])
            bad += int((~PX.check(et, q["p"], a["tri"], a["dist*"], a["c*"], q["rmax"])).sum())
            # the attributes: the normal under attr_exact's Kn; (u, v) must name the closest point c - the float64 point
            # (1 - u - v) V0 + u V1 + v V2 of the record's triangle within Kp units of c, which is that point evaluated in fp32 with two
            # fmas per component (three roundings of at most one unit each per component: under 6 units in length)
            hit = a["tri"] >= 0
            tt = np.where(hit, a["tri"], 0)
            bad += int((~AX.check_normal(RX.ExactMesh(q["verts"]), a["tri"], a["normal"])).sum())
            u, v = a["u"].astype(np.float64)[:, None], a["v"].astype(np.float64)[:, None]
            P = (1.0 - u - v) * et.v[tt, 0] + u * et.v[tt, 1] + v * et.v[tt, 2]
            with np.errstate(invalid="ignore"):
                off = np.sqrt(((P - a["c*"].astype(np.float64)) ** 2).sum(1)) / PX.unit_of(q["p"], et)
            bad += int((hit & ~(off <= PX.KP)).sum())
    elif family == "neighbors":
        qs = _points_at(k, True)
        for q, a in zip(qs, _split(ans, qs, "p", listed=("tri", "dist*"))):
            bad += int((~NX.contract(PX.ExactTris(q["verts"]), q["p"], q["rmax"], a["count"], a["offsets"], a["dist*"], a["tri"])).sum())
    elif family == "sides":
        q = _points_at(k, True, side_cases())[0]  # the sphere: "inside" is defined on closed meshes
        n = len(q["p"])
        inside, _ = SX.exact_inside(q["verts"], q["p"])
        dist, unit = SX.surface_distance(q["verts"], q["p"])
        band = ~(dist > SX.KP * unit)
        two = (SX.rays_near_an_edge(q["verts"], q["p"]).sum(1) >= 2) & ~band
        bad += int(((ans["inside"][:n] != inside) & ~band & ~two).sum())
        bad += int((np.abs(np.abs(ans["sdist*"][:n].astype(np.float64)) - dist) > SX.KP * unit).sum())
    return bad


# ---- the measured ranges -------------------------------------------------------------------------------------------------------
# family: (k_lo, k_hi), inclusive; measure() below.  The first failures are at k_lo - 1 and k_hi + 1.
RANGES = {
    "closest_hit": (-33, 37),      # M0 = 5.3 (grid) .. 25.8 (soup); first to differ below: t; above: t, tri
    "hit_attr": (-28, 28),         # first to differ on both sides: the normal (its nn is a product of four lengths)
    "occlusion": (-38, 35),
    "all_hits": (-33, 37),
    "closest_point": (-17, 28),    # M0 = 2.4 (needle) .. 25.8; below: u of points a few 2^-28 off a triangle; above: everything
    "neighbors": (-20, 28),        # below: dist; above: dist, tri
    "sides": (-27, 28),           # M0 = 1.41 (sphere) .. 25.8; both sides: the signed distance; inside and the crossings hold further
    "frames_lambert": (-28, 27),   # M0 = 22 (Cornell) .. 25.2 (soup); below: the soup's frame; above: both
    "frames_surfaces": (-28, 27),
}
# Scales at which oracle B's Lambert frames had non-finite pixels before the light weight's denominator d2 * d2 was guarded against
# its underflow (the surfaces reference restates the same shade step); beyond +28 they still have, where the library refuses the mesh.
NONFINITE_BEFORE = {"frames_lambert": (-41, -40, -39, -38, -37), "frames_surfaces": (-41, -40, -39, -38, -37)}
K_SCAN = 75  # no range reaches it: fp32 has 254 binades, and the products of three or four lengths leave them long before


def invariant_range(family, limit=K_SCAN):
    lo = hi = 0
    while hi < limit and holds_at(family, hi + 1)[0]:
        hi += 1
    while lo > -limit and holds_at(family, lo - 1)[0]:
        lo -= 1
    return lo, hi


def frames_finite(family, k):
    return all(bool(np.isfinite(x).all()) for key, x in answers(family, k, False).items() if key != "exact")


def measure(families=None, out=sys.stdout):
    """Prints RANGES' entries (python tests/scale_exact.py [family ...]): every k outward from 0 until the first that fails."""
    for family in families or FAMILIES:
        lo, hi = invariant_range(family)
        print(f'    "{family}": ({lo}, {hi}),  # M0 = {m0(family):.4g}; first to differ below: {holds_at(family, lo - 1)[1]}, above: {holds_at(family, hi + 1)[1]}', file=out, flush=True)
        if family in FRAME_FAMILIES:
            bad = [k for k in range(-K_SCAN, K_SCAN + 1) if not frames_finite(family, k)]
            print(f"        non-finite pixels at k = {bad}", file=out, flush=True)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure(sys.argv[1:])
