"""Exact-geometry reference of path B's closest-point query, the accuracy contract it is held to, and the point families that probe it.

Test helper (imported by tests/test_point_query_host.py and tests/test_gpu_point_query.py); a sibling of tests/ray_exact.py, whose
meshes it uses; not a conftest, no fixtures.

THE REFERENCE.  ExactTris.dist() is the float64 distance from fp32 points to the fp32 triangles, on the vertices as the triangle
record forms them (v0, v0 + e1, v0 + e2 with the fp32 edges e = fp32(v - v0), summed in float64): the minimum of the distances
to the three edge segments and, where the foot of the perpendicular falls inside, to the plane.  float64 carries 2^-53 against
fp32's 2^-24, so on fp32 inputs it serves as exact.

THE CONTRACT for a constant Kp, per point: unit = 2^-24 * S, S = the largest |coordinate| among the point
and all vertices of the mesh; D(t) = the exact distance to triangle t, Dmin = the smallest D.  An answer (tri, dist, c) is right when
    D(tri) <= Dmin + Kp unit,    |dist - D(tri)| <= Kp unit,    exact distance from c to triangle tri <= Kp unit,
    | |p - c| - dist | <= Kp unit.
Under a limit rmax a hit is REQUIRED when Dmin < rmax - Kp unit and ALLOWED only when Dmin < rmax + Kp unit; in between either
answer is right.

THE CONSTANT.  measure() (python tests/point_exact.py [points per family]) finds the smallest Kp for which the NATIVE BRUTE-FORCE
REFERENCE (tests/native/point_query_ref.cpp: csrc/point_tri.h over all triangles, no tree, no GPU) satisfies the contract on every
family.  Largest value found with 20 000 points per family (seeds as below), and in brackets with 4 000:
    Kp_measured = 3.196 (family d; g 1.70, a 1.29, f 1.23, c 1.22, b 1.04, e 0.53)      [2.558, family d]
Constant = four times the measurement, rounded up to a power of two (the families sample the worst case, they do not bound it):
    Kp = 16
A wrong region, a dropped term or a culled box moves an answer by a whole triangle or to another one, thousands of units, so the
margin costs no power: test_point_query_host.py demonstrates it on float64 answers with one vertex moved by 64 Kp units and with the
nearest triangle withheld.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import ray_exact as RX  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
KP = 16.0
REACH = 32.0
f32 = np.float32


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
class ExactTris:
    """float64 triangles of a (n, 9) fp32 vertex array, as the triangle records hold them."""

    def __init__(self, verts):
        v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
        a = v[:, 0].astype(np.float64)
        self.v = np.stack([a, a + (v[:, 1] - v[:, 0]).astype(np.float64), a + (v[:, 2] - v[:, 0]).astype(np.float64)], 1)
        self.n_tris = len(v)
        self.maxabs = float(np.abs(v).max())

    def dist(self, p, tri):
        """Exact distance from p (..., 3) to triangles tri (...), broadcast against each other."""
        p = np.asarray(p, np.float64)
        A, B, C = self.v[tri, 0], self.v[tri, 1], self.v[tri, 2]
        d = np.minimum(np.minimum(_seg(p, A, B), _seg(p, A, C)), _seg(p, B, C))
        ab, ac, ap = B - A, C - A, p - A
        n = np.cross(ab, ac)
        nn = (n * n).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = (np.cross(ap, ac) * n).sum(-1) / nn
            w = (np.cross(ab, ap) * n).sum(-1) / nn
            face = np.abs((ap * n).sum(-1)) / np.sqrt(nn)
        inside = (nn > 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
        return np.where(inside, np.minimum(face, d), d)

    def all_dists(self, p, chunk=None):
        """(n_points, n_tris) exact distances."""
        p = np.ascontiguousarray(p, f32).reshape(-1, 3)
        chunk = chunk or max(1, 300000 // self.n_tris)
        tris = np.arange(self.n_tris)[None, :]
        return np.concatenate([self.dist(p[a:a + chunk, None, :], tris) for a in range(0, len(p), chunk)]) if len(p) else np.zeros((0, self.n_tris))


def _seg(p, a, b):
    ab = b - a
    ll = (ab * ab).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ll > 0, ((p - a) * ab).sum(-1) / ll, 0.0)
    t = np.clip(t, 0.0, 1.0)
    q = a + t[..., None] * ab
    return np.sqrt(((p - q) ** 2).sum(-1))


def unit_of(p, em):
    return U * np.maximum(np.abs(np.asarray(p, np.float64)).max(-1), em.maxabs)


def needs(em, p, tri, dist, c, D=None):
    """The Kp each hit answer needs (the largest of the contract's four terms, in units); D = em.all_dists(p) if at hand."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    D = em.all_dists(p) if D is None else D
    tri = np.asarray(tri)
    hit = tri >= 0
    t = np.where(hit, tri, 0)
    unit = unit_of(p, em)
    Dt = D[np.arange(len(p)), t]
    c64 = np.asarray(c, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        terms = np.stack([Dt - D.min(1), np.abs(np.asarray(dist, np.float64) - Dt), em.dist(c64, t),
                          np.abs(np.sqrt(((p.astype(np.float64) - c64) ** 2).sum(1)) - np.asarray(dist, np.float64))], 1) / unit[:, None]
    worst = np.where(np.isnan(terms), np.inf, terms).max(1)
    return np.where(hit, worst, 0.0)


def check(em, p, tri, dist, c, rmax=None, Kp=KP, D=None):
    """ok[i]: the answer (tri[i], dist[i], c[i]) (tri = -1: miss) for point i satisfies the contract."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    D = em.all_dists(p) if D is None else D
    tri = np.asarray(tri)
    unit = unit_of(p, em)
    r = np.full(len(p), np.inf) if rmax is None else np.asarray(rmax, np.float64)
    Dmin = D.min(1)
    required, allowed = Dmin < r - Kp * unit, Dmin < r + Kp * unit
    hit = tri >= 0
    return np.where(hit, allowed & (needs(em, p, tri, dist, c, D) <= Kp), ~required & (tri == -1))


def exact_answer(em, p, D=None, withhold_nearest=False):
    """The float64 answer (tri, dist, c): the nearest triangle (lowest index among equals), or the second nearest."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    D = (em.all_dists(p) if D is None else D).copy()
    if withhold_nearest:
        D[np.arange(len(p)), D.argmin(1)] = np.inf
    tri = D.argmin(1)
    return tri, D[np.arange(len(p)), tri], closest_point64(em, p, tri)


def closest_point64(em, p, tri):
    """float64 nearest point of triangle tri to p (the candidates of ExactTris.dist)."""
    p = np.asarray(p, np.float64)
    A, B, C = em.v[tri, 0], em.v[tri, 1], em.v[tri, 2]
    cands = []
    for a, b in ((A, B), (A, C), (B, C)):
        ab = b - a
        ll = (ab * ab).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.clip(np.where(ll > 0, ((p - a) * ab).sum(-1) / ll, 0.0), 0.0, 1.0)
        cands.append(a + t[..., None] * ab)
    ab, ac, ap = B - A, C - A, p - A
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (np.cross(ap, ac) * n).sum(-1) / nn
        w = (np.cross(ab, ap) * n).sum(-1) / nn
    inside = (nn > 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
    foot = A + np.where(inside, u, 0.0)[..., None] * ab + np.where(inside, w, 0.0)[..., None] * ac
    cands.append(np.where(inside[..., None], foot, cands[0]))
    d = np.stack([((p - q) ** 2).sum(-1) for q in cands], 0)
    k = d.argmin(0)
    return np.take_along_axis(np.stack(cands, 0), k[None, ..., None], 0)[0]


# ---- the native reference ------------------------------------------------------------------------------------------------------


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/point_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("point_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, p, rmax=None, pairs=None, sanitized=False):
    """The native reference on mesh `verts` and points p.  Returns dict(brute=..., walk=..., nodes, tris[, pair_d2]); brute and
    walk are dicts of tri (int32), d2, u, v, dist (float32) and c (n, 3)."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    inputs = dict(mesh=np.asarray(verts, f32), points=p, out=NR.OUT, rmax=None if rmax is None else np.asarray(rmax, f32))
    if pairs is not None:
        inputs["pairs"] = np.asarray(pairs, np.int32)
    column = (("tri", np.int32, n), ("d2", f32, n), ("u", f32, n), ("v", f32, n), ("dist", f32, n), ("c", f32, 3 * n))
    fields = [(f"{name}.{key}", dt, count) for name in ("brute", "walk") for key, dt, count in column]
    head, flat = NR.unpack(NR.run(build_reference(sanitized), inputs), 3, fields + [("pair_d2", f32, 0 if pairs is None else inputs["pairs"].size // 2)])
    assert head[0] == n
    out = dict(nodes=head[1], tris=head[2], brute={}, walk={})
    for name in ("brute", "walk"):
        out[name] = {key: flat[f"{name}.{key}"] for key, _, _ in column}
        out[name]["c"] = out[name]["c"].reshape(n, 3)
    if pairs is not None:
        out["pair_d2"] = flat["pair_d2"]
    return out


# ---- meshes --------------------------------------------------------------------------------------------------------------------
_MESHES = {}


def needle_mesh():
    """(g) 12 triangles: a needle of aspect 1e6, three collinear vertices, three equal vertices, and nine ordinary ones about them."""
    rng = np.random.default_rng(77)
    v = (rng.uniform(-2, 2, (12, 1, 3)) + rng.uniform(-0.7, 0.7, (12, 3, 3))).astype(f32)
    v[3] = [[0.25, 0.5, -0.125], [1.25, 0.75, 0.375], [0.25 + 1e-6 * 0.3, 0.5 - 1e-6 * 0.9, -0.125 + 1e-6 * 0.2]]  # needle: length ~1.1, width ~1e-6
    v[6] = [[-1.0, 0.25, 0.5], [-0.5, 0.5, 0.75], [0.5, 1.0, 1.25]]  # collinear: v0 + t (2, 1, 1) / 4
    v[9] = [[0.75, -1.5, 0.3]] * 3  # a point
    return np.ascontiguousarray(v.reshape(-1, 9), f32)


def mesh(name):
    """Vertices (n, 9) by name: ray_exact's meshes, `soup_dup` (the soup with every triangle twice) and `needle`."""
    if name not in _MESHES:
        if name == "soup_dup":
            v = RX.mesh("soup")[0]
            _MESHES[name] = np.ascontiguousarray(np.concatenate([v, v]), f32)
        elif name == "needle":
            _MESHES[name] = needle_mesh()
        else:
            _MESHES[name] = RX.mesh(name)[0]
    return _MESHES[name]


def surface(verts):
    """(albedo, emission) for rt_set_mesh: grey, the last triangle a light."""
    a = np.full((len(verts), 3), 0.5, f32)
    e = np.zeros((len(verts), 3), f32)
    e[-1] = 1.0
    return a, e


# ---- point families ------------------------------------------------------------------------------------------------------------
FAMILIES = ("a", "b", "c", "d", "e", "f", "g")
_SEED = {k: 300 + i for i, k in enumerate(FAMILIES)}
ALL_MESHES = ("soup", "soup_small", "soup_far", "terrain", "grid")


def _split(n, k):
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def _in_box(rng, verts, n, inflate=0.5):
    v = verts.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * (1 + inflate)
    return rng.uniform(mid - half, mid + half, (n, 3)).astype(f32)


def reach_of(verts):
    """The reach as the library holds it: fp32(32 * max(1, M))."""
    return f32(REACH) * max(f32(1.0), f32(np.abs(np.asarray(verts, f32)).max()))


def _far(rng, verts, n):
    """Points at 2 .. 32 M from the origin of the coordinates (largest |component|), the last sixth exactly at the reach."""
    R = float(reach_of(verts))
    r = R / 32.0 * np.exp(rng.uniform(np.log(2.0), np.log(32.0), (n, 1)))
    o = rng.uniform(-1, 1, (n, 3))
    o = (o / np.abs(o).max(1, keepdims=True) * r * (1 - 2.0 ** -20)).astype(f32)
    k = max(1, n // 6)
    edge = rng.uniform(-1, 1, (k, 3))
    edge = (edge / np.abs(edge).max(1, keepdims=True) * R).astype(f32)  # the largest component is +-R exactly
    o[n - k:] = edge
    return np.clip(o, -f32(R), f32(R))


def _normals(verts, tri):
    v = verts.reshape(-1, 3, 3).astype(np.float64)[tri]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), [0.0, 1.0, 0.0])


def _grid_ties(rng, n):
    """(e) points straight above (and below) vertices and edge midpoints of the flat grid at heights that are binary fractions: the
    triangles round the vertex, or the two along the edge, are at the same exact distance."""
    v = mesh("grid").reshape(-1, 3, 3)
    tri = rng.integers(0, len(v), n)
    k = rng.integers(0, 3, n)
    a, b = v[tri, k], v[tri, (k + 1) % 3]
    mid = ((a.astype(np.float64) + b.astype(np.float64)) / 2).astype(f32)
    p = np.where((rng.random(n) < 0.5)[:, None], a, mid).copy()
    h = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-6, 3, n)
    p[:, 1] = (f32(5.3) + h.astype(f32)).astype(f32)
    return p.astype(f32)


def family(name, n=4000, moved=None):
    """The parts of one family: a list of dict(mesh=name, verts, p).  moved: a function verts -> verts applied to every mesh first
    (the refit tests ask on moved vertices; points at the reach follow the moved mesh's range)."""
    rng = np.random.default_rng(_SEED[name])

    def part(m, make):
        verts = mesh(m) if moved is None else moved(mesh(m))
        return dict(mesh=m, verts=verts, p=np.ascontiguousarray(make(verts), f32))

    if name == "a":
        return [part(m, lambda v, k=k: _in_box(rng, v, k)) for m, k in zip(ALL_MESHES, _split(n, 5))]
    if name == "b":
        return [part(m, lambda v, k=k: RX._targets(rng, v, k, "iev")[0]) for m, k in zip(("terrain", "grid"), _split(n, 2))]
    if name == "c":
        def offset(v, k):
            p, tri = RX._targets(rng, v, k, "i")
            h = rng.choice([-1.0, 1.0], k) * np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), k))
            return p.astype(np.float64) + _normals(v, tri) * h[:, None]
        return [part(m, lambda v, k=k: offset(v, k)) for m, k in zip(("soup", "terrain", "grid"), _split(n, 3))]
    if name == "d":
        return [part(m, lambda v, k=k: _far(rng, v, k)) for m, k in zip(ALL_MESHES, _split(n, 5))]
    if name == "e":
        return [part("grid", lambda v: _grid_ties(rng, n))]
    if name == "f":
        def both(v, k):
            return np.concatenate([_in_box(rng, v, k - k // 2), RX._targets(rng, v, k // 2, "iev")[0]])
        return [part("soup_dup", lambda v: both(v, n))]
    if name == "g":
        def around(v, k):
            p, _ = RX._targets(rng, v, k, "iiev")
            x = rng.normal(size=(k, 3))
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            r = np.where(rng.random(k) < 0.15, 0.0, np.exp(rng.uniform(np.log(1e-7), np.log(3.0), k)))
            return p.astype(np.float64) + x * r[:, None]
        return [part("needle", lambda v: around(v, n))]
    raise KeyError(name)


# ---- measuring the constant ----------------------------------------------------------------------------------------------------
def measure(n=20000, out=sys.stdout):
    """Smallest Kp for which the native brute-force reference satisfies the contract, family by family."""
    worst = (0.0, None)
    for name in FAMILIES:
        k_f = 0.0
        for part in family(name, n):
            em = ExactTris(part["verts"])
            ref = reference(part["verts"], part["p"])["brute"]
            valid = ref["tri"] >= 0
            assert valid.all(), (name, part["mesh"], int((~valid).sum()))
            k_f = max(k_f, float(needs(em, part["p"], ref["tri"], ref["dist"], ref["c"]).max()))
        print(f"family {name}: Kp needed {k_f:8.3f}", file=out, flush=True)
        if k_f > worst[0]:
            worst = (k_f, name)
    print(f"Kp_measured = {worst[0]:.3f} (family {worst[1]}) -> Kp = {RX.pow2_margin(worst[0]):g}", file=out)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
