"""Exact-geometry reference of path B's clearance query, the accuracy contract it is held to, and the query
triangles that probe it.

Test helper (imported by tests/test_clearance_query_host.py and tests/test_gpu_clearance_query.py); a sibling of tests/point_exact.py and
tests/overlap_exact.py, whose meshes and generators it uses; not a conftest, no fixtures.

THE REFERENCE.  tri_tri_dist() is the float64 distance between two triangles given by their vertices as the fp32 definition forms
them (P0, P0 + G1, P0 + G2 with the fp32 edges, summed in float64): 0 where an edge of one passes through the other (a closed
float64 segment / triangle test), else the minimum of the six vertex - triangle and the nine segment - segment distances.  It shares
no code with csrc/tri_dist.h.  exact_dists() evaluates it for every pair that a float64 box bound cannot exclude from the two nearest
of its query; the other entries of the matrix are +inf.

THE CONTRACT for a constant Kc, per query triangle: unit = 2^-24 * S, S = the largest |coordinate| among the query triangle and all
vertices of the mesh; D(t) = the exact distance to mesh triangle t, Dmin = the smallest D.  An answer (tri, dist, pq, pm) is right when
    D(tri) <= Dmin + Kc unit,    |dist - D(tri)| <= Kc unit,    exact distance from pq to the query triangle <= Kc unit,
    exact distance from pm to triangle tri <= Kc unit,    | |pq - pm| - dist | <= Kc unit.
Under a limit rmax a hit is REQUIRED when Dmin < rmax - Kc unit and ALLOWED only when Dmin < rmax + Kc unit.

THE CONSTANT.  measure() (python tests/clearance_exact.py) finds the smallest Kc for which the NATIVE BRUTE-FORCE REFERENCE
(tests/native/clearance_query_ref.cpp: csrc/tri_dist.h over all triangles, no tree, no GPU) satisfies the contract on every family:
    Kc_measured = 2.572 (family d on soup_far; c 1.44, g 1.39, a 1.32, f 1.05, b 0.62, e 0.00)
Constant = four times the measurement, rounded up to a power of two (the families sample the worst case, they do not bound it):
    Kc = 16

THE QUERY FAMILIES (fixed seeds; a part has at most 2 000 mesh triangles and 600 query triangles):
  a  the mesh's own triangles displaced by 0.05, 1 and 5 of their size in a random direction
  b  the mesh's own triangles unmoved: every d2 is 0, the lowest index among the zero-distance triangles wins
  c  overlap_exact._planted: an edge of the query pierces a mesh triangle well inside; a pierce candidate wins, the points are the pierce point
  d  far away, up to and exactly at the reach, soup_far included
  e  exact ties: grid triangles lifted off the flat grid by binary fractions, parallel to it
  f  the first 1 000 triangles of the soup, every one twice: the first copy wins
  g  the needle / collinear / point mesh, and query triangles that are themselves a needle, a segment and a point
  h  non-finite coordinates, coordinates beyond the reach and exactly at it, NaN rmax
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import overlap_exact as OX  # noqa: E402
import point_exact as PX  # noqa: E402

RX = PX.RX
ROOT = PX.ROOT
U = 2.0 ** -24
KC_MEASURED = 2.572
KC = 16.0
f32 = np.float32
MISS, INVALID = -1, -2
FAMILIES = ("a", "b", "c", "d", "e", "f", "g")  # the answered ones; h is the invalid queries
_SEED = {k: 700 + i for i, k in enumerate(FAMILIES + ("h",))}
ALL_MESHES = ("soup", "soup_small", "soup_far", "terrain", "grid", "needle")
COLUMNS = (("tri", np.int32, 1), ("d2", f32, 1), ("uq", f32, 1), ("vq", f32, 1), ("um", f32, 1), ("vm", f32, 1), ("dist", f32, 1), ("cand", np.int32, 1),
           ("pq", f32, 3), ("pm", f32, 3))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def tri_verts64(verts):
    """(n, 3, 3) float64 vertices of (n, 9) fp32 triangles as the fp32 definition forms them: P0, P0 + fp32(P1 - P0), P0 + fp32(P2 - P0)."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
    a = v[:, 0].astype(np.float64)
    return np.stack([a, a + (v[:, 1] - v[:, 0]).astype(np.float64), a + (v[:, 2] - v[:, 0]).astype(np.float64)], 1)


def _dot(a, b):
    return (a * b).sum(-1)


def _point_seg(p, a, b):
    ab = b - a
    ll = _dot(ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.clip(np.where(ll > 0, _dot(p - a, ab) / np.where(ll > 0, ll, 1.0), 0.0), 0.0, 1.0)
    return np.sqrt(((p - (a + t[..., None] * ab)) ** 2).sum(-1))


def point_tri_dist(p, T):
    """Exact distance from points p (..., 3) to triangles T (..., 3, 3)."""
    A, B, C = T[..., 0, :], T[..., 1, :], T[..., 2, :]
    d = np.minimum(np.minimum(_point_seg(p, A, B), _point_seg(p, A, C)), _point_seg(p, B, C))
    ab, ac, ap = B - A, C - A, p - A
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    safe = np.where(nn > 0, nn, 1.0)
    u = _dot(np.cross(ap, ac), n) / safe
    w = _dot(np.cross(ab, ap), n) / safe
    face = np.abs(_dot(ap, n)) / np.sqrt(safe)
    inside = (nn > 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
    return np.where(inside, np.minimum(face, d), d)


def _seg_seg(p1, q1, p2, q2):
    """Exact distance between the segments p1 q1 and p2 q2: the interior critical point where the lines are not parallel and it lies in
    both segments, else an endpoint against the other segment."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > 1e-30 * a * e
    safe = np.where(ok, den, 1.0)
    s = (b * f - c * e) / safe
    t = (a * f - b * c) / safe
    inner = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    di = np.sqrt((((p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)) ** 2).sum(-1))
    ends = np.minimum(np.minimum(_point_seg(p1, p2, q2), _point_seg(q1, p2, q2)), np.minimum(_point_seg(p2, p1, q1), _point_seg(q2, p1, q1)))
    return np.where(inner, np.minimum(di, ends), ends)


def _seg_hits_tri(o, q, T):
    """The closed segment o q meets the closed triangle T, where it is not parallel to its plane (float64 Moller-Trumbore)."""
    d = q - o
    g1, g2 = T[..., 1, :] - T[..., 0, :], T[..., 2, :] - T[..., 0, :]
    pvec = np.cross(d, g2)
    det = _dot(g1, pvec)
    safe = np.where(det != 0, det, 1.0)
    tvec = o - T[..., 0, :]
    qvec = np.cross(tvec, g1)
    u, v, t = _dot(tvec, pvec) / safe, _dot(d, qvec) / safe, _dot(g2, qvec) / safe
    return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def tri_tri_dist(A, B):
    """Exact distance between triangles A and B (..., 3, 3), broadcast against each other; 0 where they intersect."""
    A, B = np.broadcast_arrays(A, B)
    d = None
    hit = np.zeros(A.shape[:-2], bool)
    for k in range(3):
        for x in (point_tri_dist(A[..., k, :], B), point_tri_dist(B[..., k, :], A)):
            d = x if d is None else np.minimum(d, x)
        hit |= _seg_hits_tri(A[..., k, :], A[..., (k + 1) % 3, :], B) | _seg_hits_tri(B[..., k, :], B[..., (k + 1) % 3, :], A)
        for j in range(3):
            d = np.minimum(d, _seg_seg(A[..., k, :], A[..., (k + 1) % 3, :], B[..., j, :], B[..., (j + 1) % 3, :]))
    return np.where(hit, 0.0, d)


def closest_pair64(A, B):
    """(d, pa, pb): the exact distance of tri_tri_dist and a pair of points of A and B at that distance, for a batch of pairs
    (n, 3, 3): where an edge passes through the other triangle, the pierce point twice."""
    cands = []

    def seg_point(p, a, b):
        ab = b - a
        ll = _dot(ab, ab)
        t = np.clip(np.where(ll > 0, _dot(p - a, ab) / np.where(ll > 0, ll, 1.0), 0.0), 0.0, 1.0)
        return a + t[..., None] * ab

    def tri_point(p, T):
        A0, B0, C0 = T[:, 0], T[:, 1], T[:, 2]
        pts = [seg_point(p, A0, B0), seg_point(p, A0, C0), seg_point(p, B0, C0)]
        ab, ac, ap = B0 - A0, C0 - A0, p - A0
        n = np.cross(ab, ac)
        nn = _dot(n, n)
        safe = np.where(nn > 0, nn, 1.0)
        u, w = _dot(np.cross(ap, ac), n) / safe, _dot(np.cross(ab, ap), n) / safe
        inside = (nn > 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
        pts.append(np.where(inside[:, None], A0 + u[:, None] * ab + w[:, None] * ac, pts[0]))
        d = np.stack([((p - x) ** 2).sum(-1) for x in pts])
        return np.take_along_axis(np.stack(pts), d.argmin(0)[None, :, None], 0)[0]

    for k in range(3):
        cands.append((A[:, k], tri_point(A[:, k], B)))
        cands.append((tri_point(B[:, k], A), B[:, k]))
        for j in range(3):
            p1, q1, p2, q2 = A[:, k], A[:, (k + 1) % 3], B[:, j], B[:, (j + 1) % 3]
            d1, d2, r = q1 - p1, q2 - p2, p1 - p2
            a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
            den = a * e - b * b
            ok = den > 1e-30 * a * e
            safe = np.where(ok, den, 1.0)
            s, t = (b * f - c * e) / safe, (a * f - b * c) / safe
            inner = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
            x = np.where(inner[:, None], p1 + s[:, None] * d1, p1)
            cands.append((x, seg_point(x, p2, q2)))
    for X, Y, swap in ((A, B, False), (B, A, True)):
        for k in range(3):
            o, q = X[:, k], X[:, (k + 1) % 3]
            hit = _seg_hits_tri(o, q, Y)
            d = q - o
            g1, g2 = Y[:, 1] - Y[:, 0], Y[:, 2] - Y[:, 0]
            det = _dot(g1, np.cross(d, g2))
            t = _dot(g2, np.cross(o - Y[:, 0], g1)) / np.where(det != 0, det, 1.0)
            x = np.where(hit[:, None], o + t[:, None] * d, o)
            y = np.where(hit[:, None], x, tri_point(o, Y))
            cands.append((y, x) if swap else (x, y))
    d = np.stack([np.sqrt(((x - y) ** 2).sum(-1)) for x, y in cands])
    k = d.argmin(0)[None, :, None]
    return d.min(0), np.take_along_axis(np.stack([x for x, _ in cands]), k, 0)[0], np.take_along_axis(np.stack([y for _, y in cands]), k, 0)[0]


class Exact:
    """The float64 side of one part: the mesh's and the queries' vertices and the matrix D of exact_dists()."""

    def __init__(self, verts, q):
        self.T = tri_verts64(verts)
        self.A = tri_verts64(np.where(np.isfinite(q), q, 0).astype(f32))
        self.maxabs = float(np.abs(np.asarray(verts, f32)).max())
        self.unit = U * np.maximum(np.abs(self.A).max((1, 2)), self.maxabs)
        self.D = exact_dists(self.A, self.T)

    def pair(self, i, t):
        return tri_tri_dist(self.A[i], self.T[t])


def exact_dists(A, T, chunk=200000):
    """(n_queries, n_tris) exact distances; +inf where a box bound shows that the triangle is not among the two nearest of its query
    (the distance between the boxes exceeds the second smallest of an upper bound: first vertex to first vertex)."""
    lo_a, hi_a, lo_t, hi_t = A.min(1), A.max(1), T.min(1), T.max(1)
    gap = np.maximum(np.maximum(lo_t[None] - hi_a[:, None], lo_a[:, None] - hi_t[None]), 0.0)
    lb = np.sqrt((gap * gap).sum(-1))
    ub = np.sqrt(((A[:, None, 0] - T[None, :, 0]) ** 2).sum(-1))
    second = np.sort(ub, 1)[:, min(1, ub.shape[1] - 1)]
    i, t = np.nonzero(lb <= second[:, None])
    D = np.full(lb.shape, np.inf)
    for at in range(0, len(i), chunk):
        D[i[at:at + chunk], t[at:at + chunk]] = tri_tri_dist(A[i[at:at + chunk]], T[t[at:at + chunk]])
    return D


def needs(ex, tri, dist, pq, pm):
    """The Kc each hit answer needs (the largest of the contract's five terms, in units)."""
    tri = np.asarray(tri)
    hit = tri >= 0
    t = np.where(hit, tri, 0)
    idx = np.arange(len(tri))
    Dt = ex.pair(idx, t)
    dist = np.asarray(dist, np.float64)
    pq, pm = np.asarray(pq, np.float64).reshape(-1, 3), np.asarray(pm, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        terms = np.stack([Dt - ex.D.min(1), np.abs(dist - Dt), point_tri_dist(pq, ex.A), point_tri_dist(pm, ex.T[t]),
                          np.abs(np.sqrt(((pq - pm) ** 2).sum(1)) - dist)], 1) / ex.unit[:, None]
    worst = np.where(np.isnan(terms), np.inf, terms).max(1)
    return np.where(hit, worst, 0.0)


def check(ex, tri, dist, pq, pm, rmax=None, Kc=KC):
    """ok[i]: the answer (tri[i], dist[i], pq[i], pm[i]) (tri = -1: a miss) of query i satisfies the contract."""
    tri = np.asarray(tri)
    r = np.full(len(tri), np.inf) if rmax is None else np.asarray(rmax, np.float64)
    Dmin = ex.D.min(1)
    required, allowed = Dmin < r - Kc * ex.unit, Dmin < r + Kc * ex.unit
    hit = tri >= 0
    return np.where(hit, allowed & (needs(ex, tri, dist, pq, pm) <= Kc), ~required & (tri == MISS))


def exact_answer(ex, withhold_nearest=False):
    """The float64 answer (tri, dist): the nearest triangle (lowest index among equals), or the second nearest."""
    D = ex.D.copy()
    if withhold_nearest:
        D[np.arange(len(D)), D.argmin(1)] = np.inf
    tri = D.argmin(1)
    return tri, D[np.arange(len(D)), tri]


# ---- the native reference ------------------------------------------------------------------------------------------------------


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/clearance_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("clearance_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, q, rmax=None, pairs=None, sanitized=False, nopad=False):
    """The native reference on mesh `verts` and query triangles q (n, 9).  Returns dict(brute=..., walk=..., nodes, tris (uint32 per
    query), nodes_total, tris_total[, pair_d2]); brute and walk are dicts of tri, cand (int32: the winning candidate of tri_dist, 0 .. 5 a pierce), d2, uq, vq, um, vm, dist (float32), pq
    and pm (n, 3)."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 9)
    n = len(q)
    inputs = dict(mesh=np.asarray(verts, f32), queries=q, out=NR.OUT, rmax=None if rmax is None else np.asarray(rmax, f32),
                  pairs=None if pairs is None else np.asarray(pairs, np.int32))
    if nopad:
        inputs["mode"] = "nopad"
    fields = [("nodes", np.uint32, n), ("tris", np.uint32, n)] + [(f"{name}.{key}", dt, n * width) for name in ("brute", "walk") for key, dt, width in COLUMNS]
    head, flat = NR.unpack(NR.run(build_reference(sanitized), inputs), 3, fields + [("pair_d2", f32, 0 if pairs is None else inputs["pairs"].size // 2)])
    assert head[0] == n
    out = dict(nodes_total=head[1], tris_total=head[2], nodes=flat["nodes"], tris=flat["tris"])
    for name in ("brute", "walk"):
        out[name] = {key: flat[f"{name}.{key}"] for key, _, _ in COLUMNS}
        out[name]["pq"], out[name]["pm"] = out[name]["pq"].reshape(n, 3), out[name]["pm"].reshape(n, 3)
    if pairs is not None:
        out["pair_d2"] = flat["pair_d2"]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    return a.dtype == b.dtype and a.shape == b.shape and a.view(np.uint32).tolist() == b.view(np.uint32).tolist()


def walk_is_brute(ref):
    """The tree walk's answers are the brute force's, bit for bit in every column."""
    return all(same_bits(ref["brute"][key], ref["walk"][key]) for key, _, _ in COLUMNS)


# ---- the query families --------------------------------------------------------------------------------------------------------
def _far(rng, verts, n):
    """Small triangles at 2 .. 32 M from the origin of the coordinates, the last sixth with a coordinate exactly at the reach: the first
    vertex is point_exact._far's, the other two lie inward of it."""
    p = PX._far(rng, verts, n).astype(np.float64)
    size = float(np.median(OX._size(verts.reshape(-1, 3, 3))))
    inward = -np.sign(p)[:, None] * rng.uniform(0.1, 1.0, (n, 2, 3)) * size
    return np.concatenate([p[:, None], p[:, None] + np.where(inward == 0, size, inward)], 1).astype(f32).reshape(-1, 9)


def _lifted(rng, verts, n):
    """(e) grid triangles lifted off the grid's plane by +-2^k, k = -6 .. 2: parallel to it, the triangle below (or above) and its
    neighbours along the edges and round the vertices at the same exact distance."""
    v = verts.reshape(-1, 3, 3)
    t = v[rng.integers(0, len(v), n)].copy()
    h = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-6, 3, n)
    t[:, :, 1] = (t[:, :, 1] + h.astype(f32)[:, None]).astype(f32)
    return t.reshape(-1, 9)


def _degenerate(rng, verts, n):
    """(g) needles, segments and points about the mesh: a mesh triangle displaced, then squeezed."""
    q = np.concatenate([OX._displaced(rng, verts, n - n // 2, 0.3), OX._displaced(rng, verts, n // 2, 2.0)]).reshape(-1, 3, 3).astype(np.float64)
    kind = np.arange(len(q)) % 4
    k = kind == 0  # a needle: the third vertex 1e-6 of an edge beside the first
    q[k, 2] = q[k, 0] + (q[k, 2] - q[k, 0]) * 1e-6
    k = kind == 1  # a segment: two equal vertices
    q[k, 2] = q[k, 1]
    k = kind == 2  # a point
    q[k, 1] = q[k, 0]
    q[k, 2] = q[k, 0]
    k = kind == 3  # three collinear vertices
    q[k, 2] = q[k, 0] + (q[k, 1] - q[k, 0]) * 0.25
    return q.astype(f32).reshape(-1, 9)


def _invalid(rng, verts):
    """(h) (queries, rmax, valid): non-finite coordinates, coordinates beyond the reach and exactly at it, NaN rmax."""
    reach = PX.reach_of(verts)
    base = OX._displaced(rng, verts, 40, 1.0)
    q, rmax, valid = [], [], []

    def add(t, r, ok):
        q.append(np.asarray(t, f32).reshape(9))
        rmax.append(r)
        valid.append(ok)

    for n, t in enumerate(base[:27]):
        t = t.copy()
        t[n % 9] = (np.nan, np.inf, -np.inf)[n // 9]
        add(t, np.inf, False)
    for n, (k, sign) in enumerate(((1, 1.0), (3, -1.0), (8, 1.0))):
        t = base[27 + n].copy()
        t[k] = sign * np.nextafter(reach, f32(np.inf))
        add(t, np.inf, False)
        t = t.copy()
        t[k] = sign * reach  # exactly at the reach: valid
        add(t, np.inf, True)
    for t in base[30:34]:
        add(t, np.nan, False)
    for t in base[34:]:
        add(t, np.inf, True)
    return np.asarray(q, f32), np.asarray(rmax, f32), np.asarray(valid)


def family(name, moved=False):
    """The parts of one family: a list of dict(mesh, verts, q[, rmax, valid]).  moved: on ray_exact.moved() vertices (the refit tests)."""
    rng = np.random.default_rng(_SEED[name])

    def verts_of(m):
        v = np.ascontiguousarray(np.concatenate([PX.mesh("soup")[:1000]] * 2)) if m == "soup_dup" else PX.mesh(m)  # (2 000 triangles a part)
        return RX.moved(v) if moved else v

    def part(m, make):
        v = verts_of(m)
        return dict(mesh=m, verts=v, q=np.ascontiguousarray(make(v), f32))

    if name == "a":
        return [part(m, lambda v: np.concatenate([OX._displaced(rng, v, 50, s) for s in (0.05, 1.0, 5.0)])) for m in ALL_MESHES]
    if name == "b":
        return [part(m, lambda v: OX._own(rng, v, 120)) for m in ALL_MESHES]
    if name == "c":
        return [part(m, lambda v: OX._planted(rng, v, 100)) for m in ("soup", "soup_far", "terrain", "grid")]
    if name == "d":
        return [part(m, lambda v: _far(rng, v, 36)) for m in ("soup", "soup_small", "soup_far", "terrain", "grid")]
    if name == "e":
        return [part("grid", lambda v: _lifted(rng, v, 150))]
    if name == "f":
        return [part("soup_dup", lambda v: np.concatenate([OX._displaced(rng, v, 60, 0.05), OX._displaced(rng, v, 60, 1.0)]))]
    if name == "g":
        return [part("needle", lambda v: np.concatenate([OX._displaced(rng, v, 60, 0.3), _degenerate(rng, v, 60)])), part("soup", lambda v: _degenerate(rng, v, 80))]
    if name == "h":
        out = []
        for m in ("soup", "soup_far"):
            v = verts_of(m)
            q, rmax, valid = _invalid(rng, v)
            out.append(dict(mesh=m, verts=v, q=q, rmax=rmax, valid=valid))
        return out
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def family_case(name, moved=False):
    """family(name) with each part's native reference: dict(mesh, verts, q, ref[, rmax, valid]).  Computed once, left unchanged."""
    out = []
    for part in family(name, moved):
        assert len(part["q"]) <= 600 and len(part["verts"]) <= 2000
        out.append(dict(part, ref=reference(part["verts"], part["q"], part.get("rmax"))))
    return out


@functools.lru_cache(maxsize=None)
def family_exact(name):
    """The float64 side of each part of family_case(name)."""
    return [Exact(c["verts"], c["q"]) for c in family_case(name)]


# ---- measuring the constant ----------------------------------------------------------------------------------------------------
def measure(out=sys.stdout):
    """Smallest Kc for which the native brute-force reference satisfies the contract, family by family."""
    worst = (0.0, None)
    for name in FAMILIES:
        k_f = 0.0
        for c, ex in zip(family_case(name), family_exact(name)):
            a = c["ref"]["brute"]
            assert (a["tri"] >= 0).all(), (name, c["mesh"])
            k_p = float(needs(ex, a["tri"], a["dist"], a["pq"], a["pm"]).max())
            print(f"family {name} {c['mesh']:10s}: Kc needed {k_p:8.3f}   ({int(((a['cand'] >= 0) & (a['cand'] < 6)).sum())} pierced of {len(a['tri'])}; {c['ref']['tris_total'] / len(a['tri']):.1f} records, "
                  f"{c['ref']['nodes_total'] / len(a['tri']):.1f} nodes per query)", file=out, flush=True)
            k_f = max(k_f, k_p)
        if k_f > worst[0]:
            worst = (k_f, name)
    print(f"Kc_measured = {worst[0]:.3f} (family {worst[1]}) -> Kc = {RX.pow2_margin(worst[0]):g}", file=out)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure()
