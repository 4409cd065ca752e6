"""Exact-geometry contract of path B's sphere-cast query, the native reference it is measured on, and the
item families that probe it.

Test helper (imported by tests/test_sweep_query_host.py and tests/test_gpu_sweep_query.py); a sibling of tests/point_exact.py and
tests/clearance_exact.py, whose meshes, exact distances and generators it uses; not a conftest, no fixtures.

THE CONTRACT needs no second time-of-impact formula, only exact distances: D_T(x) = point_exact.ExactTris.dist, the float64
distance from x to triangle T, and clearance_exact.tri_tri_dist with a path segment as a triangle without area.  Per item (o, d, r,
tmax), all in float64 on the fp32 inputs: c = o + t d;  unit = 2^-24 S, S = the largest |coordinate| among o, c (or the far end of
the path), every vertex of the mesh, and r.  For a constant K:
    a hit (t, tri) with t > 0 is right when   D_tri(c) <= r + K unit            the sphere has reached the triangle,
                                              m(o, c) >= r - K unit            nothing was penetrated on the way: m(a, b) is the
                                                                               exact distance from the segment a b to the mesh,
                                              t < tmax;
    a hit with t == 0 is right when           D_tri(o) <= r + K unit;
    a miss is right when                      m(o, e) >= r - K unit,           e = o + tmax d, or where the path leaves the mesh's
                                                                               box inflated by r; tmax <= 0 admits no time: a miss;
    point lies within K unit of triangle tri, and |c - point| within K unit of r (t > 0) or of D_tri(o) (t == 0).
(The end of the segment alone, min_T D_T(c) >= r - K unit, follows from it; the whole segment also notices a sphere that passed
through a triangle and out of it again.)  With r = 0 nothing can be penetrated by a distance, so a ray's answers are also held to
the float64 ray reference (tests/test_sweep_query_host.py).  A grazing path, r - K unit <= m <= r + K unit, is right either way.

THE CONSTANT.  measure() (python tests/sweep_exact.py [items per family]) finds the smallest K for which the NATIVE BRUTE-FORCE
REFERENCE (tests/native/sweep_query_ref.cpp: csrc/sweep_tri.h over all triangles, no tree, no GPU) satisfies the contract on every
family.  Largest value found with 20 000 items per family (seeds as below):
    K_measured = 8.816 (family e; b 8.49, g 8.01, d 7.88, a 2.86, c 2.16, f 0.53)
Constant = four times the measurement, rounded up to a power of two (the families sample the worst case, they do not bound it):
    K = 64
No family needs 16 times what the others need: the needles (g) need what the grazing paths and the rays need.  Of the 8.8 units,
8 are the acceptance slack of csrc/sweep_tri.h (kSweepTol = 8 x 2^-24 S): a candidate is accepted up to that far outside r.

THE FAMILIES (fixed seeds; meshes: soup_small, terrain, grid, needle, tetra):
  a  origins in the inflated box, random directions of random length, radii from 0 to a few edge lengths
  b  aimed to graze: the path passes at r (1 +- 1e-7 .. 1e-2) from a point of an edge or from a vertex of a chosen triangle
  c  starts in contact (the centre within r of a triangle), and on the grid starts exactly at distance r: the <=
  d  far origins up to the reach, long paths; tmax at the answer, one ulp above it, half of it, +inf, 0, negative
  e  r = 0: rays at interior points, edges and vertices
  f  the grid's ties: straight down onto a shared edge or a shared vertex, where the lowest index wins
  g  the needle / collinear / point mesh
  h  invalid items of every sort, between valid ones
  m  (the mutation tests' probes, not measured) b with the path well inside: it passes at r (0.1 .. 0.8) from the edge or vertex
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_exact as CX  # noqa: E402
import native_ref as NR  # noqa: E402
import point_exact as PX  # noqa: E402

RX = PX.RX
ROOT = PX.ROOT
U = 2.0 ** -24
f32 = np.float32
MISS, INVALID = -1, -2
# python tests/sweep_exact.py 20000, per family: the K the brute-force reference needs
K_FAMILY = dict(a=2.858, b=8.486, c=2.156, d=7.881, e=8.816, f=0.534, g=8.013)
K_MEASURED = 8.816
K = 64.0  # four times the measurement, rounded up to a power of two
FAMILIES = ("a", "b", "c", "d", "e", "f", "g")  # the answered ones; h is the invalid items
_SEED = {k: 900 + i for i, k in enumerate(FAMILIES + ("h", "m"))}
MESHES = ("soup_small", "terrain", "grid", "needle", "tetra")
_MESHES = {}


def mesh(name):
    """Vertices (n, 9) by name: point_exact's meshes and `tetra`, a tetrahedron."""
    if name == "tetra":
        if name not in _MESHES:
            p = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.75 + [0.3, -0.2, 0.1]
            _MESHES[name] = np.ascontiguousarray(np.array([[p[0], p[1], p[2]], [p[0], p[3], p[1]], [p[0], p[2], p[3]], [p[1], p[3], p[2]]]).reshape(-1, 9), f32)
        return _MESHES[name]
    return PX.mesh(name)


def edge_length(verts):
    v = verts.reshape(-1, 3, 3).astype(np.float64)
    e = np.linalg.norm(np.concatenate([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]]), axis=1)
    return float(np.median(e[e > 0]))


# ---- float64 side --------------------------------------------------------------------------------------------------------------
def segment_mesh_dist(em, a, b, pad):
    """Exact distance from each segment a[i] b[i] to the mesh, over the triangles whose box inflated by pad[i] the segment crosses
    (+inf where it crosses none: then the distance is above pad[i])."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lo, hi = em.v.min(1), em.v.max(1)
    out = np.full(len(a), np.inf)
    for i in range(len(a)):
        d = b[i] - a[i]
        L, H = lo - pad[i], hi + pad[i]
        still = d == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (L - a[i]) / d, (H - a[i]) / d
        inside = (a[i] >= L) & (a[i] <= H)
        tn = np.where(still, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(1)
        tf = np.where(still, np.inf, np.maximum(t0, t1)).min(1)
        idx = np.nonzero(np.maximum(tn, 0.0) <= np.minimum(tf, 1.0))[0]
        if len(idx):
            out[i] = CX.tri_tri_dist(np.stack([a[i], b[i], b[i]])[None], em.v[idx]).min()
    return out


def path_end(em, o, d, r, tmax):
    """Where the contract's path of a miss ends: o + tmax d, or where it leaves the mesh's box inflated by r + 1 (beyond it nothing is
    within r); float64."""
    lo, hi = em.v.min((0, 1)) - (r[:, None] + 1.0), em.v.max((0, 1)) + (r[:, None] + 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tf = np.where(d == 0, np.inf, np.maximum(t0, t1)).min(1)
    t_end = np.minimum(np.where(np.isfinite(tf) & (tf > 0), tf, 0.0), np.where(tmax > 0, tmax, 0.0))
    return o + t_end[:, None] * d


class Items:
    """The float64 side of one part: its items and the exact triangles."""

    def __init__(self, verts, o, d, r, tmax=None):
        self.em = PX.ExactTris(verts)
        self.o, self.d = np.asarray(o, f32).reshape(-1, 3).astype(np.float64), np.asarray(d, f32).reshape(-1, 3).astype(np.float64)
        self.r = np.asarray(r, f32).astype(np.float64)
        self.tmax = np.full(len(self.r), np.inf) if tmax is None else np.asarray(tmax, f32).astype(np.float64)


def needs(it, t, tri, point=None):
    """The K each answer needs: the largest of the contract's terms in units (a miss: how far inside r the path comes).  An answer
    at or beyond tmax needs +inf."""
    em, t, tri = it.em, np.asarray(t, np.float64), np.asarray(tri)
    hit = tri >= 0
    tt = np.where(hit, t, 0.0)
    c = it.o + tt[:, None] * it.d
    end = np.where(hit[:, None], c, path_end(em, it.o, it.d, it.r, it.tmax))
    S = np.maximum(np.maximum(np.abs(it.o).max(1), np.abs(end).max(1)), np.maximum(em.maxabs, it.r))
    unit = U * S
    m = segment_mesh_dist(em, it.o, end, it.r + 4096.0 * unit)
    need = np.maximum((it.r - m) / unit, 0.0)  # penetration on the way (a hit at t == 0: of the start; it is then dropped below)
    tr = np.where(hit, tri, 0)
    Dt = em.dist(c, tr)
    need = np.where((hit & (tt == 0)) | (~hit & ~(it.tmax > 0)), 0.0, need)  # (tmax <= 0 admits no time at all: a miss is right)
    need = np.where(hit, np.maximum(need, (Dt - it.r) / unit), need)
    need = np.where(hit & ~(t < it.tmax), np.inf, need)
    if point is not None:
        p = np.asarray(point, np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            on_tri = em.dist(p, tr) / unit
            far = np.abs(np.sqrt(((c - p) ** 2).sum(1)) - np.where(tt == 0, Dt, it.r)) / unit
        bad = np.where(np.isnan(on_tri) | np.isnan(far), np.inf, np.maximum(on_tri, far))
        need = np.where(hit, np.maximum(need, bad), need)
    return need


def check(it, t, tri, point=None, Kc=K):
    """ok[i]: the answer (t[i], tri[i][, point[i]]) (tri = -1: a miss) of item i satisfies the contract."""
    return needs(it, t, tri, point) <= Kc


# ---- the native reference ------------------------------------------------------------------------------------------------------
def build_reference(sanitized=False, where=None):
    """Compiles tests/native/sweep_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("sweep_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, o, d, r, tmax=None, mode="all", pairs=None, sanitized=False):
    """The native reference on mesh `verts`.  Returns dict(brute=..., walk=..., nodes, tris (uint32 per item), nodes_total,
    tris_total, tree_nodes[, pair_t]); brute and walk are dicts of t (float32), tri (int32) and point (n, 3)."""
    o, d = np.ascontiguousarray(o, f32).reshape(-1, 3), np.ascontiguousarray(d, f32).reshape(-1, 3)
    n = len(o)
    inputs = dict(mesh=np.asarray(verts, f32), origins=o, dirs=d, radius=np.ascontiguousarray(r, f32), out=NR.OUT, tmax=None if tmax is None else np.asarray(tmax, f32),
                  mode=mode)
    if pairs is not None:
        inputs["pairs"] = np.ascontiguousarray(pairs, np.int32)
    fields = [("nodes", np.uint32, n), ("tris", np.uint32, n)] + [(f"{name}.{key}", dt, n * w) for name in ("brute", "walk")
                                                                  for key, dt, w in (("t", f32, 1), ("tri", np.int32, 1), ("point", f32, 3))]
    head, flat = NR.unpack(NR.run(build_reference(sanitized), inputs), 4, fields + [("pair_t", f32, 0 if pairs is None else inputs["pairs"].size // 2)])
    assert head[0] == n
    out = dict(nodes_total=head[1], tris_total=head[2], tree_nodes=head[3], nodes=flat["nodes"], tris=flat["tris"])
    for name in ("brute", "walk"):
        out[name] = dict(t=flat[f"{name}.t"], tri=flat[f"{name}.tri"], point=flat[f"{name}.point"].reshape(n, 3))
    if pairs is not None:
        out["pair_t"] = flat["pair_t"]
    return out


def walk_is_brute(ref):
    """The tree walk's answers are the brute force's, bit for bit in every column."""
    return all(NR.same_bits(ref["brute"][key], ref["walk"][key]) for key in ("t", "tri", "point"))


# ---- the item families ---------------------------------------------------------------------------------------------------------
def _scaled(rng, u):
    """Directions that are not normalised: unit vectors times 2^-3 .. 2^3."""
    return u * np.exp(rng.uniform(np.log(0.125), np.log(8.0), (len(u), 1)))


def _radii(rng, n, L, zero_share=0.1):
    r = L * np.exp(rng.uniform(np.log(0.01), np.log(4.0), n))
    return np.where(rng.random(n) < zero_share, 0.0, r)


def _random(rng, v, n):
    """(a)"""
    return PX._in_box(rng, v, n), _scaled(rng, RX._unit(rng, n)), _radii(rng, n, edge_length(v))


def _perp(rng, u):
    w = np.cross(u, RX._unit(rng, len(u)))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _grazing(rng, v, n, deep=False):
    """(b) the path passes at r (1 + s) from an edge point or a vertex p, |s| = 1e-7 .. 1e-2: past an edge along the common
    perpendicular of the path and the edge, past a vertex along any perpendicular of the path.  deep (m): s = -0.9 .. -0.2."""
    L = edge_length(v)
    p, tri = RX._targets(rng, v, n, "eev")
    T = v.reshape(-1, 3, 3).astype(np.float64)[tri]
    u = RX._unit(rng, n)
    edges = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
    on = np.abs(np.linalg.norm(np.cross(edges, (p.astype(np.float64)[:, None] - T)), axis=2)).argmin(1)  # the edge p lies on
    w = np.cross(u, edges[np.arange(n), on])
    ln = np.linalg.norm(w, axis=1, keepdims=True)
    w = np.where(ln > 1e-9, w / np.where(ln > 1e-9, ln, 1.0), _perp(rng, u))
    w *= rng.choice([-1.0, 1.0], (n, 1))
    r = L * np.exp(rng.uniform(np.log(0.02), np.log(2.0), n))
    s = rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), n))
    if deep:
        s = rng.uniform(-0.9, -0.2, n)
    back = r + L * rng.uniform(0.5, 6.0, n)
    o = p.astype(np.float64) + w * (r * (1 + s))[:, None] - u * back[:, None]
    return o, _scaled(rng, u), r


def _contact(rng, v, n, exact_r=False):
    """(c) the centre within r of a triangle; exact_r (the grid): straight above an interior point at exactly r, a binary fraction."""
    L = edge_length(v)
    p, tri = RX._targets(rng, v, n, "i" if exact_r else "iiev")
    if exact_r:
        r = 2.0 ** rng.integers(-6, 2, n)
        o = p.astype(np.float64)
        o[:, 1] = (p[:, 1] + r.astype(f32)).astype(np.float64)
        return o, _scaled(rng, RX._unit(rng, n)), r
    r = L * np.exp(rng.uniform(np.log(0.02), np.log(2.0), n))
    o = p.astype(np.float64) + PX._normals(v, tri) * (r * rng.uniform(0.0, 1.0, n) * rng.choice([-1.0, 1.0], n))[:, None]
    return o, _scaled(rng, RX._unit(rng, n)), r


def _aimed(rng, v, n, kinds, o=None, jitter=0.0):
    """Paths from o (default: 1 .. 20 edge lengths away, within the reach) towards points of the mesh, the direction not normalised."""
    L = edge_length(v)
    p, _ = RX._targets(rng, v, n, kinds)
    p = p.astype(np.float64) + RX._unit(rng, n) * (jitter * L * rng.random((n, 1)))
    if o is None:
        o = p + RX._unit(rng, n) * L * rng.uniform(1.0, 20.0, (n, 1))
        o = np.clip(o, -0.99 * float(PX.reach_of(v)), 0.99 * float(PX.reach_of(v)))
    o = np.asarray(o, f32).astype(np.float64)
    d = p - o
    short = np.linalg.norm(d, axis=1) < 1e-9
    d[short] = [0.0, 0.0, 1.0]
    return o, d * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (n, 1)))


def _far(rng, v, n):
    """(d) origins at 2 .. 32 M (the last sixth exactly at the reach), aimed at the mesh."""
    o, d = _aimed(rng, v, n, "iiev", o=PX._far(rng, v, n), jitter=0.5)
    return o, d, _radii(rng, n, edge_length(v), zero_share=0.05)


def _rays(rng, v, n):
    """(e)"""
    o, d = _aimed(rng, v, n, "iiev")
    return o, d, np.zeros(n)


def _ties(rng, n):
    """(f) straight down (or up) onto vertices and edge midpoints of the flat grid, r a binary fraction below the height."""
    o = PX._grid_ties(rng, n).astype(np.float64)
    h = o[:, 1] - 5.3
    d = np.zeros((n, 3))
    d[:, 1] = -np.sign(h) * 2.0 ** rng.integers(-2, 3, n)
    return o, d, np.abs(h) * 2.0 ** -rng.integers(1, 4, n)


def _needles(rng, v, n):
    """(g)"""
    o, d = _aimed(rng, v, n, "iiev", jitter=0.3)
    return o, d, np.where(rng.random(n) < 0.1, 0.0, np.exp(rng.uniform(np.log(1e-4), np.log(1.0), n)))


def _invalid(rng, v):
    """(h) (o, d, r, tmax, valid)"""
    reach = PX.reach_of(v)
    base_o, base_d, base_r = _random(rng, v, 64)
    rows = []

    def add(k, ok, o=None, d=None, r=None, tmax=np.inf):
        oo, dd = base_o[k].astype(f32).copy(), base_d[k].astype(f32).copy()
        if o is not None:
            oo[o[0]] = o[1]
        if d is not None:
            dd[d[0]] = d[1]
        rows.append((oo, dd, f32(base_r[k] if r is None else r), f32(tmax), ok))

    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            add(k, False, o=(axis, bad))
            add(k + 1, False, d=(axis, bad))
            k += 2
    for bad in (np.nan, -1.0, -1e-30, np.inf, -np.inf, np.nextafter(reach, f32(np.inf))):
        add(k, False, r=bad)
        k += 1
    add(k, False, tmax=np.nan)
    add(k + 1, True, tmax=-np.inf)  # valid: a miss without a walk
    add(k + 2, True, tmax=0.0)
    add(k + 3, True, r=reach)  # exactly at the limit
    add(k + 4, True, r=0.0)
    add(k + 5, True, r=-0.0)
    k += 6
    for axis, sign in ((0, 1.0), (1, -1.0), (2, 1.0)):
        add(k, False, o=(axis, sign * np.nextafter(reach, f32(np.inf))))
        add(k + 1, True, o=(axis, sign * reach))
        k += 2
    while k < 64:
        add(k, True)
        k += 1
    return (np.array([x[0] for x in rows], f32), np.array([x[1] for x in rows], f32), np.array([x[2] for x in rows], f32), np.array([x[3] for x in rows], f32),
            np.array([x[4] for x in rows]))


def family(name, n=2400, moved=False):
    """The parts of one family: a list of dict(mesh, verts, o, d, r[, tmax, valid]), fp32.  moved: on ray_exact.moved() vertices."""
    rng = np.random.default_rng(_SEED[name])

    def verts_of(m):
        return RX.moved(mesh(m)) if moved else mesh(m)

    def part(m, make, k):
        v = verts_of(m)
        o, d, r = make(v, k)
        return dict(mesh=m, verts=v, o=np.ascontiguousarray(o, f32), d=np.ascontiguousarray(d, f32), r=np.ascontiguousarray(r, f32))

    def parts(meshes, make):
        return [part(m, make, k) for m, k in zip(meshes, PX._split(n, len(meshes)))]

    if name == "a":
        return parts(MESHES, lambda v, k: _random(rng, v, k))
    if name == "b":
        return parts(("soup_small", "terrain", "grid", "tetra"), lambda v, k: _grazing(rng, v, k))
    if name == "c":
        return parts(("soup_small", "terrain", "tetra"), lambda v, k: _contact(rng, v, k)) + [part("grid", lambda v, k: _contact(rng, v, k, exact_r=True), max(1, n // 4))]
    if name == "d":
        out = parts(("soup_small", "terrain", "grid", "tetra"), lambda v, k: _far(rng, v, k))
        for p in out:  # tmax in six variants about the unlimited answer
            t = reference(p["verts"], p["o"], p["d"], p["r"])["brute"]["t"]
            kind = np.arange(len(t)) % 6
            with np.errstate(invalid="ignore", over="ignore"):
                p["tmax"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [t, np.nextafter(t, f32(np.inf)), (t * f32(0.5)).astype(f32), np.full_like(t, np.inf),
                                                                                                  np.zeros_like(t)], f32(-1.0)).astype(f32)
        return out
    if name == "e":
        return parts(("soup_small", "terrain", "grid", "tetra"), lambda v, k: _rays(rng, v, k))
    if name == "f":
        return [part("grid", lambda v, k: _ties(rng, k), n)]
    if name == "g":
        return [part("needle", lambda v, k: _needles(rng, v, k), n)]
    if name == "m":
        return parts(("soup_small", "terrain", "tetra"), lambda v, k: _grazing(rng, v, k, deep=True))
    if name == "h":
        out = []
        for m in ("soup_small", "terrain"):
            v = verts_of(m)
            o, d, r, tmax, valid = _invalid(rng, v)
            out.append(dict(mesh=m, verts=v, o=o, d=d, r=r, tmax=tmax, valid=valid))
        return out
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def family_case(name, n=2400, moved=False):
    """family(name) with each part's native reference: dict(mesh, verts, o, d, r, ref[, tmax, valid]).  Computed once, left unchanged."""
    return [dict(p, ref=reference(p["verts"], p["o"], p["d"], p["r"], p.get("tmax"))) for p in family(name, n, moved)]


def items_of(part):
    return Items(part["verts"], part["o"], part["d"], part["r"], part.get("tmax"))


# ---- measuring the constant ----------------------------------------------------------------------------------------------------
def measure(n=20000, out=sys.stdout):
    """Smallest K for which the native brute-force reference satisfies the contract, family by family."""
    worst = (0.0, None)
    for name in FAMILIES:
        k_f = 0.0
        for c in family_case(name, n):
            a = c["ref"]["brute"]
            assert (a["tri"] >= MISS).all(), (name, c["mesh"])
            k_p = float(needs(items_of(c), a["t"], a["tri"], a["point"]).max())
            hit = a["tri"] >= 0
            print(f"family {name} {c['mesh']:10s}: K needed {k_p:8.3f}   ({int(hit.sum())} hits of {len(hit)}, {int((hit & (a['t'] == 0)).sum())} at the start; "
                  f"{c['ref']['tris_total'] / len(hit):.1f} records, {c['ref']['nodes_total'] / len(hit):.1f} of {c['ref']['tree_nodes']} nodes per item)", file=out, flush=True)
            k_f = max(k_f, k_p)
        print(f"family {name}: K needed {k_f:8.3f}", file=out, flush=True)
        if k_f > worst[0]:
            worst = (k_f, name)
    print(f"K_measured = {worst[0]:.3f} (family {worst[1]}) -> K = {RX.pow2_margin(worst[0]):g}", file=out)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
