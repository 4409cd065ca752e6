"""Exact reference of path B's inside/outside query, the contract it is held to, the closed meshes and the point families that probe it.

Test helper (imported by tests/test_side_query_host.py and tests/test_gpu_side_query.py); a sibling of tests/point_exact.py, whose
float64 distances and point generators it uses, and of tests/ray_exact.py, whose edge distance delta it uses; not a conftest, no fixtures.

THE REFERENCE.  winding() is the float64 winding number of the fp32 triangles about a point: the solid angles of van Oosterom and
Strackee, tan(W/2) = a.(b x c) / (|a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), summed over the triangles as the records form them
(v0, v0 + e1, v0 + e2) and divided by 4 pi.  On a closed mesh it is an integer away from the surface; inside means the rounded value
is odd.  float64 carries 2^-53 against fp32's 2^-24, so on fp32 inputs it serves as exact (its distance from an integer is recorded).

THE CONTRACT.  For every point whose exact distance to the surface is above Kp * unit (Kp = 16 and unit =
2^-24 * the largest |coordinate| among the point and the vertices, both of tests/point_exact.py), `inside` equals the exact answer.  A
point may also be excluded when two of its three rays pass within K = 8 units of an edge by tests/ray_exact.py's delta (there the
triangle test may count an edge twice or not at all on two rays at once); that share is at most 0.1 % per family, and 0 is expected.
No family puts a point into the distance band by construction, so the share excluded by it must be 0.

THE FAMILIES, on every mesh.  a: uniform in the bounding box inflated by half.  b: +-(1e-4 .. 1e-1) M along the normal from random
surface points.  c: far, up to and exactly at the reach 32 max(1, M).  d0, d1, d2: p = vertex - s D[k], so that ray k goes through a
mesh vertex (to the rounding of p).  e0, e1, e2: the same through a random point of an edge.  The aimed families are where a single
ray is wrong: the power test requires direction k alone to be wrong for at least 5 % of dk and ek on every closed mesh, and the
majority to be wrong for none.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import point_exact as PX  # noqa: E402
import ray_exact as RX  # noqa: E402

ROOT = PX.ROOT
f32 = np.float32
KP = PX.KP
K_EDGE = RX.K_BAND
# kParityDir of csrc/ray_parity.h (test_side_query_host.py checks them against the reference's own rays bit for bit)
D = np.array([[0.6350, 0.5127, 0.5779], [-0.4382, 0.7561, -0.4861], [0.3097, -0.4203, -0.8529]], f32)
INVALID = -2
MISS = -1


# ---- closed meshes -------------------------------------------------------------------------------------------------------------
def _grid_tris(P, wrap_j, wrap_i=False):
    """Triangles (n, 3, 3) of the quads of a vertex grid P (ni, nj, 3); vertices are shared by index, so shared edges are bit-equal."""
    ni, nj = P.shape[:2]
    out = []
    for i in range(ni if wrap_i else ni - 1):
        for j in range(nj if wrap_j else nj - 1):
            a, b, c, d = P[i, j], P[(i + 1) % ni, j], P[i, (j + 1) % nj], P[(i + 1) % ni, (j + 1) % nj]
            out += [[a, b, d], [a, d, c]]
    return np.array(out, f32)


def _outward(tris, out_dir):
    """Every triangle wound so that e1 x e2 points along out_dir(centroid)."""
    t = tris.astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = (n * out_dir(t.mean(1))).sum(1) < 0
    tris = tris.copy()
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris


def uv_sphere(stacks=16, slices=32, radius=1.3, centre=(0.11, -0.07, 0.05), reverse=False):
    """stacks x slices UV sphere: two poles of valence `slices`, no degenerate triangle.  2 slices (stacks - 1) triangles."""
    c = np.asarray(centre, np.float64)
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.cos(th)[:, None] * np.ones_like(ph), np.sin(th)[:, None] * np.sin(ph)], -1)
    P = (c + radius * ring).astype(f32)
    north, south = (c + [0, radius, 0]).astype(f32), (c - [0, radius, 0]).astype(f32)
    tris = [_grid_tris(P, wrap_j=True)]
    tris.append(np.array([[north, P[0, j], P[0, (j + 1) % slices]] for j in range(slices)], f32))
    tris.append(np.array([[south, P[-1, (j + 1) % slices], P[-1, j]] for j in range(slices)], f32))
    tris = _outward(np.concatenate(tris), lambda m: m - c)
    return tris[:, [0, 2, 1]] if reverse else tris


def torus(nu=32, nv=16, R=1.1, r=0.45, centre=(-0.06, 0.09, 0.03)):
    c = np.asarray(centre, np.float64)
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    ring = R + r * np.cos(v)
    P = (c + np.stack([ring[None, :] * np.cos(u)[:, None], np.ones_like(u)[:, None] * (r * np.sin(v))[None, :], ring[None, :] * np.sin(u)[:, None]], -1)).astype(f32)

    def out_dir(m):
        q = m - c
        flat = q * [1, 0, 1]
        return q - R * flat / np.linalg.norm(flat, axis=1, keepdims=True)
    return _outward(_grid_tris(P, wrap_j=True, wrap_i=True), out_dir)


def box(cells=8, half=1.0):
    """A cube with cells x cells quads per axis-aligned face at binary-fraction coordinates: every vertex and edge product is exact."""
    g = (np.arange(cells + 1) * (2 * half / cells) - half)
    A, B = np.meshgrid(g, g, indexing="ij")
    tris = []
    for axis in range(3):
        for side in (-half, half):
            P = np.zeros(A.shape + (3,))
            P[..., axis] = side
            P[..., (axis + 1) % 3] = A
            P[..., (axis + 2) % 3] = B
            tris.append(_grid_tris(P.astype(f32), wrap_j=False))
    return _outward(np.concatenate(tris), lambda m: m)


CLOSED = ("sphere", "torus", "shell", "box")
OPEN = ("soup", "grid")  # bit-equality only: parity is defined there, "inside" is not
_MESHES = {}


def mesh(name):
    """Vertices (n, 9) by name."""
    if name not in _MESHES:
        if name == "sphere":
            v = uv_sphere()
        elif name == "torus":
            v = torus()
        elif name == "shell":  # the cavity of the reversed inner sphere is outside
            v = np.concatenate([uv_sphere(), uv_sphere(12, 24, 0.6, (0.02, 0.1, -0.04), reverse=True)])
        elif name == "box":
            v = box()
        else:
            v = RX.mesh(name)[0]
        _MESHES[name] = np.ascontiguousarray(np.asarray(v, f32).reshape(-1, 9))
    return _MESHES[name]


def is_closed(verts):
    """Every undirected edge is used exactly twice, once in each direction (bit-equal vertices)."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
    _, idx = np.unique(v.reshape(-1, 3), axis=0, return_inverse=True)
    idx = idx.reshape(-1, 3)
    directed = np.concatenate([np.stack([idx[:, k], idx[:, (k + 1) % 3]], 1) for k in range(3)])
    key = directed[:, 0].astype(np.int64) * (idx.max() + 1) + directed[:, 1]
    rev = directed[:, 1].astype(np.int64) * (idx.max() + 1) + directed[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def winding(verts, p, chunk=None):
    """float64 winding number of the mesh about each point (not rounded)."""
    tv = PX.ExactTris(verts).v
    p = np.ascontiguousarray(p, f32).reshape(-1, 3).astype(np.float64)
    chunk = chunk or max(1, 300000 // len(tv))
    out = np.empty(len(p))
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None, :]
        a, b, c = tv[None, :, 0] - q, tv[None, :, 1] - q, tv[None, :, 2] - q
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = (2 * np.arctan2(num, den)).sum(1) / (4 * np.pi)
    return out


def exact_inside(verts, p):
    """(inside as the exact winding number has it, its largest distance from an integer)."""
    w = winding(verts, p)
    return (np.rint(w).astype(np.int64) & 1).astype(np.int32), float(np.abs(w - np.rint(w)).max()) if len(w) else 0.0


def surface_distance(verts, p):
    """(exact distance to the surface, unit) per point."""
    em = PX.ExactTris(verts)
    return em.all_dists(p).min(1), PX.unit_of(np.ascontiguousarray(p, f32).reshape(-1, 3), em)


def rays_near_an_edge(verts, p, K=K_EDGE):
    """(n, 3) bool: ray k of point i passes within K units of an edge of a triangle in front of it (ray_exact's delta)."""
    em = RX.ExactMesh(verts)
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    return np.stack([RX.Candidates(p, np.broadcast_to(D[k], p.shape), em).band(K)[0] for k in range(3)], 1)


# ---- point families ------------------------------------------------------------------------------------------------------------
FAMILIES = ("a", "b", "c", "d0", "d1", "d2", "e0", "e1", "e2")
AIMED = FAMILIES[3:]


def family(name, verts, n, seed=0):
    """n fp32 points of one family on one mesh."""
    rng = np.random.default_rng(500 + 17 * FAMILIES.index(name) + seed)
    M = max(1.0, float(np.abs(verts).max()))
    if name == "a":
        return PX._in_box(rng, verts, n)
    if name == "b":
        p, tri = RX._targets(rng, verts, n, "i")
        h = rng.choice([-1.0, 1.0], n) * M * np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), n))
        return (p.astype(np.float64) + PX._normals(verts, tri) * h[:, None]).astype(f32)
    if name == "c":
        return PX._far(rng, verts, n)
    k = int(name[1])
    if name[0] == "d":
        corners = np.unique(verts.reshape(-1, 3), axis=0)
        target = corners[rng.integers(0, len(corners), n)]
    else:
        target = RX._targets(rng, verts, n, "e")[0]
    s = M * rng.uniform(0.2, 2.5, (n, 1))
    return (target.astype(np.float64) - s * D[k].astype(np.float64)).astype(f32)


# ---- the native reference ------------------------------------------------------------------------------------------------------


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/side_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("side_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, p, rays=None, sanitized=False):
    """The native reference on mesh `verts` and points p: dict(inside (n,), third (n,), brute, walk (n, 3) crossings, t, tri (n, 3)
    closest accepted triangle along D[k], nodes, tris, thirds[, ray_t, ray_tri for rays = (origins, dirs)])."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    inputs = dict(mesh=np.asarray(verts, f32), points=p, out=NR.OUT)
    if rays is not None:
        inputs["rays"] = np.concatenate([np.asarray(rays[0], f32).reshape(-1, 3), np.asarray(rays[1], f32).reshape(-1, 3)], 1).astype(f32, copy=False)
    head, out = NR.unpack(NR.run(build_reference(sanitized), inputs), 5,
                          lambda h: (("inside", np.int32, n), ("third", np.int32, n), ("brute", np.int32, 3 * n), ("walk", np.int32, 3 * n), ("t", f32, 3 * n),
                                     ("tri", np.int32, 3 * n), ("ray_t", f32, h[4]), ("ray_tri", np.int32, h[4])))
    assert head[0] == n
    for key in ("brute", "walk", "t", "tri"):
        out[key] = out[key].reshape(n, 3)
    return dict(out, nodes=head[1], tris=head[2], thirds=head[3])


# ---- one case per mesh: the points of every family and their reference, computed once and shared ---------------------------------
N_FAMILY = 400


@functools.lru_cache(maxsize=None)
def case(name, n=N_FAMILY):
    """dict(verts, p (all families, concatenated), rows {family: slice}, ref): the families of one mesh and the native reference."""
    verts = mesh(name)
    parts = [family(f, verts, n) for f in FAMILIES]
    rows, at = {}, 0
    for f, q in zip(FAMILIES, parts):
        rows[f] = slice(at, at + len(q))
        at += len(q)
    p = np.ascontiguousarray(np.concatenate(parts), f32)
    return dict(name=name, verts=verts, p=p, rows=rows, ref=reference(verts, p))


@functools.lru_cache(maxsize=None)
def exact_case(name, n=N_FAMILY):
    """What the contract needs on a closed mesh: dict(inside, frac, dist, unit, near (n, 3))."""
    c = case(name, n)
    inside, frac = exact_inside(c["verts"], c["p"])
    dist, unit = surface_distance(c["verts"], c["p"])
    return dict(inside=inside, frac=frac, dist=dist, unit=unit, near=rays_near_an_edge(c["verts"], c["p"]))


def judge(name, inside, n=N_FAMILY):
    """{family: (wrong, excluded by the distance band, excluded by two rays near an edge, points)} of answers `inside` for case(name)."""
    c, ex = case(name, n), exact_case(name, n)
    band = ~(ex["dist"] > KP * ex["unit"])
    two = (ex["near"].sum(1) >= 2) & ~band
    wrong = (np.asarray(inside) != ex["inside"]) & ~band & ~two
    return {f: (int(wrong[r].sum()), int(band[r].sum()), int(two[r].sum()), r.stop - r.start) for f, r in c["rows"].items()}
