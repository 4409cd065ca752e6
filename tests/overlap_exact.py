"""Reference of path B's overlap queries, the query triangles that probe them, and the float64 contract they are held to.

Test helper (imported by tests/test_overlap_query_host.py and tests/test_gpu_overlap_query.py); a sibling of tests/neighbor_exact.py; the
meshes are tests/point_exact.py's, at most 2 000 triangles; not a conftest, no fixtures.

THE REFERENCE is tests/native/overlap_query_ref.cpp: csrc/tri_overlap.h over all pairs - cand, then the six segment tests, every mesh
triangle with a mask != 0 kept, ascending by original index: the definition, no tree, no GPU - and beside it a walk of the host-built
BVH8 under the kernel's culling rule with its nodes and records per query.

THE QUERY FAMILIES (fixed seeds; a part has at most 600 query triangles):
  a  the mesh's own triangles displaced by 0.05 and by 1 of their size (the longest edge) in a random direction
  b  the mesh's own triangles unmoved: every edge and vertex is shared with the mesh
  c  random triangles planted across a mesh triangle so that edge A0A1 pierces it well inside (bit 0 is set)
  d  triangles whose box spans the whole mesh, on `needle` (12 triangles) and on a 256-triangle cut of the soup only: the insertion is
     O(k^2), so the longest list outside d is asserted <= LONGEST on the CPU
  e  a query coplanar with a mesh triangle (the flat grid: det == 0 exactly), queries without area (a segment, a point), queries far
     away but in reach, and NaN, +-inf and beyond-reach vertices

THE CONTRACT in float64 (contract()): for a pair with cand and each of its six tests, on the fp32 inputs of the test (origin, fp32
direction, fp32 v0 and edges), u/det, v/det, 1 - u/det - v/det, t and 1 - t in float64; low = their minimum.  low > M: the bit must be
set; low < -M: it must be clear; a float64 det == 0 decides nothing.
    largest |low| among the (test, pair) cases where the fp32 verdict and the sign of low differ, all families, all meshes:
        measured 1.97e-08 (one case, family b on the needle mesh; python tests/overlap_exact.py)
    M = 16 x that, the KP convention of tests/point_exact.py, rounded up to a power of two:  M = 2^-21 = 4.77e-07
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import point_exact as PX  # noqa: E402

RX = PX.RX
ROOT = PX.ROOT
f32 = np.float32
INVALID = -2
LONGEST = 256  # the longest list outside family d (asserted on the CPU: test_overlap_query_host.py)
M_MEASURED = 1.97e-08
M = 2.0 ** -21
FAMILIES = ("a", "b", "c", "d", "e")
_SEED = {k: 500 + i for i, k in enumerate(FAMILIES)}
ALL_MESHES = ("soup", "soup_small", "soup_far", "terrain", "grid", "needle")
SOUP_CUT = 256


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/overlap_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("overlap_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, q, sanitized=False):
    """The native reference on mesh `verts` and query triangles q (n, 9).  Returns a dict: count (int32; INVALID for an invalid query),
    offsets (int64, n + 1), tri, edges (int32): the brute-force lists; walk_count, walk_tri, walk_edges: the tree walk's; nodes, tris
    (uint32 per query): what the walk fetched; overlaps, walk_overlaps, nodes_total, tris_total, invalid: the sums; pair_q, pair_t,
    pair_mask: every pair with cand (mask 0 included)."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 9)
    n = len(q)
    raw = NR.run(build_reference(sanitized), dict(mesh=np.asarray(verts, f32), queries=q))
    head, out = NR.unpack(raw, 7, lambda h: (("count", np.int32, n), ("walk_count", np.int32, n), ("nodes", np.uint32, n), ("tris", np.uint32, n), ("offsets", np.int64, n + 1),
                                             ("tri", np.int32, h[1]), ("edges", np.int32, h[1]), ("walk_tri", np.int32, h[2]), ("walk_edges", np.int32, h[2]),
                                             ("pair_q", np.int32, h[6]), ("pair_t", np.int32, h[6]), ("pair_mask", np.int32, h[6])))
    assert head[0] == n
    return dict(out, overlaps=head[1], walk_overlaps=head[2], nodes_total=head[3], tris_total=head[4], invalid=head[5])


def walk_is_brute(ref):
    """The tree walk's lists are the brute force's, entry for entry."""
    return np.array_equal(ref["count"], ref["walk_count"]) and np.array_equal(ref["tri"], ref["walk_tri"]) and np.array_equal(ref["edges"], ref["walk_edges"])


def rows(ref, sel):
    """The reference `ref` cut to the queries sel (a slice or an index array), offsets rebased: what a query of those triangles alone returns."""
    idx = np.arange(len(ref["count"]))[sel]
    count = ref["count"][idx]
    lens = np.maximum(count, 0).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(ref["offsets"][idx] - offsets[:-1], lens) + np.arange(offsets[-1])  # entry k of the cut = entry take[k] of ref
    return dict(count=count, offsets=offsets, tri=ref["tri"][take], edges=ref["edges"][take], overlaps=int(lens.sum()), invalid=int((count == INVALID).sum()),
                nodes=ref["nodes"][idx], tris=ref["tris"][idx], nodes_total=int(ref["nodes"][idx].sum(dtype=np.uint64)),
                tris_total=int(ref["tris"][idx].sum(dtype=np.uint64)))


# ---- the query families -----------------------------------------------------------------------------------------------------------
def _size(tri):
    """The longest edge of each (n, 3, 3) triangle."""
    t = tri.astype(np.float64)
    return np.sqrt(np.maximum(np.maximum(((t[:, 1] - t[:, 0]) ** 2).sum(1), ((t[:, 2] - t[:, 1]) ** 2).sum(1)), ((t[:, 0] - t[:, 2]) ** 2).sum(1)))


def _displaced(rng, verts, n, share):
    v = verts.reshape(-1, 3, 3)
    pick = rng.integers(0, len(v), n)
    t = v[pick].astype(np.float64)
    size = _size(v[pick])
    size = np.where(size > 0, size, 1.0)  # (the needle mesh has a triangle that is a point)
    return (t + (RX._unit(rng, n) * (share * size)[:, None])[:, None, :]).astype(f32).reshape(-1, 9)


def _own(rng, verts, n):
    v = verts.reshape(-1, 9)
    return v[rng.permutation(len(v))[:n]].copy()


def _planted(rng, verts, n):
    """Edge A0A1 passes through an interior point of a mesh triangle (every barycentric weight >= 0.15), 0.2 .. 0.8 of its way along, at
    30 degrees or more to the plane; A2 is anywhere about."""
    p, tri = RX._targets(rng, verts, n, "i")
    v = verts.reshape(-1, 3, 3)[tri]
    size = _size(v)
    size = np.where(size > 0, size, 1.0)
    nrm = PX._normals(verts, tri)
    d = RX._unit(rng, n)
    d = d + nrm * (np.sign((d * nrm).sum(1)) * 0.6)[:, None]  # |cos| to the normal >= about 0.5
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = size * rng.uniform(0.3, 1.5, n)
    s = rng.uniform(0.2, 0.8, n)
    a0 = p.astype(np.float64) - d * (s * length)[:, None]
    a1 = a0 + d * length[:, None]
    a2 = p.astype(np.float64) + RX._unit(rng, n) * (size * rng.uniform(0.3, 1.5, n))[:, None]
    return np.concatenate([a0, a1, a2], 1).astype(f32)


def _spanning(rng, verts, n):
    """Triangles whose box contains the mesh's: two vertices beyond opposite corners, the third anywhere in between."""
    v = verts.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    flip = rng.random((n, 3)) < 0.5
    a0 = np.where(flip, hi + ext * rng.uniform(0.01, 0.5, (n, 3)), lo - ext * rng.uniform(0.01, 0.5, (n, 3)))
    a1 = np.where(flip, lo - ext * rng.uniform(0.01, 0.5, (n, 3)), hi + ext * rng.uniform(0.01, 0.5, (n, 3)))
    a2 = rng.uniform(lo - ext, hi + ext, (n, 3))
    return np.concatenate([a0, a1, a2], 1).astype(f32)


def _special(rng, verts, mesh):
    """Family e.  Returns (queries, kinds): kinds[i] names what query i is."""
    v = verts.reshape(-1, 3, 3)
    reach = PX.reach_of(verts)
    out, kinds = [], []

    def add(kind, t):
        out.append(np.asarray(t, np.float64).reshape(9))
        kinds.append(kind)

    if mesh == "grid":  # in the plane of the grid: shifted within it, and rotated within it
        for t in v[rng.permutation(len(v))[:12]].astype(np.float64):
            c = t.mean(0)
            turned = (t - c)[:, [2, 1, 0]] * [1.0, 1.0, -1.0] * 1.7 + c
            turned[:, 1] = t[:, 1]  # the plane's own coordinate, bit for bit
            add("coplanar", t + np.array([0.11, 0.0, -0.07]))
            add("coplanar", turned)
    for t in v[rng.permutation(len(v))[:12]].astype(np.float64):
        size = max(float(_size(t[None])[0]), 1e-3)
        c, d = t.mean(0), RX._unit(rng, 1)[0]
        add("segment", [c - d * size, c + d * size, c + d * size])  # pierces, or not: three segments, two of them the same
        add("segment", [c - d * size, c - d * size, c + d * size])
        add("point", [c, c, c])
        far = c + RX._unit(rng, 1)[0] * float(reach) * 0.4
        add("far", t - c + far)
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 4, 8):
            t = v[rng.integers(len(v))].astype(np.float64).reshape(9)
            t[k] = bad
            add("invalid", t)
    for k, sign in ((1, 1.0), (3, -1.0), (8, 1.0)):
        t = v[rng.integers(len(v))].astype(f32).reshape(9).copy()
        t[k] = sign * np.nextafter(reach, f32(np.inf))
        add("invalid", t)
        t = t.copy()
        t[k] = sign * reach  # exactly at the reach: valid
        add("edge", t)
    return np.asarray(out).astype(f32), np.asarray(kinds)


def soup_cut():
    return np.ascontiguousarray(PX.mesh("soup")[:SOUP_CUT])


def family(name, moved=False):
    """The parts of one family: a list of dict(mesh, verts, q[, kinds]).  moved: on ray_exact.moved() vertices (the refit tests)."""
    rng = np.random.default_rng(_SEED[name])

    def verts_of(m):
        v = soup_cut() if m == "soup_cut" else PX.mesh(m)
        return RX.moved(v) if moved else v

    def part(m, make):
        v = verts_of(m)
        return dict(mesh=m, verts=v, q=np.ascontiguousarray(make(v), f32))

    if name == "a":
        return [part(m, lambda v: np.concatenate([_displaced(rng, v, 100, 0.05), _displaced(rng, v, 100, 1.0)])) for m in ALL_MESHES]
    if name == "b":
        return [part(m, lambda v: _own(rng, v, 200)) for m in ALL_MESHES]
    if name == "c":
        return [part(m, lambda v: _planted(rng, v, 150)) for m in ("soup", "soup_far", "terrain", "grid")]
    if name == "d":
        return [part(m, lambda v: _spanning(rng, v, 40)) for m in ("needle", "soup_cut")]
    if name == "e":
        out = []
        for m in ("grid", "soup"):
            v = verts_of(m)
            q, kinds = _special(rng, v, m)
            out.append(dict(mesh=m, verts=v, q=np.ascontiguousarray(q, f32), kinds=kinds))
        return out
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def family_case(name, moved=False):
    """family(name) with each part's reference: dict(mesh, verts, q, ref[, kinds])."""
    out = []
    for part in family(name, moved):
        assert len(part["q"]) <= 600 and len(part["verts"]) <= 2000
        out.append(dict(part, ref=reference(part["verts"], part["q"])))
    return out


def edge_segments(q):
    """The 3 n edge segments of the query triangles q (n, 9) as (origins, fp32 directions), edge-major per triangle: A0A1, A1A2, A2A0."""
    t = np.ascontiguousarray(q, f32).reshape(-1, 3, 3)
    o = t.reshape(-1, 3)
    d = (np.roll(t, -1, axis=1) - t).astype(f32).reshape(-1, 3)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def cand_numpy(verts, q):
    """cand(i, T) in numpy fp32: (n, n_tris) bool."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
    v0 = v[:, 0]
    e1, e2 = (v[:, 1] - v0).astype(f32), (v[:, 2] - v0).astype(f32)
    b = np.stack([v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)], 1)
    blo, bhi = b.min(1), b.max(1)
    t = np.ascontiguousarray(q, f32).reshape(-1, 3, 3)
    qlo, qhi = t.min(1), t.max(1)
    return ((qlo[:, None, :] <= bhi[None]) & (blo[None] <= qhi[:, None, :])).all(2)


# ---- the float64 contract -----------------------------------------------------------------------------------------------------------
def _seg_low(o, d, w0, g1, g2):
    """min(u/det, v/det, 1 - u/det - v/det, t, 1 - t) in float64 on fp32 inputs (NaN where det == 0)."""
    o, d, w0, g1, g2 = (np.asarray(x, f32).astype(np.float64) for x in (o, d, w0, g1, g2))
    pvec = np.cross(d, g2)
    det = (g1 * pvec).sum(-1)
    tvec = o - w0
    qvec = np.cross(tvec, g1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (tvec * pvec).sum(-1) / det
        v = (d * qvec).sum(-1) / det
        t = (g2 * qvec).sum(-1) / det
        low = np.minimum(np.minimum(np.minimum(u, v), 1.0 - u - v), np.minimum(t, 1.0 - t))
    return np.where(det == 0, np.nan, low)


def pair_lows(verts, q, pair_q, pair_t):
    """(pairs, 6) float64: low of each of the six tests of each pair, on the fp32 inputs tri_overlap.h hands to ray_tri_t."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)[pair_t]
    a = np.ascontiguousarray(q, f32).reshape(-1, 3, 3)[pair_q]
    v0 = v[:, 0]
    e1, e2 = (v[:, 1] - v0).astype(f32), (v[:, 2] - v0).astype(f32)
    a0, a1, a2 = a[:, 0], a[:, 1], a[:, 2]
    f1, f2 = (a1 - a0).astype(f32), (a2 - a0).astype(f32)
    return np.stack([_seg_low(a0, (a1 - a0).astype(f32), v0, e1, e2), _seg_low(a1, (a2 - a1).astype(f32), v0, e1, e2), _seg_low(a2, (a0 - a2).astype(f32), v0, e1, e2),
                     _seg_low(v0, e1, a0, f1, f2), _seg_low((v0 + e1).astype(f32), (e2 - e1).astype(f32), a0, f1, f2), _seg_low(v0, e2, a0, f1, f2)], 1)


def contract(lows, masks, m=M):
    """(violations, must_set): how many (test, pair) cases break the contract under margin m, and which set bits are in the "must be set" class."""
    bits = ((np.asarray(masks)[:, None] >> np.arange(6)) & 1).astype(bool)
    with np.errstate(invalid="ignore"):
        must_set, must_clear = lows > m, lows < -m
    return int((must_set & ~bits).sum() + (must_clear & bits).sum()), must_set & bits


def measure(out=sys.stdout):
    """The largest |low| among the cases where the fp32 verdict and the sign of the float64 low differ."""
    worst = (0.0, None)
    for name in FAMILIES:
        for c in family_case(name):
            ref = c["ref"]
            lows = pair_lows(c["verts"], c["q"], ref["pair_q"], ref["pair_t"])
            bits = ((ref["pair_mask"][:, None] >> np.arange(6)) & 1).astype(bool)
            with np.errstate(invalid="ignore"):
                differ = (bits & (lows < 0)) | (~bits & (lows > 0))
            w = float(np.abs(lows[differ]).max()) if differ.any() else 0.0
            print(f"family {name} {c['mesh']:10s}: {len(lows):7d} pairs, {int(bits.sum()):6d} bits set, {int(differ.sum()):4d} verdicts differ, largest |low| {w:.3g}", file=out, flush=True)
            if w > worst[0]:
                worst = (w, (name, c["mesh"]))
    print(f"M_measured = {worst[0]:.3g} {worst[1]} -> M = 2^{int(np.ceil(np.log2(16 * worst[0]))) if worst[0] else 0}", file=out)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure()
