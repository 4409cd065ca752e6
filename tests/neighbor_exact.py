"""Reference of path B's neighbour queries, the radii that probe them, and the float64 contract they are held to.

Test helper (imported by tests/test_neighbor_query_host.py and tests/test_gpu_neighbor_query.py); a sibling of tests/point_exact.py,
whose meshes, point families, float64 distances and constant Kp it uses; not a conftest, no fixtures.

THE REFERENCE is tests/native/neighbor_query_ref.cpp: csrc/point_tri.h over all triangles, every one with d2 < rmax * rmax kept, sorted
by (d2, original index) - the definition, no tree, no GPU - and beside it a walk of the host-built BVH8 under the kernel's culling rule
with its nodes and triangles per point.

THE RADII of a point come from its own unlimited list (VARIANTS): exactly the dist of its k-th nearest triangle for k = 1, 8, 40 (the
test is strict, so that entry and its ties fall out wherever fp32(dist * dist) <= d2 - the product is not always the d2 the root came
from, and the reference decides), one ulp above it, half the nearest dist (nothing), 0, a negative one, one whose square underflows
(2^-76), and +inf on the meshes of at most INF_MAX_TRIS triangles, for the first INF_POINTS points of a part: a list as long as
the mesh costs its length squared in insertions however few points ask for one, and eight meet everything the others would.

THE CONTRACT in float64, with point_exact's Kp = 16 and unit: every triangle with exact distance D < rmax - Kp unit is listed, none with
D > rmax + Kp unit is, and each listed dist is within Kp unit of its triangle's D."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import point_exact as PX  # noqa: E402

ROOT = PX.ROOT
f32 = np.float32
INF = f32(np.inf)
INVALID = -2
KS = (1, 8, 40)
VARIANTS = tuple(f"k{k}_{how}" for k in KS for how in ("at", "above")) + ("half", "zero", "negative", "underflow")
INF_MAX_TRIS = 2000
INF_POINTS = 8
LONGEST = 256  # the longest list outside the +inf block (asserted on the CPU: test_neighbor_query_host.py)
N_FAMILY = 600


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/neighbor_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("neighbor_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, p, rmax, sanitized=False):
    """The native reference on mesh `verts`, points p and radii rmax (an array, or one value for all).  Returns a dict: count (int32;
    INVALID for an invalid point), offsets (int64, n + 1), d2, dist (float32), tri (int32): the brute-force lists; walk_count, walk_d2,
    walk_tri: the tree walk's; nodes, tris (uint32 per point): what the walk fetched and tested; neighbors, walk_neighbors, nodes_total,
    tris_total, invalid: the sums."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    raw = NR.run(build_reference(sanitized), dict(mesh=np.asarray(verts, f32), points=p, rmax=np.broadcast_to(np.asarray(rmax, f32), (n,))))
    head, out = NR.unpack(raw, 6, lambda h: (("count", np.int32, n), ("walk_count", np.int32, n), ("nodes", np.uint32, n), ("tris", np.uint32, n), ("offsets", np.int64, n + 1),
                                             ("d2", f32, h[1]), ("dist", f32, h[1]), ("tri", np.int32, h[1]), ("walk_d2", f32, h[2]), ("walk_tri", np.int32, h[2])))
    assert head[0] == n
    return dict(out, neighbors=head[1], walk_neighbors=head[2], nodes_total=head[3], tris_total=head[4], invalid=head[5])


same_bits = NR.same_bits


def walk_is_brute(ref):
    """The tree walk's lists are the brute force's, entry for entry and bit for bit."""
    return np.array_equal(ref["count"], ref["walk_count"]) and same_bits(ref["d2"], ref["walk_d2"]) and np.array_equal(ref["tri"], ref["walk_tri"])


def rows(ref, sel):
    """The reference `ref` cut to the points sel (a slice or an index array), offsets rebased: what a query of those points alone returns."""
    idx = np.arange(len(ref["count"]))[sel]
    count = ref["count"][idx]
    lens = np.maximum(count, 0).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(ref["offsets"][idx] - offsets[:-1], lens) + np.arange(offsets[-1])  # entry k of the cut = entry take[k] of ref
    return dict(count=count, offsets=offsets, d2=ref["d2"][take], dist=ref["dist"][take], tri=ref["tri"][take], neighbors=int(lens.sum()),
                invalid=int((count == INVALID).sum()), nodes=ref["nodes"][idx], tris=ref["tris"][idx], nodes_total=int(ref["nodes"][idx].sum(dtype=np.uint64)),
                tris_total=int(ref["tris"][idx].sum(dtype=np.uint64)))


def first_entries(ref):
    """(dist, tri) of every point's first list entry; (+inf, -1) for an empty list, (NaN, INVALID) for an invalid point: query_points' answer."""
    n = len(ref["count"])
    dist, tri = np.full(n, INF, f32), np.full(n, -1, np.int32)
    has = ref["count"] > 0
    dist[has], tri[has] = ref["dist"][ref["offsets"][:-1][has]], ref["tri"][ref["offsets"][:-1][has]]
    bad = ref["count"] == INVALID
    dist[bad], tri[bad] = np.nan, INVALID
    return dist, tri


# ---- the radii --------------------------------------------------------------------------------------------------------------------
def kth_dist(free, k):
    """dist of the k-th nearest triangle (1-based; the last one where a list is shorter) of every point of the unlimited reference `free`."""
    count = free["count"].astype(np.int64)
    assert (count > 0).all()
    return free["dist"][free["offsets"][:-1] + np.minimum(k, count) - 1]


def radii(free, variant):
    n = len(free["count"])
    if variant == "half":
        return (kth_dist(free, 1) * f32(0.5)).astype(f32)
    if variant == "zero":
        return np.where(np.arange(n) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)
    if variant == "negative":
        return np.where(np.arange(n) % 2 == 0, f32(-1.0), -INF).astype(f32)
    if variant == "underflow":
        return np.full(n, 2.0 ** -76, f32)
    k, how = variant[1:].split("_")
    at = kth_dist(free, int(k))
    return at if how == "at" else np.nextafter(at, INF)


def with_radii(verts, p, ks=KS):
    """(p, rmax, ref, free, blocks) of the points once per variant (blocks of len(p), in VARIANTS' order; `blocks` maps a variant's name to
    its slice), then the +inf block of the first INF_POINTS points where the mesh is small enough."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    free = reference(verts, p, INF)
    names = [v for v in VARIANTS if v in ("half", "zero", "negative", "underflow") or int(v[1:].split("_")[0]) in ks]
    blocks = {v: slice(i * n, (i + 1) * n) for i, v in enumerate(names)}
    ps, rs = [p] * len(names), [radii(free, v) for v in names]
    if len(verts) <= INF_MAX_TRIS:
        m = min(n, INF_POINTS)
        blocks["inf"] = slice(len(names) * n, len(names) * n + m)
        ps.append(p[:m])
        rs.append(np.full(m, INF, f32))
    p_all, rmax = np.ascontiguousarray(np.concatenate(ps)), np.ascontiguousarray(np.concatenate(rs), f32)
    return p_all, rmax, reference(verts, p_all, rmax), free, blocks


@functools.lru_cache(maxsize=None)
def family_case(name, n=N_FAMILY, moved=False):
    """The parts of family `name` of tests/point_exact.py, on its meshes or on ray_exact.moved() vertices: a list of dict(mesh, verts, p,
    rmax, ref, free, blocks, n) (n = points per variant)."""
    out = []
    for part in PX.family(name, n, moved=PX.RX.moved if moved else None):
        p, rmax, ref, free, blocks = with_radii(part["verts"], part["p"])
        out.append(dict(mesh=part["mesh"], verts=part["verts"], p=p, rmax=rmax, ref=ref, free=free, blocks=blocks, n=len(part["p"])))
    return out


def longest_limited(case):
    """The longest list of a part outside its +inf block."""
    count = case["ref"]["count"]
    stop = case["blocks"]["inf"].start if "inf" in case["blocks"] else len(count)
    return int(count[:stop].max())


# ---- the float64 contract ---------------------------------------------------------------------------------------------------------
def contract(em, p, rmax, count, offsets, dist, tri, D=None, Kp=PX.KP):
    """ok[i]: the list of point i (entries offsets[i] .. offsets[i] + count[i] of dist / tri) satisfies the contract under rmax[i]."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    D = em.all_dists(p) if D is None else D
    band = Kp * PX.unit_of(p, em)
    r = np.asarray(rmax, np.float64)
    lens = np.maximum(np.asarray(count), 0).astype(np.int64)
    owner = np.repeat(np.arange(n), lens)
    entry = np.repeat(np.asarray(offsets)[:-1], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    listed = np.zeros(D.shape, bool)
    listed[owner, tri[entry]] = True
    ok = ~((D < (r - band)[:, None]) & ~listed).any(1) & ~((D > (r + band)[:, None]) & listed).any(1)
    off = np.abs(np.asarray(dist, np.float64)[entry] - D[owner, tri[entry]]) > band[owner]
    ok[owner[off]] = False
    return ok
