"""Reference of path B's k-nearest queries, the cases that probe them, and the float64 contract they are held to.

Test helper (imported by tests/test_knn_query_host.py and tests/test_gpu_knn_query.py); a sibling of tests/neighbor_exact.py, whose
cases - the meshes, point families and radius variants of tests/point_exact.py and tests/neighbor_exact.py - it asks under several k;
not a conftest, no fixtures.

THE REFERENCE is tests/native/knn_query_ref.cpp: csrc/point_tri.h over all triangles, every one with d2 < rmax * rmax kept, sorted by
(d2, original index), cut at k - the definition, no tree, no GPU - and beside it a walk of the host-built BVH8 under the kernel's culling
rule and in its order, with its nodes and triangles per point.  The program takes one k per point, so one run answers a batch under all
its k.

THE CASES of a part of a family (family_case): neighbor_exact's batch - the part's points once per radius variant, with the +inf block
- and behind it the part's points once more without a limit (the block "none": rmax = +inf here, rmax = None on the GPU), each under
every k of KS, on the needle mesh also under k = n_tris and k = n_tris + 4 (rows as long as the mesh, and short rows); and the first
BIG_POINTS points of the part without a limit under k = BIG_K = RT_KNN_MAX_K.

THE CONTRACT in float64, with point_exact's Kp = 16 and unit: every listed dist is within Kp unit of its triangle's exact distance D;
no triangle that is not listed (and lies more than the band inside rmax) has D below the row's last D - 2 Kp unit; a short row lists
every triangle with D < rmax - Kp unit; none with D > rmax + Kp unit is listed."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import neighbor_exact as NX  # noqa: E402
import point_exact as PX  # noqa: E402

ROOT = PX.ROOT
f32 = np.float32
INF = NX.INF
MISS, INVALID = -1, -2
KS = (1, 2, 7, 8, 40)
BIG_K = 1024  # RT_KNN_MAX_K
BIG_POINTS = 8
N_FAMILY = NX.N_FAMILY


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/knn_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("knn_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, p, k, rmax=None, sanitized=False):
    """The native reference on mesh `verts`, points p, k (one value, or one per point) and radii rmax (None: no limit; an array, or one
    value for all).  Returns a dict: k (uint32 per point), starts (int64, n + 1: where each row begins in the flat arrays), count (int32;
    INVALID for an invalid point), d2, dist (float32), tri (int32): the brute force's rows, k[i] entries each, padded with +inf / MISS
    (an invalid point's row: NaN / INVALID); walk_count, walk_d2, walk_tri: the tree walk's; nodes, tris (uint32 per point): what the walk
    fetched and tested; neighbors, walk_neighbors, nodes_total, tris_total, invalid: the sums."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    rmax = np.broadcast_to(np.asarray(INF if rmax is None else rmax, f32), (n,))
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.uint32), (n,)), np.uint32)
    e = int(k.sum(dtype=np.uint64))
    raw = NR.run(build_reference(sanitized), dict(mesh=np.asarray(verts, f32), points=p, rmax=rmax, k=k))
    head, out = NR.unpack(raw, 7, (("count", np.int32, n), ("walk_count", np.int32, n), ("nodes", np.uint32, n), ("tris", np.uint32, n), ("d2", f32, e), ("dist", f32, e),
                                   ("tri", np.int32, e), ("walk_d2", f32, e), ("walk_tri", np.int32, e)))
    assert head[:2] == (n, e)
    return dict(out, k=k, starts=np.concatenate([[0], np.cumsum(k.astype(np.int64))]), neighbors=head[2], walk_neighbors=head[3], nodes_total=head[4],
                tris_total=head[5], invalid=head[6])


same_bits = NX.same_bits


def walk_is_brute(ref):
    """The tree walk's rows are the brute force's, entry for entry and bit for bit (padding and invalid rows included)."""
    return np.array_equal(ref["count"], ref["walk_count"]) and same_bits(ref["d2"], ref["walk_d2"]) and np.array_equal(ref["tri"], ref["walk_tri"])


def rows(ref, sel):
    """The rectangular answer of the points sel (a slice or an index array) of `ref`, which must share one k: dict(k, count (m,), d2, dist,
    tri (m, k), nodes, tris (m,)): what a query of those points alone returns."""
    idx = np.arange(len(ref["count"]))[sel]
    k = int(ref["k"][idx[0]]) if len(idx) else 1
    assert (ref["k"][idx] == k).all()
    take = ref["starts"][idx][:, None] + np.arange(k)[None, :]
    return dict(k=k, count=ref["count"][idx], d2=ref["d2"][take], dist=ref["dist"][take], tri=ref["tri"][take], nodes=ref["nodes"][idx], tris=ref["tris"][idx])


def expected(count, dist, tri):
    """True where (count, dist, tri) are well-formed rows: ascending inside count, padded with (+inf, MISS) behind it, (NaN, INVALID)
    throughout for count == INVALID."""
    count, dist, tri = np.asarray(count), np.asarray(dist), np.asarray(tri)
    j = np.arange(dist.shape[1])[None, :]
    bad = (count == INVALID)[:, None]
    inside = (j < np.maximum(count, 0)[:, None]) & ~bad
    pad = ~inside & ~bad
    ok = (np.isnan(dist) & (tri == INVALID))[bad.repeat(dist.shape[1], 1)].all()
    ok = ok and (np.isposinf(dist) & (tri == MISS))[pad].all()
    ok = ok and (np.isfinite(dist) & (tri >= 0))[inside].all()
    both = inside[:, 1:]
    return bool(ok and ((dist[:, 1:] >= dist[:, :-1]) | ~both).all())


def ks_of(verts):
    """The k values a mesh is asked under: KS, and on the needle mesh (12 triangles) also n_tris and n_tris + 4."""
    return KS + ((len(verts), len(verts) + 4) if len(verts) < 40 else ())


@functools.lru_cache(maxsize=None)
def family_case(name, n=N_FAMILY, moved=False):
    """The parts of family `name`: a list of dict(mesh, verts, p, rmax, blocks, n, ks, ref, big) - neighbor_exact.family_case's batch with
    the block "none" (the part's points, rmax = +inf) appended; ref[k]: rows() of the whole batch under k; big: dict(p, k, ref) of the
    first BIG_POINTS points without a limit under BIG_K; nx: neighbor_exact's case (its lists are the radius query's answer)."""
    out = []
    # (asked the way the neighbour tests ask, so that functools' cache answers both from one computation)
    cases = NX.family_case(name, moved=True) if moved and n == N_FAMILY else NX.family_case(name, n, moved) if moved else NX.family_case(name) if n == N_FAMILY else NX.family_case(name, n)
    for c in cases:
        base = c["p"][:c["n"]]
        p = np.ascontiguousarray(np.concatenate([c["p"], base]))
        rmax = np.ascontiguousarray(np.concatenate([c["rmax"], np.full(len(base), INF, f32)]), f32)
        blocks = dict(c["blocks"], none=slice(len(c["p"]), len(p)))
        ks = ks_of(c["verts"])
        m = min(len(base), BIG_POINTS)
        # every point under all its k in a row: the reference program sorts a point's list once
        ref = reference(c["verts"], np.concatenate([np.repeat(p, len(ks), 0), base[:m]]), np.concatenate([np.tile(np.asarray(ks, np.uint32), len(p)), np.full(m, BIG_K, np.uint32)]),
                        np.concatenate([np.repeat(rmax, len(ks)), np.full(m, INF, f32)]))
        per_k = {k: rows(ref, np.arange(len(p)) * len(ks) + i) for i, k in enumerate(ks)}
        big = dict(p=np.ascontiguousarray(base[:m]), k=BIG_K, ref=rows(ref, slice(len(ks) * len(p), len(ks) * len(p) + m)))
        out.append(dict(mesh=c["mesh"], verts=c["verts"], p=p, rmax=rmax, blocks=blocks, n=c["n"], ks=ks, ref=per_k, big=big, nx=c, walk=ref))
    return out


def prefix_of_list(nx_ref, row, sel=slice(None)):
    """True where every row of `row` (rows() of some points) is the first min(k, length) entries of the same points' slices in the radius
    query's reference nx_ref (neighbor_exact.reference), bit for bit, and count = min(k, length)."""
    idx = np.arange(len(nx_ref["count"]))[sel]
    k = row["k"]
    lens = np.maximum(nx_ref["count"][idx], 0).astype(np.int64)
    want = np.where(nx_ref["count"][idx] == INVALID, INVALID, np.minimum(lens, k))
    if not np.array_equal(row["count"], want):
        return False
    j = np.arange(k)[None, :]
    inside = j < np.minimum(lens, k)[:, None]
    src = (nx_ref["offsets"][:-1][idx][:, None] + j)[inside]
    return same_bits(row["dist"][inside], nx_ref["dist"][src]) and np.array_equal(row["tri"][inside], nx_ref["tri"][src]) and same_bits(row["d2"][inside], nx_ref["d2"][src])


# ---- the float64 contract ---------------------------------------------------------------------------------------------------------
def contract(em, p, rmax, k, count, dist, tri, D=None, Kp=PX.KP):
    """ok[i]: row i (count[i] entries of dist[i] / tri[i]) satisfies the contract under k and rmax[i]."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    n = len(p)
    D = em.all_dists(p) if D is None else D
    band = Kp * PX.unit_of(p, em)
    r = np.broadcast_to(np.asarray(np.inf if rmax is None else rmax, np.float64), (n,))
    count, dist, tri = np.asarray(count), np.asarray(dist, np.float64), np.asarray(tri)
    j = np.arange(dist.shape[1])[None, :]
    inside = j < np.maximum(count, 0)[:, None]
    t = np.where(inside, tri, 0)
    Dt = np.take_along_axis(D, t, 1)
    ok = ~(inside & (np.abs(dist - Dt) > band[:, None])).any(1)            # every listed dist is its triangle's
    ok &= ~(inside & (Dt > (r + band)[:, None])).any(1)                    # nothing beyond the limit is listed
    listed = np.zeros(D.shape, bool)
    np.put_along_axis(listed, t, inside, 1)
    listed[:, 0] = (inside & (tri == 0)).any(1)                            # (column 0 took the padding's writes)
    within = D < (r - band)[:, None]
    full = count == min(k, D.shape[1])
    last = np.where(count > 0, np.take_along_axis(Dt, np.maximum(count - 1, 0)[:, None], 1)[:, 0], -np.inf)
    ok &= ~(full & (within & ~listed & (D < (last - 2 * band)[:, None])).any(1))  # a full row: nothing unlisted is nearer than its last
    ok &= ~(~full & (within & ~listed).any(1))                             # a short row: everything within the limit is listed
    ok &= (count >= 0) & (count <= k)
    return ok
