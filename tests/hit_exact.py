"""Reference of path B's all-hits ray queries, the ray batches that probe them and the two meshes built for them.

Test helper (imported by tests/test_hit_query_host.py and tests/test_gpu_hit_query.py); a sibling of tests/sign_exact.py, whose meshes,
points and directions it uses, and of tests/ray_exact.py, whose ray families it uses; not a conftest, no fixtures.

THE REFERENCE is tests/native/hit_query_ref.cpp: for every ray the triangles that csrc/ray_parity.h's ray_tri_t accepts with
0 < t < tmax over ALL triangles, sorted by (t, original index) - the definition, no tree - and beside it a BVH8 walk with the kernels'
slab test whose sorted list must be the same (tree independence).  Everything is compared bit for bit, so there is no tolerance here.

THE BATCHES.  family_case(f): the rays of family f of tests/ray_exact.py, part by part, four times over - without a limit, then with
tmax = the t of one of the ray's own hits (that hit and all behind it drop out: the comparison is strict), one ulp above it (the hit is
in) and half of it.  side_case(mesh): the points of tests/sign_exact.py's case on that mesh along each of the three directions D[k]
without a limit, whose counts are the side reference's crossings.  stack(): 256 parallel quads and rays through all of them;
duplicates(): every triangle twice, so that every t comes twice and the index decides the order.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import ray_exact as RX  # noqa: E402
import sign_exact as SX  # noqa: E402

ROOT = SX.ROOT
f32 = np.float32
INF = f32(np.inf)
INVALID = -2


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/hit_query_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("hit_query_ref", [NR.BVH_BUILD], sanitized, where, flags=("-pthread",))


def reference(verts, o, d, tmax=None, sanitized=False):
    """The native reference on mesh `verts` and rays (o, d, tmax; None: +inf): dict(count (n,) with INVALID = -2, walk_count (n,), same
    (n,) - the walk's sorted list is the brute force's -, offsets (n + 1,) int64, t, tri (hits,), hits, nodes, tris, invalid)."""
    o = np.ascontiguousarray(o, f32).reshape(-1, 3)
    d = np.ascontiguousarray(d, f32).reshape(-1, 3)
    n = len(o)
    tmax = np.full(n, INF, f32) if tmax is None else np.ascontiguousarray(tmax, f32).reshape(n)
    raw = NR.run(build_reference(sanitized), dict(mesh=np.asarray(verts, f32), rays=np.concatenate([o, d, tmax[:, None]], 1).astype(f32, copy=False)))
    head, out = NR.unpack(raw, 5, lambda h: (("count", np.int32, n), ("walk_count", np.int32, n), ("same", np.int32, n), ("offsets", np.int64, n + 1), ("t", f32, h[1]),
                                             ("tri", np.int32, h[1])))
    assert head[0] == n
    return dict(out, hits=head[1], nodes=head[2], tris=head[3], invalid=head[4])


def rows(ref, sel):
    """The reference `ref` cut to the rays sel (a slice or an index array), offsets rebased: what a query of those rays alone returns."""
    idx = np.arange(len(ref["count"]))[sel]
    count = ref["count"][idx]
    lens = np.maximum(count, 0).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(ref["offsets"][idx] - offsets[:-1], lens) + np.arange(offsets[-1])  # entry k of the cut = entry take[k] of ref
    return dict(count=count, offsets=offsets, t=ref["t"][take], tri=ref["tri"][take], hits=int(lens.sum()), invalid=int((count == INVALID).sum()))


same_bits = NR.same_bits


def first_hits(ref):
    """(t, tri) of every ray's first list entry; (+inf, -1) for an empty list."""
    n = len(ref["count"])
    t, tri = np.full(n, INF, f32), np.full(n, -1, np.int32)
    has = ref["count"] > 0
    t[has], tri[has] = ref["t"][ref["offsets"][:-1][has]], ref["tri"][ref["offsets"][:-1][has]]
    return t, tri


# ---- the ray families, with and without limits -----------------------------------------------------------------------------------
N_FAMILY = 600
VARIANTS = ("none", "at", "above", "half")


def with_limits(verts, o, d, seed):
    """(o, d, tmax, ref, picked) of the batch four times over (VARIANTS, in blocks of len(o)); picked[i] = the index, in ray i's unlimited
    list, of the hit whose t the limits are made of (-1: the ray hits nothing and its limits are 1)."""
    n = len(o)
    free = reference(verts, o, d)
    rng = np.random.default_rng(seed)
    picked = np.where(free["count"] > 0, (rng.random(n) * np.maximum(free["count"], 1)).astype(np.int64), -1)
    at = np.ones(n, f32)
    has = picked >= 0
    at[has] = free["t"][(free["offsets"][:-1] + picked)[has]]
    tmax = np.concatenate([np.full(n, INF, f32), at, np.nextafter(at, INF), (at * f32(0.5)).astype(f32)])
    o4, d4 = np.tile(o, (4, 1)), np.tile(d, (4, 1))
    ref = reference(verts, o4, d4, tmax)
    assert same_bits(ref["t"][:free["hits"]], free["t"]) and same_bits(ref["count"][:n], free["count"])
    return o4, d4, tmax, ref, picked


@functools.lru_cache(maxsize=None)
def family_case(name, n=N_FAMILY):
    """The parts of family `name` of tests/ray_exact.py: a list of dict(mesh, verts, o, d, tmax, ref, picked, n) (n = rays per variant)."""
    out = []
    for k, part in enumerate(RX.family(name, n)):
        verts = RX.mesh(part["mesh"])[0]
        o, d, tmax, ref, picked = with_limits(verts, part["o"], part["d"], 900 + 31 * RX.FAMILIES.index(name) + k)
        out.append(dict(mesh=part["mesh"], verts=verts, o=o, d=d, tmax=tmax, ref=ref, picked=picked, n=len(part["o"]), part=part))
    return out


@functools.lru_cache(maxsize=None)
def side_case(name):
    """tests/sign_exact.py's case on mesh `name` as rays: its points along D[0], D[1], D[2] (blocks of len(p)), no limit.
    dict(verts, o, d, ref, side): side = sign_exact's case, whose ref["brute"][:, k] are the counts of block k."""
    c = SX.case(name)
    p = c["p"]
    o = np.tile(p, (3, 1))
    d = np.repeat(SX.D, len(p), axis=0)
    return dict(verts=c["verts"], o=o, d=d, ref=reference(c["verts"], o, d), side=c, n=len(p))


# ---- the two meshes built for the lists ------------------------------------------------------------------------------------------
STACK_QUADS = 256


def stack_mesh():
    """256 parallel quads [-1, 1]^2 at z = 0.5 + 0.037 k (not binary fractions), two triangles each, diagonal x = y."""
    z = (0.5 + 0.037 * np.arange(STACK_QUADS)).astype(f32)
    quads = []
    for zk in z:
        p00, p10, p01, p11 = [-1, -1, zk], [1, -1, zk], [-1, 1, zk], [1, 1, zk]
        quads += [p00 + p10 + p11, p00 + p11 + p01]
    return np.ascontiguousarray(np.array(quads, f32).reshape(-1, 9))


@functools.lru_cache(maxsize=None)
def stack():
    """Rays through the stack: axis-parallel ones off the diagonal from both ends (the first is THE axis-offset ray: count 256,
    strictly ascending t), tilted ones, some with limits inside the stack, some that miss."""
    rng = np.random.default_rng(77)
    n = 96
    xy = rng.uniform(-0.9, 0.9, (n, 2))
    xy[np.abs(xy[:, 0] - xy[:, 1]) < 0.05, 0] += 0.1  # off the diagonal
    xy[0] = [0.3, 0.2]
    o = np.concatenate([xy, np.full((n, 1), -1.0)], 1)
    d = np.tile([0.0, 0.0, 1.0], (n, 1))
    back = slice(n // 3, 2 * n // 3)  # from behind the stack: the walk meets the hits in the other order
    o[back, 2], d[back, 2] = 12.0, -1.0
    tilt = slice(2 * n // 3, n)
    d[tilt, :2] = rng.uniform(-0.15, 0.15, (n - 2 * n // 3, 2))
    tmax = np.full(n, INF, f32)
    tmax[8:n // 3:3] = rng.uniform(1.5, 11.0, len(tmax[8:n // 3:3]))
    o[5], o[6] = [1.5, 0.2, -1.0], [0.1, -1.2, -1.0]  # beside the stack
    verts = stack_mesh()
    o, d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
    return dict(verts=verts, o=o, d=d, tmax=tmax, ref=reference(verts, o, d, tmax), n=n)


@functools.lru_cache(maxsize=None)
def duplicates():
    """The sphere of tests/sign_exact.py twice over (triangle i again as i + n): family a's points along D[0] and D[1]."""
    c = SX.case("sphere")
    verts = np.ascontiguousarray(np.concatenate([c["verts"], c["verts"]]))
    p = c["p"][c["rows"]["a"]]
    o = np.tile(p, (2, 1))
    d = np.repeat(SX.D[:2], len(p), axis=0)
    return dict(verts=verts, o=o, d=d, tmax=None, ref=reference(verts, o, d), n=len(o), half=len(c["verts"]))
