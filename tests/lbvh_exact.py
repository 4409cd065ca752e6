"""Reference of path B's device BVH build and refit (DESIGN.md sections 6.9 and 6.10), the meshes that probe them, and the comparison.

Test helper (imported by tests/test_lbvh_ref_host.py, tests/test_gpu_device_bvh_exact.py and tests/test_gpu_device_bvh.py); a sibling of
tests/neighbor_exact.py; not a conftest, no fixtures.

THE REFERENCE is tests/native/lbvh_ref.cpp: section 6.9 restated on the CPU (std::sort, a top-down recursion on the highest differing
key bit, recursive unions, a queue) and, in its second mode, section 6.10 on the topology of an existing tree.  The build is a
deterministic function of the mesh, so rt_read_bvh of a device-built tree must equal the reference BYTE FOR BYTE: there is no tolerance.

THE SIZES are the smallest triangle counts at which a mechanism of csrc/bvh_build_gpu.hip changes behaviour (SIZES, each beside its
constant), THE FAMILIES the meshes whose keys stress the sort, the tie breaks and the quantiser (FAMILIES); all seeded."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from raytracing_engine_amd import scenes  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402

f32 = np.float32
NODE_WORDS = 20

# constants of csrc/bvh_build_gpu.hip that the sizes below are derived from
K_THREADS = 256            # kThreads: one workgroup round of a sort tile, one reduction block
K_SORT_TILE = 4096         # kSortTile = kScanTile = 16 * kThreads: keys per workgroup of a radix pass, elements per scan tile
K_TOP_LEVEL_NODES = 4096   # kTopLevelNodes: segment-tree levels of at most this many nodes are built by bvhd_box_top
K_REFIT_TOP_NODES = 1024   # kRefitTopNodes: tree levels of at most this many nodes are refitted by bvhr_top
K_REFIT_TOP_MAX = 16       # kRefitTopMax: bvhr_top takes at most this many levels

SIZES = (
    1, 2, 8, 9,                                            # single-node and two-node trees
    K_THREADS - 1, K_THREADS, K_THREADS + 1,               # one round of a sort tile; one reduction block and the second
    K_SORT_TILE - 1, K_SORT_TILE, K_SORT_TILE + 1,         # the second sort tile; tail lanes of the last round
    2 * K_TOP_LEVEL_NODES, 2 * K_TOP_LEVEL_NODES + 1, 2 * K_TOP_LEVEL_NODES + 2, 3 * K_TOP_LEVEL_NODES + 1,
    # ^ n - 1 >= 2 * kTopLevelNodes: the first segment-tree level (nodes [8192, n)) that bvhd_box_level builds and bvhd_box_top does not,
    #   with one, two, three and 4097 nodes in it: n is no power of two
    16 * K_SORT_TILE, 16 * K_SORT_TILE + 1,                # 16 and 17 sort tiles: 256 * 17 histogram entries exceed one scan tile (kScanTile)
    300_000,                                               # collapse levels above kScanTile nodes (several scan tiles, several 1024-element
                                                           # chunks per tile); refit levels above and below kRefitTopNodes
)
FAMILY_SIZES = (K_SORT_TILE + 1, 16 * K_SORT_TILE + 1)
SANITIZED_MAX = 2 * K_TOP_LEVEL_NODES + 2  # the sanitized reference runs on every case of at most this many triangles


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/lbvh_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("lbvh_ref", (), sanitized, where, flags=("-Wall", "-Wextra", "-Werror"))


def _parse(raw):
    head, out = NR.unpack(raw, 6, lambda h: (("scale", f32, 2), ("keys", np.uint64, h[4]), ("nodes", np.uint32, h[1] * NODE_WORDS), ("leaf", np.uint32, h[0]),
                                             ("level_start", np.uint32, h[3]), ("binary", np.uint32, 3 * h[5])))
    n, nn, depth = head[:3]
    maxabs, pad = out.pop("scale")
    return dict(out, n=n, n_nodes=nn, depth=depth, maxabs=f32(maxabs), pad=f32(pad), raw=raw, nodes=out["nodes"].reshape(nn, NODE_WORDS), binary=out["binary"].reshape(head[5], 3))


def reference(verts, sanitized=False):
    """The reference build of mesh `verts` (n x 9).  Returns a dict: n, n_nodes, depth, maxabs (M), pad, keys (uint64, sorted), nodes
    (uint32, n_nodes x 20), leaf (uint32), level_start (uint32, depth + 1), binary (uint32, (n - 1) x 3: first, last and split position of
    every internal node of the radix tree, in preorder) and raw, the program's output file."""
    return _parse(NR.run(build_reference(sanitized), dict(mode="build", mesh=np.asarray(verts, f32))))


def topology_of(nodes):
    """What the refit keeps of a tree: the imask byte of word 3 and words 4-7; every other word is zeroed."""
    topo = np.zeros_like(np.ascontiguousarray(nodes, np.uint32))
    topo[:, 3] = nodes[:, 3] & np.uint32(0xFF000000)
    topo[:, 4:8] = nodes[:, 4:8]
    return topo


def reference_refit(nodes, leaf, verts, sanitized=False):
    """The reference refit of the tree (nodes, leaf), as rt_read_bvh returned it BEFORE the refit, to the vertices `verts`: only the
    topology (topology_of) reaches the program.  Returns reference()'s dict without keys, level starts and the binary tree."""
    return _parse(NR.run(build_reference(sanitized), dict(mode="refit", topo=topology_of(nodes), leaf=np.asarray(leaf, np.uint32), mesh=np.asarray(verts, f32))))


# ---- the structure check (the array part of test_gpu_device_bvh.check_bvh) ------------------------------------------------------------
def level_ranges(nodes):
    """[first, last) of every level of a breadth-first tree, from the node words alone."""
    slots = np.arange(8, dtype=np.uint32)
    n_in = (((nodes[:, 3] >> 24)[:, None] >> slots) & 1).sum(1)
    levels, first, count = [], 0, 1
    while count:
        levels.append((first, first + count))
        nxt = int(n_in[first:first + count].sum())
        first, count = first + count, nxt
    return levels


def check_tree(nodes, leaf, verts):
    """Structural invariants of a tree (layout: raytracing_engine_amd/csrc/bvh_node.h): permutation, indexing, breadth-first order,
    inverted empty slots, containment along every root path.  Returns its depth."""
    verts = np.ascontiguousarray(verts, f32).reshape(-1, 9)
    n = len(verts)
    nn = len(nodes)
    assert nn >= 1 and len(leaf) == n
    assert np.array_equal(np.sort(leaf), np.arange(n, dtype=np.uint32)), "leaf order is not a permutation"
    w3 = nodes[:, 3]
    imask, leafmask = (w3 >> 24) & 0xFF, nodes[:, 6]
    assert (nodes[:, 7] == 0).all() and (leafmask <= 0xFF).all() and ((leafmask & imask) == 0).all()
    slots = np.arange(8, dtype=np.uint32)
    inner = ((imask[:, None] >> slots) & 1).astype(bool)
    leafs = ((leafmask[:, None] >> slots) & 1).astype(bool)
    n_in, n_lf = inner.sum(1), leafs.sum(1)
    child_base, tri_base = nodes[:, 4].astype(np.int64), nodes[:, 5].astype(np.int64)
    # breadth-first order: the inner children of node k follow those of nodes 0..k-1, its leaf triangles likewise;
    # with the counts below every node but the root is some node's child exactly once and every leaf position is used once
    assert np.array_equal(child_base, 1 + np.concatenate([[0], np.cumsum(n_in)[:-1]])), "child indexing / breadth-first order"
    assert np.array_equal(tri_base, np.concatenate([[0], np.cumsum(n_lf)[:-1]])), "leaf indexing"
    assert n_in.sum() == nn - 1 and n_lf.sum() == n
    q = np.ascontiguousarray(nodes[:, 8:20]).view(np.uint8).reshape(nn, 6, 8)
    qlo, qhi = q[:, :3, :].transpose(0, 2, 1), q[:, 3:, :].transpose(0, 2, 1)  # (nodes, slot, axis)
    empty = ~(inner | leafs)
    assert (qlo[empty] == 255).all() and (qhi[empty] == 0).all(), "empty slot without an inverted box"
    p = np.ascontiguousarray(nodes[:, :3]).view(f32)
    scale = ((np.stack([(w3 >> (8 * a)) & 0xFF for a in range(3)], 1).astype(np.uint32)) << np.uint32(23)).view(f32)
    lo = p[:, None, :] + qlo.astype(f32) * scale[:, None, :]  # fp32, as the kernels de-quantise
    hi = p[:, None, :] + qhi.astype(f32) * scale[:, None, :]
    assert lo.dtype == f32
    v0 = verts[:, 0:3]
    x1, x2 = v0 + (verts[:, 3:6] - v0), v0 + (verts[:, 6:9] - v0)
    tmin, tmax = np.minimum(np.minimum(v0, x1), x2), np.maximum(np.maximum(v0, x1), x2)
    rank_in = np.cumsum(inner, 1) - inner
    rank_lf = np.cumsum(leafs, 1) - leafs
    levels, first, count = [], 0, 1
    while count:  # breadth-first numbering: every level is a contiguous index range
        levels.append((first, first + count))
        nxt = int(n_in[first:first + count].sum())
        first, count = first + count, nxt
    assert first == nn
    sub_lo = np.full((nn, 3), np.inf, f32)
    sub_hi = np.full((nn, 3), -np.inf, f32)
    for a, b in reversed(levels):  # bottom-up: every slot's box holds every triangle below it
        ks = slice(a, b)
        li = np.where(leafs[ks], tri_base[ks, None] + rank_lf[ks], 0)
        ch = np.where(inner[ks], child_base[ks, None] + rank_in[ks], 0)
        tri = leaf[li]
        slo = np.where(leafs[ks][..., None], tmin[tri], np.where(inner[ks][..., None], sub_lo[ch], np.inf)).astype(f32)
        shi = np.where(leafs[ks][..., None], tmax[tri], np.where(inner[ks][..., None], sub_hi[ch], -np.inf)).astype(f32)
        occ = ~empty[ks]
        assert (lo[ks][occ] <= slo[occ]).all() and (hi[ks][occ] >= shi[occ]).all(), "a triangle lies outside a box on its root path"
        sub_lo[ks] = slo.min(1)
        sub_hi[ks] = shi.max(1)
    return len(levels)


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
WORD_NAMES = ("origin x", "origin y", "origin z", "exponent bytes | imask", "child_base", "tri_base", "leafmask", "reserved") + tuple(
    f"{side} planes {axis}, slots {half}" for side in ("lower", "upper") for axis in "xyz" for half in ("0-3", "4-7"))


def difference(nodes, leaf, want_nodes, want_leaf):
    """None if the tree (nodes, leaf) equals the expected one byte for byte; otherwise a message that names the first differing node, its
    level and word, the first differing leaf position with the node that holds it, and which of the two comes first in node order."""
    nodes, leaf = np.ascontiguousarray(nodes, np.uint32), np.ascontiguousarray(leaf, np.uint32)
    want_nodes, want_leaf = np.ascontiguousarray(want_nodes, np.uint32), np.ascontiguousarray(want_leaf, np.uint32)
    if nodes.ndim != 2 or nodes.shape[1] != NODE_WORDS or leaf.shape != want_leaf.shape:
        return f"node words of shape {nodes.shape} and {len(leaf)} leaves, expected {want_nodes.shape} and {len(want_leaf)}"
    if nodes.shape == want_nodes.shape and nodes.tobytes() == want_nodes.tobytes() and leaf.tobytes() == want_leaf.tobytes():
        return None
    levels = level_ranges(want_nodes)
    level_of = lambda k: next((j for j, (a, b) in enumerate(levels) if a <= k < b), -1)  # noqa: E731
    tri_base = want_nodes[:, 5].astype(np.int64)  # expected: non-decreasing in node order
    parts = []
    if len(nodes) != len(want_nodes):  # the common part is still compared: where the trees part says more than that they do
        parts.append(f"{len(nodes)} nodes, expected {len(want_nodes)}")
        nodes, want_nodes = nodes[:len(want_nodes)], want_nodes[:len(nodes)]
    bad_nodes = np.flatnonzero((nodes != want_nodes).any(1))
    bad_leaf = np.flatnonzero(leaf != want_leaf)
    node_first = int(bad_nodes[0]) if len(bad_nodes) else None
    if node_first is not None:
        word = int(np.flatnonzero(nodes[node_first] != want_nodes[node_first])[0])
        parts.append(f"{len(bad_nodes)} of {len(nodes)} nodes differ, first node {node_first} (level {level_of(node_first)} of {len(levels)}), word {word} "
                     f"({WORD_NAMES[word]}): 0x{int(nodes[node_first, word]):08x}, expected 0x{int(want_nodes[node_first, word]):08x}")
    else:
        parts.append("all node words are equal")
    if len(bad_leaf):
        at = int(bad_leaf[0])
        holder = int(np.searchsorted(tri_base, at, side="right") - 1)
        parts.append(f"{len(bad_leaf)} of {len(leaf)} leaf positions differ, first position {at} (triangle {int(leaf[at])}, expected {int(want_leaf[at])}) in "
                     f"node {holder} (level {level_of(holder)})")
        parts.append("the leaf order differs first" if node_first is None or holder < node_first else "the node words differ first")
    else:
        parts.append("the leaf order is equal")
    return "; ".join(parts)


# ---- the meshes -----------------------------------------------------------------------------------------------------------------------
def random_mesh(n):
    """The generator of test_gpu_device_bvh.test_device_tree_structure."""
    rng = np.random.default_rng(n)
    return (rng.uniform(-8, 8, size=(n, 1, 3)) + rng.uniform(-0.7, 0.7, size=(n, 3, 3))).astype(f32).reshape(n, 9)


def _around(centre, half, rng):
    """Triangles whose boxes are [centre - half, centre + half] (fp32): two vertices at opposite corners, the third anywhere inside."""
    centre, half = np.asarray(centre, f32), np.asarray(half, f32)
    n = len(centre)
    sign = np.where(rng.integers(0, 2, size=(n, 3)) == 1, f32(1), f32(-1)).astype(f32)
    p0, p1 = centre - sign * half, centre + sign * half
    p2 = (centre + half * rng.uniform(-1, 1, size=(n, 3)).astype(f32)).astype(f32)
    p2 = np.minimum(np.maximum(p2, np.minimum(p0, p1)), np.maximum(p0, p1))
    tri = np.stack([p0, p1, p2], 1).astype(f32)
    order = rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)  # which vertex comes first differs from triangle to triangle
    return np.take_along_axis(tri, order[:, :, None], 1).reshape(n, 9)


def family(name, n):
    """Mesh `name` of n triangles (n x 9 float32), seeded by (name, n)."""
    rng = np.random.default_rng([FAMILIES.index(name), n])
    if name == "random":
        return random_mesh(n)
    if name == "identical":  # all Morton codes equal: the order is the index word's, every Morton digit is skipped
        return np.tile(np.array([[-1, 5, -1, 1, 5, -1, 0, 6, 1]], f32), (n, 1))
    if name == "two_clusters":  # two centroids = the two corners of the bounds: Morton codes 0 and 2^30 - 1; the index digits above n are skipped
        a = np.array([-5, -3, -4, -4.5, -3, -4, -5, -2.5, -3.5], f32)
        b = np.array([5, 3, 4, 4.5, 3, 4, 5, 2.5, 3.5], f32)
        return np.where((rng.permutation(n) < n // 2)[:, None], a, b).astype(f32)
    if name == "shared_centroids":  # groups of 2-40 different triangles around one centre, scattered over the index range
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.integers(2, 41)))
        sizes[-1] -= sum(sizes) - n
        group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        centre = (rng.integers(-512, 513, size=(len(sizes), 3)) / 64.0).astype(f32)  # dyadic: centre +- half is exact
        half = (rng.integers(1, 65, size=(n, 3)) / 128.0).astype(f32)
        return _around(centre[group], half, rng)
    if name == "flat":  # every vertex on the plane y = 2: a zero-extent axis
        v = rng.uniform(-10, 10, size=(n, 9)).astype(f32)
        v[:, 1::3] = 2.0
        return v
    if name == "grid":  # box centroids on the cell borders k / 1024 of the centroid bounds [0, 16]^3 (to within the rounding of the padding)
        k = rng.integers(0, 1025, size=(n, 3))
        k[0], k[-1] = 0, 1024
        half = (rng.integers(1, 9, size=(n, 3)) / 256.0).astype(f32)
        return _around((k / 64.0).astype(f32), half, rng)
    if name == "mixed_scale":  # tiny triangles near the origin and huge ones far away
        small = rng.uniform(-1e-3, 1e-3, size=(n // 2, 9)).astype(f32)
        big = rng.uniform(-1e4, 1e4, size=(n - n // 2, 9)).astype(f32)
        return np.concatenate([small, big])
    if name == "huge":  # coordinates up to 1e30: every fp32 half_area is +inf, the collapse is decided by its tie break alone
        c = rng.uniform(-0.98e30, 0.98e30, size=(n, 1, 3))
        return (c + rng.uniform(-1e28, 1e28, size=(n, 3, 3))).astype(f32).reshape(n, 9)
    if name == "deep":
        return np.ascontiguousarray(scenes.deep_scene()[0], f32).reshape(-1, 9)
    raise ValueError(name)


FAMILIES = ("random", "identical", "two_clusters", "shared_centroids", "flat", "grid", "mixed_scale", "huge", "deep")
DEEP_TRIS = 48 * 24 + 4  # scenes.deep_scene()
CASES = tuple(("random", n) for n in SIZES) + tuple((name, n) for name in FAMILIES[1:-1] for n in FAMILY_SIZES) + (("deep", DEEP_TRIS),)


def case_id(case):
    return f"{case[0]}-{case[1]}"


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(verts, reference(verts)) of one case; computed once per process and shared: do not write to it."""
    verts = family(name, n)
    assert verts.shape == (n, 9) and verts.dtype == f32
    verts.setflags(write=False)
    return verts, reference(verts)


# ---- motions for the refit --------------------------------------------------------------------------------------------------------------
MOTIONS = ("offsets", "scale_7.5", "scale_0.3", "scale_0.01", "one_point", "back")


def moved(verts, motion):
    """The vertices `verts` after `motion`: per-triangle rigid offsets of about 2.0, a uniform scale, every vertex at one point, or unchanged."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
    if motion == "offsets":
        off = np.random.default_rng(3).normal(size=(len(v), 1, 3)).astype(f32) * f32(2.0)
        return (v + off).astype(f32).reshape(-1, 9)
    if motion.startswith("scale_"):
        return (v * f32(float(motion[6:]))).astype(f32).reshape(-1, 9)
    if motion == "one_point":
        return np.broadcast_to(np.array([0.25, -3.0, 1.5], f32), v.shape).astype(f32).reshape(-1, 9).copy()
    if motion == "back":
        return v.reshape(-1, 9).copy()
    raise ValueError(motion)
