"""CPU tests of the reference that judges the device BVH build and refit (tests/native/lbvh_ref.cpp through tests/lbvh_exact.py): its trees
pass the structure check, the program is clean under AddressSanitizer + UBSan, its key order equals a numpy computation written
separately, small meshes give the trees worked out by hand below, its binary tree is a radix tree, its refit mode reproduces its own
build, and the comparison the GPU tests use sees single-byte changes.  No GPU."""
import numpy as np
import pytest

import lbvh_exact as LX

f32 = np.float32
CASE_IDS = [LX.case_id(c) for c in LX.CASES]


# ---- structure --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LX.CASES, ids=CASE_IDS)
def test_reference_tree_structure(case):
    verts, ref = LX.case(*case)
    depth = LX.check_tree(ref["nodes"], ref["leaf"], verts)
    levels = LX.level_ranges(ref["nodes"])
    assert ref["depth"] == depth == len(levels)
    assert ref["level_start"].tolist() == [a for a, _ in levels] + [ref["n_nodes"]]
    assert ref["n"] == len(verts) and len(ref["keys"]) == len(verts) and len(ref["binary"]) == len(verts) - 1
    assert np.array_equal(np.sort(ref["keys"] & np.uint64(0xFFFFFFFF)), np.arange(len(verts), dtype=np.uint64))
    if len(verts) <= 9:
        assert ref["n_nodes"] == (1 if len(verts) <= 8 else 2)


# ---- sanitizers -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in LX.CASES if c[1] <= LX.SANITIZED_MAX], ids=[LX.case_id(c) for c in LX.CASES if c[1] <= LX.SANITIZED_MAX])
def test_sanitized_reference_prints_the_same_bytes(case):
    verts, ref = LX.case(*case)
    assert LX.reference(verts, sanitized=True)["raw"] == ref["raw"]
    moved = LX.moved(verts, "offsets")
    assert LX.reference_refit(ref["nodes"], ref["leaf"], moved, sanitized=True)["raw"] == LX.reference_refit(ref["nodes"], ref["leaf"], moved)["raw"]


# ---- a second opinion on the order --------------------------------------------------------------------------------------------------------

SPREAD = np.array([int("".join(bit + "00" for bit in format(cell, "010b")), 2) for cell in range(1024)], np.uint64)  # bit b of a cell -> bit 3 b + 2


def numpy_keys(verts):
    """DESIGN.md section 6.9 (1)-(3) in numpy fp32: M, pad, padded boxes, centroids, cells, Morton code << 32 | index; unsorted."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)
    p0 = v[:, 0]
    p1, p2 = p0 + (v[:, 1] - p0), p0 + (v[:, 2] - p0)
    corners = np.stack([p0, p1, p2])
    maxabs = max(f32(np.abs(corners).max()), f32(1.0))
    pad = f32(2e-5) * maxabs
    lo, hi = corners.min(0) - pad, corners.max(0) + pad
    c = f32(0.5) * (lo + hi)
    assert c.dtype == f32 and pad.dtype == f32
    c_lo, c_hi = c.min(0), c.max(0)
    ext = c_hi - c_lo
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (c - c_lo) / ext * f32(1024.0)
    assert x.dtype == f32
    cell = np.where(ext > 0, np.minimum(np.maximum(x, f32(0.0)), f32(1023.0)), f32(0.0)).astype(np.uint32)
    morton = SPREAD[cell[:, 0]] | (SPREAD[cell[:, 1]] >> np.uint64(1)) | (SPREAD[cell[:, 2]] >> np.uint64(2))
    return (morton << np.uint64(32)) | np.arange(len(v), dtype=np.uint64), maxabs, pad


@pytest.mark.parametrize("case", LX.CASES, ids=CASE_IDS)
def test_sorted_keys_equal_a_numpy_computation(case):
    verts, ref = LX.case(*case)
    keys, maxabs, pad = numpy_keys(verts)
    assert ref["maxabs"] == maxabs and ref["pad"] == pad
    assert np.array_equal(np.sort(keys), ref["keys"])


def test_the_families_are_what_they_claim():
    """The properties the families exist for, on the keys: ties, skipped digits, a zero-extent axis, centroids at cell borders."""
    n = LX.FAMILY_SIZES[0]
    morton = lambda name: LX.case(name, n)[1]["keys"] >> np.uint64(32)  # noqa: E731
    assert len(np.unique(morton("identical"))) == 1
    two = np.unique(morton("two_clusters"), return_counts=True)
    assert two[0].tolist() == [0, (1 << 30) - 1] and two[1].tolist() == [n // 2, n - n // 2]
    shared = LX.case("shared_centroids", n)[1]["keys"]
    code, index = shared >> np.uint64(32), (shared & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ties = code[1:] == code[:-1]
    assert ties.sum() > n // 2, "Morton ties broken by the index"
    assert (ties & ((index[1:] // LX.K_SORT_TILE) != (index[:-1] // LX.K_SORT_TILE))).any(), "a tie whose two triangles lie in different sort tiles"
    assert not (morton("flat") & np.uint64(0x12492492)).any(), "the y bits of a flat mesh"
    verts = LX.case("grid", n)[0].reshape(-1, 3, 3)
    centre = 0.5 * (verts.min(1).astype(np.float64) + verts.max(1))
    assert np.abs(centre * 64 - np.round(centre * 64)).max() < 1e-9 and centre.min() == 0 and centre.max() == 16
    huge = LX.case("huge", n)[0]
    assert np.abs(huge).max() > 9e29
    with np.errstate(over="ignore"):
        ext = (huge.reshape(-1, 3, 3).max(1) - huge.reshape(-1, 3, 3).min(1)).astype(f32)
        assert np.isinf(ext[:, 0] * ext[:, 1]).all(), "fp32 areas overflow"


# ---- known answers, worked out by hand ----------------------------------------------------------------------------------------------------

def unit_triangle(x):
    """The triangle (x, 0, 0), (x + 1, 0, 0), (x, 1, 0)."""
    return [x, 0, 0, x + 1, 0, 0, x, 1, 0]


def slots_of(ref):
    """Per node: (imask, leafmask, {slot: ("leaf", triangle) or ("node", index)})."""
    out = []
    for w in ref["nodes"]:
        imask, leafmask = int(w[3] >> 24), int(w[6])
        slot, inner, leaves = {}, 0, 0
        for s in range(8):
            if (imask >> s) & 1:
                slot[s] = ("node", int(w[4]) + inner)
                inner += 1
            elif (leafmask >> s) & 1:
                slot[s] = ("leaf", int(ref["leaf"][int(w[5]) + leaves]))
                leaves += 1
        out.append((imask, leafmask, slot))
    return out


def test_known_answer_one_triangle():
    ref = LX.reference(np.array([unit_triangle(3.0)], f32))
    assert ref["n_nodes"] == 1 and ref["depth"] == 1 and ref["leaf"].tolist() == [0]
    assert slots_of(ref) == [(0x00, 0x01, {0: ("leaf", 0)})]  # every score is 0: the first slot
    assert ref["nodes"][0, 4:8].tolist() == [1, 0, 1, 0]


def test_known_answer_two_triangles():
    """Triangle 0 at x = 4, triangle 1 at x = 0: cells 1023 and 0 on x, so triangle 1 sorts first.  The root's children are (1, 0); their
    centres lie left and right of the node's on x and at it on y and z, so they score highest in slots 0-3 and 4-7: the first of each."""
    ref = LX.reference(np.array([unit_triangle(4.0), unit_triangle(0.0)], f32))
    assert (ref["keys"] >> np.uint64(32)).tolist() == [0, 0x24924924] and (ref["keys"] & np.uint64(0xFFFFFFFF)).tolist() == [1, 0]
    assert ref["n_nodes"] == 1 and ref["depth"] == 1 and ref["leaf"].tolist() == [1, 0]
    assert slots_of(ref) == [(0x00, 0x11, {0: ("leaf", 1), 4: ("leaf", 0)})]
    assert ref["binary"].tolist() == [[0, 1, 0]]


def test_known_answer_nine_triangles_on_the_x_axis():
    """Sorted position i = 0..8 holds triangle 8 - i, a unit triangle at x = 0, 2 + 1/128, 4 + 1/128, 6 + 3/256, 8 + 1/128, ..., 14 + 1/128, 16: the
    centroid bounds are 16 wide, so the x cells are 0, 128, 256, 384, 512, 640, 768, 896 (each from the middle of its cell) and 1023.
    Radix tree: root = (A = [0..3], B = [4..8]); A = ([0, 1], [2, 3]); B = ([4, 5], B1 = [6..8]); B1 = (6, C = [7, 8]).
    Collapse of the root, opening the widest entry (the area grows with the x extent here; no two are equal):
    (A 7.01, B 8.99) -> (A, [4,5], B1) -> ([0,1], [4,5], B1 4.99, [2,3]) -> ([0,1] 3.008, [4,5] 3.0, 6, [2,3] 3.004, C 2.99) -> (0, [4,5], 6, [2,3], C, 1)
    -> (0, [4,5], 6, 2, C, 1, 3) -> (0, 4, 6, 2, C, 1, 3, 5).  Only x separates the children; by distance from the node's centre 8.5:
    0 (-8) slot 0, C (+7) slot 4, 1 (-6) slot 1, 6 (+4) slot 5, 2 (-4) slot 2, 5 (+2) slot 6, 3 (-2) slot 3, 4 (+0.008) the last slot 7."""
    xs = [0.0, 2 + 1 / 128, 4 + 1 / 128, 6 + 3 / 256, 8 + 1 / 128, 10 + 1 / 128, 12 + 1 / 128, 14 + 1 / 128, 16.0]
    verts = np.array([unit_triangle(x) for x in reversed(xs)], f32)
    ref = LX.reference(verts)
    tri = lambda pos: 8 - pos  # noqa: E731
    assert (ref["keys"] & np.uint64(0xFFFFFFFF)).tolist() == [tri(i) for i in range(9)]
    x_cells = [0, 128, 256, 384, 512, 640, 768, 896, 1023]
    assert (ref["keys"] >> np.uint64(32)).tolist() == [int(SPREAD[c]) for c in x_cells]
    assert ref["binary"].tolist() == [[0, 8, 3], [0, 3, 1], [0, 1, 0], [2, 3, 2], [4, 8, 5], [4, 5, 4], [6, 8, 6], [7, 8, 7]]
    assert ref["n_nodes"] == 2 and ref["depth"] == 2 and ref["level_start"].tolist() == [0, 1, 2]
    assert ref["leaf"].tolist() == [tri(p) for p in (0, 1, 2, 3, 6, 5, 4, 7, 8)]
    root, second = slots_of(ref)
    assert root == (0x10, 0xEF, {0: ("leaf", tri(0)), 1: ("leaf", tri(1)), 2: ("leaf", tri(2)), 3: ("leaf", tri(3)), 4: ("node", 1), 5: ("leaf", tri(6)),
                                 6: ("leaf", tri(5)), 7: ("leaf", tri(4))})
    assert second == (0x00, 0x11, {0: ("leaf", tri(7)), 4: ("leaf", tri(8))})
    assert ref["nodes"][:, 4:8].tolist() == [[1, 0, 0xEF, 0], [2, 7, 0x11, 0]]


def test_known_answer_sixteen_triangles_at_the_corners_of_two_cubes():
    """Triangle o (0..7) sits at the corner of the inner cube (half edge 1 + 127/256) in octant o = 4 [x > 0] + 2 [y > 0] + [z > 0], triangle
    8 + o at the outer cube's (half edge 4); every box is its corner +- 1/4.  Centroid bounds [-4, 4]^3: cells 0 | 1023 outside, 320 | 703
    inside.  The top bit of every axis is the octant, the next bit is set for the inner triangle where the coordinate is negative and for
    the outer one where it is positive: the order is octant by octant, (outer, inner) for x < 0 and (inner, outer) for x > 0, and the
    radix tree is the complete binary tree over x, y, z with one pair node per octant.
    Collapse of the root: its two halves mirror each other, so their fp32 areas are EQUAL and the first (x < 0) is opened; then the
    half x > 0 (larger than the two quarters), then the four quarters, equal again, in array order: (000, 100, 010, 110, 001, 101,
    011, 111) as xyz.  The node's centre is the origin, so octant o scores highest in slot o alone: eight inner children, nodes 1 + o.
    In pair node o the outer triangle lies away from the origin, slot o, and the inner one towards it, slot 7 - o."""
    inner_c, outer_c, h = 1 + 127 / 256, 4.0, 0.25
    tris = []
    for t in range(16):
        o, c = t % 8, (inner_c if t < 8 else outer_c)
        corner = np.array([c if (o >> 2) & 1 else -c, c if (o >> 1) & 1 else -c, c if o & 1 else -c])
        tris.append(np.concatenate([corner - h, corner + h, corner + np.array([h, -h, h])]))
    verts = np.array(tris, f32)
    ref = LX.reference(verts)
    order = [8, 0, 9, 1, 10, 2, 11, 3, 4, 12, 5, 13, 6, 14, 7, 15]
    assert (ref["keys"] & np.uint64(0xFFFFFFFF)).tolist() == order
    assert ref["binary"].tolist() == [[0, 15, 7], [0, 7, 3], [0, 3, 1], [0, 1, 0], [2, 3, 2], [4, 7, 5], [4, 5, 4], [6, 7, 6],
                                      [8, 15, 11], [8, 11, 9], [8, 9, 8], [10, 11, 10], [12, 15, 13], [12, 13, 12], [14, 15, 14]]
    assert ref["n_nodes"] == 9 and ref["depth"] == 2 and ref["level_start"].tolist() == [0, 1, 9]
    assert ref["leaf"].tolist() == order
    nodes = slots_of(ref)
    assert nodes[0] == (0xFF, 0x00, {s: ("node", 1 + s) for s in range(8)})
    for o in range(8):
        assert nodes[1 + o] == ((0x00, (1 << o) | (1 << (7 - o)), {o: ("leaf", 8 + o), 7 - o: ("leaf", o)})), o
        assert ref["nodes"][1 + o, 4:8].tolist() == [9, 2 * o, (1 << o) | (1 << (7 - o)), 0]


# ---- the binary tree is a radix tree --------------------------------------------------------------------------------------------------------

def common_prefix(keys, i, j):
    """Length of the common prefix of keys[i] and keys[j] as 64-bit strings; 64 where i == j."""
    x = keys[i] ^ keys[j]
    out = np.full(len(x), 64, np.int64)
    nz = x != 0
    out[nz] = 63 - np.floor(np.log2(x[nz].astype(np.longdouble))).astype(np.int64)
    return out


@pytest.mark.parametrize("case", [c for c in LX.CASES if c[0] in ("random", "shared_centroids")],
                         ids=[LX.case_id(c) for c in LX.CASES if c[0] in ("random", "shared_centroids")])
def test_binary_tree_is_a_radix_tree(case):
    """Every internal node [a, b] with split s has the children [a, s] and [s + 1, b] (adjacent, covering it), each of them a leaf or a node
    of the tree, and each child's keys share a strictly longer prefix than the parent's."""
    _, ref = LX.case(*case)
    keys, n = ref["keys"], ref["n"]
    if n == 1:
        assert len(ref["binary"]) == 0
        return
    assert (keys[1:] > keys[:-1]).all()
    a, b, s = (ref["binary"][:, k].astype(np.int64) for k in range(3))
    assert (a[0], b[0]) == (0, n - 1) and ((a <= s) & (s < b)).all()
    ranges = set(zip(a.tolist(), b.tolist()))
    assert len(ranges) == n - 1
    parent = common_prefix(keys, a, b)
    assert (parent < 64).all()
    left, right = common_prefix(keys, a, s), common_prefix(keys, s + 1, b)
    assert (left > parent).all() and (right > parent).all()
    assert (common_prefix(keys, s, s + 1) == parent).all(), "the split is where the parent's prefix ends"
    for lo, hi in ((a, s), (s + 1, b)):
        inner = lo < hi
        assert all(r in ranges for r in zip(lo[inner].tolist(), hi[inner].tolist()))


def test_common_prefix_helper():
    keys = np.array([0, 1, 1 << 63, (1 << 63) | 5, (1 << 32) - 1, 1 << 32], np.uint64)
    i, j = np.array([0, 0, 2, 4, 1]), np.array([1, 2, 3, 5, 1])
    assert common_prefix(keys, i, j).tolist() == [63, 0, 61, 31, 64]


# ---- refit mode -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LX.CASES, ids=CASE_IDS)
def test_reference_refit_to_unchanged_vertices_reproduces_the_build(case):
    verts, ref = LX.case(*case)
    again = LX.reference_refit(ref["nodes"], ref["leaf"], verts)
    assert LX.difference(again["nodes"], again["leaf"], ref["nodes"], ref["leaf"]) is None
    assert again["nodes"].tobytes() == ref["nodes"].tobytes() and again["maxabs"] == ref["maxabs"] and again["pad"] == ref["pad"]


def test_reference_refit_after_motion_is_a_tight_valid_tree():
    """After a move the refitted reference tree keeps its topology, passes the structure check, and a fresh reference build of the moved
    mesh refitted to itself agrees with the fresh build: the refit mode computes what the build computes for the same topology."""
    verts, ref = LX.case("random", LX.K_SORT_TILE + 1)
    for motion in LX.MOTIONS:
        new = LX.moved(verts, motion)
        out = LX.reference_refit(ref["nodes"], ref["leaf"], new)
        assert np.array_equal(out["nodes"][:, 4:8], ref["nodes"][:, 4:8]) and np.array_equal(out["nodes"][:, 3] >> 24, ref["nodes"][:, 3] >> 24)
        LX.check_tree(out["nodes"], out["leaf"], new)
        assert (out["nodes"].tobytes() == ref["nodes"].tobytes()) == (motion == "back")


# ---- the comparison sees what it must -------------------------------------------------------------------------------------------------------

def test_difference_flags_single_changes():
    _, ref = LX.case("random", LX.K_SORT_TILE + 1)
    nodes, leaf = ref["nodes"], ref["leaf"]
    assert LX.difference(nodes.copy(), leaf.copy(), nodes, leaf) is None
    k = next(i for i in range(len(nodes) // 2, len(nodes)) if bin(int(nodes[i, 6])).count("1") >= 2)  # a node with two leaves
    level = next(j for j, (a, b) in enumerate(LX.level_ranges(nodes)) if a <= k < b)
    plane = nodes.copy()
    plane[k, 13] ^= np.uint32(1 << 16)  # one bit of one plane byte
    msg = LX.difference(plane, leaf, nodes, leaf)
    assert msg and f"first node {k} (level {level} " in msg and "word 13" in msg and "the leaf order is equal" in msg
    swapped = leaf.copy()
    at = int(nodes[k, 5])
    swapped[[at, at + 1]] = swapped[[at + 1, at]]
    msg = LX.difference(nodes, swapped, nodes, leaf)
    assert msg and "all node words are equal" in msg and f"first position {at} " in msg and f"in node {k} " in msg and "the leaf order differs first" in msg
    # two occupied slots of one node exchanged: masks and tri_base stay, twelve plane bytes move
    leafmask = int(nodes[k, 6]) | int(nodes[k, 3] >> 24)
    s0, s1 = [s for s in range(8) if (leafmask >> s) & 1][:2]
    slots = nodes.copy()
    q = slots[k, 8:20].view(np.uint8).reshape(6, 8)
    q[:, [s0, s1]] = q[:, [s1, s0]]
    slots[k, 8:20] = q.reshape(-1).view(np.uint32)
    assert not np.array_equal(slots[k], nodes[k])
    msg = LX.difference(slots, leaf, nodes, leaf)
    assert msg and f"first node {k} " in msg and "1 of" in msg
    both = LX.difference(slots, swapped, nodes, leaf)
    assert both and "the leaf order differs first" not in both and "the node words differ first" in both  # same node: the words are named
    assert LX.difference(nodes[:-1], leaf, nodes, leaf) is not None
