"""Reference of path B's overlap segments and the float64 contract it is held to.

Test helper (imported by tests/test_overlap_segment_host.py and tests/test_gpu_overlap_segments.py); a sibling of tests/overlap_exact.py,
whose meshes, query families and list reference it uses; not a conftest, no fixtures.

THE REFERENCE is tests/native/overlap_segment_ref.cpp: brute force over all pairs through csrc/tri_overlap.h (which pairs are listed) and
csrc/tri_section.h (the segment, `ends` and the fifteen pair lengths d2 of each listed pair): the definition, no tree, no GPU.

THE FLOAT64 REFERENCE (segment64) shares no code and no formula with the header: the interval method in numpy float64 on the fp32
inputs.  The line where the two planes meet; each triangle's interval on it, from the signed distances of its vertices to the other
triangle's plane; the two ends of the intersection of the two intervals are the reference endpoints.

THE CONTRACT.  The checked class is the entries whose mask has exactly two bits, both with low > M, and whose four other tests have
low < -M or det == 0 (low and M = 2^-21 are overlap_exact's): the pairs whose intersection is, by float64, a segment between exactly
those two edges.  For such an entry err = the larger of the two endpoint distances (endpoints matched as unordered pairs) divided by
S = the largest |coordinate| among A0, A1, A2, v0, fl(v0 + e1), fl(v0 + e2).
    E_measured = the largest err over every checked entry of families a, b, c, d on every mesh, on still and on moved vertices:
        measured 2.90e-05 (one entry of family b on the moved terrain, whose triangles no longer share their vertices: two former
        neighbours 0.03 % of an edge inside each other, their planes almost parallel, so the place of the cut is ill-conditioned; on
        still vertices the largest is 4.56e-07, family d on the soup cut; python tests/section_exact.py)
    E = 16 x that, the KP convention of tests/point_exact.py, rounded up to a power of two:  E = 2^-11 = 4.88e-04
    (A triangle without area - the needle mesh's collinear one, normal exactly 0 in float64 - has no plane: segment64 takes it as the
    segment it is and answers where it crosses the other triangle's plane, both ends that point.)
    The checked class covers 1 373 of the 1 375 entries of families a, c and d on still vertices (a: 141 of 143, the two left out are
    one-bit entries on the needle mesh; c: 959 of 959; d: 273 of 273); at least 99 % is asserted.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import overlap_exact as OX  # noqa: E402

ROOT = OX.ROOT
f32 = np.float32
E_MEASURED = 2.90e-05
E = 2.0 ** -11
CHECKED_FAMILIES = ("a", "b", "c", "d")
COVERED_FAMILIES = ("a", "c", "d")
PAIRS = [(b, c) for b in range(6) for c in range(b + 1, 6)]  # the order of the native program's d2 columns


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/overlap_segment_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("overlap_segment_ref", (), sanitized, where)


def reference(verts, q, pairs=None, sanitized=False):
    """The native reference on mesh `verts` and query triangles q (n, 9).  Returns a dict: count (int32; INVALID for an invalid query),
    offsets (int64, n + 1), tri, mask, ends (int32 per entry of the brute-force list), seg (entries, 2, 3) float32, d2 (entries, 15)
    float32 (PAIRS order, NaN where a bit of the pair is clear), entries, invalid; with pairs ((k, 2) int32: query, triangle):
    pair_mask, pair_seg, pair_ends of those pairs, listed or not."""
    q = np.ascontiguousarray(q, f32).reshape(-1, 9)
    n = len(q)
    inputs = dict(mesh=np.asarray(verts, f32), queries=q, out=NR.OUT)
    if pairs is not None:
        inputs["pairs"] = np.asarray(pairs, np.int32).reshape(-1, 2)
    head, out = NR.unpack(NR.run(build_reference(sanitized), inputs), 4,
                          lambda h: (("count", np.int32, n), ("offsets", np.int64, n + 1), ("tri", np.int32, h[1]), ("mask", np.int32, h[1]), ("seg", f32, 6 * h[1]),
                                     ("ends", np.int32, h[1]), ("d2", f32, 15 * h[1]), ("pair_mask", np.int32, h[3]), ("pair_seg", f32, 6 * h[3]), ("pair_ends", np.int32, h[3])))
    assert head[0] == n
    k, npairs = head[1], head[3]
    out["seg"], out["d2"], out["pair_seg"] = out["seg"].reshape(k, 2, 3), out["d2"].reshape(k, 15), out["pair_seg"].reshape(npairs, 2, 3)
    return dict(out, entries=k, invalid=head[2])


@functools.lru_cache(maxsize=None)
def family_case(name, moved=False):
    """overlap_exact.family_case(name, moved) with each part's segment reference beside its list reference: dict(mesh, verts, q, ref, sref)."""
    return [dict(c, sref=reference(c["verts"], c["q"])) for c in OX.family_case(name, moved)]


def owners(offsets):
    """The query triangle of each entry of a list with these offsets."""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def same_bits(a, b):
    """Two float32 arrays agree bit for bit (NaNs included)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the float64 reference: the interval method -------------------------------------------------------------------------------------
def _plane_crossings(p, dist):
    """Where the edges of the triangles p (k, 3, 3) cross the plane their vertices have the signed distances dist (k, 3) to: (k, 3, 3)
    points, NaN for an edge that does not cross."""
    out = np.full(p.shape, np.nan)
    for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        di, dj = dist[:, i], dist[:, j]
        crosses = (di * dj <= 0) & (di != dj)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(crosses, di / np.where(crosses, di - dj, 1.0), np.nan)
        out[:, e] = p[:, i] + s[:, None] * (p[:, j] - p[:, i])
    return out


def segment64(verts, q, pair_q, pair_t):
    """(k, 2, 3) float64: the intersection segment of query triangle pair_q[k] and mesh triangle pair_t[k] (NaN where the planes are
    parallel or the intervals do not meet), on the fp32 query vertices and the fp32 record words v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)[pair_t]
    v0 = v[:, 0].astype(np.float64)
    b = np.stack([v0, v0 + (v[:, 1] - v[:, 0]).astype(f32), v0 + (v[:, 2] - v[:, 0]).astype(f32)], 1)  # the triangle the records describe
    a = np.ascontiguousarray(q, f32).reshape(-1, 3, 3)[pair_q].astype(np.float64)
    na, nb = np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]), np.cross(b[:, 1] - b[:, 0], b[:, 2] - b[:, 0])
    line = np.cross(na, nb)  # the direction of the line where the planes meet
    dist_a = ((a - b[:, :1]) * nb[:, None]).sum(2)  # of A's vertices to B's plane (scaled by |nb|)
    dist_b = ((b - a[:, :1]) * na[:, None]).sum(2)
    pts = np.concatenate([_plane_crossings(a, dist_a), _plane_crossings(b, dist_b)], 1)  # (k, 6, 3): points on the line
    along = (pts * line[:, None]).sum(2)
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        lo_a, hi_a = np.nanmin(along[:, :3], 1), np.nanmax(along[:, :3], 1)
        lo_b, hi_b = np.nanmin(along[:, 3:], 1), np.nanmax(along[:, 3:], 1)
        lo, hi = np.maximum(lo_a, lo_b), np.minimum(hi_a, hi_b)
        meet = (lo <= hi) & ((line * line).sum(1) > 0)
    out = np.full((len(a), 2, 3), np.nan)
    for k in np.nonzero(meet)[0]:  # the points that realise the two ends
        out[k, 0] = pts[k, np.nanargmin(np.abs(along[k] - lo[k]))]
        out[k, 1] = pts[k, np.nanargmin(np.abs(along[k] - hi[k]))]
    # A triangle without area (a normal of exactly 0 in float64: the needle mesh's collinear one) has no plane and is a segment; where
    # the other triangle has a plane, the answer is where that segment crosses it, ordered along the segment's longest edge
    for tri, other_n, first in ((b, na, 3), (a, nb, 0)):
        n2 = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1)
        for k in np.nonzero((n2 == 0) & ((other_n * other_n).sum(1) > 0))[0]:
            cross = pts[k, first:first + 3]
            edges = tri[k, [1, 2, 0]] - tri[k]
            s = (cross * edges[np.argmax((edges ** 2).sum(1))]).sum(1)
            if not np.isnan(s).all():
                out[k, 0], out[k, 1] = cross[np.nanargmin(s)], cross[np.nanargmax(s)]
    return out


def scale_of(verts, q, pair_q, pair_t):
    """S: the largest |coordinate| among A0, A1, A2, v0, fl(v0 + e1), fl(v0 + e2) of each pair."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3, 3)[pair_t]
    v0 = v[:, 0]
    b = np.stack([v0, (v0 + (v[:, 1] - v0).astype(f32)).astype(f32), (v0 + (v[:, 2] - v0).astype(f32)).astype(f32)], 1)
    a = np.ascontiguousarray(q, f32).reshape(-1, 3, 3)[pair_q]
    return np.maximum(np.abs(a).reshape(len(a), 9).max(1), np.abs(b).reshape(len(b), 9).max(1)).astype(np.float64)


def checked_class(lows, masks, m=OX.M):
    """Which entries are in the checked class: exactly two bits, both with low > m, the four other tests low < -m or det == 0 (low NaN)."""
    bits = ((np.asarray(masks)[:, None] >> np.arange(6)) & 1).astype(bool)
    with np.errstate(invalid="ignore"):
        good = np.where(bits, lows > m, (lows < -m) | np.isnan(lows))
    return (bits.sum(1) == 2) & good.all(1)


def errors(verts, q, sref):
    """(checked, err): the checked class of the reference's entries and, for each entry, the larger endpoint distance to the float64
    segment over S, endpoints matched as unordered pairs."""
    pq, pt = owners(sref["offsets"]), sref["tri"]
    checked = checked_class(OX.pair_lows(verts, q, pq, pt), sref["mask"])
    want = segment64(verts, q, pq, pt)
    got = sref["seg"].astype(np.float64)

    def dist(x, y):
        return np.sqrt(((x - y) ** 2).sum(-1))

    with np.errstate(invalid="ignore"):
        straight = np.maximum(dist(got[:, 0], want[:, 0]), dist(got[:, 1], want[:, 1]))
        crossed = np.maximum(dist(got[:, 0], want[:, 1]), dist(got[:, 1], want[:, 0]))
        err = np.fmin(straight, crossed) / scale_of(verts, q, pq, pt)
    return checked, np.where(np.isnan(err), np.inf, err)  # no float64 segment: never within a bound


def measure(out=sys.stdout):
    """E_measured and the checked-class share, family by family."""
    worst = (0.0, None)
    covered = [0, 0]
    for moved in (False, True):
        for name in CHECKED_FAMILIES:
            for c in family_case(name, moved):
                checked, err = errors(c["verts"], c["q"], c["sref"])
                w = float(err[checked].max()) if checked.any() else 0.0
                nbits = np.array([bin(int(x)).count("1") for x in c["sref"]["mask"]], np.int64)
                print(f"family {name} {c['mesh']:10s} {'moved' if moved else 'still'}: {len(err):5d} entries, {int(checked.sum()):5d} checked, "
                      f"{int((nbits == 1).sum()):4d} one-bit, {int((nbits >= 3).sum()):3d} three-bit, largest err checked {w:.3g}, "
                      f"all set bits {float(err[np.isfinite(err)].max()) if np.isfinite(err).any() else 0.0:.3g}", file=out, flush=True)
                if w > worst[0]:
                    worst = (w, (name, c["mesh"], "moved" if moved else "still"))
                if name in COVERED_FAMILIES and not moved:
                    covered[0] += int(checked.sum())
                    covered[1] += len(err)
    print(f"E_measured = {worst[0]:.3g} {worst[1]} -> E = 2^{int(np.ceil(np.log2(16 * worst[0]))) if worst[0] else 0}; "
          f"checked class covers {covered[0]} of {covered[1]} entries of families {', '.join(COVERED_FAMILIES)} (still)", file=out)
    return worst, covered


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure()
