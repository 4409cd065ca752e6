"""The nine query kinds of one context side by side (csrc/rt_abi_query.hip, rt::Queries in csrc/rt_internal.h): each kind's counters
reach the members of its own public struct that they belong in, and they stay until the kind's statistics are read, whatever the
other kinds do meanwhile.

The mesh is a closed tetrahedron around the origin, so that what a query finds follows from the geometry and not from a reference
implementation.  Kind j of eight (rays 1, closest points 2, sides 3, all hits 4, neighbours 5, overlaps 6, clearance 7, k nearest 8)
gets a batch of its own of 3 + j items: three valid ones and j with a NaN component, so that no two kinds have the same number of
items or of invalid ones; the ninth kind, the overlap segments, runs on the overlaps' list.  All nine are issued back to back and
their statistics are read in the reverse order, each twice."""
import numpy as np
import pytest

from gpu_query import set_mesh_px_surface, tdev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID = -2  # RT_RAY_INVALID = RT_POINT_INVALID
V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], f32)  # the centroid is the origin, the inscribed sphere's radius 1 / sqrt(3)
TETRAHEDRON = np.array([[V[0], V[1], V[2]], [V[0], V[3], V[1]], [V[0], V[2], V[3]], [V[1], V[3], V[2]]], f32).reshape(4, 9)
# outside, and the line from each through the origin passes through no edge (no two of its coordinates agree in magnitude)
OUTSIDE = np.array([[3.1, 0.7, -0.4], [-0.9, 2.8, 0.35], [0.45, -0.6, -3.3]], f32)
# near the centroid: every face is nearer than 1
INSIDE = np.array([[0.0, 0.0, 0.0], [0.05, -0.1, 0.02], [-0.07, 0.03, 0.11]], f32)
# z is +1 at two vertices and -1 at the other two, so a plane of small constant z cuts all four faces; these triangles cover the cut
SLICES = np.array([[[-9, -8, z], [9, -8, z], [0.5, 9, z]] for z in (0.1, 0.2, -0.15)], f32).reshape(3, 9)
# far from the mesh
AWAY = SLICES + np.tile(np.array([0, 0, 5], f32), 3)
LAUNCHES = {"ray": 1, "point": 1, "side": 1, "hit": 5, "neighbor": 5, "overlap": 5, "overlap_segment": 2, "knn": 1}  # a list call: two walks and the scan's three


def batch(valid, j):
    """The three valid rows, then j copies of the first with a NaN in component i of row i."""
    bad = np.repeat(valid[:1], j, axis=0)
    bad[np.arange(j), np.arange(j) % valid.shape[1]] = np.nan
    return np.concatenate([valid, bad]).astype(f32)


def test_every_kind_reports_its_own_counters_whatever_the_others_do(renderer):
    r = renderer
    set_mesh_px_surface(r, TETRAHEDRON)
    n = {name: 3 + j for j, name in enumerate(("ray", "point", "side", "hit", "neighbor", "overlap", "clearance", "knn"), 1)}
    bad = {name: count - 3 for name, count in n.items()}

    # all nine, back to back
    ray_o = batch(OUTSIDE, bad["ray"])
    _, ray_tri = r.query_rays(tdev(ray_o), tdev(np.where(np.isnan(ray_o), f32(1), -ray_o)))
    _, point_tri, _ = r.query_points(tdev(batch(INSIDE, bad["point"])), count_traversal=True)
    side_p = batch(np.concatenate([INSIDE[1:2], OUTSIDE[:2]]), bad["side"])  # (not the centroid: a ray along an axis leaves it through an edge)
    inside, crossings = r.query_sides(tdev(side_p), want_crossings=True, count_traversal=True)
    hit_o = batch(OUTSIDE, bad["hit"])
    hit_offsets, _, _, hit_counts = r.list_ray_hits(tdev(hit_o), tdev(np.where(np.isnan(hit_o), f32(1), -hit_o)), capacity=64)
    nb_offsets, _, _, nb_counts = r.list_neighbors(tdev(batch(INSIDE, bad["neighbor"])), 1.0, capacity=64)
    tris = tdev(batch(SLICES, bad["overlap"]))
    ov_offsets, ov_tri, _, ov_counts = r.list_overlaps(tris, capacity=64)
    r.overlap_segments(tris, ov_offsets, ov_tri)
    _, clear_tri, _, _ = r.query_clearance(tdev(batch(AWAY, bad["clearance"])), count_traversal=True)
    _, _, knn_counts = r.query_knn(tdev(batch(INSIDE, bad["knn"])), 2, count_traversal=True)

    # read in the reverse order, each twice: the second reading is the host's copy
    stats = {}
    for name in ("knn_query", "clearance_query", "overlap_segment", "overlap_query", "neighbor_query", "hit_query", "side_query", "point_query", "ray_query"):
        first = getattr(r, name + "_stats")()
        assert getattr(r, name + "_stats")() == first, name
        stats[name.replace("_query", "")] = first
        assert first["ms"] > 0, (name, first)
        assert first.get("stack_overflow", 0) == 0, (name, first)
        assert first.get("launches") == LAUNCHES.get(name.replace("_query", "")), (name, first)  # (clearance has neither)
    counted = {"point", "side", "clearance", "knn"}  # the list calls of the wrapper do not count
    for name, st in stats.items():
        if "nodes_visited" in st:
            assert (st["nodes_visited"] > 0) == (name in counted) and (st["tris_tested"] > 0) == (name in counted), (name, st)

    def marked(t):
        return int((t == INVALID).sum())

    def found(counts):
        return int(counts.clamp(min=0).sum())

    st = stats["ray"]
    assert (st["rays"], st["invalid_rays"]) == (n["ray"], bad["ray"]) and marked(ray_tri) == bad["ray"] and bool((ray_tri[:3] >= 0).all()), st
    st = stats["point"]
    assert (st["points"], st["invalid_points"]) == (n["point"], bad["point"]) and marked(point_tri) == bad["point"], st
    st = stats["side"]
    assert (st["points"], st["invalid_points"], st["skipped_points"]) == (n["side"], bad["side"], 0) and marked(inside) == bad["side"], st
    assert inside[:3].tolist() == [1, 0, 0] and st["walks"] == 3 * 3, (st, inside)  # with crossings all three rays of every valid point are walked
    assert st["third_walks"] == int(((crossings[:3, 0] ^ crossings[:3, 1]) & 1).sum()), (st, crossings)
    st = stats["hit"]  # a line through the inside of a convex closed surface crosses it twice
    assert (st["rays"], st["invalid_rays"], st["hits"]) == (n["hit"], bad["hit"], 2 * 3) and marked(hit_counts) == bad["hit"], st
    assert st["hits"] == found(hit_counts) and st["hits_written"] == int(hit_offsets[-1]) and (st["incomplete_rays"], st["slice_overflow"]) == (0, 0), st
    st = stats["neighbor"]  # all four faces lie within 1 of a point near the centroid
    assert (st["points"], st["invalid_points"], st["neighbors"]) == (n["neighbor"], bad["neighbor"], 4 * 3) and marked(nb_counts) == bad["neighbor"], st
    assert st["neighbors"] == found(nb_counts) and st["neighbors_written"] == int(nb_offsets[-1]) and (st["incomplete_points"], st["slice_overflow"]) == (0, 0), st
    st = stats["overlap"]  # the plane of a slice cuts all four faces
    assert (st["triangles"], st["invalid_triangles"], st["overlaps"]) == (n["overlap"], bad["overlap"], 4 * 3) and marked(ov_counts) == bad["overlap"], st
    assert st["overlaps"] == found(ov_counts) and st["overlaps_written"] == int(ov_offsets[-1]) and (st["incomplete_triangles"], st["slice_overflow"]) == (0, 0), st
    st = stats["overlap_segment"]  # two edges of every face pierce the slice that covers the cut: a segment each, nothing else
    assert st["entries"] == int(ov_offsets[-1]) == 12 and st["segments"] + st["touches"] + st["skipped_incomplete"] + st["bad_entries"] == st["entries"], st
    assert (st["segments"], st["touches"], st["skipped_incomplete"], st["bad_entries"]) == (12, 0, 0, 0), st
    st = stats["clearance"]
    assert (st["queries"], st["invalid_triangles"]) == (n["clearance"], bad["clearance"]) and marked(clear_tri) == bad["clearance"], st
    st = stats["knn"]  # min(k, the mesh's four triangles) = 2 per valid point
    assert (st["points"], st["invalid_points"], st["neighbors"]) == (n["knn"], bad["knn"], 2 * 3) and marked(knn_counts) == bad["knn"], st
    assert st["neighbors"] == found(knn_counts), st
