"""Overlap queries on device tensors (Renderer.count_overlaps / list_overlaps, rt_count_overlaps_device / rt_fill_overlaps_device /
rt_list_overlaps_device) on the GPU.

The reference is tests/overlap_exact.py's native brute force (tests/native/overlap_query_ref.cpp: the arithmetic of csrc/tri_overlap.h
over all pairs, no tree), which the kernel must match bit for bit in counts, offsets, indices and masks; its tree walk under the kernel's
culling rule gives the nodes and records the kernel must count, exactly.  That reference in turn is held to its own walk, to answers
computed by hand, to the all-hits reference and to float64 on the CPU (tests/test_overlap_query_host.py).  The first tests run every
family on its meshes; the others need ONE batch on ONE mesh whose size they can cut: 600 query triangles of families a, b and c on the
terrain, shuffled.  The listing protocol's tests are tests/gpu_listing.py's, on this batch."""
import functools

import numpy as np
import pytest

import gpu_listing as L
import gpu_query as Q
import overlap_exact as OX
import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, dev, ptr, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID = OX.INVALID


def check_lists(got, ref, what):
    """(offsets, tri, edges, counts) as tensors against a reference dict, bit for bit."""
    L.check_lists(L.OVERLAPS, got, ref, what)


def check_case(renderer, q, ref, what, exact_work=False, **kw):
    """The three ways to ask against the reference of the query triangles q: count, list without a capacity (count + fill), list with
    capacity k + 3.  exact_work: the tree is the host-built single-level one, whose walk the reference has made: nodes and records
    agree exactly."""
    L.check_case(renderer, L.OVERLAPS, (q,), ref, what, exact_work=exact_work, **kw)


# ---- 1. every family, every tree ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", OX.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, fam):
    for c in OX.family_case(fam):
        set_mesh(renderer, c["verts"])
        check_case(renderer, c["q"], c["ref"], (fam, c["mesh"]), exact_work=True)


@pytest.mark.parametrize("tree", ["two-level", "device build", "refit to moved vertices"])
@pytest.mark.parametrize("fam", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, fam, tree):
    for c in OX.family_case(fam, moved=tree.startswith("refit")):
        n_tris = len(c["verts"])
        if tree == "two-level":
            set_mesh(renderer, c["verts"], bvh_levels=2, blas_chunks=max(1, min(64, n_tris // 8)))
        else:
            still = OX.soup_cut() if c["mesh"] == "soup_cut" else PX.mesh(c["mesh"])
            renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(still)))
            if tree.startswith("refit"):
                assert not np.array_equal(c["verts"], still)
                renderer.refit_mesh_device(tdev(c["verts"]))
        check_case(renderer, c["q"], c["ref"], (fam, c["mesh"], tree))


# ---- 2. one batch on the terrain ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    v = PX.mesh("terrain")
    parts = [next(c for c in OX.family_case(f) if c["mesh"] == "terrain")["q"] for f in ("a", "b", "c")]
    parts.append(OX._planted(np.random.default_rng(17), v, 50))
    q = np.concatenate(parts)
    q = np.ascontiguousarray(q[np.random.default_rng(13).permutation(len(q))], f32)
    ref = OX.reference(v, q)
    assert len(q) == 600 and ref["overlaps"] > 600 and ref["invalid"] == 0 and ref["count"].max() <= OX.LONGEST and (ref["count"] == 0).sum() > 50
    return dict(v=v, q=q, ref=ref, n=len(q), reach=PX.reach_of(v))


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_batch_edges(renderer, n):
    """16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry while others are
    not; beyond the batch's own size its triangles repeat, each against its own brute-force rows (no new geometry: these sizes are
    about the queue's streams)."""
    b = set_batch(renderer)
    sel = np.arange(n) % len(b["q"])
    check_case(renderer, np.ascontiguousarray(b["q"][sel]), OX.rows(b["ref"], sel), n, exact_work=True)


@pytest.mark.parametrize("refill_min", [1, 24, 64])
def test_refill_through_one_workgroup(renderer, refill_min):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 600 query triangles every lane refills."""
    b = set_batch(renderer)
    check_case(renderer, b["q"], b["ref"], refill_min, exact_work=True, tune_max_blocks=1, tune_refill_min=refill_min)


@pytest.mark.parametrize("n_tris", [1, 8, 9])
def test_meshes_of_a_root_and_of_two_levels(renderer, n_tris):
    """1 and 8 triangles: the root alone; 9: the first inner child."""
    v = np.ascontiguousarray(PX.mesh("soup")[:n_tris])
    rng = np.random.default_rng(19 + n_tris)
    q = np.concatenate([OX._planted(rng, v, 40), OX._spanning(rng, v, 10), OX._displaced(rng, v, 20, 0.05), v])
    ref = OX.reference(v, q)
    assert OX.walk_is_brute(ref) and ref["overlaps"] >= 40 and (ref["nodes"].max() > 1) == (n_tris > 8)
    set_mesh(renderer, v)
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        check_case(renderer, q, ref, (n_tris, kw), exact_work=True, **kw)


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest in global memory; no overflow (check_case asserts it)."""
    b = set_batch(renderer)
    assert renderer.pt_stats()["bvh_depth"] > 2
    check_case(renderer, b["q"], b["ref"], "one LDS entry", exact_work=True, tune_lds_stack=1)
    c = OX.family_case("d")[1]  # boxes that span the mesh: every level holds a pending group
    set_mesh(renderer, c["verts"])
    assert renderer.pt_stats()["bvh_depth"] > 2
    check_case(renderer, c["q"], c["ref"], "one LDS entry, spanning boxes", exact_work=True, tune_lds_stack=1)


def test_bits_0_to_2_against_list_ray_hits(renderer):
    """Cross-kernel pin: the 3 n edge segments through Renderer.list_ray_hits with tmax = 1 on the device, cut to cand in numpy fp32."""
    import torch

    b = set_batch(renderer)
    o, d = OX.edge_segments(b["q"])
    offsets, _, hit_tri, counts = renderer.list_ray_hits(tdev(o), tdev(d), torch.ones(len(o), dtype=torch.float32, device=dev()))
    counts, hit_tri = counts.cpu().numpy(), hit_tri.cpu().numpy()
    assert (counts >= 0).all() and int(offsets[-1]) == counts.sum()
    ray = np.repeat(np.arange(len(o)), counts)
    cand = OX.cand_numpy(b["v"], b["q"])[ray // 3, hit_tri]
    got = set(zip((ray // 3)[cand].tolist(), (ray % 3)[cand].tolist(), hit_tri[cand].tolist()))
    _, tri, edges, cnt = (x.cpu().numpy() for x in renderer.list_overlaps(tdev(b["q"])))
    owner = np.repeat(np.arange(b["n"]), cnt)
    want = {(int(i), k, int(t)) for i, t, m in zip(owner, tri, edges) for k in range(3) if (m >> k) & 1}
    assert got == want and len(want) > 500


# ---- 3. capacity and offsets -----------------------------------------------------------------------------------------------------

def test_capacity(renderer):
    """Capacity at the total, one below it, half of it and 0: a slice that does not fit is not touched, every other one is complete, the
    offsets are the full sums."""
    import torch

    b = set_batch(renderer)
    n, ref = b["n"], b["ref"]
    L.capacity(renderer, L.OVERLAPS, (b["q"],), ref)
    # capacity 0 with NULL arrays
    tq, cnt, offs = tdev(b["q"]), Q.sentinel(n, torch.int32), Q.sentinel(n + 1, torch.int64)
    assert R.load().rt_list_overlaps_device(renderer._ctx, ptr(tq), n, None, ptr(cnt), ptr(offs), 0, None, None) == 0
    assert renderer.overlap_query_stats()["overlaps_written"] == 0
    assert np.array_equal(offs.cpu().numpy(), ref["offsets"]) and np.array_equal(cnt.cpu().numpy(), ref["count"])


def test_foreign_offsets_are_safe(renderer):
    """The fill step on offsets it did not make: nothing outside [0, capacity) is written, a slice shorter than its query's list keeps the
    entries with the lowest indices, and slice_overflow counts the rest."""
    b = set_batch(renderer)
    L.foreign_offsets(renderer, L.OVERLAPS, (b["q"],), b["ref"])


# ---- 4. invalid queries, refusals ----------------------------------------------------------------------------------------------------

def test_invalid_triangles(renderer):
    """NaN, +-inf and one step beyond the reach in every one of the nine coordinates; exactly at the reach is valid.  And the early-exit
    trap: refills that hand out 64 entries and leave no lane alive."""
    b = set_batch(renderer)
    reach, n = b["reach"], b["n"]
    where = np.random.default_rng(43).permutation(n)
    q = b["q"].copy()
    k = 0
    for comp in range(9):
        for bad in (np.nan, np.inf, -np.inf, np.nextafter(reach, f32(np.inf)), -np.nextafter(reach, f32(np.inf))):
            q[where[k], comp] = bad
            k += 1
    edge = where[k:k + 9]
    for j, i in enumerate(edge):
        q[i, j] = (1 if j % 2 else -1) * reach
    exp = OX.reference(b["v"], q)
    assert exp["invalid"] == 45 and (exp["count"][where[:45]] == INVALID).all() and (exp["count"][edge] >= 0).all() and OX.walk_is_brute(exp)
    for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
        check_case(renderer, q, exp, ("invalid triangles", kw), exact_work=True, **kw)
    q_bad = b["q"].copy()
    q_bad[:, 4] = np.nan
    offsets, tri, edges, counts = renderer.list_overlaps(tdev(q_bad), capacity=16, tune_max_blocks=1)
    st = renderer.overlap_query_stats()
    assert (counts == INVALID).all() and (offsets == 0).all()
    assert (st["invalid_triangles"], st["overlaps"], st["overlaps_written"], st["triangles"]) == (n, 0, 0, n)


def test_errors_write_nothing(renderer):
    b = set_batch(renderer)
    n, ref = b["n"], b["ref"]
    e = L.Refusals(renderer, L.OVERLAPS, (b["q"],), ref, short9=36)  # (one row short of n x 9)
    fresh = R.Renderer(0)
    try:
        e.every_entry(fresh._ctx, RT_ERR_STATE, "no mesh")
        set_mesh(fresh, np.ldexp(PX.mesh("grid"), 19).astype(f32))  # 5.3 x 2^19 > 2^20: taken as a mesh, refused by the queries
        e.every_entry(fresh._ctx, RT_ERR_INVALID, "a mesh beyond 2^20")
    finally:
        fresh.close()
    tq, = e.t
    e.tables([(None, n, None), (e.bp.hp, n, None), (e.bp.short9, n, None), (ptr(tq), (1 << 30) + 1, None)] + [(ptr(tq), n, prm) for prm in e.bad_params])
    e.nothing_to_do((tq[:0],), (tq[:0],))
    # the context still answers; (n, 3, 3) and flat tensors are the same triangles
    e.still_answers()
    check_lists(renderer.list_overlaps(tq.view(n, 3, 3)), ref, "(n, 3, 3)")
    check_lists(renderer.list_overlaps(tq.view(-1)), ref, "flat")


# ---- 5. what the rest of the process keeps ---------------------------------------------------------------------------------------

def test_a_shared_mesh_stays_shared(renderer):
    b = set_batch(renderer)
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        check_case(other, b["q"], b["ref"], "the other context", exact_work=True)
        check_case(renderer, b["q"], b["ref"], "this context", exact_work=True)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
    finally:
        other.close()


def test_stream_order_behind_a_refit(renderer):
    """The refit and the query behind it on one stream of torch's, no host synchronisation between them and the comparison: the query
    sees the moved mesh."""
    import torch

    c = next(c for c in OX.family_case("b", moved=True) if c["mesh"] == "terrain")
    still = PX.mesh("terrain")
    ref, n = c["ref"], len(c["q"])
    k = ref["overlaps"]
    assert k > 0 and not np.array_equal(ref["count"], OX.reference(still, c["q"])["count"])  # the unmoved mesh answers otherwise
    renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(still)))
    tq, moved = tdev(c["q"]), tdev(c["verts"])
    ref_c, ref_o, ref_t, ref_e = tdev(ref["count"]), tdev(ref["offsets"]), tdev(ref["tri"]), tdev(ref["edges"])
    counts = torch.full((n,), -7, dtype=torch.int32, device=dev())
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device=dev())
    tri = torch.full((k,), -7, dtype=torch.int32, device=dev())
    edges = torch.full((k,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    renderer.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            renderer.refit_mesh_device(moved)
            renderer.list_overlaps(tq, capacity=k, out=(offsets, tri, edges, counts), sync=False)
            wrong = (counts != ref_c).sum() + (offsets != ref_o).sum() + (tri != ref_t).sum() + (edges != ref_e).sum()
        s.synchronize()
        assert int(wrong) == 0
    finally:
        renderer.synchronize()
        renderer.set_stream(None)


@pytest.mark.parametrize("k", [-16, 14])
def test_scale(renderer, k):
    """Every length x 2^k: bit-identical counts, indices and masks (the reference itself is covariant: test_overlap_query_host.py)."""
    for fam in ("a", "b", "c"):
        for c in OX.family_case(fam):
            if c["mesh"] not in ("soup", "grid", "terrain", "needle"):
                continue
            set_mesh(renderer, np.ldexp(c["verts"], k).astype(f32))
            check_lists(renderer.list_overlaps(tdev(np.ldexp(c["q"], k).astype(f32))), c["ref"], (fam, c["mesh"], k))
