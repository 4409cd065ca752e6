"""Overlap segments on device tensors (Renderer.overlap_segments, rt_overlap_segments_device) on the GPU.

Every case takes its list from Renderer.list_overlaps and compares segments and `ends` bit for bit with tests/section_exact.py's native
reference (tests/native/overlap_segment_ref.cpp: csrc/tri_overlap.h + csrc/tri_section.h over all pairs, no tree), which in turn is held to
hand-computed answers, to its own selection rule and to float64 on the CPU (tests/test_overlap_segment_host.py).  What the call does
with arrays it did not make - offsets that do not ascend, indices outside the mesh, a capacity that cuts a slice - is stated entry by
entry by expect() below, from the header's rules and the same native program, and asserted behind guard words: no case provokes a fault."""
import functools

import numpy as np
import pytest

import overlap_exact as OX
import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
import section_exact as SX
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_pointers, dev, ptr, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 256  # untouched entries asserted on either side of every output array of the raw calls


def bits_of(mask):
    return ((np.asarray(mask)[:, None] >> np.arange(6)) & 1).sum(1)


def check_case(renderer, q, sref, what):
    """The list from Renderer.list_overlaps, then its segments: with `ends`, without (ends_out_dev = NULL), and into out= tensors."""
    import torch

    tq = tdev(q)
    offsets, tri, edges, counts = renderer.list_overlaps(tq)
    k = sref["entries"]
    assert np.array_equal(offsets.cpu().numpy(), sref["offsets"]) and np.array_equal(tri.cpu().numpy(), sref["tri"]) and np.array_equal(edges.cpu().numpy(), sref["mask"]), what
    seg, ends = renderer.overlap_segments(tq, offsets, tri, want_ends=True)
    assert tuple(seg.shape) == (k, 2, 3) and seg.dtype == torch.float32 and tuple(ends.shape) == (k,) and ends.dtype == torch.int32
    got_seg, got_ends = seg.cpu().numpy(), ends.cpu().numpy()
    assert np.array_equal(got_ends, sref["ends"]), (what, np.nonzero(got_ends != sref["ends"])[0][:8])
    assert SX.same_bits(got_seg, sref["seg"]), (what, np.nonzero((got_seg.view(np.uint32) != sref["seg"].view(np.uint32)).any((1, 2)))[0][:8])
    if k == 0:  # nothing to ask: the library is not called
        return
    st = renderer.overlap_segment_stats()
    nbits = bits_of(sref["mask"])
    assert (st["entries"], st["segments"], st["touches"], st["skipped_incomplete"], st["bad_entries"], st["launches"]) == \
        (k, int((nbits >= 2).sum()), int((nbits == 1).sum()), 0, 0, 2) and st["ms"] > 0, (what, st)
    alone = renderer.overlap_segments(tq, offsets, tri)
    assert SX.same_bits(alone.cpu().numpy(), sref["seg"]), what
    out = (torch.full((k, 2, 3), -7.0, device=dev()), torch.full((k,), -7, dtype=torch.int32, device=dev()))
    back = renderer.overlap_segments(tq, offsets, tri, capacity=k, out=out, want_ends=True)
    assert back[0].data_ptr() == out[0].data_ptr() and back[1] is out[1]
    assert SX.same_bits(out[0].cpu().numpy(), sref["seg"]) and np.array_equal(out[1].cpu().numpy(), sref["ends"]), what


# ---- 1. every family, every tree ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", OX.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, fam):
    """(Family d: the long lists, 226 entries from 40 queries on the soup cut.)"""
    for c in SX.family_case(fam):
        set_mesh(renderer, c["verts"])
        check_case(renderer, c["q"], c["sref"], (fam, c["mesh"]))


@pytest.mark.parametrize("tree", ["two-level", "device build", "refit to moved vertices"])
@pytest.mark.parametrize("fam", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, fam, tree):
    """Each tree has a leaf order of its own: what the map from original index to leaf position can get wrong."""
    for c in SX.family_case(fam, moved=tree.startswith("refit")):
        n_tris = len(c["verts"])
        if tree == "two-level":
            set_mesh(renderer, c["verts"], bvh_levels=2, blas_chunks=max(1, min(64, n_tris // 8)))
        else:
            still = OX.soup_cut() if c["mesh"] == "soup_cut" else PX.mesh(c["mesh"])
            renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(still)))
            if tree.startswith("refit"):
                renderer.refit_mesh_device(tdev(c["verts"]))
        if n_tris >= 256:
            assert not np.array_equal(renderer.read_bvh()[1], np.arange(n_tris)), (fam, c["mesh"], tree)  # (the leaf order is a permutation worth the name)
        check_case(renderer, c["q"], c["sref"], (fam, c["mesh"], tree))


def test_after_a_chunk_update_on_a_two_level_mesh(renderer):
    """rt_update_mesh_chunk rebuilds one chunk: its records move and change; the next call's map follows without being told."""
    c = next(c for c in SX.family_case("b") if c["mesh"] == "terrain")
    v = c["verts"].copy()
    set_mesh(renderer, v, bvh_levels=2, blas_chunks=16)
    check_case(renderer, c["q"], c["sref"], "before the update")
    for chunk in (3, 11):
        ids = renderer.mesh_chunk(chunk)
        v[ids] += np.tile(np.array([0.3, -0.2, 0.1], f32), 3)
        renderer.update_mesh_chunk(chunk, v[ids])
    sref = SX.reference(v, c["q"])
    assert sref["entries"] > 0 and not (np.array_equal(sref["offsets"], c["sref"]["offsets"]) and SX.same_bits(sref["seg"], c["sref"]["seg"]))
    check_case(renderer, c["q"], sref, "after the update")


# ---- 2. one batch on the terrain ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch():
    """overlap_exact's kind of batch: 600 query triangles of families a, b and c on the terrain, shuffled."""
    v = PX.mesh("terrain")
    parts = [next(c for c in OX.family_case(f) if c["mesh"] == "terrain")["q"] for f in ("a", "b", "c")]
    parts.append(OX._planted(np.random.default_rng(17), v, 50))
    q = np.concatenate(parts)
    q = np.ascontiguousarray(q[np.random.default_rng(13).permutation(len(q))], f32)
    sref = SX.reference(v, q)
    assert len(q) == 600 and sref["entries"] > 600 and sref["invalid"] == 0
    return dict(v=v, q=q, sref=sref, n=len(q))


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


@pytest.mark.parametrize("entries", [1, 63, 64, 65])
def test_lists_that_straddle_one_wave(renderer, entries):
    """Lists of exactly 1, 63, 64 and 65 entries: queries of the batch that list one triangle each, and one that lists none between them."""
    b = set_batch(renderer)
    count = b["sref"]["count"]
    one, none = np.nonzero(count == 1)[0], np.nonzero(count == 0)[0]
    assert len(one) >= 65 and len(none) >= 1
    pick = np.concatenate([one[:entries // 2], none[:1], one[entries // 2:entries]])
    sref = SX.reference(b["v"], b["q"][pick])
    assert sref["entries"] == entries
    check_case(renderer, b["q"][pick], sref, entries)


@pytest.mark.parametrize("n_tris", [1, 8, 9])
def test_meshes_of_a_root_and_of_two_levels(renderer, n_tris):
    v = np.ascontiguousarray(PX.mesh("soup")[:n_tris])
    rng = np.random.default_rng(19 + n_tris)
    q = np.concatenate([OX._planted(rng, v, 40), OX._spanning(rng, v, 10), OX._displaced(rng, v, 20, 0.05), v])
    sref = SX.reference(v, q)
    assert sref["entries"] >= 40
    set_mesh(renderer, v)
    check_case(renderer, q, sref, n_tris)


def expect(verts, q, offsets, tri, capacity):
    """What rt_overlap_segments_device leaves in arrays prefilled with -7, entry by entry after the header: K = min(max(offsets[n], 0),
    capacity) entries are visited; entry k's owner is the last i the halving search reaches with offsets[i] <= k, kept if offsets[i] <= k <
    offsets[i + 1]; an owned entry of a slice that ends beyond the capacity is untouched; every other one is answered - by the native
    reference for the pair (owner, tri[k]), which gives NaNs and -1 for an index outside the mesh, no cand or no bit - or, without an
    owner, with NaNs and -1.  Returns (seg, ends, stats)."""
    n, offsets, tri = len(q), np.asarray(offsets, np.int64), np.asarray(tri, np.int32)
    k_end = int(min(max(int(offsets[n]), 0), capacity))
    seg, ends = np.full((capacity, 2, 3), -7.0, f32), np.full(capacity, -7, np.int32)
    answered, pairs, skipped = [], [], 0
    for k in range(k_end):
        lo, hi = 0, n
        while hi - lo > 1:
            mid = lo + ((hi - lo) >> 1)
            if offsets[mid] <= k:
                lo = mid
            else:
                hi = mid
        owned = offsets[lo] <= k < offsets[lo + 1]
        if owned and offsets[lo + 1] > capacity:
            skipped += 1
            continue
        answered.append(k)
        pairs.append((lo if owned else -1, int(tri[k])))
    if answered:
        got = SX.reference(verts, q, pairs=np.asarray(pairs, np.int64).astype(np.int32))
        seg[answered], ends[answered] = got["pair_seg"], got["pair_ends"]
    e = ends[answered] if answered else np.zeros(0, np.int32)
    stats = dict(entries=k_end, segments=int(((e >= 0) & ((e & 7) != (e >> 3))).sum()), touches=int(((e >= 0) & ((e & 7) == (e >> 3))).sum()),
                 skipped_incomplete=skipped, bad_entries=int((e < 0).sum()))
    return seg, ends, stats


def raw_call(renderer, b, offsets, tri, capacity, what, with_ends=True):
    """The C call on the batch's triangles with arrays of the test's own, outputs between guard words; compared with expect()."""
    import torch

    lib = R.load()
    seg_buf, ends_buf = sentinel(capacity, torch.float32, 2 * GUARD, cols=6), sentinel(capacity, torch.int32, 2 * GUARD)
    tq, to, tt = tdev(b["q"]), tdev(np.ascontiguousarray(offsets, np.int64)), tdev(np.ascontiguousarray(tri, np.int32))
    assert len(tri) >= capacity
    torch.cuda.synchronize()
    assert lib.rt_overlap_segments_device(renderer._ctx, ptr(tq), b["n"], ptr(to), capacity, ptr(tt), ptr(seg_buf[GUARD:]), ptr(ends_buf[GUARD:]) if with_ends else None) == 0, what
    st = renderer.overlap_segment_stats()  # (waits for it)
    want_seg, want_ends, want_st = expect(b["v"], b["q"], offsets, tri, capacity)
    got_seg, got_ends = seg_buf.cpu().numpy(), ends_buf.cpu().numpy()
    assert still_sentinel(got_seg, GUARD, GUARD + capacity) and still_sentinel(got_ends, GUARD, GUARD + capacity), what
    assert SX.same_bits(got_seg[GUARD:GUARD + capacity].reshape(-1, 2, 3), want_seg), what
    assert np.array_equal(got_ends[GUARD:GUARD + capacity], want_ends if with_ends else np.full(capacity, -7, np.int32)), what
    assert {k: st[k] for k in want_st} == want_st and st["launches"] == 2, (what, st, want_st)
    return want_st


def test_a_capacity_that_cuts_a_slice(renderer):
    """The list call under a capacity that ends inside a slice writes the complete slices before it; the segment call answers exactly
    those, leaves the cut slice and everything behind it untouched, and counts the entries below the capacity that it skipped."""
    import torch

    b = set_batch(renderer)
    off, count = b["sref"]["offsets"], b["sref"]["count"]
    j = int(np.nonzero((count >= 3) & (off[:-1] > 300))[0][0])
    for capacity in (int(off[j]) + 2, int(off[j]), b["sref"]["entries"] - 1):
        t_buf, e_buf = sentinel(b["sref"]["entries"], torch.int32), sentinel(b["sref"]["entries"], torch.int32)
        offsets, tri, _, _ = renderer.list_overlaps(tdev(b["q"]), capacity=capacity, out=(None, t_buf[:capacity], e_buf[:capacity], None))
        assert np.array_equal(offsets.cpu().numpy(), off)
        st = raw_call(renderer, b, off, t_buf.cpu().numpy(), capacity, ("capacity", capacity))
        fits = off[1:] <= capacity
        written = int(off[1:][fits].max())
        assert (st["entries"], st["skipped_incomplete"], st["bad_entries"]) == (capacity, capacity - written, 0) and st["segments"] + st["touches"] == written
        if capacity == int(off[j]) + 2:
            assert written == int(off[j]) and st["skipped_incomplete"] == 2
    raw_call(renderer, b, off, b["sref"]["tri"], b["sref"]["entries"], "without ends", with_ends=False)
    # a capacity beyond the list: offsets[n] ends the work
    tri = np.concatenate([b["sref"]["tri"], np.full(100, -1, np.int32)])
    st = raw_call(renderer, b, off, tri, b["sref"]["entries"] + 100, "capacity beyond the list")
    assert (st["entries"], st["bad_entries"]) == (b["sref"]["entries"], 0)


def test_foreign_input_is_safe(renderer):
    """Offsets the library did not make - they need not ascend - and indices outside the mesh: nothing is written out of range, what
    cannot be answered gets NaNs and ends = -1, and bad_entries counts it exactly."""
    b = set_batch(renderer)
    off, tri, total, n = b["sref"]["offsets"], b["sref"]["tri"], b["sref"]["entries"], b["n"]
    rng = np.random.default_rng(29)
    shuffled = off.copy()
    shuffled[1:-1] = rng.permutation(off[1:-1])
    cases = {"halved": off // 2, "shifted up": off + 100, "shifted down": off - 100, "reversed": off[::-1].copy(), "shuffled": shuffled, "far": off + (1 << 40),
             "negative": -off - 1, "zeros": np.zeros(n + 1, np.int64), "huge total": np.concatenate([off[:-1], [1 << 62]])}
    seen_bad = 0
    for name, foreign in cases.items():
        for capacity in (total, total // 3):
            seen_bad += raw_call(renderer, b, foreign, tri, capacity, (name, capacity))["bad_entries"]
    assert seen_bad > 0
    planted = tri.copy()
    where = rng.permutation(total)[:60]
    planted[where[:20]], planted[where[20:40]], planted[where[40:]] = -1, len(b["v"]), 2 ** 31 - 1
    st = raw_call(renderer, b, off, planted, total, "indices outside the mesh")
    assert st["bad_entries"] == 60 and st["skipped_incomplete"] == 0
    # a listed triangle replaced by another one of the mesh: answered for that pair (NaNs where it has no cand or no bit)
    swapped = tri.copy()
    swapped[where] = (tri[where] + 577) % len(b["v"])
    st = raw_call(renderer, b, off, swapped, total, "other triangles of the mesh")
    assert 0 < st["bad_entries"] <= 60
    # an invalid query triangle: every entry of its slice is bad
    q_bad = b["q"].copy()
    i = int(np.nonzero(b["sref"]["count"] >= 2)[0][0])
    q_bad[i, 4] = np.nan
    st = raw_call(renderer, dict(b, q=q_bad), off, tri, total, "a query triangle with a NaN")
    assert st["bad_entries"] == int(b["sref"]["count"][i])


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_batch(renderer)
    n, cap = b["n"], b["sref"]["entries"]
    tq, off, tri = tdev(b["q"]), tdev(b["sref"]["offsets"]), tdev(b["sref"]["tri"])
    seg, ends = sentinel(cap, torch.float32, cols=6), sentinel(cap, torch.int32)
    bp = bad_pointers(n, short9=36, short8=(8, n + 1), short4=(4, cap), short24=(24, cap))  # one row short each
    hp, short9, short8, short4, short24 = bp.hp, bp.short9, bp.short8, bp.short4, bp.short24

    def untouched(k):
        assert_untouched(renderer, (seg, ends), bp.big, k)

    good = (ptr(tq), n, ptr(off), cap, ptr(tri), ptr(seg), ptr(ends))
    fresh = R.Renderer(0)
    try:
        assert lib.rt_overlap_segments_device(fresh._ctx, *good) == RT_ERR_STATE
        untouched("no mesh")
        set_mesh(fresh, np.ldexp(PX.mesh("grid"), 19).astype(f32))  # 5.3 x 2^19 > 2^20: taken as a mesh, refused by the queries
        assert lib.rt_overlap_segments_device(fresh._ctx, *good) == RT_ERR_INVALID
        untouched("a mesh beyond 2^20")
    finally:
        fresh.close()
    ctx = renderer._ctx
    calls = []
    for at, bad in ((0, (None, hp, short9)), (2, (None, hp, short8)), (4, (None, hp, short4)), (5, (None, hp, short24)), (6, (hp, short4))):
        for x in bad:
            calls.append(good[:at] + (x,) + good[at + 1:])
    calls.append((ptr(tq), (1 << 30) + 1) + good[2:])
    calls.append(good[:3] + ((1 << 40) + 1,) + good[4:])
    for k, args in enumerate(calls):
        assert lib.rt_overlap_segments_device(ctx, *args) == RT_ERR_INVALID, k
        untouched(k)
    # n == 0 and capacity == 0 are accepted, and do nothing
    assert lib.rt_overlap_segments_device(ctx, None, 0, None, cap, None, None, None) == 0
    assert lib.rt_overlap_segments_device(ctx, None, n, None, 0, None, None, None) == 0
    assert lib.rt_overlap_segments_device(ctx, ptr(tq), n, ptr(off), 0, ptr(tri), ptr(seg), ptr(ends)) == 0
    untouched("n = 0, capacity = 0")
    assert tuple(renderer.overlap_segments(tq[:0], off[:1], tri[:0]).shape) == (0, 2, 3)
    # the context still answers; (n, 3, 3) and flat tensors are the same triangles
    for view in (tq, tq.view(n, 3, 3), tq.view(-1)):
        got = renderer.overlap_segments(view, off, tri, out=(seg, ends), want_ends=True)
        assert SX.same_bits(got[0].cpu().numpy(), b["sref"]["seg"]) and np.array_equal(ends.cpu().numpy(), b["sref"]["ends"])
        seg.fill_(-7.0)


# ---- 4. what the rest of the process keeps -------------------------------------------------------------------------------------------

def test_a_shared_mesh_stays_shared(renderer):
    """The map is written into scratch of the context's own, never into the mesh: two contexts on one mesh answer alike and stay sharers."""
    b = set_batch(renderer)
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        check_case(other, b["q"], b["sref"], "the other context")
        check_case(renderer, b["q"], b["sref"], "this context")
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
    finally:
        other.close()


def test_stream_order_behind_a_refit_and_a_list(renderer):
    """The refit, the list call and the segment call behind it on one stream of torch's, no host synchronisation between them and the
    comparison: the segments are those of the moved mesh, from the list the call before them wrote."""
    import torch

    c = next(c for c in SX.family_case("b", moved=True) if c["mesh"] == "terrain")
    still = PX.mesh("terrain")
    sref, n = c["sref"], len(c["q"])
    k = sref["entries"]
    assert k > 0 and not np.array_equal(sref["count"], SX.reference(still, c["q"])["count"])  # the unmoved mesh answers otherwise
    renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(still)))
    tq, moved = tdev(c["q"]), tdev(c["verts"])
    ref_seg, ref_ends = tdev(sref["seg"]).view(torch.int32), tdev(sref["ends"])
    counts, offsets, tri, edges = sentinel(n, torch.int32), sentinel(n + 1, torch.int64), sentinel(k, torch.int32), sentinel(k, torch.int32)
    seg, ends = torch.full((k, 2, 3), -7.0, device=dev()), sentinel(k, torch.int32)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    renderer.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            renderer.refit_mesh_device(moved)
            renderer.list_overlaps(tq, capacity=k, out=(offsets, tri, edges, counts), sync=False)
            renderer.overlap_segments(tq, offsets, tri, out=(seg, ends), sync=False, want_ends=True)
            wrong = (seg.view(torch.int32) != ref_seg).sum() + (ends != ref_ends).sum()
        s.synchronize()
        assert int(wrong) == 0
    finally:
        renderer.synchronize()
        renderer.set_stream(None)


@pytest.mark.parametrize("k", [-16, 14])
def test_scale(renderer, k):
    """Every length x 2^k (tests/scale_exact.py's two scales): the same lists and `ends`, endpoints that scale exactly."""
    for fam in ("a", "b", "c"):
        for c in SX.family_case(fam):
            if c["mesh"] not in ("soup", "grid", "terrain", "needle"):
                continue
            set_mesh(renderer, np.ldexp(c["verts"], k).astype(f32))
            check_case(renderer, np.ldexp(c["q"], k).astype(f32), dict(c["sref"], seg=np.ldexp(c["sref"]["seg"], k).astype(f32)), (fam, c["mesh"], k))
