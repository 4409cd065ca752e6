"""Overlap segments (rt_overlap_segments_device, Renderer.overlap_segments) without a GPU: the C boundary, the
wrapper's argument checks, and the native reference of tests/section_exact.py (csrc/tri_overlap.h + csrc/tri_section.h over all pairs) held
to answers computed by hand, to the list reference of tests/overlap_exact.py, to its own selection rule, to the float64 interval method
and to covariance under scale.  The kernel is compared with this reference bit for bit in tests/test_gpu_overlap_segments.py."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import overlap_exact as OX
import raytracing_engine_amd as R
import section_exact as SX

f32 = np.float32
STATS = ["entries", "segments", "touches", "skipped_incomplete", "bad_entries", "launches", "ms"]
V = C.c_void_p(16)
KIND = AB.Kind(functions=("rt_overlap_segments_device", "rt_get_overlap_segment_stats"), methods=("overlap_segments", "overlap_segment_stats"),
               stats="OverlapSegmentStats", stats_c="rt_overlap_segment_stats", stats_fields=STATS,  # no parameter struct
               null_calls=(("rt_overlap_segments_device", (None, 0, None, 0, None, None, None)), ("rt_overlap_segments_device", (V, 1, V, 1, V, V, V)),
                           ("rt_get_overlap_segment_stats", (C.byref(R.OverlapSegmentStats()),))))


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_the_stats_layout_matches_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirror."""
    AB.struct_layout(KIND, tmp_path)


def test_the_wrapper_checks_its_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    good = torch.zeros(4, 9)  # float32, contiguous, the right shape - but a CPU tensor
    off, tri = torch.zeros(5, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    for bad in (np.zeros((4, 9), f32), good, good.double(), torch.zeros(4, 8), None):
        with pytest.raises(ValueError):
            r.overlap_segments(bad, off, tri)


def test_the_wrapper_compares_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    q, off, tri = torch.zeros(4, 9), torch.zeros(5, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="tris"):
        r.overlap_segments(torch.zeros(4, 8), off, tri)
    for bad in (torch.zeros(4, dtype=torch.int64), off.int(), None):
        with pytest.raises(ValueError, match="offsets"):
            r.overlap_segments(q, bad, tri)
    for bad in (tri.long(), torch.zeros(2, 4, dtype=torch.int32), tri.numpy()):
        with pytest.raises(ValueError, match="tri"):
            r.overlap_segments(q, off, bad)
    with pytest.raises(ValueError, match="capacity"):
        r.overlap_segments(q, off, tri, capacity=-1)
    with pytest.raises(ValueError, match="tri"):
        r.overlap_segments(q, off, tri, capacity=9)  # tri holds 8
    with pytest.raises(ValueError, match="seg"):
        r.overlap_segments(q, off, tri, out=torch.zeros(7, 2, 3))
    with pytest.raises(ValueError, match="ends"):
        r.overlap_segments(q, off, tri, out=torch.zeros(8, 2, 3), want_ends=True)  # the pair is asked for
    with pytest.raises(ValueError, match="ends"):
        r.overlap_segments(q, off, tri, out=(torch.zeros(8, 2, 3), torch.zeros(7, dtype=torch.int32)), want_ends=True)
    # n == 0 and capacity == 0 never reach the library
    seg, ends = r.overlap_segments(q[:0], off[:1], tri, want_ends=True)
    assert tuple(seg.shape) == (8, 2, 3) and tuple(ends.shape) == (8,)
    assert tuple(r.overlap_segments(q, off, tri, capacity=0).shape) == (0, 2, 3)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
T0 = [0, 0, 0, 4, 0, 0, 0, 4, 0]  # the mesh of the hand-computed answers: one triangle in the plane z = 0


def test_answers_computed_by_hand():
    """Against the one triangle T0, fp32-exact throughout.  (1) the query lies in the plane x = 1: its edge A0A1 pierces T0 at t = 0.5,
    (1, 1, 0), A1A2 crosses z = 0 at (1, 5, 0) beyond the hypotenuse, A2A0 runs parallel to it; T0's edge v0v1 crosses x = 1 at (1, 0, 0)
    outside the query, v1v2 pierces it at t = 0.75, (1, 3, 0), v0v2 runs parallel: mask 010001, the segment (1, 1, 0) - (1, 3, 0), ends =
    0 | 4 << 3.  (2) overlap_exact's second query: A0A1 and A2A0 pierce at (1, 1.5, 0) and (1.5, 1, 0): bits 0 and 2, in that order.
    (3) its first: bits 0 and 3, (1, 1, 0) and (1, 0, 0).  (4) a cand pair without a piercing edge and (5) a pair with disjoint boxes,
    asked for as planted pairs: NaNs, ends = -1, mask 0."""
    q = f32([[1, 1, -1, 1, 1, 1, 1, 9, -1],
             [1, 1, 1, 1, 2, -1, 2, 1, -1],
             [1, 1, -1, 1, 1, 1, 1, -3, -1],
             [3.5, 3.5, -1, 3.5, 3.5, 1, 3.9, 3.9, 0],
             [10, 10, 1, 11, 10, 1, 10, 11, 1]])
    ref = SX.reference(f32([T0]), q, pairs=[[0, 0], [3, 0], [4, 0], [0, 1], [5, 0], [-1, 0]])
    assert ref["count"].tolist() == [1, 1, 1, 0, 0] and ref["offsets"].tolist() == [0, 1, 2, 3, 3, 3] and ref["tri"].tolist() == [0, 0, 0]
    assert ref["mask"].tolist() == [0b010001, 0b000101, 0b001001] and ref["ends"].tolist() == [0 | 4 << 3, 0 | 2 << 3, 0 | 3 << 3]
    assert ref["seg"].tolist() == [[[1, 1, 0], [1, 3, 0]], [[1, 1.5, 0], [1.5, 1, 0]], [[1, 1, 0], [1, 0, 0]]]
    assert ref["d2"][0, SX.PAIRS.index((0, 4))] == 4.0 and np.isnan(np.delete(ref["d2"][0], SX.PAIRS.index((0, 4)))).all()
    assert ref["pair_mask"].tolist() == [17, 0, 0, 0, 0, 0] and ref["pair_ends"].tolist() == [32, -1, -1, -1, -1, -1]
    assert SX.same_bits(ref["pair_seg"][0], ref["seg"][0]) and np.isnan(ref["pair_seg"][1:]).all()
    assert np.array_equal(OX.cand_numpy(f32([T0]), q)[:, 0], [True, True, True, True, False])  # (4) is a cand pair, (5) is not


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("fam", OX.FAMILIES)
def test_the_lists_and_masks_are_overlap_exacts(fam, moved):
    """The segment reference lists what the list reference lists, and its recomputed masks are the stored ones, on every entry; `ends`
    names two set bits of the mask in ascending order, or one bit twice exactly when the mask has one bit; every endpoint is finite."""
    for c in SX.family_case(fam, moved):
        ref, s, what = c["ref"], c["sref"], (fam, c["mesh"], moved)
        for key, other in (("count", "count"), ("offsets", "offsets"), ("tri", "tri"), ("mask", "edges")):
            assert np.array_equal(s[key], ref[other]), (what, key)
        assert s["entries"] == ref["overlaps"] and s["invalid"] == ref["invalid"]
        b, e = s["ends"] & 7, s["ends"] >> 3
        nbits = ((s["mask"][:, None] >> np.arange(6)) & 1).sum(1)
        assert (s["ends"] >= 0).all() and (b <= e).all() and (e < 6).all(), what
        assert (((s["mask"] >> b) & 1) == 1).all() and (((s["mask"] >> e) & 1) == 1).all(), what
        assert np.array_equal(b == e, nbits == 1), what
        assert np.isfinite(s["seg"]).all(), what


def test_a_touch_returns_the_same_point_twice():
    """Every one-bit entry: both endpoints are the pierce point, bit for bit, and every d2 is NaN (no pair).  Family b on the terrain -
    the mesh asked with its own triangles - has 458 of them."""
    seen = 0
    for fam in ("a", "b"):
        for c in SX.family_case(fam):
            s = c["sref"]
            one = ((s["mask"][:, None] >> np.arange(6)) & 1).sum(1) == 1
            assert SX.same_bits(s["seg"][one, 0], s["seg"][one, 1]) and np.isnan(s["d2"][one]).all()
            assert np.array_equal(s["ends"][one], np.log2(s["mask"][one]).astype(np.int32) * 9)  # b | b << 3
            seen += int(one.sum())
            if (fam, c["mesh"]) == ("b", "terrain"):
                assert (len(one), int(one.sum())) == (544, 458)
    assert seen == 460


def test_the_chosen_pair_is_the_farthest():
    """The selection rule against the d2 values the native program emits for every pair of set bits: the chosen pair's d2 is not smaller
    than any other's, no earlier pair (lexicographic) has the same d2, and the endpoints' own distance is that d2.  The four three-bit
    entries of family b on the terrain (and one on the moved terrain) are what gives the rule a choice."""
    three = 0
    for moved in (False, True):
        for fam in SX.CHECKED_FAMILIES:
            for c in SX.family_case(fam, moved):
                s = c["sref"]
                b, e = s["ends"] & 7, s["ends"] >> 3
                pair = b != e
                col = np.array([SX.PAIRS.index((int(x), int(y))) if x != y else 0 for x, y in zip(b, e)], np.int64)
                d2 = s["d2"][pair]
                chosen = d2[np.arange(len(d2)), col[pair]]
                assert not np.isnan(chosen).any() and (chosen[:, None] >= np.where(np.isnan(d2), -np.inf, d2)).all(), (fam, c["mesh"], moved)
                earlier = np.arange(15)[None, :] < col[pair][:, None]
                assert not (earlier & (d2 == chosen[:, None])).any(), (fam, c["mesh"], moved)
                w = (s["seg"][pair, 1] - s["seg"][pair, 0]).astype(f32).astype(np.float64)  # (three squares, summed with three roundings of 2^-24)
                assert (np.abs(chosen - (w * w).sum(1)) <= 4 * 2.0 ** -24 * chosen).all(), (fam, c["mesh"], moved)
                nbits = ((s["mask"][:, None] >> np.arange(6)) & 1).sum(1)
                assert np.array_equal((~np.isnan(s["d2"])).sum(1), nbits * (nbits - 1) // 2)
                many = nbits >= 3
                three += int(many.sum())
                if (fam, c["mesh"], moved) == ("b", "terrain", False):
                    # neighbours that meet in a vertex: three edges pierce there, and in two of the four all three points coincide (d2 = 0)
                    assert int(many.sum()) == 4 and int((chosen[many[pair]] > 0).sum()) == 2
    assert three >= 5


def test_a_planted_pair_without_cand_is_not_answered():
    """A pair whose boxes are disjoint, and a cand pair whose mask is 0: NaNs and ends = -1; the listed pairs asked for the same way get
    their entries' answers."""
    c = next(c for c in SX.family_case("a") if c["mesh"] == "terrain")
    ref, s = c["ref"], c["sref"]
    cand = OX.cand_numpy(c["verts"], c["q"])
    far = np.argwhere(~cand)[:50]
    quiet = np.stack([ref["pair_q"], ref["pair_t"]], 1)[ref["pair_mask"] == 0][:50]
    listed = np.stack([SX.owners(s["offsets"]), s["tri"]], 1)
    assert len(far) == 50 and len(quiet) == 50 and len(listed) > 50
    got = SX.reference(c["verts"], c["q"], pairs=np.concatenate([far, quiet, listed]))
    assert (got["pair_mask"][:100] == 0).all() and (got["pair_ends"][:100] == -1).all() and np.isnan(got["pair_seg"][:100]).all()
    assert np.array_equal(got["pair_mask"][100:], s["mask"]) and np.array_equal(got["pair_ends"][100:], s["ends"]) and SX.same_bits(got["pair_seg"][100:], s["seg"])


def test_the_float64_contract():
    """Every checked entry of families a, b, c, d, on every mesh, on still and on moved vertices, lies within E x S of the float64
    interval method's segment, as an unordered pair; the checked class covers at least 99 % of the entries of families a, c and d; an
    endpoint moved by 2 E S, and a segment returned as a touch, are seen."""
    worst, covered, entries, checked_total = 0.0, 0, 0, 0
    for moved in (False, True):
        for fam in SX.CHECKED_FAMILIES:
            for c in SX.family_case(fam, moved):
                checked, err = SX.errors(c["verts"], c["q"], c["sref"])
                print(f"family {fam} {c['mesh']} {'moved' if moved else 'still'}: {int(checked.sum())} of {len(err)} checked, largest err {float(err[checked].max()) if checked.any() else 0.0:.3g}")
                assert (err[checked] <= SX.E).all(), (fam, c["mesh"], moved, float(err[checked].max()))
                worst = max(worst, float(err[checked].max()) if checked.any() else 0.0)
                checked_total += int(checked.sum())
                if fam in SX.COVERED_FAMILIES and not moved:
                    covered += int(checked.sum())
                    entries += len(err)
    print(f"E_measured = {worst:.3g}, E = {SX.E:.3g}; the checked class covers {covered} of {entries} entries of families a, c, d; {checked_total} checked entries in all")
    assert entries > 1000 and covered >= 0.99 * entries
    assert SX.E == 2.0 ** -11 and 16 * SX.E_MEASURED <= SX.E < 32 * SX.E_MEASURED and worst <= SX.E_MEASURED * 1.005
    # the contract sees a wrong answer
    c = next(c for c in SX.family_case("c") if c["mesh"] == "terrain")
    checked, err = SX.errors(c["verts"], c["q"], c["sref"])
    k = int(np.nonzero(checked)[0][0])
    s_k = float(SX.scale_of(c["verts"], c["q"], SX.owners(c["sref"]["offsets"])[k:k + 1], c["sref"]["tri"][k:k + 1])[0])
    for wrong in ("moved", "touch"):
        bad = dict(c["sref"], seg=c["sref"]["seg"].copy())
        if wrong == "moved":
            bad["seg"][k, 1, 0] += f32(2 * SX.E * s_k)
        else:
            bad["seg"][k, 1] = bad["seg"][k, 0]
        assert SX.errors(c["verts"], c["q"], bad)[1][k] > SX.E, wrong


@pytest.mark.parametrize("k", [-16, 14])
def test_the_reference_is_covariant_under_scale(k):
    """Every length x 2^k: the same lists, masks and `ends`, and endpoints that scale exactly (what tests/test_gpu_overlap_segments.py asks
    of the kernel)."""
    for fam in ("a", "b", "c"):
        for c in SX.family_case(fam):
            if c["mesh"] not in ("soup", "grid", "terrain", "needle"):
                continue
            ref = SX.reference(np.ldexp(c["verts"], k).astype(f32), np.ldexp(c["q"], k).astype(f32))
            for key in ("count", "offsets", "tri", "mask", "ends"):
                assert np.array_equal(ref[key], c["sref"][key]), (fam, c["mesh"], key)
            assert SX.same_bits(ref["seg"], np.ldexp(c["sref"]["seg"], k).astype(f32)), (fam, c["mesh"])


def test_the_reference_is_clean_under_asan_and_ubsan():
    """Family e on the grid (coplanar, degenerate, far, invalid queries), family d on the needle mesh and family b on the terrain (the
    one- and three-bit entries), with planted pairs in and out of range, through the sanitised build run as a program of its own."""
    for c in (SX.family_case("e")[0], SX.family_case("d")[0], next(c for c in SX.family_case("b") if c["mesh"] == "terrain")):
        pairs = [[0, 0], [len(c["q"]) - 1, len(c["verts"]) - 1], [len(c["q"]), 0], [0, len(c["verts"])], [-1, -1]]
        clean = SX.reference(c["verts"], c["q"], pairs=pairs, sanitized=True)
        for key in ("count", "offsets", "tri", "mask", "ends"):
            assert np.array_equal(clean[key], c["sref"][key]), key
        assert SX.same_bits(clean["seg"], c["sref"]["seg"]) and SX.same_bits(clean["d2"], c["sref"]["d2"])
        assert (clean["pair_ends"][2:] == -1).all() and np.isnan(clean["pair_seg"][2:]).all()
