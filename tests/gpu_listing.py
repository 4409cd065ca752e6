"""The listing protocol of the query kinds that answer with a list per item (all hits, neighbours, overlaps), described once
(Listing) and tested once: count, fill on the count's offsets, and list = both in one call, with a capacity, offsets that are always
the full sums, slices that fit or are not touched, and stats that say what was written.  The product has them as one template too
(listing_call<K> in csrc/rt_abi_query.hip, Renderer._list_listing).

A batch is `src`, the tuple of numpy arrays the wrapper takes in order (None for an optional one left out), and `ref`, the
reference dict of the kind's *_exact module for exactly those rows.

Test helper (imported by the three tests/test_gpu_*_query.py files of these kinds); not a conftest, no fixtures."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gpu_query as Q
import native_ref as NR
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, ptr, tdev

f32 = np.float32


@dataclasses.dataclass(frozen=True)
class Listing:
    """One listing kind.  stem: of rt_{count,fill,list}_<stem>_device and of Renderer.count_<stem> / list_<stem>; stats: the
    Renderer method that reads its counters, stats_class / params: its ctypes classes in raytracing_engine_amd; items, invalid,
    found, written, incomplete: the names of the counters for the items asked, the invalid ones, the entries found, the entries
    written and the items whose slice did not fit; total, key: the reference dict's keys for the number of entries and for the
    array that comes with `tri`; key_dtype: that array's type; tri_first: (tri, key) and not (key, tri) is the order of the
    wrapper's tuple and of the library's arguments; raw_tail: what follows the source pointers in a C call (the neighbours'
    rmax_all), null_source: the source arguments of a call with n = 0 and nothing to read.
    What the three texts differed in when they were written one by one, kept as it was: count_kw, the keywords check_case counts
    with; exact_work, whether the reference has made the host-built tree's walk (nodes_total, tris_total); fill_walks_uncounted,
    whether check_case asserts nodes_visited == 0 of a fill step that did not ask for the walk's counters."""
    stem: str
    stats: str
    stats_class: str
    params: str
    items: str
    invalid: str
    found: str
    written: str
    incomplete: str
    total: str
    key: str
    key_dtype: type
    tri_first: bool = False
    raw_tail: tuple = ()
    null_source: tuple = ()
    count_kw: tuple = ()
    exact_work: bool = True
    fill_walks_uncounted: bool = True

    @property
    def payload(self):
        """((reference key, dtype), (reference key, dtype)) of the two entry arrays in the wrapper's and the library's order."""
        pair = ((self.key, self.key_dtype), ("tri", np.int32))
        return pair[::-1] if self.tri_first else pair

    def functions(self):
        return tuple(f"rt_{step}_{self.stem}_device" for step in ("count", "fill", "list"))

    def entries(self, renderer):
        """(count, list, stats) of a renderer and (count, fill, list) of the library."""
        lib = R.load()
        return ((getattr(renderer, "count_" + self.stem), getattr(renderer, "list_" + self.stem), getattr(renderer, self.stats)),
                tuple(getattr(lib, name) for name in self.functions()))

    def raw(self, tensors):
        """The source arguments of a C call on the device tensors of a batch."""
        return tuple(ptr(x) for x in tensors) + self.raw_tail

    def new_params(self, **kw):
        return getattr(R, self.params)(**kw)

    def new_payload(self, rows, guard=0):
        """The two entry arrays, rows + guard long, filled with -7."""
        import torch

        return tuple(Q.sentinel(rows, torch.float32 if dt == f32 else torch.int32, guard) for _, dt in self.payload)


HITS = Listing("ray_hits", "hit_query_stats", "HitQueryStats", "HitQueryParams", "rays", "invalid_rays", "hits", "hits_written", "incomplete_rays",
               total="hits", key="t", key_dtype=f32, null_source=(None, None, None), exact_work=False, fill_walks_uncounted=False)
NEIGHBORS = Listing("neighbors", "neighbor_query_stats", "NeighborQueryStats", "NeighborQueryParams", "points", "invalid_points", "neighbors",
                    "neighbors_written", "incomplete_points", total="neighbors", key="dist", key_dtype=f32, raw_tail=(0.0,),
                    null_source=(None, None, 1.0), count_kw=(("count_traversal", True),))
OVERLAPS = Listing("overlaps", "overlap_query_stats", "OverlapQueryStats", "OverlapQueryParams", "triangles", "invalid_triangles", "overlaps",
                   "overlaps_written", "incomplete_triangles", total="overlaps", key="edges", key_dtype=np.int32, tri_first=True,
                   null_source=(None,), count_kw=(("count_traversal", True),))
KINDS = (HITS, NEIGHBORS, OVERLAPS)


def expected_fill(foreign, capacity, offsets, count):
    """What the fill step does on `foreign` offsets (n + 1) it did not make, for items whose lists have `count` entries (an invalid
    item's negative count: none) and stand at `offsets` in the reference: item i has the slice [foreign[i], foreign[i + 1]); a slice
    that is reversed or not within [0, capacity) gets nothing, every other one its list's first entries as far as it is long.
    Returns dict(src, dst: the reference's entries and where they go; written: how many; beyond: the entries that found no room in
    a slice of their own length (slice_overflow); incomplete: the items with entries whose slice is not one they can use whole)."""
    foreign, count = np.asarray(foreign, np.int64), np.asarray(count, np.int64)
    lo, hi = foreign[:-1], foreign[1:]
    length = np.maximum(hi - lo, 0)
    room = np.where((lo >= 0) & (hi <= capacity), length, 0)
    keep = np.minimum(room, np.maximum(count, 0))
    within = np.arange(keep.sum()) - np.repeat(np.cumsum(keep) - keep, keep)
    return dict(src=np.repeat(np.asarray(offsets, np.int64)[:-1], keep) + within, dst=np.repeat(lo, keep) + within, written=int(keep.sum()),
                beyond=int(np.maximum(count - length, 0).sum()), incomplete=int(((count > 0) & (room != length)).sum()))


def check_lists(kind, got, ref, what):
    """The wrapper's four tensors against a reference dict, bit for bit."""
    offsets, a, b, counts = (x.cpu().numpy() for x in got)
    (key_a, type_a), (key_b, type_b) = kind.payload
    assert counts.dtype == np.int32 and np.array_equal(counts, ref["count"]), (what, np.nonzero(counts != ref["count"])[0][:8])
    assert offsets.dtype == np.int64 and np.array_equal(offsets, ref["offsets"]), what
    assert a.dtype == type_a and b.dtype == type_b and len(a) == len(b), (what, a.dtype, b.dtype, len(a), len(b))
    k = ref[kind.total]
    for x, key in ((a, key_a), (b, key_b)):
        assert NR.same_bits(x[:k], ref[key]), (what, key, np.nonzero(x[:k] != ref[key])[0][:8] if len(x) >= k else len(x))


def check_case(renderer, kind, src, ref, what, exact_work=False, **kw):
    """The three ways to ask against the reference: count, list without a capacity (count + fill), list with one.  exact_work: the
    tree is the host-built single-level one, whose walk the reference has made: nodes and triangles agree exactly."""
    (count, lst, stats), _ = kind.entries(renderer)
    n, k = len(src[0]), ref[kind.total]
    t = tuple(tdev(x) for x in src)
    assert kind.exact_work or not exact_work, (what, "the reference has no walk")
    counts = count(*t, **dict(kind.count_kw), **kw)
    st = stats()
    assert np.array_equal(counts.cpu().numpy(), ref["count"]), (what, np.nonzero(counts.cpu().numpy() != ref["count"])[0][:8])
    assert (st[kind.items], st[kind.invalid], st[kind.found], st[kind.written], st["stack_overflow"], st["launches"]) == (n, ref["invalid"], k, 0, 0, 1) \
        and st["ms"] > 0, (what, st)
    if exact_work:  # what is culled is fixed, so the work does not depend on the order of the walk
        assert (st["nodes_visited"], st["tris_tested"]) == (ref["nodes_total"], ref["tris_total"]), (what, st, ref["nodes_total"], ref["tris_total"])
    got = lst(*t, **kw)
    st = stats()  # of the fill step
    assert len(got[1]) == k, (what, len(got[1]), k)
    check_lists(kind, got, ref, what)
    assert (st[kind.items], st[kind.invalid], st[kind.found], st[kind.written], st[kind.incomplete], st["slice_overflow"], st["stack_overflow"], st["launches"]) == \
        (n, ref["invalid"], k, k, 0, 0, 0, 1), (what, st)
    if kind.fill_walks_uncounted:
        assert st["nodes_visited"] == 0, (what, st)
    got = lst(*t, capacity=k + 3, **kw)
    st = stats()
    check_lists(kind, got, ref, what)
    assert (st[kind.items], st[kind.invalid], st[kind.found], st[kind.written], st[kind.incomplete], st["slice_overflow"], st["stack_overflow"], st["launches"]) == \
        (n, ref["invalid"], k, k, 0, 0, 0, 5) and st["ms"] > 0, (what, st)


def scan_around_its_tile(renderer, kind, src, ref, what):
    """One list call with the capacity at the total: for batches whose n + 1 offsets lie around the scan's tile."""
    (_, lst, stats), _ = kind.entries(renderer)
    k = ref[kind.total]
    got = lst(*(tdev(x) for x in src), capacity=k)
    check_lists(kind, got, ref, what)
    st = stats()
    assert (st[kind.items], st[kind.found], st[kind.written], st[kind.incomplete], st["slice_overflow"], st["launches"]) == (len(src[0]), k, k, 0, 0, 5), (what, st)


def capacity(renderer, kind, src, ref):
    """Capacity at the total, one below it, half of it and 0: a slice that does not fit is not touched, every other one is complete, the
    offsets are the full sums.  Then the caller's second try: the fill step alone on the offsets it has."""
    (_, lst, stats), (_, fill, _) = kind.entries(renderer)
    n, total, off = len(src[0]), ref[kind.total], ref["offsets"]
    t = tuple(tdev(x) for x in src)
    (key_a, _), (key_b, _) = kind.payload
    for cap in (total, total - 1, total // 2, 0):
        for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
            a_buf, b_buf = kind.new_payload(cap, 64)
            offsets, _, _, counts = lst(*t, capacity=cap, out=(None, a_buf[:cap], b_buf[:cap], None), **kw)
            st = stats()
            fits = off[1:] <= cap
            written = int(off[1:][fits].max()) if fits.any() else 0  # the slices that fit are a prefix of the items
            incomplete = int(((ref["count"] > 0) & ~fits).sum())
            assert np.array_equal(offsets.cpu().numpy(), off) and np.array_equal(counts.cpu().numpy(), ref["count"]), cap
            ga, gb = a_buf.cpu().numpy(), b_buf.cpu().numpy()
            assert NR.same_bits(ga[:written], ref[key_a][:written]) and NR.same_bits(gb[:written], ref[key_b][:written]), (cap, kw)
            assert Q.still_sentinel(ga, 0, written) and Q.still_sentinel(gb, 0, written), (cap, kw)
            assert (st[kind.found], st[kind.written], st[kind.incomplete], st["slice_overflow"], st["stack_overflow"]) == (total, written, incomplete, 0, 0), (cap, kw, st)
            assert (cap == total) == (incomplete == 0) and (cap > 0 or written == 0), (cap, incomplete, written)
    a, b = kind.new_payload(total)
    prm = kind.new_params()
    assert fill(renderer._ctx, *kind.raw(t), n, C.byref(prm), ptr(offsets), total, ptr(a), ptr(b)) == 0, "second try"
    st = stats()  # (waits for it)
    assert (st[kind.found], st[kind.written], st[kind.incomplete], st["launches"]) == (total, total, 0, 1), st
    check_lists(kind, (offsets, a, b, counts), ref, "second try")


def foreign_offsets(renderer, kind, src, ref):
    """The fill step on offsets it did not make: nothing outside [0, capacity) is written, a slice shorter than its item's list keeps the
    first entries, and slice_overflow counts the rest (expected_fill).  And on the count step's own offsets: no overflow."""
    (_, _, stats), (_, fill, _) = kind.entries(renderer)
    n, total, off, count = len(src[0]), ref[kind.total], ref["offsets"], ref["count"]
    t = tuple(tdev(x) for x in src)
    (key_a, type_a), (key_b, type_b) = kind.payload
    guard = 4096
    cases = {"halved": off // 2, "shifted up": off + 1000, "shifted down": off - 1000, "reversed": off[::-1].copy(), "far": off + (1 << 40),
             "negative": -off - 1, "zeros": np.zeros(n + 1, np.int64)}
    for name, foreign in cases.items():
        for cap in (total, total // 3):
            a_buf, b_buf = kind.new_payload(cap, 2 * guard)
            fo = tdev(np.ascontiguousarray(foreign, np.int64))
            assert fill(renderer._ctx, *kind.raw(t), n, None, ptr(fo), cap, ptr(a_buf[guard:]), ptr(b_buf[guard:])) == 0, (name, cap)
            st = stats()
            exp = expected_fill(foreign, cap, off, count)
            exp_a, exp_b = np.full(cap + 2 * guard, Q.SENTINEL, type_a), np.full(cap + 2 * guard, Q.SENTINEL, type_b)
            ga, gb = a_buf.cpu().numpy(), b_buf.cpu().numpy()
            assert Q.still_sentinel(ga, guard, guard + cap) and Q.still_sentinel(gb, guard, guard + cap), (name, cap)
            exp_a[guard + exp["dst"]], exp_b[guard + exp["dst"]] = ref[key_a][exp["src"]], ref[key_b][exp["src"]]
            assert NR.same_bits(ga, exp_a) and NR.same_bits(gb, exp_b), (name, cap)
            assert (st[kind.found], st[kind.written], st["slice_overflow"], st["stack_overflow"], st["launches"]) == (total, exp["written"], exp["beyond"], 0, 1), (name, cap, st)
            assert st[kind.incomplete] == exp["incomplete"], (name, cap, st)
            if name in ("halved", "reversed", "negative", "zeros"):
                assert st["slice_overflow"] > 0, name
    (a_own, b_own), own = kind.new_payload(total), tdev(off)
    assert fill(renderer._ctx, *kind.raw(t), n, None, ptr(own), total, ptr(a_own), ptr(b_own)) == 0, "own offsets"
    assert stats()["slice_overflow"] == 0, "own offsets"


def list_is_count_then_fill(renderer, kind, src, ref):
    """The list call against the count and the fill call on the same arrays: the same four outputs, and stats that add up."""
    import torch

    (_, _, stats), (count, fill, lst) = kind.entries(renderer)
    ctx, n, total = renderer._ctx, len(src[0]), ref[kind.total]
    t = tuple(tdev(x) for x in src)  # (held: raw has only their addresses)
    raw = kind.raw(t)
    for cap in (total, total // 2):
        c1, o1, (a1, b1) = Q.sentinel(n, torch.int32), Q.sentinel(n + 1, torch.int64), kind.new_payload(cap)
        c2, o2, (a2, b2) = Q.sentinel(n, torch.int32), Q.sentinel(n + 1, torch.int64), kind.new_payload(cap)
        prm = kind.new_params(count_traversal=1)
        assert lst(ctx, *raw, n, C.byref(prm), ptr(c1), ptr(o1), cap, ptr(a1), ptr(b1)) == 0, cap
        both = stats()
        assert count(ctx, *raw, n, C.byref(prm), ptr(c2), ptr(o2)) == 0, cap
        counted = stats()
        assert fill(ctx, *raw, n, C.byref(prm), ptr(o2), cap, ptr(a2), ptr(b2)) == 0, cap
        filled = stats()
        assert torch.equal(c1, c2) and torch.equal(o1, o2) and torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and torch.equal(b1.view(torch.int32), b2.view(torch.int32)), cap
        assert (counted["launches"], filled["launches"], both["launches"]) == (4, 1, 5), (counted, filled, both)
        for key in (kind.items, kind.invalid, kind.found):
            assert both[key] == counted[key] == filled[key], key
        for key in (kind.written, kind.incomplete, "slice_overflow"):
            assert both[key] == filled[key] and counted[key] == 0, key
        for key in ("nodes_visited", "tris_tested"):  # the two walks are the same walk
            assert counted[key] == filled[key] > 0 and both[key] == 2 * counted[key], key
    # offsets without counts, counts without offsets
    o3, c3 = Q.sentinel(n + 1, torch.int64), Q.sentinel(n, torch.int32)
    assert count(ctx, *raw, n, None, None, ptr(o3)) == 0, "offsets alone"
    assert count(ctx, *raw, n, None, ptr(c3), None) == 0, "counts alone"
    renderer.synchronize()
    assert np.array_equal(o3.cpu().numpy(), ref["offsets"]) and np.array_equal(c3.cpu().numpy(), ref["count"]), "one output each"


def bounds_and_out_tensors(renderer, kind, batches):
    """Sentinels behind every output; the inputs are only read.  batches: [(src, ref)], each with more items than the one before."""
    import torch

    (count, lst, _), _ = kind.entries(renderer)
    for src, ref in batches:
        n, k = len(src[0]), ref[kind.total]
        t = tuple(tdev(x) for x in src)
        keep = [x.clone() for x in t]
        c_buf, o_buf, (a_buf, b_buf) = Q.sentinel(n, torch.int32, 64), Q.sentinel(n + 1, torch.int64, 64), kind.new_payload(k, 64)
        got = lst(*t, capacity=k, out=(o_buf[:n + 1], a_buf[:k], b_buf[:k], c_buf[:n]))
        assert [x.data_ptr() for x in got] == [o_buf.data_ptr(), a_buf.data_ptr() if k else got[1].data_ptr(), b_buf.data_ptr() if k else got[2].data_ptr(), c_buf.data_ptr()], n
        check_lists(kind, got, ref, n)
        assert Q.still_sentinel(c_buf, 0, n) and Q.still_sentinel(o_buf, 0, n + 1) and Q.still_sentinel(a_buf, 0, k) and Q.still_sentinel(b_buf, 0, k), n
        c_buf.fill_(Q.SENTINEL)
        counts = count(*t, out=c_buf[:n])
        assert counts.data_ptr() == c_buf.data_ptr() and Q.still_sentinel(c_buf, 0, n) and np.array_equal(counts.cpu().numpy(), ref["count"]), n
        for x, y in zip(t, keep):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), n
    with pytest.raises(ValueError):
        count(*t, out=c_buf[:n - 1])
    with pytest.raises(ValueError):
        lst(*t, capacity=k, out=(o_buf[:n], a_buf[:k], b_buf[:k], c_buf[:n]))


def stream_order(renderer, kind, src, ref):
    """The first source array made by torch on a stream (halving and doubling is exact), the queries behind it on that stream without
    a host synchronisation, a torch reduction of the answers behind the queries; one synchronisation at the end."""
    import torch

    (count, lst, _), _ = kind.entries(renderer)
    n, k = len(src[0]), ref[kind.total]
    half, rest = tdev(src[0] * f32(0.5)), tuple(tdev(x) for x in src[1:])
    (key_a, _), (key_b, _) = kind.payload
    ref_c, ref_o, ref_a, ref_b = tdev(ref["count"]), tdev(ref["offsets"]), tdev(ref[key_a]), tdev(ref[key_b])
    counts, counts2, offsets, (a, b) = Q.sentinel(n, torch.int32), Q.sentinel(n, torch.int32), Q.sentinel(n + 1, torch.int64), kind.new_payload(k)
    with Q.busy_stream(renderer):
        first = half * 2.0
        count(first, *rest, out=counts2, sync=False)
        lst(first, *rest, capacity=k, out=(offsets, a, b, counts), sync=False)
        wrong = (counts != ref_c).sum() + (counts2 != ref_c).sum() + (offsets != ref_o).sum() + (a.view(torch.int32) != ref_a.view(torch.int32)).sum() + \
            (b.view(torch.int32) != ref_b.view(torch.int32)).sum()
    assert int(wrong) == 0, int(wrong)


class Refusals:
    """test_errors_write_nothing of a listing kind: sentinel outputs for a batch, the pointers and parameters to refuse, and the
    steps of the test.  The rows of bad source arguments are the kind's signature and come from its module (tables())."""

    def __init__(self, renderer, kind, src, ref, **short):
        import torch

        self.renderer, self.kind, self.ref = renderer, kind, ref
        (self.count_w, self.list_w, _), self.lib = kind.entries(renderer)
        self.n, self.cap = len(src[0]), ref[kind.total]
        self.t = tuple(tdev(x) for x in src)
        self.cnt, self.off = Q.sentinel(self.n, torch.int32), Q.sentinel(self.n + 1, torch.int64)
        self.a, self.b = kind.new_payload(self.cap)
        self.good_off = tdev(ref["offsets"])
        self.good = kind.raw(self.t) + (self.n, None)
        self.bp = Q.bad_pointers(self.n, short1=4, short8=(8, self.n + 1), shortc=(4, self.cap), **short)  # one row short of n, n + 1 i64, capacity
        self.bad_params = Q.bad_params(getattr(R, kind.params))

    def untouched(self, what):
        Q.assert_untouched(self.renderer, (self.cnt, self.off, self.a, self.b), self.bp.big, what)

    def every_entry(self, ctx, code, what):
        """The three entries with nothing wrong in their arguments on a context that must answer `code`."""
        count, fill, lst = self.lib
        cnt, off, good_off, cap, a, b = ptr(self.cnt), ptr(self.off), ptr(self.good_off), self.cap, ptr(self.a), ptr(self.b)
        assert count(ctx, *self.good, cnt, off) == code, (what, "count")
        assert fill(ctx, *self.good, good_off, cap, a, b) == code, (what, "fill")
        assert lst(ctx, *self.good, cnt, off, cap, a, b) == code, (what, "list")
        self.untouched(what)

    def tables(self, sources):
        """Every row of `sources` (bad source arguments, n, params) in front of good outputs, and the good source in front of every
        bad output, through count, fill and list: refused, nothing written.  The pair: a refusal of the SECOND step comes before
        the first step is enqueued."""
        count, fill, lst = self.lib
        ctx, good, bp = self.renderer._ctx, self.good, self.bp
        hp, short1, short8, shortc = bp.hp, bp.short1, bp.short8, bp.shortc
        cnt, off, good_off, cap, a, b = ptr(self.cnt), ptr(self.off), ptr(self.good_off), self.cap, ptr(self.a), ptr(self.b)
        count_calls = [s + (cnt, off) for s in sources] + [good + x for x in ((None, None), (hp, off), (cnt, hp), (short1, off), (cnt, short8))]
        fill_calls = [s + (good_off, cap, a, b) for s in sources] + \
            [good + x for x in ((None, cap, a, b), (hp, cap, a, b), (short8, cap, a, b), (good_off, cap, None, b), (good_off, cap, a, None), (good_off, cap, hp, b),
                                (good_off, cap, a, hp), (good_off, cap, shortc, b), (good_off, cap, a, shortc), (good_off, 1 << 62, a, b))]
        list_calls = [s + (cnt, off, cap, a, b) for s in sources] + \
            [good + x for x in ((cnt, None, cap, a, b), (hp, off, cap, a, b), (cnt, hp, cap, a, b), (short1, off, cap, a, b), (cnt, short8, cap, a, b),
                                (cnt, off, cap, None, b), (cnt, off, cap, a, None), (cnt, off, cap, hp, b), (cnt, off, cap, a, hp), (cnt, off, cap, shortc, b),
                                (cnt, off, cap, a, shortc), (cnt, off, 1 << 62, a, b))]
        for step, fn, calls in (("count", count, count_calls), ("fill", fill, fill_calls), ("list", lst, list_calls)):
            for k, args in enumerate(calls):
                assert fn(ctx, *args) == RT_ERR_INVALID, (step, k)
                self.untouched((step, k))

    def nothing_to_do(self, empty, empty_with_capacity):
        """n = 0 is accepted, and does nothing; `empty`, `empty_with_capacity`: the wrappers' arguments for no items."""
        count, fill, lst = self.lib
        ctx, null = self.renderer._ctx, self.kind.null_source
        assert count(ctx, *self.good[:-2], 0, None, ptr(self.cnt), ptr(self.off)) == 0, "n = 0"
        assert count(ctx, *null, 0, None, None, None) == 0, "n = 0, count"
        assert fill(ctx, *null, 0, None, None, 0, None, None) == 0, "n = 0, fill"
        assert lst(ctx, *null, 0, None, None, None, 0, None, None) == 0, "n = 0, list"
        self.untouched("n = 0")
        assert len(self.count_w(*empty)) == 0, "no items"
        assert [len(x) for x in self.list_w(*empty)] == [1, 0, 0, 0], "no items"
        assert [len(x) for x in self.list_w(*empty_with_capacity, capacity=5)] == [1, 5, 5, 0], "no items, a capacity"

    def still_answers(self):
        check_lists(self.kind, self.list_w(*self.t, capacity=self.cap, out=(self.off, self.a, self.b, self.cnt)), self.ref, "after the refusals")
