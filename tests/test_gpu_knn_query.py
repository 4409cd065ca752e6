"""k-nearest queries on device tensors (Renderer.query_knn, rt_query_knn_device) on the GPU.

The reference is tests/knn_exact.py's native brute force (tests/native/knn_query_ref.cpp: the arithmetic of csrc/point_tri.h over all
triangles, everything with d2 < rmax * rmax, sorted by (d2, index), cut at k, no tree), which the kernel must match bit for bit in every
element of dist, tri and counts, padding and invalid rows included.  That reference in turn is held to its own tree walk, to the radius
query's and the closest-point reference and to float64 on the CPU (tests/test_knn_query_host.py).  The first tests run every family on
its meshes under every k and radius; the others need ONE batch on ONE mesh whose size they can cut, tile and plant points into: family
b's 300 points on the terrain under the ten finite radius variants and without a radius, shuffled, under k = 8."""
import functools

import numpy as np
import pytest

import knn_exact as KX
import neighbor_exact as NX
import point_exact as PX
import ray_exact as X
import raytracing_engine_amd as R
from gpu_query import RT_ERR_INVALID, RT_ERR_STATE, assert_untouched, bad_params, bad_pointers, busy_stream, dev, pt_frame, ptr, sentinel, still_sentinel, tdev
from gpu_query import set_mesh_with_surface as set_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = NX.INF
MISS, INVALID = KX.MISS, KX.INVALID


def check_rows(got, row, what):
    """(dist, tri, counts) as tensors against rows() of the reference, bit for bit, every element."""
    dist, tri, counts = (x.cpu().numpy() for x in got)
    assert dist.dtype == f32 and tri.dtype == np.int32 and counts.dtype == np.int32 and dist.shape == tri.shape == row["dist"].shape and counts.shape == row["count"].shape, what
    assert np.array_equal(counts, row["count"]), (what, np.nonzero(counts != row["count"])[0][:8])
    assert np.array_equal(tri, row["tri"]), (what, np.argwhere(tri != row["tri"])[:8])
    assert KX.same_bits(dist, row["dist"]), (what, np.argwhere(dist.view(np.uint32) != row["dist"].view(np.uint32))[:8])


def check_case(renderer, p, rmax, row, what, **kw):
    """query_knn of points p under radii rmax (None: without) and the reference rows' k against those rows, and the call's statistics."""
    got = renderer.query_knn(tdev(p), row["k"], rmax=tdev(rmax), count_traversal=True, **kw)
    st = renderer.knn_query_stats()
    check_rows(got, row, what)
    n, invalid, found = len(p), int((row["count"] == INVALID).sum()), int(np.maximum(row["count"], 0).sum())
    assert (st["points"], st["invalid_points"], st["neighbors"], st["stack_overflow"], st["launches"]) == (n, invalid, found, 0, 1) and st["ms"] > 0, (what, st)
    assert (st["nodes_visited"] > 0) == bool((row["nodes"] > 0).any()), (what, st)  # a walk where the reference walks
    return st


def check_every_k(renderer, c, what):
    """A part of a family on the mesh the renderer holds: the whole batch (every radius variant, and the block without a limit) under every
    k; that block once more with rmax = None; RT_KNN_MAX_K on the first points."""
    none = c["blocks"]["none"]
    for k in c["ks"]:
        row = c["ref"][k]
        check_case(renderer, c["p"], c["rmax"], row, what + (k,))
        cut = {key: (val[none] if isinstance(val, np.ndarray) else val) for key, val in row.items()}
        check_case(renderer, c["p"][none], None, cut, what + (k, "no rmax"))
    check_case(renderer, c["big"]["p"], None, c["big"]["ref"], what + (KX.BIG_K,))


# ---- 1. every family, every k, every radius, every tree ---------------------------------------------------------------------------

@pytest.mark.parametrize("fam", PX.FAMILIES)
def test_every_family_on_the_host_built_tree(renderer, fam):
    for c in KX.family_case(fam):
        set_mesh(renderer, c["verts"])
        check_every_k(renderer, c, (fam, c["mesh"]))


@pytest.mark.parametrize("tree", ["two-level", "device build", "refit to moved vertices"])
@pytest.mark.parametrize("fam", ["a", "b", "d"])
def test_two_level_device_built_and_refitted_trees(renderer, fam, tree):
    for c in (KX.family_case(fam, moved=True) if tree.startswith("refit") else KX.family_case(fam)):
        if tree == "two-level":
            renderer.set_mesh(*X._with_surface(c["verts"]), bvh_levels=2, blas_chunks=64)
        else:
            renderer.set_mesh_device(*(tdev(x) for x in X._with_surface(PX.mesh(c["mesh"]))))
            if tree.startswith("refit"):
                assert not np.array_equal(c["verts"], PX.mesh(c["mesh"]))
                renderer.refit_mesh_device(tdev(c["verts"]))
        check_every_k(renderer, c, (fam, c["mesh"], tree))


# ---- 2. one batch on the terrain ---------------------------------------------------------------------------------------------------
K = 8


@functools.lru_cache(maxsize=None)
def batch():
    c = KX.family_case("b")[0]
    assert c["mesh"] == "terrain"
    keep = np.concatenate([np.arange(c["blocks"]["inf"].start), np.arange(c["blocks"]["none"].start, c["blocks"]["none"].stop)])  # the finite radii, and none
    perm = keep[np.random.default_rng(13).permutation(len(keep))]
    p, rmax = np.ascontiguousarray(c["p"][perm]), np.ascontiguousarray(c["rmax"][perm])
    rows = {k: {key: (val[perm] if isinstance(val, np.ndarray) else val) for key, val in c["ref"][k].items()} for k in c["ks"]}
    unlimited = np.nonzero(perm >= c["blocks"]["none"].start)[0]
    assert ((rows[K]["count"] > 0) & (rows[K]["count"] < K)).sum() > 100 and (rows[K]["count"] == K).sum() > 300 and (rows[K]["count"] == 0).sum() > 100
    return dict(v=c["verts"], p=p, rmax=rmax, rows=rows, row=rows[K], n=len(p), reach=PX.reach_of(c["verts"]), unlimited=unlimited, case=c, perm=perm)


def set_batch(renderer):
    b = batch()
    set_mesh(renderer, b["v"])
    return b


def cut(row, sel):
    return {key: (val[sel] if isinstance(val, np.ndarray) else val) for key, val in row.items()}


def first(b, n, k=K):
    return b["p"][:n], b["rmax"][:n], cut(b["rows"][k], slice(0, n))


def test_against_query_points_and_list_neighbors_on_the_same_arrays(renderer):
    """k = 1 is query_points' (dist, tri) bit for bit; every row is the prefix of list_neighbors' slice for the same rmax."""
    import torch

    b = set_batch(renderer)
    tp, tr = tdev(b["p"]), tdev(b["rmax"])
    d1, t1, c1 = renderer.query_knn(tp, 1, rmax=tr)
    pd, pt, _ = renderer.query_points(tp, tr, want_points=False)
    assert torch.equal(d1[:, 0].view(torch.int32), pd.view(torch.int32)) and torch.equal(t1[:, 0], pt) and torch.equal(c1, (pt >= 0).int())
    limited = np.nonzero(np.isfinite(b["rmax"]))[0]  # (an unlimited list is the whole mesh: the +inf block of the neighbour tests)
    tpl, trl = tdev(b["p"][limited]), tdev(b["rmax"][limited])
    offsets, dist, tri, counts = (x.cpu().numpy() for x in renderer.list_neighbors(tpl, trl))
    lists = dict(count=counts, offsets=offsets, dist=dist, tri=tri, d2=dist)
    for k in (1, 2, 7, 8, 40):
        gd, gt, gc = (x.cpu().numpy() for x in renderer.query_knn(tpl, k, rmax=trl))
        assert KX.prefix_of_list(lists, dict(k=k, count=gc, dist=gd, tri=gt, d2=gd)), k
        assert KX.expected(gc, gd, gt)


def test_a_scalar_radius_is_a_tensor_of_it(renderer):
    import torch

    b = set_batch(renderer)
    p = b["p"][b["unlimited"]]
    tp = tdev(p)
    c = b["case"]
    for r in (float(np.median(NX.kth_dist(c["nx"]["free"], 8))), 0.0, -1.0, float("inf"), 2.0 ** -76, float("nan")):
        ref = KX.rows(KX.reference(b["v"], p, K, f32(r)), slice(None))
        one = renderer.query_knn(tp, K, rmax=r)
        many = renderer.query_knn(tp, K, rmax=torch.full((len(p),), r, dtype=torch.float32, device=dev()))
        for x, y in zip(one, many):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), r
        check_rows(one, ref, r)
        assert renderer.knn_query_stats()["invalid_points"] == (len(p) if r != r else 0)
    without = renderer.query_knn(tp, K)
    with_inf = renderer.query_knn(tp, K, rmax=float("inf"))
    for x, y in zip(without, with_inf):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_count_out_may_be_null(renderer):
    import torch

    b = set_batch(renderer)
    n = b["n"]
    tp, tr = tdev(b["p"]), tdev(b["rmax"])
    dist, tri = sentinel(n, torch.float32, cols=K), sentinel(n, torch.int32, cols=K)
    assert R.load().rt_query_knn_device(renderer._ctx, ptr(tp), ptr(tr), n, K, None, ptr(dist), ptr(tri), None) == 0
    st = renderer.knn_query_stats()
    assert KX.same_bits(dist.cpu().numpy(), b["row"]["dist"]) and np.array_equal(tri.cpu().numpy(), b["row"]["tri"])
    assert (st["points"], st["neighbors"], st["nodes_visited"], st["tris_tested"]) == (n, int(np.maximum(b["row"]["count"], 0).sum()), 0, 0)  # count_traversal = 0


TUNINGS = [dict(tune_max_blocks=1, tune_refill_min=1), dict(tune_max_blocks=1, tune_refill_min=24), dict(tune_max_blocks=1, tune_refill_min=64)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 1023, 1024, 1025])
def test_batch_edges_and_refill(renderer, n):
    """One workgroup (tune_max_blocks = 1) has 4 waves for the 16 streams: every stream is reached only by waves moving on from a dry
    one, and with 1 000 points every lane refills.  16 streams of 64 entries: 1 023 / 1 024 / 1 025 are the first sizes at which a wave's home stream is dry
    while others are not."""
    b = set_batch(renderer)
    assert n <= b["n"]
    for k in (K, 1, 40):
        p, rmax, row = first(b, n, k)
        for kw in TUNINGS:
            check_case(renderer, p, rmax, row, (n, k, kw), **kw)


def test_more_points_than_lanes(renderer):
    """600 000 points with k = 4: the batch drawn by a fixed scatter; the reference answers the batch once and is gathered."""
    b = set_batch(renderer)
    n = 600000
    assert n > 256 * 8 * 256
    ref = KX.rows(KX.reference(b["v"], b["p"], 4, b["rmax"]), slice(None))
    idx = (np.arange(n, dtype=np.int64) * 2654435761) % b["n"]
    check_case(renderer, b["p"][idx], b["rmax"][idx], cut(ref, idx), n)


def test_stack_spill(renderer):
    """tune_lds_stack = 1: one entry of every lane's stack in LDS, the rest in global memory; no overflow (check_case asserts it)."""
    b = set_batch(renderer)
    assert renderer.pt_stats()["bvh_depth"] > 2
    for k in (K, 40):
        check_case(renderer, b["p"], b["rmax"], b["rows"][k], ("one LDS entry", k), tune_lds_stack=1)
    c = KX.family_case("f")[0]
    set_mesh(renderer, c["verts"])
    check_case(renderer, c["p"], c["rmax"], c["ref"][7], "one LDS entry, duplicated soup", tune_lds_stack=1)


def test_pruning_happens(renderer):
    """Family b on the terrain with k = 8 and no rmax: mean triangles tested per point <= n_tris / 8 = 144 (brute force: n_tris).  A bound,
    not an equality with the reference walk: the kernel pushes siblings in slot order and a shrinking bound makes the work depend on order."""
    b = set_batch(renderer)
    sel = b["unlimited"]
    n, n_tris = len(sel), len(b["v"])
    assert n_tris == 1154
    st = check_case(renderer, b["p"][sel], None, cut(b["row"], sel), "pruning")
    print(f"terrain, family b, k = 8, no rmax: {st['tris_tested'] / n:.2f} triangles and {st['nodes_visited'] / n:.2f} nodes per point ({n_tris} triangles);"
          f" the reference walk: {b['row']['tris'][sel].mean():.2f} and {b['row']['nodes'][sel].mean():.2f}")
    assert st["stack_overflow"] == 0 and 0 < st["tris_tested"] / n <= n_tris / 8
    renderer.query_knn(tdev(b["p"][sel][:100]), K)
    st = renderer.knn_query_stats()
    assert (st["nodes_visited"], st["tris_tested"]) == (0, 0)  # count_traversal = 0: not counted


# ---- 3. invalid points, bounds, refusals -------------------------------------------------------------------------------------------

def test_invalid_points(renderer):
    b = set_batch(renderer)
    reach, n = b["reach"], b["n"]
    rng = np.random.default_rng(43)
    where = rng.permutation(n)
    p, rmax = b["p"].copy(), b["rmax"].copy()
    invalid = np.zeros(n, bool)
    k = 0
    for comp in range(3):  # a NaN or an infinity in one component
        for bad in (np.nan, np.inf, -np.inf):
            p[where[k], comp] = bad
            invalid[where[k]] = True
            k += 1
    for comp in range(3):  # one step beyond the reach
        for sign in (1, -1):
            p[where[k], comp] = sign * np.nextafter(reach, INF)
            invalid[where[k]] = True
            k += 1
    rmax[where[k:k + 3]] = np.nan
    invalid[where[k:k + 3]] = True
    k += 3
    edge = where[k:k + 12]  # exactly at the reach: valid
    for j, i in enumerate(edge):
        p[i, j % 3] = (1 if j % 2 else -1) * reach
    rmax[edge[:6]] = INF  # and every triangle is within +inf of them
    k += 12
    nothing = where[k:k + 9]  # valid, and no neighbour: no radius
    rmax[nothing[:3]], rmax[nothing[3:6]], rmax[nothing[6:]] = 0.0, -INF, 2.0 ** -76
    for kk in (K, 1):
        ref = KX.reference(b["v"], p, kk, rmax)
        exp = KX.rows(ref, slice(None))
        assert KX.walk_is_brute(ref) and np.array_equal(exp["count"] == INVALID, invalid) and (exp["count"][edge[:6]] == kk).all() and (exp["count"][nothing] == 0).all()
        assert np.isnan(exp["dist"][invalid]).all() and (exp["tri"][invalid] == INVALID).all()  # the whole row
        for kw in (dict(), dict(tune_max_blocks=1, tune_refill_min=1)):
            check_case(renderer, p, rmax, exp, ("invalid points", kk, kw), **kw)
    # the early-exit trap: refills that hand out 64 entries and leave no lane alive - 4 000 invalid points through one workgroup
    p_bad = np.tile(b["p"], (2, 1))[:4000].copy()
    p_bad[:, 1] = np.nan
    dist, tri, counts = renderer.query_knn(tdev(p_bad), K, rmax=1.0, tune_max_blocks=1)
    st = renderer.knn_query_stats()
    assert (counts == INVALID).all() and (tri == INVALID).all() and bool(dist.isnan().all())
    assert (st["invalid_points"], st["neighbors"], st["points"]) == (4000, 0, 4000)
    p_bad = b["p"].copy()
    p_bad[:1024, 2] = -np.inf
    exp = KX.rows(KX.reference(b["v"], p_bad, K, b["rmax"]), slice(None))
    assert (exp["count"][:1024] == INVALID).all() and (exp["count"][1024:] >= 0).all()
    for kw in (dict(), dict(tune_max_blocks=1), dict(tune_max_blocks=3)):
        check_case(renderer, p_bad, b["rmax"], exp, ("1 024 invalid points in front", kw), **kw)


def test_bounds_and_out_tensors(renderer):
    """Sentinels directly behind all three outputs; the inputs are only read; out= is filled in place and can be used again."""
    import torch

    b = set_batch(renderer)
    for n, k in ((1, K), (65, K), (b["n"], K), (b["n"], 1), (257, 40)):
        p, rmax, row = first(b, n, k)
        tp, tr = tdev(p), tdev(rmax)
        keep = [x.clone() for x in (tp, tr)]
        d_buf, i_buf, c_buf = sentinel(n * k, torch.float32, 64), sentinel(n * k, torch.int32, 64), sentinel(n, torch.int32, 64)
        out = (d_buf[:n * k].view(n, k), i_buf[:n * k].view(n, k), c_buf[:n])
        for again in range(2):  # reuse: the second call overwrites the first's answers with the same
            got = renderer.query_knn(tp, k, rmax=tr, out=out, **(dict(tune_max_blocks=1) if again else {}))
            assert [x.data_ptr() for x in got] == [d_buf.data_ptr(), i_buf.data_ptr(), c_buf.data_ptr()]
            check_rows(got, row, (n, k, again))
            assert still_sentinel(d_buf, 0, n * k) and still_sentinel(i_buf, 0, n * k) and still_sentinel(c_buf, 0, n), (n, k)
            for x, y in zip((tp, tr), keep):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ValueError):
        renderer.query_knn(tp, k, rmax=tr, out=(out[0], out[1], c_buf[:n - 1]))
    with pytest.raises(ValueError):
        renderer.query_knn(tp, k + 1, rmax=tr, out=out)


def test_stream_order(renderer):
    """Points made by torch on a stream, the query behind them on that stream without a host synchronisation, a torch reduction of the
    answers behind the query; one synchronisation at the end.  (Halving and doubling is exact: the points are the batch's.)"""
    import torch

    b = set_batch(renderer)
    n, row = b["n"], b["row"]
    p_half, tr = tdev(b["p"] * f32(0.5)), tdev(b["rmax"])
    ref_c, ref_d, ref_i = tdev(row["count"]), tdev(row["dist"]), tdev(row["tri"])
    counts, dist, tri = sentinel(n, torch.int32), sentinel(n, torch.float32, cols=K), sentinel(n, torch.int32, cols=K)
    with busy_stream(renderer):
        p = p_half * 2.0
        renderer.query_knn(p, K, rmax=tr, out=(dist, tri, counts), sync=False)
        wrong = (counts != ref_c).sum() + (dist.view(torch.int32) != ref_d.view(torch.int32)).sum() + (tri != ref_i).sum()
    assert int(wrong) == 0


def test_errors_write_nothing(renderer):
    import torch

    lib = R.load()
    b = set_batch(renderer)
    n = 1000
    p, rmax, row = first(b, n)
    tp, tr = tdev(p), tdev(rmax)
    cnt, dist, tri = sentinel(n, torch.int32), sentinel(n, torch.float32, cols=K), sentinel(n, torch.int32, cols=K)
    fresh = R.Renderer(0)
    try:  # no mesh
        assert lib.rt_query_knn_device(fresh._ctx, ptr(tp), ptr(tr), n, K, None, ptr(dist), ptr(tri), ptr(cnt)) == RT_ERR_STATE
    finally:
        fresh.close()
    ctx = renderer._ctx
    bp = bad_pointers(n, short3=12, short1=4, shortk=(4, n * K))  # one row short of n x 3 and n, one element short of n x k
    hp, short3, short1, shortk = bp.hp, bp.short3, bp.short1, bp.shortk

    def untouched(what):
        assert_untouched(renderer, (cnt, dist, tri), bp.big, what)

    outs = (ptr(dist), ptr(tri), ptr(cnt))
    calls = [(None, ptr(tr), n, K, None) + outs, (hp, ptr(tr), n, K, None) + outs, (ptr(tp), hp, n, K, None) + outs, (short3, ptr(tr), n, K, None) + outs,
             (ptr(tp), short1, n, K, None) + outs, (short3, None, n, K, None) + outs, (ptr(tp), ptr(tr), (1 << 30) + 1, K, None) + outs,
             (ptr(tp), ptr(tr), n, 0, None) + outs, (ptr(tp), ptr(tr), n, 1025, None) + outs, (ptr(tp), ptr(tr), n, 0xffffffff, None) + outs,]
    calls += [(ptr(tp), ptr(tr), n, K, prm) + outs for prm in bad_params(R.KnnQueryParams)]
    good = (ptr(tp), ptr(tr), n, K, None)
    calls += [good + x for x in ((None, ptr(tri), ptr(cnt)), (ptr(dist), None, ptr(cnt)), (hp, ptr(tri), ptr(cnt)), (ptr(dist), hp, ptr(cnt)), (ptr(dist), ptr(tri), hp),
                                 (shortk, ptr(tri), ptr(cnt)), (ptr(dist), shortk, ptr(cnt)), (ptr(dist), ptr(tri), short1))]
    for i, args in enumerate(calls):
        assert lib.rt_query_knn_device(ctx, *args) == RT_ERR_INVALID, i
        untouched(i)
    with pytest.raises(ValueError):
        renderer.query_knn(tp, 0)
    with pytest.raises(ValueError):
        renderer.query_knn(tp, 1025)
    # n = 0 is accepted, and does nothing
    assert lib.rt_query_knn_device(ctx, ptr(tp), ptr(tr), 0, K, None, *outs) == 0
    assert lib.rt_query_knn_device(ctx, None, None, 0, 1, None, None, None, None) == 0
    untouched("n = 0")
    assert [tuple(x.shape) for x in renderer.query_knn(tp[:0], 5)] == [(0, 5), (0, 5), (0,)]
    # the context still answers
    check_rows(renderer.query_knn(tp, K, rmax=tr, out=(dist, tri, cnt)), row, "after the refusals")


# ---- 4. what the rest of the process keeps ---------------------------------------------------------------------------------------

def test_point_neighbor_and_knn_stats_do_not_mix(renderer):
    """Each query kind keeps its own counters until somebody reads them: a point, a neighbour and a k-nearest query issued back to back, in
    every order, each report their own call; neighbors = the sum of the counts."""
    import itertools

    b = set_batch(renderer)
    n, m = b["n"], 1200
    rng = np.random.default_rng(47)

    def spoiled(base, k, comp, bad):
        q = base.copy()
        q[rng.permutation(len(q))[:k], comp] = bad
        return q

    tpp = tdev(spoiled(b["p"][:m], 300, 1, np.inf))
    limited = np.nonzero(np.isfinite(b["rmax"]))[0]
    pn = spoiled(b["p"][limited], 500, 2, np.nan)
    exp_n = NX.reference(b["v"], pn, b["rmax"][limited])
    tpn, trn = tdev(pn), tdev(b["rmax"][limited])
    pk = spoiled(b["p"], 900, 0, -np.inf)
    exp_k = KX.rows(KX.reference(b["v"], pk, K, b["rmax"]), slice(None))
    tpk, trk = tdev(pk), tdev(b["rmax"])

    def points():
        renderer.query_points(tpp, count_traversal=True)

    def neighbors():
        assert np.array_equal(renderer.count_neighbors(tpn, trn, count_traversal=True).cpu().numpy(), exp_n["count"])

    def knn():
        check_rows(renderer.query_knn(tpk, K, rmax=trk, count_traversal=True), exp_k, "knn")

    for order in itertools.permutations((points, neighbors, knn)):
        for q in order:
            q()
        pst, ns, ks = renderer.point_query_stats(), renderer.neighbor_query_stats(), renderer.knn_query_stats()  # only now
        assert (pst["invalid_points"], pst["points"]) == (300, m) and pst["nodes_visited"] > 0, pst
        assert (ns["invalid_points"], ns["points"], ns["neighbors"], ns["launches"]) == (500, len(limited), exp_n["neighbors"], 1), ns
        assert (ns["nodes_visited"], ns["tris_tested"]) == (exp_n["nodes_total"], exp_n["tris_total"]), ns
        assert (ks["invalid_points"], ks["points"], ks["neighbors"], ks["launches"]) == (900, n, int(np.maximum(exp_k["count"], 0).sum()), 1), ks
        assert ks["nodes_visited"] > 0 and ks["tris_tested"] > 0 and ks["stack_overflow"] == 0
        assert pst["ms"] > 0 and ns["ms"] > 0 and ks["ms"] > 0
        assert renderer.knn_query_stats() == ks  # read again: the same call's


def test_rendering_and_sharing_are_undisturbed(renderer):
    b = set_batch(renderer)
    renderer.resize(64, 64)
    kw = dict(pos=(0, 30.0, 40.0), spp=2, bounces=2, seed=3, sky=(0.2, 0.2, 0.3))

    def frame(r, **more):
        return pt_frame(r, **kw, **more)

    before, before_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert before[1][0] > 0 and before[1][3] == 0
    check_case(renderer, b["p"], b["rmax"], b["row"], "between frames", tune_lds_stack=1)
    after, after_spilling = frame(renderer), frame(renderer, tune_lds_stack=1, tune_no_overlap=2)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before_spilling[0], after_spilling[0]) and before_spilling[1] == after_spilling[1]
    # a shared mesh stays shared: the query only reads it
    other = R.Renderer(0)
    try:
        set_mesh(other, b["v"])
        other.resize(64, 64)
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        check_case(other, b["p"], b["rmax"], b["row"], "the other context")
        assert renderer.mesh_sharers() == 2 and other.mesh_sharers() == 2
        mine, theirs = frame(renderer), frame(other)
        assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1] and np.array_equal(mine[0], before[0])
    finally:
        other.close()
