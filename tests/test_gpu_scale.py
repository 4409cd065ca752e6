"""Path B's kernels across coordinate scale (tests/scale_exact.py), on the GPU.

The whole problem is multiplied by 2^k - exact in fp32 - at k = 0, +-1, +-12, the innermost edge on each side of the range that
applies (the range measured on the CPU references, cut at the library's coordinate limit) and one step inside it.  On every builder
- host single-level, host two-level, built on the device, refitted on the device from the k = 0 mesh to the scaled one - every query
family's outputs are the transformed k = 0 outputs of the same kernel bit for bit, and they are the native reference's answers at
that scale bit for bit.  The float64 contracts follow from the second equality: tests/test_scale_host.py holds exactly those
reference answers, at exactly these scales (scale_exact.gpu_scales), to ray_exact's, attr_exact's, point_exact's, neighbor_exact's
and sign_exact's contracts with their constants unchanged.  Frames are the oracle's at the scaled scene and the k = 0 frame.
Above the limit every render and query entry refuses before it writes, the context's own frame included; below the covariant range
frames stay finite."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import point_exact as PX
import raytracing_engine_amd as R
import scale_exact as S
from gpu_query import dev, ptr, same_floats, tdev

pytestmark = pytest.mark.gpu

f32 = np.float32
RT_ERR_INVALID = -1
MISS, INVALID = -1, -2
BUILDERS = ("host", "two_level", "device", "refit")
W, H = S.FRAME["width"], S.FRAME["height"]


def build(r, how, verts0, verts, surface=None):
    """The mesh `verts` (verts0 scaled) in the renderer, by one of the four builders."""
    a, e = surface or PX.surface(verts)
    if how == "host":
        r.set_mesh(verts, a, e)
    elif how == "two_level":
        r.set_mesh(verts, a, e, bvh_levels=2, blas_chunks=max(1, min(64, len(verts) // 8)))
    elif how == "device":
        r.set_mesh_device(tdev(verts), tdev(a), tdev(e))
    else:
        r.set_mesh_device(tdev(verts0), tdev(a), tdev(e))
        r.refit_mesh_device(tdev(verts))


def cpu(xs):
    return tuple(None if x is None else x.cpu().numpy() for x in xs)


def scales(families):
    """{k: the families tested at k}, over the families' own gpu_scales."""
    out = {}
    for f in families:
        for k in S.gpu_scales(f):
            out.setdefault(k, []).append(f)
    return dict(sorted(out.items(), key=lambda kv: abs(kv[0])))  # k = 0 first: its outputs are what the others are compared with


def same(got, want, what):
    """Every answer of `got` is `want`'s bit for bit (NaN for NaN)."""
    assert set(got) == set(want), what
    for key in got:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        ok = same_floats(g, w) if g.dtype == f32 else np.array_equal(g, w)
        assert ok, (what, key, np.nonzero(g.ravel() != w.ravel())[0][:8])


def reference(family, k, cases, key, listed=()):
    """The native reference's answers of the family at scale k, case by case, without the bookkeeping entry."""
    return S._split(S.answers(family, k), cases, key, listed)


# ---- queries -------------------------------------------------------------------------------------------------------------------
def ray_answers(r, q, family):
    o, d = tdev(q["o"]), tdev(q["d"])
    if family == "closest_hit":
        t, tri = cpu(r.query_rays(o, d))
        st = r.ray_query_stats()
        out = {"tri": tri, "t*": t}
    elif family == "hit_attr":
        t, tri, uv, nrm = cpu(r.query_rays(o, d, tdev(q["tmax"]), attributes=True))
        st = r.ray_query_stats()
        out = {"tri": tri, "t*": t, "ub": uv[:, 0], "vb": uv[:, 1], "normal": nrm}
    elif family == "occlusion":
        occ = r.query_rays(o, tdev(q["seg"]), any_hit=True).cpu().numpy()
        st = r.ray_query_stats()
        out = {"occluded": occ.astype(bool)}
    else:
        offsets, t, tri, counts = cpu(r.list_ray_hits(o, d, tdev(q["tmax"])))
        st = r.hit_query_stats()
        assert np.array_equal(r.count_ray_hits(o, d, tdev(q["tmax"])).cpu().numpy(), counts)
        out = {"count": counts, "offsets": offsets, "tri": tri, "t*": t}
    assert st["stack_overflow"] == 0 and st["invalid_rays"] == 0, (family, st)
    return out


def point_answers(r, q, family):
    p = tdev(q["p"])
    if family == "closest_point":
        dist, tri, c, uv, nrm = cpu(r.query_points(p, tdev(q["rmax"]), attributes=True))
        st = r.point_query_stats()
        out = {"tri": tri, "dist*": dist, "c*": c, "u": uv[:, 0], "v": uv[:, 1], "normal": nrm}
    elif family == "neighbors":
        offsets, dist, tri, counts = cpu(r.list_neighbors(p, tdev(q["rmax"])))
        st = r.neighbor_query_stats()
        assert np.array_equal(r.count_neighbors(p, tdev(q["rmax"])).cpu().numpy(), counts)
        out = {"count": counts, "offsets": offsets, "tri": tri, "dist*": dist}
    else:
        inside, crossings = cpu(r.query_sides(p, want_crossings=True))
        st = r.side_query_stats()
        sd, _, _ = cpu(r.query_signed_distance(p))
        assert r.side_query_stats()["stack_overflow"] == 0 and r.point_query_stats()["stack_overflow"] == 0
        out = {"inside": inside, "crossings": crossings, "sdist*": sd}
    assert st["stack_overflow"] == 0 and st["invalid_points"] == 0, (family, st)
    return out


def check_queries(r, how, families, cases_at, key, answers_of, listed):
    base = {}
    cases0 = cases_at(0)
    for f in families:  # what makes the contracts follow from the equality with the reference: the host test holds it to them at these scales
        assert set(S.gpu_scales(f)) <= set(S.host_scales(f)), f
    for k, fams in scales(families).items():
        for i, (q0, q) in enumerate(zip(cases0, cases_at(k))):
            build(r, how, q0["verts"], q["verts"])
            for f in fams:
                got = answers_of(r, q, f)
                ref = reference(f, k, cases0, key, listed.get(f, ()))[i]
                same(got, ref, (how, f, k, q["mesh"], "the reference at this scale"))
                if k == 0:
                    base[f, i] = got
                same(got, S.transformed(base[f, i], k), (how, f, k, q["mesh"], "the transformed k = 0 outputs of the same kernel"))


@pytest.mark.parametrize("how", BUILDERS)
def test_ray_queries_are_scale_covariant(renderer, how):
    check_queries(renderer, how, S.RAY_FAMILIES, lambda k: S._rays_at(k, True), "o", ray_answers, {"all_hits": ("tri", "t*")})


@pytest.mark.parametrize("how", BUILDERS)
def test_point_queries_are_scale_covariant(renderer, how):
    def points_at(k):  # both radii: the neighbours' (every point limited) and the closest point's (every fourth point unlimited)
        return [dict(q, rmax_point=qp["rmax"]) for q, qp in zip(S._points_at(k, True), S._points_at(k, True, rmax="rmax_point"))]

    def answers_of(r, q, f):
        return point_answers(r, dict(q, rmax=q["rmax_point"]) if f == "closest_point" else q, f)

    check_queries(renderer, how, S.POINT_FAMILIES, points_at, "p", answers_of, {"neighbors": ("tri", "dist*")})


@pytest.mark.parametrize("how", BUILDERS)
def test_side_queries_are_scale_covariant(renderer, how):
    check_queries(renderer, how, S.SIDE_FAMILIES, lambda k: S._points_at(k, True, S.side_cases()), "p", point_answers, {})


@pytest.mark.parametrize("how", BUILDERS)
def test_validity_follows_the_reach_of_the_scaled_mesh(renderer, how):
    """The reach is 32 x max(1, M): for M >= 1 it scales with the mesh, for M < 1 it stays at 32 - deliberately not covariant.  M is
    measured by each builder's own code: the host build, the two-level build, the device build, the refit."""
    c = S.point_cases()[0]
    M0 = f32(np.abs(c["verts"]).max())
    assert M0 > 1
    for k in (-12, -5, -4, 0, 12, S.k_limit("closest_point")):
        verts = S.scaled(c["verts"], k)
        M = S.scaled(M0, k)
        reach = f32(32) * max(f32(1), M)
        assert (M < 1) == (k <= -5) and PX.reach_of(verts) == reach
        build(renderer, how, c["verts"], verts)
        at = np.array([[reach, 0, 0], [np.nextafter(reach, f32(np.inf)), 0, 0], [0, -reach, 0], [0, 0, np.nextafter(-reach, -f32(np.inf))],
                       [f32(32) * M, 0, 0], [np.nextafter(f32(32) * M, f32(np.inf)), 0, 0]], f32)
        want = np.array([True, False, True, False, True, M < 1])  # the last: beyond 32 M, and valid all the same while M < 1
        d = np.tile(np.array([[-1, 0.25, 0.125]], f32), (len(at), 1))
        _, tri = cpu(renderer.query_rays(tdev(at), tdev(d)))
        assert np.array_equal(tri != INVALID, want), (k, tri)
        assert renderer.ray_query_stats()["invalid_rays"] == (~want).sum()
        _, tri, _ = cpu(renderer.query_points(tdev(at)))
        assert np.array_equal(tri != INVALID, want) and (tri[want] >= 0).all(), (k, tri)
        assert renderer.point_query_stats()["invalid_points"] == (~want).sum()
        assert np.array_equal(renderer.query_sides(tdev(at)).cpu().numpy() != INVALID, want), k
        assert np.array_equal(renderer.count_ray_hits(tdev(at), tdev(d)).cpu().numpy() != INVALID, want), k
        assert np.array_equal(renderer.count_neighbors(tdev(at), float(M)).cpu().numpy() != INVALID, want), k


# ---- frames --------------------------------------------------------------------------------------------------------------------
def render(r, how, name, k):
    s = S.frame_scenes()[name]
    v, a, e = s["mesh"]
    build(r, how, v, S.scaled_problem(k, verts=v)["verts"], (a, e))
    if "kind" in s:
        r.set_surfaces(s["kind"], s["ior"])
    r.resize(W, H)
    kw, _ = S.scaled_view(s["view"], k)
    out = []
    for no_packet in (0, 1):
        out.append(r.render_pt(tune_no_packet=no_packet, **kw))
        assert r.pt_stats()["stack_overflow"] == 0
    return out


@pytest.mark.parametrize("how", BUILDERS)
@pytest.mark.parametrize("family", S.FRAME_FAMILIES)
def test_frames_are_scale_invariant(renderer, family, how):
    names = [n for n in S.answers(family, 0) if n != "exact"]
    base = {}
    for k in scales([family]):
        for name in names:
            for rgb in render(renderer, how, name, k):
                assert np.array_equal(rgb.view(np.uint32), S.answers(family, k)[name].view(np.uint32)), (how, name, k, "the oracle at this scale")
                base.setdefault(name, rgb)
                assert np.array_equal(rgb.view(np.uint32), base[name].view(np.uint32)), (how, name, k, "the k = 0 frame")


@pytest.mark.parametrize("how", BUILDERS)
@pytest.mark.parametrize("family", S.FRAME_FAMILIES)
def test_frames_stay_finite_below_the_covariant_range(renderer, family, how):
    """The scales at which the references had non-finite pixels before the light weight's denominator was guarded: finite, and the guarded
    reference's frame."""
    names = [n for n in S.answers(family, 0) if n != "exact"]
    ks = [k for k in S.NONFINITE_BEFORE[family] if k < 0]
    assert ks and max(ks) < S.RANGES[family][0]
    for k in ks:
        for name in names:
            want = S.answers(family, k, False)[name]
            assert np.isfinite(want).all()
            for rgb in render(renderer, how, name, k):
                assert np.isfinite(rgb).all() and np.array_equal(rgb.view(np.uint32), want.view(np.uint32)), (how, name, k)


# ---- the refusal ---------------------------------------------------------------------------------------------------------------
def test_a_mesh_at_the_limit_is_served(renderer):
    import sign_exact as SX

    box = SX.mesh("box")  # |coordinates| up to 1, binary fractions
    at_limit = S.scaled(box, S.COORD_LIMIT_LOG2)
    assert np.abs(at_limit).max() == 2.0 ** S.COORD_LIMIT_LOG2
    for how in BUILDERS:
        build(renderer, how, box, at_limit)
        assert renderer.query_sides(tdev(np.zeros((1, 3), f32))).cpu().numpy()[0] == 1  # served: the centre of the box is inside


def beyond_the_limit():
    """(the soup of the ray cases, the same one scale above the limit, its largest |coordinate|)"""
    c = S.ray_cases()[0]
    big = S.scaled(c["verts"], S.k_limit("closest_hit") + 1)
    M = float(np.abs(big).max())
    assert 2.0 ** S.COORD_LIMIT_LOG2 < M < 2.0 ** (S.COORD_LIMIT_LOG2 + 1)
    return c, big, M


@pytest.mark.parametrize("how", BUILDERS)
def test_a_mesh_beyond_the_limit_is_refused_by_every_entry_before_anything_is_written(renderer, how):
    import torch

    lib, r = R.load(), renderer
    c, big, M = beyond_the_limit()
    k = S.k_limit("closest_hit") + 1
    n = 64
    o, d, p = tdev(S.scaled(c["o"][:n], k)), tdev(c["d"][:n]), tdev(S.scaled(c["o"][:n], k))
    full = lambda shape, dt: torch.full(shape, -7, dtype=dt, device=dev())  # noqa: E731
    ff, fi, fl = (lambda *s: full(s, torch.float32)), (lambda *s: full(s, torch.int32)), (lambda *s: full(s, torch.int64))  # noqa: E731
    rot, pos = np.array([0, 0, 0, 1], f32), np.zeros(3, f32)
    fptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    prm = r.pt_params(spp=1, bounces=1, sky=(0.2, 0.2, 0.25))
    rgb_host = np.full((H, W, 3), -7, f32)
    rgb_dev = ff(H * W * 3)
    outs = dict(t=ff(n), tri=fi(n), uv=ff(n, 2), nrm=ff(n, 3), c=ff(n, 3), cross=fi(n, 3), count=fi(n), offsets=fl(n + 1), keys=ff(4096), tris=fi(4096))
    offsets_in = torch.zeros(n + 1, dtype=torch.int64, device=dev())
    x = outs
    entries = {
        "rt_render_pt": lambda: lib.rt_render_pt(r._ctx, fptr(rot), fptr(pos), C.byref(prm), fptr(rgb_host)),
        "rt_render_pt_device": lambda: lib.rt_render_pt_device(r._ctx, fptr(rot), fptr(pos), C.byref(prm), ptr(rgb_dev), 0),
        "rt_query_rays_device": lambda: lib.rt_query_rays_device(r._ctx, ptr(o), ptr(d), None, n, None, ptr(x["t"]), ptr(x["tri"])),
        "rt_query_rays_attr_device": lambda: lib.rt_query_rays_attr_device(r._ctx, ptr(o), ptr(d), None, n, None, ptr(x["t"]), ptr(x["tri"]), ptr(x["uv"]), ptr(x["nrm"])),
        "rt_query_points_device": lambda: lib.rt_query_points_device(r._ctx, ptr(p), None, n, None, ptr(x["t"]), ptr(x["tri"]), ptr(x["c"])),
        "rt_query_points_attr_device": lambda: lib.rt_query_points_attr_device(r._ctx, ptr(p), None, n, None, ptr(x["t"]), ptr(x["tri"]), ptr(x["c"]), ptr(x["uv"]), ptr(x["nrm"])),
        "rt_query_sides_device": lambda: lib.rt_query_sides_device(r._ctx, ptr(p), n, None, ptr(x["tri"]), ptr(x["cross"]), None),
        "rt_query_signed_distance_device": lambda: lib.rt_query_signed_distance_device(r._ctx, ptr(p), None, n, None, None, ptr(x["t"]), ptr(x["tri"]), ptr(x["c"]), None),
        "rt_count_ray_hits_device": lambda: lib.rt_count_ray_hits_device(r._ctx, ptr(o), ptr(d), None, n, None, ptr(x["count"]), ptr(x["offsets"])),
        "rt_fill_ray_hits_device": lambda: lib.rt_fill_ray_hits_device(r._ctx, ptr(o), ptr(d), None, n, None, ptr(offsets_in), 4096, ptr(x["keys"]), ptr(x["tris"])),
        "rt_list_ray_hits_device": lambda: lib.rt_list_ray_hits_device(r._ctx, ptr(o), ptr(d), None, n, None, ptr(x["count"]), ptr(x["offsets"]), 4096, ptr(x["keys"]), ptr(x["tris"])),
        "rt_count_neighbors_device": lambda: lib.rt_count_neighbors_device(r._ctx, ptr(p), None, 1.0, n, None, ptr(x["count"]), ptr(x["offsets"])),
        "rt_fill_neighbors_device": lambda: lib.rt_fill_neighbors_device(r._ctx, ptr(p), None, 1.0, n, None, ptr(offsets_in), 4096, ptr(x["keys"]), ptr(x["tris"])),
        "rt_list_neighbors_device": lambda: lib.rt_list_neighbors_device(r._ctx, ptr(p), None, 1.0, n, None, ptr(x["count"]), ptr(x["offsets"]), 4096, ptr(x["keys"]), ptr(x["tris"])),
    }
    a, e = PX.surface(big)
    # a frame of the mesh inside the domain: what the context holds, and what it must still hold after every refusal
    r.resize(W, H)
    build(r, how, c["verts"], c["verts"], (a, e))
    frame = r.render_pt(params=prm)
    held = r.read_rgba8()
    assert np.isfinite(frame).all() and len(np.unique(held)) > 8  # not black, not one colour
    # the mesh itself is taken by this builder, and read back
    if how == "refit":
        r.refit_mesh_device(tdev(big))
    else:
        build(r, how, c["verts"], big, (a, e))
    assert len(r.read_bvh()[1]) == len(big)
    for name, call in entries.items():
        assert call() == RT_ERR_INVALID, (how, name)
        msg = lib.rt_last_error(r._ctx).decode()
        assert f"{M:g}" in msg and f"{2.0 ** S.COORD_LIMIT_LOG2:g}" in msg, (name, msg)
        r.synchronize()
        assert (rgb_host == -7).all() and (rgb_dev == -7).all() and all(bool((t == -7).all()) for t in outs.values()), (how, name, "a refusal wrote")
        assert np.array_equal(r.read_rgba8(), held), (how, name, "a refusal touched the context's frame")
    # back inside the domain - by a refit where the builder can refit, else by setting the mesh again - everything is served as before
    if how in ("device", "refit"):
        r.refit_mesh_device(tdev(c["verts"]))
    else:
        build(r, how, c["verts"], c["verts"], (a, e))
    o.copy_(tdev(c["o"][:n]))
    assert entries["rt_query_rays_device"]() == 0
    r.synchronize()
    assert (outs["tri"] != -7).all()
    assert np.array_equal(r.render_pt(params=prm), frame)


def test_a_frame_slot_refuses_a_mesh_beyond_the_limit_and_keeps_its_frame():
    c, big, M = beyond_the_limit()
    a, e = PX.surface(big)
    with R.Renderer(0) as fr:  # a context of its own: the session's keeps no slots
        prm = fr.pt_params(spp=1, bounces=1, sky=(0.2, 0.2, 0.25))
        fr.set_mesh(c["verts"], a, e)
        fr.resize(W, H)
        fr.frames_configure(2, fr.FRAME_F32)
        fr.frame_submit(0, pt_params=prm)
        frame = np.array(fr.frame_wait(0))
        assert np.isfinite(frame).all() and len(np.unique(frame)) > 50
        fr.set_mesh(big, a, e)
        for slot in (0, 1):
            with pytest.raises(R.RtError) as err:
                fr.frame_submit(slot, pt_params=prm)
            assert err.value.code == RT_ERR_INVALID and f"{M:g}" in str(err.value)
        assert np.array_equal(np.array(fr.frame_wait(0)), frame)  # the slot still holds the frame it had
        fr.set_mesh(c["verts"], a, e)  # the swap back: the slot takes a frame again, the same one
        fr.frame_submit(1, pt_params=prm)
        assert np.array_equal(np.array(fr.frame_wait(1)), frame)
