"""Refit of a path B mesh's BVH to new vertex positions on the GPU (rt_refit_mesh_device / Renderer.refit_mesh_device).

The tree keeps its topology and leaf order; every box is recomputed from the new vertices with the padding of a build for the
new coordinate range and quantised outward.  By DESIGN.md §6.3 a frame depends only on every box along a triangle's root path
containing that triangle padded by 2e-5·M, so frames after a refit equal the oracle's on the moved mesh bit for bit, and a
refit to unchanged vertices reproduces the tree byte for byte, whichever builder made it."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import raytracing_engine_amd as R
from raytracing_engine_amd import scenes
from gpu_query import ptr, segment_end
from test_gpu_device_bvh import check_bvh, dev

pytestmark = pytest.mark.gpu
RT_ERR_INVALID, RT_ERR_STATE = -1, -4
f32 = np.float32


def tdev(v, device=0):
    import torch

    return torch.from_numpy(np.ascontiguousarray(v, f32).reshape(-1, 9)).to(f"cuda:{device}")


def build(r, mesh, how):
    if how == "host":
        r.set_mesh(*mesh)
    else:
        r.set_mesh_device(*dev(mesh, r.device))


def refit(r, v):
    r.refit_mesh_device(tdev(v, r.device))


def check_frame(r, mesh, w, h, rot=(0, 0, 0, 1), pos=(0, 0, 0), ratio=None, **kw):
    """Frames of the current (refitted) mesh, with and without the packet kernel, equal the oracle's on `mesh`."""
    v, a, e = mesh
    r.resize(w, h, ratio)
    okw = {k: kw[k] for k in ("spp", "bounces", "seed", "sky", "ray_eps") if k in kw}
    ref, ct = O.TriScene(v, a, e).render(w, h, rot=rot, pos=pos, ratio=ratio, **okw)
    for no_packet in (0, 1):
        rgb = r.render_pt(rot, pos, tune_no_packet=no_packet, **kw)
        assert np.array_equal(rgb, ref), f"no_packet={no_packet}: {np.count_nonzero(rgb != ref)} values differ, max {np.abs(rgb - ref).max()}"
        st = r.pt_stats()
        assert st["stack_overflow"] == 0
        assert (st["camera_rays"], st["bounce_rays"], st["shadow_rays"]) == (ct["camera_rays"], ct["bounce_rays"], ct["shadow_rays"])
    return rgb


# ---- scenes and their motion (seeded, deterministic) -------------------------------------------------------------------------

TERRAIN_VIEW = dict(rot=tuple(R.camera_quat(0.0, -0.25)), pos=(0, 0, 4))


def terrain(grid=40):
    return scenes.terrain_scene(grid, seed=1)


def terrain_wave(mesh, t, amp=1.5):
    """A travelling wave on the height field's heights (z); the light quad (the last two triangles) stays."""
    v = np.asarray(mesh[0], f32).reshape(-1, 3, 3).copy()
    body = v[:-2]
    x, y = body[..., 0].astype(np.float64), body[..., 1].astype(np.float64)
    body[..., 2] += (amp * np.sin(0.35 * x + 0.2 * y - t)).astype(f32)
    return v.reshape(-1, 9), mesh[1], mesh[2]


def soup_offsets(mesh, scale, seed=3):
    """Every triangle but the light moved rigidly by its own offset of about `scale`."""
    v = np.asarray(mesh[0], f32).reshape(-1, 3, 3).copy()
    off = np.random.default_rng(seed).normal(size=(len(v) - 2, 1, 3)).astype(f32) * f32(scale)
    v[:-2] += off
    return v.reshape(-1, 9), mesh[1], mesh[2]


def cornell_moved():
    """The tall box (triangles 14-25) and the emissive quad (12-13) moved: NEE samples the moved light geometry."""
    v, a, e = scenes.cornell_tri_scene()
    v = v.reshape(-1, 3, 3).copy()
    assert (e[12:14] > 0).all() and (e[:12] == 0).all() and (e[14:] == 0).all()
    v[14:26] += np.array([1.2, -2.5, 0.8], f32)
    v[12:14] += np.array([1.5, 2.0, 0.0], f32)
    return v.reshape(-1, 9), a, e


def scaled(mesh, s):
    return (np.asarray(mesh[0], f32) * f32(s)).astype(f32), mesh[1], mesh[2]


# ---- 1. identity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("kind", ["cornell", "soup50k", "terrain"])
def test_identity_refit_reproduces_the_tree(renderer, how, kind):
    mesh = {"cornell": scenes.cornell_tri_scene, "soup50k": lambda: scenes.soup_scene(50000, seed=6, edge=0.4), "terrain": terrain}[kind]()
    build(renderer, mesh, how)
    before = renderer.read_bvh()
    st0 = renderer.pt_stats()
    refit(renderer, mesh[0])
    after = renderer.read_bvh()
    st1 = renderer.pt_stats()
    assert before[0].tobytes() == after[0].tobytes(), f"{np.count_nonzero((before[0] != after[0]).any(1))} nodes differ"
    assert before[1].tobytes() == after[1].tobytes()
    for k in ("n_tris", "n_nodes", "bvh_depth", "stack_need", "n_lights", "bvh_levels"):
        assert st0[k] == st1[k], k
    assert st1["bvh_build_ms"] > 0


# ---- 2. parity after motion ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [0.7, 2.1, 4.0])
def test_terrain_wave_parity(renderer, t):
    mesh = terrain()
    build(renderer, mesh, "device" if t != 2.1 else "host")
    moved = terrain_wave(mesh, t)
    refit(renderer, moved[0])
    check_frame(renderer, moved, 96, 64, spp=2, bounces=1, seed=4, sky=(0.4, 0.5, 0.7), **TERRAIN_VIEW)


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("scale", [0.02, 0.3, 3.0])
def test_soup_offsets_parity(renderer, how, scale):
    mesh = scenes.soup_scene(20000, seed=2, edge=0.3)
    build(renderer, mesh, how)
    moved = soup_offsets(mesh, scale)
    refit(renderer, moved[0])
    check_frame(renderer, moved, 96, 54, spp=2, bounces=1, seed=5, sky=(0.2, 0.2, 0.25))


@pytest.mark.parametrize("how", ["device", "host"])
def test_cornell_moved_box_and_light_parity(renderer, how):
    build(renderer, scenes.cornell_tri_scene(), how)
    moved = cornell_moved()
    refit(renderer, moved[0])
    rgb = check_frame(renderer, moved, 96, 96, pos=(0, 1, 0), spp=4, bounces=2, seed=7)
    assert rgb.mean() > 0.05


@pytest.mark.parametrize("s,pos", [(10.0, (0, 10, 0)), (0.1, (0, 0.1, 0))])
def test_uniform_scale_parity(renderer, s, pos):
    build(renderer, scenes.cornell_tri_scene(), "device")
    moved = scaled(scenes.cornell_tri_scene(), s)
    refit(renderer, moved[0])
    check_frame(renderer, moved, 80, 80, pos=pos, spp=2, bounces=2, seed=3)


# ---- 3. structure ------------------------------------------------------------------------------------------------------------

def max_abs(verts):
    """build_bvh's M: the largest |coordinate| of the vertices rebuilt in fp32 from the edges, at least 1."""
    v = np.ascontiguousarray(verts, f32).reshape(-1, 9)
    v0 = v[:, 0:3]
    return max(f32(np.abs(np.concatenate([v0, v0 + (v[:, 3:6] - v0), v0 + (v[:, 6:9] - v0)])).max()), f32(1.0))


def padded_containment(nodes, leaf, verts, pad):
    """Every occupied slot's de-quantised box (fp32, as the kernels de-quantise) contains the boxes of all triangles below it,
    padded by `pad`."""
    verts = np.ascontiguousarray(verts, f32).reshape(-1, 9)
    nn = len(nodes)
    w3 = nodes[:, 3]
    imask, leafmask = (w3 >> 24) & 0xFF, nodes[:, 6]
    slots = np.arange(8, dtype=np.uint32)
    inner = ((imask[:, None] >> slots) & 1).astype(bool)
    leafs = ((leafmask[:, None] >> slots) & 1).astype(bool)
    child_base, tri_base = nodes[:, 4].astype(np.int64), nodes[:, 5].astype(np.int64)
    q = np.ascontiguousarray(nodes[:, 8:20]).view(np.uint8).reshape(nn, 6, 8)
    qlo, qhi = q[:, :3, :].transpose(0, 2, 1), q[:, 3:, :].transpose(0, 2, 1)
    p = np.ascontiguousarray(nodes[:, :3]).view(f32)
    scale = ((np.stack([(w3 >> (8 * a)) & 0xFF for a in range(3)], 1).astype(np.uint32)) << np.uint32(23)).view(f32)
    lo = p[:, None, :] + qlo.astype(f32) * scale[:, None, :]
    hi = p[:, None, :] + qhi.astype(f32) * scale[:, None, :]
    v0 = verts[:, 0:3]
    x1, x2 = v0 + (verts[:, 3:6] - v0), v0 + (verts[:, 6:9] - v0)
    tmin = (np.minimum(np.minimum(v0, x1), x2) - pad).astype(f32)
    tmax = (np.maximum(np.maximum(v0, x1), x2) + pad).astype(f32)
    rank_in, rank_lf = np.cumsum(inner, 1) - inner, np.cumsum(leafs, 1) - leafs
    n_in = inner.sum(1)
    levels, first, count = [], 0, 1
    while count:
        levels.append((first, first + count))
        first, count = first + count, int(n_in[first:first + count].sum())
    sub_lo, sub_hi = np.full((nn, 3), np.inf, f32), np.full((nn, 3), -np.inf, f32)
    for a, b in reversed(levels):
        ks = slice(a, b)
        li = np.where(leafs[ks], tri_base[ks, None] + rank_lf[ks], 0)
        ch = np.where(inner[ks], child_base[ks, None] + rank_in[ks], 0)
        tri = leaf[li]
        slo = np.where(leafs[ks][..., None], tmin[tri], np.where(inner[ks][..., None], sub_lo[ch], np.inf)).astype(f32)
        shi = np.where(leafs[ks][..., None], tmax[tri], np.where(inner[ks][..., None], sub_hi[ch], -np.inf)).astype(f32)
        occ = inner[ks] | leafs[ks]
        assert (lo[ks][occ] <= slo[occ]).all() and (hi[ks][occ] >= shi[occ]).all(), "a padded triangle box lies outside a box on its root path"
        sub_lo[ks], sub_hi[ks] = slo.min(1), shi.max(1)


@pytest.mark.parametrize("how", ["device", "host"])
def test_refitted_tree_structure(renderer, how):
    mesh = scenes.soup_scene(30000, seed=4, edge=0.5)
    build(renderer, mesh, how)
    n0, l0 = renderer.read_bvh()
    for moved in (soup_offsets(mesh, 2.0)[0], scaled(mesh, 7.5)[0], scaled(mesh, 0.3)[0]):
        refit(renderer, moved)
        n1, l1 = renderer.read_bvh()
        check_bvh(renderer, moved)
        assert np.array_equal(n1[:, 4:8], n0[:, 4:8]) and np.array_equal(l1, l0), "topology or leaf order changed"
        padded_containment(n1, l1, moved, f32(2e-5) * max_abs(moved))
        assert not np.array_equal(n1[:, :4], n0[:, :4])


# ---- 4. rays ---------------------------------------------------------------------------------------------------------------

def test_trace_rays_after_refit_matches_bruteforce(renderer):
    mesh = scenes.soup_scene(8000, seed=4, edge=1.0)
    build(renderer, mesh, "device")
    v, a, e = soup_offsets(mesh, 1.5, seed=9)
    refit(renderer, v)
    sc = O.TriScene(v, a, e)
    rng = np.random.default_rng(8)
    n = 1500
    o = rng.uniform([-12, 0, -12], [12, 30, 12], size=(n, 3)).astype(f32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    # rays aimed through vertices and edge midpoints of the moved triangles
    tv = v.reshape(-1, 3, 3)
    pick = rng.integers(0, len(tv) - 2, size=600)
    target = np.concatenate([tv[pick[:300], pick[:300] % 3], 0.5 * (tv[pick[300:], 0] + tv[pick[300:], 1])]).astype(f32)
    o[:600] = target + f32(6.0) * rng.normal(size=(600, 3)).astype(f32)
    dd = target - o[:600]
    d[:600] = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(f32)
    t, tri = renderer.trace_rays(o, d)
    hits = 0
    for i in range(n):
        rt_, rtt = sc.closest_hit(o[i], d[i], use_bvh=False)
        assert tri[i] == rt_, i
        if rt_ >= 0:
            hits += 1
            assert t[i] == np.float32(rtt), i
        else:
            assert np.isinf(t[i])
    assert hits > 600
    seg = (d * rng.uniform(1, 25, size=(n, 1))).astype(f32)
    _, occ = renderer.trace_rays(o, seg, any_hit=True)
    ref = np.array([sc.occluded(o[i], seg[i], use_bvh=False) for i in range(n)])
    assert np.array_equal(occ.astype(bool), ref) and 0.05 < ref.mean() < 0.95


# ---- 5. the camera range follows M -----------------------------------------------------------------------------------------

def test_camera_range_follows_the_refit(renderer):
    mesh = scenes.cornell_tri_scene()  # M = 22
    build(renderer, mesh, "device")
    renderer.resize(48, 48)
    big = scaled(mesh, 100.0)
    far = (0.0, -31.0 * 2200.0, 0.0)  # 31 M of the scaled mesh, beyond 32 M of the original
    with pytest.raises(R.RtError) as ei:
        renderer.render_pt(pos=far, spp=1, bounces=1, seed=1)
    assert ei.value.code == RT_ERR_INVALID
    refit(renderer, big[0])
    # a narrow view (the room spans about 0.009 rad from 31 M): most pixels see the room, bounces and shadow rays included
    rgb = check_frame(renderer, big, 64, 64, pos=far, ratio=(0.012, 0.012), spp=2, bounces=1, seed=1, sky=(0.3, 0.3, 0.3))
    assert np.count_nonzero(rgb != f32(0.3)) > rgb.size // 2
    renderer.resize(48, 48)
    build(renderer, mesh, "device")
    near = (0.0, -100.0, 0.0)  # inside 32 M = 704 of the original, outside 32 x max(0.22, 1) of the shrunk mesh
    renderer.render_pt(pos=near, spp=1, bounces=1, seed=1)
    refit(renderer, scaled(mesh, 0.01)[0])
    with pytest.raises(R.RtError) as ei:
        renderer.render_pt(pos=near, spp=1, bounces=1, seed=1)
    assert ei.value.code == RT_ERR_INVALID


# ---- 6. errors -------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_mesh(renderer):
    import torch

    lib = R.load()
    mesh = scenes.cornell_tri_scene()
    build(renderer, mesh, "device")
    refit(renderer, cornell_moved()[0])  # the errors below must also leave a refitted mesh (and its scratch) alone
    renderer.resize(48, 48)
    before = renderer.render_pt(pos=(0, 1, 0), spp=2, bounces=1, seed=3)
    bvh_before = renderer.read_bvh()
    n = len(mesh[0])
    ctx = renderer._ctx
    v = tdev(mesh[0])
    host = np.zeros((n, 9), f32)
    assert lib.rt_refit_mesh_device(ctx, None, n) == RT_ERR_INVALID
    assert lib.rt_refit_mesh_device(ctx, C.c_void_p(host.ctypes.data), n) == RT_ERR_INVALID
    big = torch.zeros(1 << 20, dtype=torch.float32, device="cuda:0")
    short = segment_end(big.data_ptr()) - 36 * (n - 1)  # the allocation holds n - 1 triangles from here
    assert lib.rt_refit_mesh_device(ctx, C.c_void_p(short), n) == RT_ERR_INVALID
    v_more = tdev(np.concatenate([mesh[0], mesh[0][:1]]))
    assert lib.rt_refit_mesh_device(ctx, ptr(v_more), n + 1) == RT_ERR_INVALID
    assert lib.rt_refit_mesh_device(ctx, ptr(v), n - 1) == RT_ERR_INVALID
    assert lib.rt_refit_mesh_device(ctx, ptr(v), 0) == RT_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        vb = v.clone()
        vb[n // 2, 4] = bad
        with pytest.raises(R.RtError) as ei:
            renderer.refit_mesh_device(vb)
        assert ei.value.code == RT_ERR_INVALID
    for arg in (v.double(), v.cpu(), v.t(), v[:, :8].contiguous(), v.reshape(-1)[:-1], np.asarray(mesh[0], f32)):
        with pytest.raises(ValueError):
            renderer.refit_mesh_device(arg)
    if torch.cuda.device_count() > 1:  # memory of another device
        assert lib.rt_refit_mesh_device(ctx, ptr(tdev(mesh[0], 1)), n) == RT_ERR_INVALID
    bvh_after = renderer.read_bvh()
    assert bvh_before[0].tobytes() == bvh_after[0].tobytes() and bvh_before[1].tobytes() == bvh_after[1].tobytes()
    assert np.array_equal(renderer.render_pt(pos=(0, 1, 0), spp=2, bounces=1, seed=3), before)
    del big


def test_refit_needs_a_single_level_mesh():
    mesh = scenes.cornell_tri_scene()
    v = tdev(mesh[0])
    lib = R.load()
    with R.Renderer(0) as r:
        assert lib.rt_refit_mesh_device(r._ctx, C.c_void_p(v.data_ptr()), len(mesh[0])) == RT_ERR_STATE  # no mesh
        soup = scenes.soup_scene(3000, seed=5, edge=1.0)
        r.set_mesh(*soup, bvh_levels=2, blas_chunks=8)
        with pytest.raises(R.RtError) as ei:
            r.refit_mesh_device(tdev(soup[0]))
        assert ei.value.code == RT_ERR_STATE
        r.resize(48, 32)
        r.render_pt(spp=1, bounces=1)  # the two-level mesh is still there


# ---- 7. determinism and path independence ----------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["device", "host"])
def test_refits_are_deterministic_and_path_independent(renderer, how):
    mesh = scenes.soup_scene(40000, seed=7, edge=0.3)
    a, b = mesh[0], soup_offsets(mesh, 0.8, seed=1)[0]
    build(renderer, mesh, how)
    refit(renderer, a)
    ident = renderer.read_bvh()
    refit(renderer, b)
    b1 = renderer.read_bvh()
    refit(renderer, b)
    b2 = renderer.read_bvh()
    assert b1[0].tobytes() == b2[0].tobytes() and b1[1].tobytes() == b2[1].tobytes()
    assert b1[0].tobytes() != ident[0].tobytes()
    refit(renderer, a)
    back = renderer.read_bvh()
    assert back[0].tobytes() == ident[0].tobytes() and back[1].tobytes() == ident[1].tobytes()
    with R.Renderer(0) as other:
        build(other, mesh, how)
        refit(other, b)
        b3 = other.read_bvh()
    assert b3[0].tobytes() == b1[0].tobytes() and b3[1].tobytes() == b1[1].tobytes()


# ---- 8. interplay ----------------------------------------------------------------------------------------------------------

def test_frame_slots_render_the_refitted_mesh():
    base = scenes.cornell_tri_scene()
    moves = [base, cornell_moved(), scaled(base, 1.5), cornell_moved()]
    poses = [(0.0, 1.0 + 0.1 * k, 0.0) for k in range(4)]
    with R.Renderer(0) as r:
        build(r, base, "device")
        r.resize(64, 48)
        prm = r.pt_params(spp=2, bounces=2, seed=5)
        want = []
        for k in range(4):
            refit(r, moves[k][0])
            want.append(r.render_pt(pos=poses[k], params=prm))
        # refits after configure: slots submitted afterwards render the moved mesh
        r.frames_configure(2, r.FRAME_F32)
        refit(r, moves[1][0])
        r.frame_submit(0, pos=poses[1], pt_params=prm)
        assert np.array_equal(r.frame_wait(0), want[1])
        # refits between submits, frames in flight: each frame renders the mesh as it was when it was submitted
        got = []
        for k in range(4):
            refit(r, moves[k][0])
            r.frame_submit(k % 2, pos=poses[k], pt_params=prm)
            if k >= 1:
                got.append(r.frame_wait((k - 1) % 2))
        got.append(r.frame_wait(3 % 2))
        for k in range(4):
            assert np.array_equal(got[k], want[k]), k


def test_partition_union_after_refit_equals_single(renderer):
    import torch

    build(renderer, scenes.cornell_tri_scene(), "device")
    refit(renderer, cornell_moved()[0])
    w, h, n_ranks = 200, 136, 8
    renderer.resize(w, h)
    renderer.set_partition(0, 1)
    prm = renderer.pt_params(spp=2, bounces=2, seed=9)
    full = renderer.render_pt(pos=(0, 1, 0), params=prm)
    tx, ty, _ = renderer.tile_info()
    per = -(-(tx * ty) // n_ranks)
    gathered = torch.zeros((n_ranks, per, 64, 64, 3), dtype=torch.float32, device="cuda")
    try:
        for rank in range(n_ranks):
            renderer.set_partition(rank, n_ranks)
            renderer.render_pt_device((0, 0, 0, 1), (0, 1, 0), prm, gathered[rank].data_ptr(), tile_major=True)
            renderer.synchronize()
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        renderer.detile_device(gathered.data_ptr(), n_ranks, per, out.data_ptr())
        renderer.synchronize()
        assert np.array_equal(out.cpu().numpy(), full)
    finally:
        renderer.set_partition(0, 1)


def test_vertices_written_just_before_the_refit(renderer):
    """The new vertices come from torch kernels on a side stream that is current when refit_mesh_device is called: the
    refit must see the finished values."""
    import torch

    v, a, e = scenes.soup_scene(200000, seed=9, edge=0.3)
    build(renderer, (v, a, e), "device")
    shift = f32(0.75)
    v_host = (np.asarray(v, f32) + shift).astype(f32)
    src = torch.from_numpy(np.ascontiguousarray(v, f32)).pin_memory()
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        vd = torch.empty(src.shape, dtype=torch.float32, device="cuda:0")
        for _ in range(20):  # keep the stream busy so that the refit would overtake an unfinished producer
            vd.copy_(src, non_blocking=True)
        vd.add_(float(shift))
        renderer.refit_mesh_device(vd)
    check_bvh(renderer, v_host)
    renderer.resize(96, 54)
    got = renderer.render_pt(spp=1, bounces=1, seed=1, sky=(0.2, 0.2, 0.25))
    renderer.set_mesh(v_host, a, e)
    assert np.array_equal(renderer.render_pt(spp=1, bounces=1, seed=1, sky=(0.2, 0.2, 0.25)), got)


def test_set_mesh_after_a_refit(renderer):
    mesh = scenes.cornell_tri_scene()
    renderer.set_mesh(*mesh)
    tree = renderer.read_bvh()
    renderer.resize(64, 48)
    kw = dict(pos=(0, 1, 0), spp=2, bounces=1, seed=2)
    first = renderer.render_pt(**kw)
    refit(renderer, cornell_moved()[0])
    assert not np.array_equal(renderer.render_pt(**kw), first)
    renderer.set_mesh(*mesh)
    again = renderer.read_bvh()
    assert tree[0].tobytes() == again[0].tobytes() and tree[1].tobytes() == again[1].tobytes()
    assert np.array_equal(renderer.render_pt(**kw), first)
    refit(renderer, mesh[0])  # a fresh mesh is refittable again (its scratch was freed with the old one)
    assert np.array_equal(renderer.render_pt(**kw), first)
