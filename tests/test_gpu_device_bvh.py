"""Path B meshes whose BVH is built on the GPU from device-resident torch tensors (rt_set_mesh_device).

The frame does not depend on the tree (conservative boxes padded by the same rule, closest hit = the
(t, triangle index) minimum), so a device-built LBVH must give frames bit-identical to the oracle's and to those of the
host-built tree.  The tree itself is checked structurally (the invariants tests/native/bvh_check.cpp checks on host
trees) in numpy over rt_read_bvh, and byte for byte against a second build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import raytracing_engine_amd as R
from gpu_query import ptr
from lbvh_exact import check_tree
from raytracing_engine_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID, RT_ERR_STATE = -1, -4


def dev(mesh, device=0):
    import torch

    v, a, e = (np.ascontiguousarray(x, np.float32) for x in mesh)
    to = lambda x: torch.from_numpy(x).to(f"cuda:{device}")  # noqa: E731
    return to(v.reshape(-1, 9)), to(a.reshape(-1, 3)), to(e.reshape(-1, 3))


def set_dev(r, mesh):
    r.set_mesh_device(*dev(mesh, r.device))


def check_pt_dev(r, mesh, w, h, rot=(0, 0, 0, 1), pos=(0, 0, 0), **kw):
    v, a, e = mesh
    set_dev(r, mesh)
    r.resize(w, h)
    rgb = r.render_pt(rot, pos, **kw)
    okw = {k: kw[k] for k in ("spp", "bounces", "seed", "sky", "ray_eps") if k in kw}
    ref, ct = O.TriScene(v, a, e).render(w, h, rot=rot, pos=pos, **okw)
    assert np.array_equal(rgb, ref), f"{np.count_nonzero(rgb != ref)} values differ, max {np.abs(rgb - ref).max()}"
    st = r.pt_stats()
    assert st["stack_overflow"] == 0 and st["bvh_levels"] == 1
    assert (st["camera_rays"], st["bounce_rays"], st["shadow_rays"]) == (ct["camera_rays"], ct["bounce_rays"], ct["shadow_rays"])
    return rgb, st


def check_bvh(r, verts):
    """Structural invariants of the current tree (layout: raytracing_engine_amd/csrc/bvh_node.h; the array part is
    lbvh_exact.check_tree); returns its depth."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
    nodes, leaf = r.read_bvh()
    st = r.pt_stats()
    assert len(nodes) == st["n_nodes"] >= 1 and len(leaf) == len(verts) == st["n_tris"]
    depth = check_tree(nodes, leaf, verts)
    assert depth == st["bvh_depth"] and depth <= st["stack_need"] - 1
    return depth


# ---- 1. oracle parity ----------------------------------------------------------------------------------------------------

def test_cornell_parity(renderer):
    rgb, st = check_pt_dev(renderer, scenes.cornell_tri_scene(), 128, 128, pos=(0, 1, 0), spp=4, bounces=2, seed=7)
    assert rgb.mean() > 0.05 and st["camera_rays"] == 128 * 128 * 4


@pytest.mark.parametrize("bounces,spp", [(0, 1), (1, 4), (3, 2), (8, 1)])
def test_bounce_and_spp_grid(renderer, bounces, spp):
    check_pt_dev(renderer, scenes.cornell_tri_scene(), 96, 64, pos=(0, 1, 0), rot=R.camera_quat(0.2, -0.1), spp=spp, bounces=bounces, seed=3)


def test_soup_2k_with_sky(renderer):
    check_pt_dev(renderer, scenes.soup_scene(2000, seed=3, edge=1.5), 160, 90, spp=2, bounces=1, seed=5, sky=(0.3, 0.3, 0.4))


def test_soup_100k_small_view(renderer):
    check_pt_dev(renderer, scenes.soup_scene(100000, seed=1), 192, 108, spp=4, bounces=1, seed=1, sky=(0.2, 0.2, 0.25))


@pytest.mark.parametrize("name,args", [("path_b_cornell_64.npz", dict(kind="cornell", w=64, h=64, spp=4, bounces=2, seed=7, pos=(0, 1, 0))),
                                       ("path_b_soup2k_96x54.npz", dict(kind="soup", w=96, h=54, spp=2, bounces=1, seed=5, sky=(0.3, 0.3, 0.4)))])
def test_against_committed_fixture(renderer, golden_dir, name, args):
    g = np.load(os.path.join(golden_dir, name))
    kind, w, h = args.pop("kind"), args.pop("w"), args.pop("h")
    set_dev(renderer, scenes.cornell_tri_scene() if kind == "cornell" else scenes.soup_scene(2000, seed=3, edge=1.5))
    renderer.resize(w, h)
    rgb = renderer.render_pt(pos=args.pop("pos", (0, 0, 0)), **args)
    assert np.array_equal(rgb, g["rgb"])
    st = renderer.pt_stats()
    assert [st["camera_rays"], st["bounce_rays"], st["shadow_rays"]] == g["counters"].tolist() and st["stack_overflow"] == 0


# ---- 2. device tree against host tree ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["soup1m", "terrain"])
def test_device_tree_frames_equal_host_tree_frames(renderer, kind):
    if kind == "soup1m":
        mesh, rot, pos, sky = scenes.soup_scene(1_000_000, seed=1, edge=0.08), (0, 0, 0, 1), (0, 0, 0), (0.2, 0.2, 0.25)
    else:
        mesh, rot, pos, sky = scenes.terrain_scene(708, seed=1), R.camera_quat(0.0, -0.25), (0, 0, 4), (0.4, 0.5, 0.7)
    renderer.resize(384, 216)
    frames = {}
    for which in ("host", "device"):
        if which == "host":
            renderer.set_mesh(*mesh)
        else:
            set_dev(renderer, mesh)
        st = renderer.pt_stats()
        assert st["bvh_levels"] == 1 and st["n_tris"] == len(mesh[0]) and st["bvh_build_ms"] > 0
        for no_packet in (0, 1):
            frames[which, no_packet] = renderer.render_pt(rot, pos, spp=2, bounces=1, seed=4, sky=sky, tune_no_packet=no_packet)
            assert renderer.pt_stats()["stack_overflow"] == 0
    for no_packet in (0, 1):
        assert np.array_equal(frames["host", no_packet], frames["device", no_packet]), no_packet
    assert np.array_equal(frames["device", 0], frames["device", 1])
    assert frames["device", 0].mean() > 0.01


# ---- 3. trace_rays against the oracle's brute force -------------------------------------------------------------------------

def test_trace_rays_matches_bruteforce_oracle(renderer):
    v, a, e = scenes.soup_scene(20000, seed=4, edge=1.0)
    set_dev(renderer, (v, a, e))
    sc = O.TriScene(v, a, e)
    rng = np.random.default_rng(8)
    n = 4000
    o = rng.uniform([-12, 0, -12], [12, 30, 12], size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:50] = [0, 1, 0]  # axis-parallel rays (zero direction components)
    d[50:100] = [1, 0, 0]
    d[100:150] = [-0.0, 1, -0.0]  # negative zeros
    d[150:200] = [-0.0, -0.0, -1]
    t, tri = renderer.trace_rays(o, d)
    hits = 0
    for i in range(n):
        rt_, rtt = sc.closest_hit(o[i], d[i], use_bvh=False)
        assert tri[i] == rt_, i
        if rt_ >= 0:
            hits += 1
            assert t[i] == np.float32(rtt)
        else:
            assert np.isinf(t[i])
    assert hits > 500
    seg = (d * rng.uniform(1, 25, size=(n, 1))).astype(np.float32)
    _, occ = renderer.trace_rays(o, seg, any_hit=True)
    ref = np.array([sc.occluded(o[i], seg[i], use_bvh=False) for i in range(n)])
    assert np.array_equal(occ.astype(bool), ref) and 0.05 < ref.mean() < 0.95


def test_rays_through_vertices_edges_and_duplicate_triangles(renderer):
    """A flat grid of quads with every triangle present twice: rays through vertices, edge midpoints and diagonals, from
    both sides, must give the brute-force closest hit (the lower index of a duplicate pair) and occlusion bit for bit."""
    f = np.float32
    tris = []
    for i in range(-4, 4):
        for j in range(-4, 4):
            a_, b_, c_, d_ = (i, 5, j), (i + 1, 5, j), (i + 1, 5, j + 1), (i, 5, j + 1)
            tris += [a_ + b_ + c_, a_ + c_ + d_]
    v = np.array(tris + tris, f)
    a = np.full((len(v), 3), 0.5, f)
    e = np.zeros((len(v), 3), f)
    e[-1] = 1.0
    set_dev(renderer, (v, a, e))
    check_bvh(renderer, v)
    sc = O.TriScene(v, a, e)
    xs = np.arange(-4.5, 4.75, 0.25, dtype=f)
    gx, gz = np.meshgrid(xs, xs)
    n = gx.size
    for y0, dy in ((0.0, 1.0), (9.0, -1.0)):
        o = np.stack([gx.ravel(), np.full(n, y0, f), gz.ravel()], 1).astype(f)
        d = np.tile(np.array([0.0, dy, 0.0], f), (n, 1))
        d[::3, 0] = -0.0
        t, tri = renderer.trace_rays(o, d)
        hits = 0
        for k in range(n):
            rt_, rtt = sc.closest_hit(o[k], d[k], use_bvh=False)
            assert tri[k] == rt_, (k, o[k], tri[k], rt_)
            if rt_ >= 0:
                hits += 1
                assert t[k] == np.float32(rtt) and rt_ < len(tris)
        assert hits > n // 2
        seg = (d * f(7.0)).astype(f)
        _, occ = renderer.trace_rays(o, seg, any_hit=True)
        ref = np.array([sc.occluded(o[k], seg[k], use_bvh=False) for k in range(n)])
        assert np.array_equal(occ.astype(bool), ref)
    check_pt_dev(renderer, (v, a, e), 65, 65, pos=(0.0, 0.0, 0.0), spp=2, bounces=1, sky=(0.4, 0.5, 0.6))


# ---- 4. structure ------------------------------------------------------------------------------------------------------------

def _mesh(v):
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 9)
    a = np.full((len(v), 3), 0.5, np.float32)
    e = np.zeros((len(v), 3), np.float32)
    e[0] = 2.0
    return v, a, e


def _special(kind):
    rng = np.random.default_rng(11)
    if kind == "identical":
        return np.tile(np.array([[-1, 5, -1, 1, 5, -1, 0, 6, 1]], np.float32), (500, 1))
    if kind == "zero_area":  # points, segments and a few proper triangles
        v = rng.uniform(-5, 5, size=(600, 9)).astype(np.float32)
        v[:200, 3:6] = v[:200, 0:3]
        v[:200, 6:9] = v[:200, 0:3]
        v[200:400, 6:9] = v[200:400, 3:6]
        return v
    if kind == "flat":  # every vertex on the plane y = 2: a zero-extent axis
        v = rng.uniform(-10, 10, size=(3000, 9)).astype(np.float32)
        v[:, 1::3] = 2.0
        return v
    if kind == "mixed_scale":  # tiny triangles near the origin and huge ones far away
        small = rng.uniform(-1e-3, 1e-3, size=(1000, 9)).astype(np.float32)
        big = rng.uniform(-1e4, 1e4, size=(1000, 9)).astype(np.float32)
        return np.concatenate([small, big])
    raise ValueError(kind)


def test_structure_checker_accepts_the_host_tree(renderer):
    v, a, e = scenes.soup_scene(30000, seed=2, edge=0.5)
    renderer.set_mesh(v, a, e)
    assert check_bvh(renderer, v) == renderer.pt_stats()["bvh_depth"]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 38, 700, 30000, 4095, 4096, 4097, 8193, 65537])
def test_device_tree_structure(renderer, n):
    rng = np.random.default_rng(n)
    v = (rng.uniform(-8, 8, size=(n, 1, 3)) + rng.uniform(-0.7, 0.7, size=(n, 3, 3))).astype(np.float32).reshape(n, 9)
    set_dev(renderer, _mesh(v))
    depth = check_bvh(renderer, v)
    st = renderer.pt_stats()
    assert st["bvh_levels"] == 1 and st["n_lights"] == 1 and st["stack_need"] == depth + 1
    if n <= 9:
        assert st["n_nodes"] == (1 if n <= 8 else 2)


@pytest.mark.parametrize("kind", ["identical", "zero_area", "flat", "mixed_scale"])
def test_device_tree_structure_degenerate(renderer, kind):
    v = _special(kind)
    set_dev(renderer, _mesh(v))
    check_bvh(renderer, v)


def test_degenerate_meshes_render_as_the_oracle(renderer):
    for kind, pos in (("identical", (0, 0, 0)), ("zero_area", (0, 0, -9)), ("flat", (0, 0, 0)), ("mixed_scale", (0, 0, 0))):
        check_pt_dev(renderer, _mesh(_special(kind)), 48, 32, pos=pos, spp=1, bounces=1, seed=2, sky=(0.3, 0.3, 0.3))


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------

def test_builds_are_byte_identical(renderer):
    mesh = scenes.soup_scene(50000, seed=6, edge=0.4)
    set_dev(renderer, mesh)
    n1, l1 = renderer.read_bvh()
    set_dev(renderer, mesh)
    n2, l2 = renderer.read_bvh()
    with R.Renderer(0) as other:
        set_dev(other, mesh)
        n3, l3 = other.read_bvh()
    assert n1.tobytes() == n2.tobytes() == n3.tobytes() and l1.tobytes() == l2.tobytes() == l3.tobytes()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_previous_mesh(renderer):
    lib = R.load()
    mesh = scenes.cornell_tri_scene()
    set_dev(renderer, mesh)
    renderer.resize(48, 48)
    before = renderer.render_pt(pos=(0, 1, 0), spp=2, bounces=1, seed=3)
    nodes_before = renderer.read_bvh()
    v, a, e = dev(mesh)
    n = len(mesh[0])
    host = np.zeros((n, 9), np.float32)
    ctx = renderer._ctx
    assert lib.rt_set_mesh_device(ctx, None, ptr(a), ptr(e), n) == RT_ERR_INVALID
    assert lib.rt_set_mesh_device(ctx, ptr(v), None, ptr(e), n) == RT_ERR_INVALID
    assert lib.rt_set_mesh_device(ctx, ptr(v), ptr(a), None, n) == RT_ERR_INVALID
    assert lib.rt_set_mesh_device(ctx, C.c_void_p(host.ctypes.data), ptr(a), ptr(e), n) == RT_ERR_INVALID
    assert lib.rt_set_mesh_device(ctx, ptr(v), ptr(a), ptr(e), 0) == RT_ERR_INVALID
    assert lib.rt_set_mesh_device(ctx, ptr(v), ptr(a), ptr(e), 1 << 28) == RT_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        vb = v.clone()
        vb[n // 2, 4] = bad
        with pytest.raises(R.RtError) as ei:
            renderer.set_mesh_device(vb, a, e)
        assert ei.value.code == RT_ERR_INVALID
    for args in ((v.double(), a, e), (v, a.cpu(), e), (v.t(), a, e), (v, a[:-1], e), (v.reshape(-1, 3), a, e)):
        with pytest.raises(ValueError):
            renderer.set_mesh_device(*args)
    after = renderer.render_pt(pos=(0, 1, 0), spp=2, bounces=1, seed=3)
    assert np.array_equal(before, after)
    nodes_after = renderer.read_bvh()
    assert nodes_before[0].tobytes() == nodes_after[0].tobytes() and nodes_before[1].tobytes() == nodes_after[1].tobytes()
    with pytest.raises(R.RtError) as ei:
        renderer.update_mesh_chunk(0, np.asarray(mesh[0], np.float32)[:1])
    assert ei.value.code == RT_ERR_STATE


# ---- 7. interplay ----------------------------------------------------------------------------------------------------------

def test_frame_slots_on_a_device_mesh(renderer):
    mesh = scenes.cornell_tri_scene()
    with R.Renderer(0) as r:
        set_dev(r, mesh)
        r.resize(64, 48)
        prm = r.pt_params(spp=2, bounces=2, seed=5)
        want = [r.render_pt(pos=(0.0, 1.0 + 0.1 * k, 0.0), params=prm) for k in range(4)]
        r.frames_configure(2, r.FRAME_F32)
        got = []
        for k in range(4):
            r.frame_submit(k % 2, pos=(0.0, 1.0 + 0.1 * k, 0.0), pt_params=prm)
            if k >= 1:
                got.append(r.frame_wait((k - 1) % 2))
        got.append(r.frame_wait(3 % 2))
        for k in range(4):
            assert np.array_equal(got[k], want[k]), k


def test_partition_union_equals_single(renderer):
    import torch

    set_dev(renderer, scenes.cornell_tri_scene())
    w, h, n_ranks = 200, 136, 2
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


def test_mesh_swaps_host_device_host(renderer):
    soup = scenes.soup_scene(3000, seed=5, edge=1.0)
    cornell = scenes.cornell_tri_scene()
    renderer.resize(64, 48)
    kw = dict(spp=2, bounces=1, seed=2, sky=(0.1, 0.1, 0.1))
    renderer.set_mesh(*cornell)
    first = renderer.render_pt(pos=(0, 1, 0), **kw)
    set_dev(renderer, soup)
    soup_dev = renderer.render_pt(**kw)
    renderer.set_mesh(*soup)
    assert np.array_equal(renderer.render_pt(**kw), soup_dev)
    set_dev(renderer, cornell)
    assert np.array_equal(renderer.render_pt(pos=(0, 1, 0), **kw), first)
    renderer.set_mesh(*cornell)
    assert np.array_equal(renderer.render_pt(pos=(0, 1, 0), **kw), first)


def test_tensors_written_just_before_the_call(renderer):
    """The mesh is produced by torch kernels on a side stream that is current when set_mesh_device is called: the build
    must see the finished values."""
    import torch

    v, a, e = scenes.soup_scene(200000, seed=9, edge=0.3)
    shift = np.float32(0.75)
    v_host = (np.asarray(v, np.float32) + shift).astype(np.float32)
    src = torch.from_numpy(np.ascontiguousarray(v, np.float32)).pin_memory()
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        vd = torch.empty(src.shape, dtype=torch.float32, device="cuda:0")
        for _ in range(20):  # keep the stream busy so that the build would overtake an unfinished producer
            vd.copy_(src, non_blocking=True)
        vd.add_(float(shift))
        ad = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0", non_blocking=True)
        ed = torch.from_numpy(np.ascontiguousarray(e, np.float32)).to("cuda:0", non_blocking=True)
        renderer.set_mesh_device(vd, ad, ed)
    check_bvh(renderer, v_host)
    renderer.resize(96, 54)
    got = renderer.render_pt(spp=1, bounces=1, seed=1, sky=(0.2, 0.2, 0.25))
    renderer.set_mesh(v_host, a, e)
    assert np.array_equal(renderer.render_pt(spp=1, bounces=1, seed=1, sky=(0.2, 0.2, 0.25)), got)


# ---- 8. CLI ----------------------------------------------------------------------------------------------------------------

def test_cli_device_bvh_writes_the_host_bvh_file(tmp_path):
    exe = os.path.join(ROOT, "host", "rt_host")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    outs = {}
    for which in ("host", "device"):
        outs[which] = tmp_path / f"{which}.pfm"
        subprocess.run([exe, "--size", "96x54", "--scene", "soup:5000", "--bvh", which, "--spp", "2", "--bounces", "1", "--seed", "3",
                        "--out", str(outs[which])], check=True, timeout=300)
    assert outs["host"].read_bytes() == outs["device"].read_bytes()
