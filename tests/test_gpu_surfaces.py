"""Mirror and glass surfaces on path B (rt_set_mesh_surfaces / Renderer.set_surfaces), on the GPU.

The frames must equal the test reference (tests/native/pt_surfaces_ref.c, pinned against oracle B and analytic answers by
tests/test_pt_surfaces_ref.py) bit for bit, with equal camera / bounce / shadow ray counts, for every builder, scheduling knob,
frame slot and partition; meshes without surfaces must keep rendering oracle B's frames."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import raytracing_engine_amd as R
from raytracing_engine_amd import scenes
from test_gpu_device_bvh import dev
from test_pt_surfaces_ref import GLASS, LAMBERT, MIRROR, SurfRef

pytestmark = pytest.mark.gpu
RT_ERR_INVALID, RT_ERR_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CORNELL_VIEW = dict(pos=(0, 1, 0))
SOUP_VIEW = dict(sky=(0.2, 0.2, 0.25))
COUNTS = ("camera_rays", "bounce_rays", "shadow_rays")


def check(r, ref, w, h, rot=(0, 0, 0, 1), pos=(0, 0, 0), packets=(0, 1), **kw):
    """The current mesh's frame (through the packet kernel and the per-lane kernel) equals the reference's, counts included."""
    r.resize(w, h)
    rkw = {k: kw[k] for k in ("spp", "bounces", "seed", "sky", "ray_eps") if k in kw}
    want, ct = ref.render(w, h, rot=rot, pos=pos, **rkw)
    for no_packet in packets:
        rgb = r.render_pt(rot, pos, tune_no_packet=no_packet, **kw)
        assert np.array_equal(rgb, want), f"no_packet={no_packet} {kw}: {np.count_nonzero(rgb != want)} values differ, max {np.abs(rgb - want).max()}"
        st = r.pt_stats()
        assert st["stack_overflow"] == 0
        assert {k: st[k] for k in COUNTS} == ct, kw
    return want


def cornell(variant="both"):
    v, a, e, kind, ior = scenes.cornell_surfaces_scene()
    if variant == "mirror":
        kind = np.where(kind == GLASS, MIRROR, kind).astype(np.uint32)
    elif variant == "glass":
        kind = np.where(kind == MIRROR, GLASS, kind).astype(np.uint32)
        a = a.copy()
        a[14:26] = 1.0
        ior = np.where(kind == GLASS, f32(1.5), ior).astype(f32)
    return (v, a, e), kind, ior


@pytest.mark.parametrize("bounces", [0, 1, 3, 8])
@pytest.mark.parametrize("spp", [1, 3, 4])
def test_cornell_surfaces_bit_exact(renderer, bounces, spp):
    mesh, kind, ior = cornell()
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    check(renderer, SurfRef(*mesh, kind, ior), 64, 48, spp=spp, bounces=bounces, seed=5, **CORNELL_VIEW)


@pytest.mark.parametrize("variant", ["mirror", "glass"])
@pytest.mark.parametrize("bounces", [1, 3, 8])
def test_mirror_only_and_glass_only(renderer, variant, bounces):
    mesh, kind, ior = cornell(variant)
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    check(renderer, SurfRef(*mesh, kind, ior), 64, 48, spp=2, bounces=bounces, seed=11, **CORNELL_VIEW)


@pytest.mark.parametrize("fracs", [(0.1, 0.1, 1.5), (0.0, 0.5, 1.33)])
def test_soup_100k_surfaces(renderer, fracs):
    mesh = scenes.soup_scene(100000, seed=1)
    kind, ior = scenes.soup_surfaces(100000, 1, *fracs)
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    ref = SurfRef(*mesh, kind, ior)
    check(renderer, ref, 96, 54, spp=3, bounces=3, seed=2, **SOUP_VIEW)
    check(renderer, ref, 96, 54, spp=1, bounces=8, seed=4, packets=(0,), **SOUP_VIEW)


@pytest.mark.parametrize("knob", [dict(tune_tri_mode=2), dict(tune_no_overlap=1), dict(tune_no_overlap=2), dict(tune_sort_rays=1),
                                  dict(tune_sort_rays=2), dict(max_paths=8192)])
def test_scheduling_knobs_give_identical_frames(renderer, knob):
    mesh, kind, ior = cornell()
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    check(renderer, SurfRef(*mesh, kind, ior), 96, 64, spp=3, bounces=3, seed=7, **CORNELL_VIEW, **knob)


# ---- builders, refit, chunk rebuild -----------------------------------------------------------------------------------------

def test_two_level_and_device_built_meshes():
    mesh = scenes.soup_scene(20000, seed=3)
    kind, ior = scenes.soup_surfaces(20000, 3, 0.15, 0.15, 1.6)
    ref = SurfRef(*mesh, kind, ior)
    with R.Renderer(0) as r:
        r.set_mesh(*mesh, bvh_levels=2, blas_chunks=16)
        r.set_surfaces(kind, ior)
        want = check(r, ref, 96, 54, spp=2, bounces=3, seed=1, **SOUP_VIEW)
        r.set_mesh_device(*dev(mesh, r.device))
        r.set_surfaces(kind, ior)
        assert np.array_equal(check(r, ref, 96, 54, spp=2, bounces=3, seed=1, **SOUP_VIEW), want)


def moved_cornell(mesh):
    """The mirror box lifted and the glass box shifted sideways: every other triangle stays."""
    v = np.asarray(mesh[0], f32).reshape(-1, 3, 3).copy()
    v[14:26, :, 2] += f32(1.25)
    v[26:38, :, 0] -= f32(1.5)
    return v.reshape(-1, 9), mesh[1], mesh[2]


@pytest.mark.parametrize("how", ["host", "device"])
def test_surfaces_survive_refit(how):
    import torch

    mesh, kind, ior = cornell()
    moved = moved_cornell(mesh)
    with R.Renderer(0) as r:
        if how == "host":
            r.set_mesh(*mesh)
        else:
            r.set_mesh_device(*dev(mesh, r.device))
        r.set_surfaces(kind, ior)
        check(r, SurfRef(*mesh, kind, ior), 64, 48, spp=2, bounces=3, seed=3, **CORNELL_VIEW)
        r.refit_mesh_device(torch.from_numpy(np.ascontiguousarray(moved[0])).to(f"cuda:{r.device}"))
        check(r, SurfRef(*moved, kind, ior), 64, 48, spp=2, bounces=3, seed=3, **CORNELL_VIEW)


def test_surfaces_survive_chunk_update():
    mesh = scenes.soup_scene(20000, seed=5)
    kind, ior = scenes.soup_surfaces(20000, 5, 0.2, 0.2, 1.5)
    with R.Renderer(0) as r:
        r.set_mesh(*mesh, bvh_levels=2, blas_chunks=8)
        r.set_surfaces(kind, ior)
        v = np.asarray(mesh[0], f32).reshape(-1, 9).copy()
        moved_chunks = 0
        for chunk in range(8):
            ids = r.mesh_chunk(chunk)
            if (ids >= len(v) - 2).any():  # the light stays where it is
                continue
            v[ids] = v[ids] + np.tile(np.array([0.3, -0.2, 0.1], f32), 3)
            r.update_mesh_chunk(chunk, v[ids])
            moved_chunks += 1
            if moved_chunks == 2:
                break
        assert moved_chunks == 2
        moved = (v, mesh[1], mesh[2])
        check(r, SurfRef(*moved, kind, ior), 96, 54, spp=2, bounces=3, seed=6, **SOUP_VIEW)


# ---- frame slots and partitions ---------------------------------------------------------------------------------------------

def test_frame_slots_render_the_surfaces():
    mesh, kind, ior = cornell()
    with R.Renderer(0) as r:
        r.set_mesh(*mesh)
        r.resize(64, 48)
        r.frames_configure(2, r.FRAME_F32)
        prm = r.pt_params(spp=2, bounces=3, seed=9)
        poses = [(0.0, 1.0 + 0.2 * k, 0.0) for k in range(4)]
        r.frame_submit(0, pos=poses[0], pt_params=prm)  # in flight while the surfaces are set: renders the Lambert mesh
        r.set_surfaces(kind, ior)
        lam, _ = O.TriScene(*mesh).render(64, 48, spp=2, bounces=3, seed=9, pos=poses[0])
        assert np.array_equal(r.frame_wait(0), lam)
        ref = SurfRef(*mesh, kind, ior)
        got = []
        for k in range(4):
            r.frame_submit(k % 2, pos=poses[k], pt_params=prm)
            if k >= 1:
                got.append(r.frame_wait((k - 1) % 2))
        got.append(r.frame_wait(1))
        for k in range(4):
            assert np.array_equal(got[k], ref.render(64, 48, spp=2, bounces=3, seed=9, pos=poses[k])[0]), k


def test_two_rank_partition_union_equals_full_frame(renderer):
    import torch

    mesh, kind, ior = cornell()
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    w, h, n_ranks = 200, 136, 2
    renderer.resize(w, h)
    renderer.set_partition(0, 1)
    prm = renderer.pt_params(spp=2, bounces=3, seed=9)
    full = renderer.render_pt(pos=(0, 1, 0), params=prm)
    assert np.array_equal(full, SurfRef(*mesh, kind, ior).render(w, h, spp=2, bounces=3, seed=9, pos=(0, 1, 0))[0])
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


# ---- unchanged behaviour and errors -----------------------------------------------------------------------------------------

def oracle_frame(r, mesh, w=64, h=48, **kw):
    r.resize(w, h)
    want, ct = O.TriScene(*mesh).render(w, h, **kw)
    assert np.array_equal(r.render_pt(**kw), want)
    assert {k: r.pt_stats()[k] for k in COUNTS} == {k: ct[k] for k in COUNTS}


def test_lambert_surfaces_and_resets_give_oracle_b(renderer):
    mesh, kind, ior = cornell()
    kw = dict(spp=2, bounces=3, seed=4, pos=(0, 1, 0))
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(np.zeros(len(kind), np.uint32))  # all Lambert through the call
    oracle_frame(renderer, mesh, **kw)
    renderer.set_surfaces(kind, ior)
    renderer.resize(64, 48)
    assert not np.array_equal(renderer.render_pt(**kw), O.TriScene(*mesh).render(64, 48, **kw)[0])
    renderer.set_surfaces(None)  # reset
    oracle_frame(renderer, mesh, **kw)
    renderer.set_surfaces(kind, ior)
    renderer.set_mesh(*mesh)  # a new mesh starts all Lambert
    oracle_frame(renderer, mesh, **kw)
    renderer.set_surfaces(kind, ior)
    renderer.set_mesh_device(*dev(mesh, renderer.device))
    oracle_frame(renderer, mesh, **kw)


def test_errors_leave_the_surfaces(renderer):
    import ctypes as C

    mesh, kind, ior = cornell()
    n = len(kind)
    lib, ctx = renderer._lib, renderer._ctx
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    with R.Renderer(0) as fresh:  # no mesh
        assert fresh._lib.rt_set_mesh_surfaces(fresh._ctx, u32p(kind), fp(ior), n) == RT_ERR_STATE
    renderer.set_mesh(*mesh)
    renderer.set_surfaces(kind, ior)
    ref = SurfRef(*mesh, kind, ior)
    kw = dict(spp=2, bounces=3, seed=8, **CORNELL_VIEW)
    check(renderer, ref, 64, 48, packets=(0,), **kw)
    bad_kind = kind.copy()
    bad_kind[3] = 3
    nan_ior, low_ior, high_ior = ior.copy(), ior.copy(), ior.copy()
    nan_ior[30], low_ior[30], high_ior[30] = np.nan, f32(0.99), f32(4.01)
    inf_ior = ior.copy()
    inf_ior[27] = np.inf
    mirror_only = np.where(kind == GLASS, MIRROR, kind).astype(np.uint32)
    cases = [
        (u32p(kind), fp(ior), n - 1),            # n_tris is not the mesh's
        (u32p(kind), fp(ior), n + 1),
        (u32p(bad_kind), fp(ior), n),            # a kind above 2
        (u32p(kind), fp(nan_ior), n),            # glass with a non-finite or out-of-range index
        (u32p(kind), fp(inf_ior), n),
        (u32p(kind), fp(low_ior), n),
        (u32p(kind), fp(high_ior), n),
        (u32p(kind), None, n),                   # glass without ior
    ]
    for k, i, cnt in cases:
        assert lib.rt_set_mesh_surfaces(ctx, k, i, cnt) == RT_ERR_INVALID
        check(renderer, ref, 64, 48, packets=(0,), **kw)
    # ior is not read where no kind is glass: NULL is fine then, and NaN at a mirror triangle is never looked at
    assert lib.rt_set_mesh_surfaces(ctx, u32p(mirror_only), None, n) == 0
    check(renderer, SurfRef(*mesh, mirror_only, ior), 64, 48, packets=(0,), **kw)
    nan_at_mirror = ior.copy()
    nan_at_mirror[14] = np.nan
    assert lib.rt_set_mesh_surfaces(ctx, u32p(kind), fp(nan_at_mirror), n) == 0
    check(renderer, ref, 64, 48, packets=(0,), **kw)
    with pytest.raises(ValueError):
        renderer.set_surfaces(kind.reshape(2, -1), ior)
    with pytest.raises(ValueError):
        renderer.set_surfaces(kind, ior[:-1])
    with pytest.raises(R.RtError) as ei:
        renderer.set_surfaces(kind[:-1])
    assert ei.value.code == RT_ERR_INVALID
    check(renderer, ref, 64, 48, packets=(0,), **kw)


# ---- the host CLI -------------------------------------------------------------------------------------------------------------

def test_host_cli_surfaces(tmp_path):
    from test_gpu_host_cli import EXE, read_pfm

    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    out = tmp_path / "s.pfm"
    subprocess.run([EXE, "--size", "96x54", "--scene", "soup:5000", "--surfaces", "0.1,0.1,1.5", "--spp", "2", "--bounces", "3", "--seed", "3",
                    "--out", str(out)], check=True)
    mesh = scenes.soup_scene(5000, seed=1, edge=0.25)
    kind, ior = scenes.soup_surfaces(5000, 1, 0.1, 0.1, 1.5)
    want, _ = SurfRef(*mesh, kind, ior).render(96, 54, spp=2, bounces=3, seed=3, sky=(0.2, 0.2, 0.25))
    assert np.array_equal(read_pfm(out), want)
    plain, _ = O.TriScene(*mesh).render(96, 54, spp=2, bounces=3, seed=3, sky=(0.2, 0.2, 0.25))
    assert not np.array_equal(want, plain)
