"""One resident device mesh for the contexts that are given the same host mesh (rt_mesh_sharers), on the GPU.

Contexts given equal arrays and build options report each other as sharers and render oracle B's frames bit for bit, as they do
with RT_AMD_MESH_SHARING=0; any difference in the input keeps them apart; a context that changes its mesh (refit, chunk rebuild,
surfaces) leaves the others' frames untouched and renders what a context built from the changed mesh renders; the mesh outlives
the context that uploaded it and dies with the last one.  The meshes here are used by no other test file, so the session's shared
renderer never counts among the sharers."""
import contextlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle as O
import raytracing_engine_amd as R
from raytracing_engine_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
VIEW = dict(spp=2, bounces=2, seed=4, sky=(0.2, 0.2, 0.25))
W, H = 96, 54
COUNTS = ("camera_rays", "bounce_rays", "shadow_rays")


@contextlib.contextmanager
def sharing(on):
    """RT_AMD_MESH_SHARING for the set_mesh calls inside the block (the library reads it at every call)."""
    old = os.environ.get("RT_AMD_MESH_SHARING")
    os.environ["RT_AMD_MESH_SHARING"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["RT_AMD_MESH_SHARING"]
        else:
            os.environ["RT_AMD_MESH_SHARING"] = old


def soup(n, seed):
    v, a, e = scenes.soup_scene(n, seed=seed, edge=0.5)
    return np.ascontiguousarray(v, f32).reshape(-1, 9), np.ascontiguousarray(a, f32).reshape(-1, 3), np.ascontiguousarray(e, f32).reshape(-1, 3)


def frame(r, **kw):
    r.resize(W, H)
    rgb = r.render_pt(**dict(VIEW, **kw))
    st = r.pt_stats()
    assert st["stack_overflow"] == 0
    return rgb, {k: st[k] for k in COUNTS}


def oracle_frame(mesh, **kw):
    rgb, ct = O.TriScene(*mesh).render(W, H, **dict(VIEW, **kw))
    return rgb, {k: ct[k] for k in COUNTS}


def scratch_frame(mesh, after_set=None, **set_kw):
    """The frame of a context that builds and uploads `mesh` for itself."""
    with sharing(False), R.Renderer(0) as r:
        r.set_mesh(*mesh, **set_kw)
        assert r.mesh_sharers() == 1
        if after_set:
            after_set(r)
        return frame(r)


def tdev(v):
    import torch

    return torch.from_numpy(np.ascontiguousarray(v, f32).reshape(-1, 9)).to("cuda:0")


# ---- sharing on and off ----------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import raytracing_engine_amd as R
from raytracing_engine_amd import scenes
n, out = int(sys.argv[2]), sys.argv[3]
mesh = scenes.soup_scene(6100, seed=61, edge=0.5)
rs = [R.Renderer(0) for _ in range(n)]
seen = []
for r in rs:
    r.set_mesh(*mesh)
    seen.append(r.mesh_sharers())
frames, counts = [], []
for r in rs:
    r.resize(96, 54)
    frames.append(r.render_pt(spp=2, bounces=2, seed=4, sky=(0.2, 0.2, 0.25)))
    st = r.pt_stats()
    counts.append([st[k] for k in ("camera_rays", "bounce_rays", "shadow_rays", "n_nodes", "n_tris", "n_lights")])
sharers = [r.mesh_sharers() for r in rs]
for r in rs:
    r.close()
np.save(out, np.stack(frames))
print(json.dumps({"seen": seen, "sharers": sharers, "counts": counts}))
"""


@pytest.mark.parametrize("n", [2, 3])
def test_same_soup_is_shared_and_frames_equal_the_unshared_ones(tmp_path, n):
    got = {}
    for mode in ("1", "0"):
        out = tmp_path / f"frames_{mode}.npy"
        env = dict(os.environ, RT_AMD_MESH_SHARING=mode)
        p = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(n), str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = (json.loads(p.stdout.strip().splitlines()[-1]), np.load(out))
    on, off = got["1"], got["0"]
    assert on[0]["seen"] == list(range(1, n + 1)) and on[0]["sharers"] == [n] * n
    assert off[0]["seen"] == [1] * n and off[0]["sharers"] == [1] * n
    assert on[0]["counts"] == off[0]["counts"] and all(c == on[0]["counts"][0] for c in on[0]["counts"])
    assert np.array_equal(on[1], off[1])
    ref, ct = oracle_frame(scenes.soup_scene(6100, seed=61, edge=0.5))
    for k in range(n):
        assert np.array_equal(on[1][k], ref), k
    assert on[0]["counts"][0][:3] == [ct[k] for k in COUNTS]


def test_unset_variable_means_sharing():
    mesh = soup(2100, 62)
    old = os.environ.pop("RT_AMD_MESH_SHARING", None)
    try:
        with R.Renderer(0) as a, R.Renderer(0) as b:
            assert a.mesh_sharers() == 0
            a.set_mesh(*mesh)
            b.set_mesh(*mesh)
            assert (a.mesh_sharers(), b.mesh_sharers()) == (2, 2)
            with sharing(False):
                b.set_mesh(*mesh)  # read at every call
            assert (a.mesh_sharers(), b.mesh_sharers()) == (1, 1)
    finally:
        if old is not None:
            os.environ["RT_AMD_MESH_SHARING"] = old


# ---- what keeps meshes apart -------------------------------------------------------------------------------------------------

def test_different_inputs_do_not_share():
    v, a, e = soup(5200, 63)
    one_vertex = v.copy()
    one_vertex[1234, 4] = np.nextafter(one_vertex[1234, 4], f32(10))
    one_albedo = a.copy()
    one_albedo[77, 2] = np.nextafter(one_albedo[77, 2], f32(0))
    one_emission = e.copy()
    one_emission[5, 0] = f32(0.25)  # one more light
    variants = [dict(mesh=(v, a, e)), dict(mesh=(one_vertex, a, e)), dict(mesh=(v, one_albedo, e)), dict(mesh=(v, a, one_emission)),
                dict(mesh=(v[1:], a[1:], e[1:])), dict(mesh=(v, a, e), bvh_levels=2), dict(mesh=(v, a, e), bvh_levels=2, blas_chunks=16)]
    with sharing(True), contextlib.ExitStack() as stack:
        rs = []
        for var in variants:
            r = stack.enter_context(R.Renderer(0))
            r.set_mesh(*var["mesh"], **{k: var[k] for k in var if k != "mesh"})
            rs.append(r)
        assert [r.mesh_sharers() for r in rs] == [1] * len(rs)
        # the same again: each variant finds its own mesh and no other
        twins = []
        for var in variants:
            r = stack.enter_context(R.Renderer(0))
            r.set_mesh(*[x.copy() for x in var["mesh"]], **{k: var[k] for k in var if k != "mesh"})  # equal bytes at other addresses
            twins.append(r)
        assert [r.mesh_sharers() for r in rs + twins] == [2] * (2 * len(rs))
        for var, r, t in zip(variants, rs, twins):
            ref, ct = oracle_frame(var["mesh"])
            for x in (r, t):
                rgb, counts = frame(x)
                assert np.array_equal(rgb, ref) and counts == ct
        assert twins[5].pt_stats()["bvh_levels"] == 2 and twins[5].pt_stats()["blas_chunks"] == 64 and twins[6].pt_stats()["blas_chunks"] == 16
        # a single-level build does not read the chunk count
        r = stack.enter_context(R.Renderer(0))
        r.set_mesh(v, a, e, bvh_levels=1, blas_chunks=16)
        assert r.mesh_sharers() == 3


def test_device_built_meshes_never_share():
    from test_gpu_device_bvh import dev

    mesh = soup(3300, 64)
    with sharing(True), R.Renderer(0) as a, R.Renderer(0) as b, R.Renderer(0) as c:
        a.set_mesh(*mesh)
        b.set_mesh_device(*dev(mesh))
        c.set_mesh_device(*dev(mesh))
        assert (a.mesh_sharers(), b.mesh_sharers(), c.mesh_sharers()) == (1, 1, 1)
        ref, _ = oracle_frame(mesh)
        for r in (a, b, c):
            assert np.array_equal(frame(r)[0], ref)


# ---- copy on write -----------------------------------------------------------------------------------------------------------

def moved(v, seed):
    rng = np.random.default_rng(seed)
    out = v.copy()
    out[:-2] += np.tile(rng.uniform(-0.05, 0.05, (len(v) - 2, 3)).astype(f32), 3)  # the light (the last two triangles) stays
    return out


def test_refit_on_one_sharer():
    v, a, e = mesh = soup(7300, 65)
    v2, v3 = moved(v, 1), moved(v, 2)
    ref, ct = oracle_frame(mesh)
    with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb, R.Renderer(0) as rc:
        for r in (ra, rb, rc):
            r.set_mesh(*mesh)
        before = [frame(r) for r in (rb, rc)]
        assert np.array_equal(before[0][0], ref) and before[0][1] == ct
        ra.refit_mesh_device(tdev(v2))
        assert [r.mesh_sharers() for r in (ra, rb, rc)] == [1, 2, 2]
        for r, (rgb, counts) in zip((rb, rc), before):
            again = frame(r)
            assert np.array_equal(again[0], rgb) and again[1] == counts
        want = scratch_frame((v2, a, e))
        got = frame(ra)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        ref2, ct2 = oracle_frame((v2, a, e))
        assert np.array_equal(got[0], ref2) and got[1] == ct2
        # the second refit writes in place (sole holder); the original is still listed for newcomers, the refitted mesh is not
        ra.refit_mesh_device(tdev(v3))
        ref3, ct3 = oracle_frame((v3, a, e))
        got = frame(ra)
        assert np.array_equal(got[0], ref3) and got[1] == ct3
        with R.Renderer(0) as rd:
            rd.set_mesh(*mesh)
            assert [r.mesh_sharers() for r in (ra, rb, rc, rd)] == [1, 3, 3, 3]
            assert np.array_equal(frame(rd)[0], ref)
        assert np.array_equal(frame(rb)[0], ref)


def test_refit_by_the_only_holder_unlists_the_mesh():
    v, a, e = mesh = soup(4100, 66)
    v2 = moved(v, 3)
    with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb:
        ra.set_mesh(*mesh)
        ra.refit_mesh_device(tdev(v2))  # in place: what is resident is no longer the mesh that was set
        rb.set_mesh(*mesh)
        assert (ra.mesh_sharers(), rb.mesh_sharers()) == (1, 1)
        assert np.array_equal(frame(rb)[0], oracle_frame(mesh)[0])
        assert np.array_equal(frame(ra)[0], oracle_frame((v2, a, e))[0])


def test_chunk_update_on_one_sharer():
    v, a, e = mesh = soup(8200, 67)
    opts = dict(bvh_levels=2, blas_chunks=8)
    ref, ct = oracle_frame(mesh)
    with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb:
        ra.set_mesh(*mesh, **opts)
        rb.set_mesh(*mesh, **opts)
        assert (ra.mesh_sharers(), rb.mesh_sharers()) == (2, 2)
        before = frame(rb)
        assert np.array_equal(before[0], ref) and before[1] == ct
        v2 = v.copy()
        chunk = next(k for k in range(8) if not (ra.mesh_chunk(k) >= len(v) - 2).any())
        ids = ra.mesh_chunk(chunk)
        assert np.array_equal(ids, rb.mesh_chunk(chunk))
        v2[ids] += np.tile(np.array([0.3, -0.2, 0.1], f32), 3)
        ra.update_mesh_chunk(chunk, v2[ids])
        assert (ra.mesh_sharers(), rb.mesh_sharers()) == (1, 1)
        again = frame(rb)
        assert np.array_equal(again[0], before[0]) and again[1] == before[1]
        assert np.array_equal(rb.mesh_chunk(chunk), ids)
        want = scratch_frame((v2, a, e), **opts)
        got = frame(ra)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        ref2, ct2 = oracle_frame((v2, a, e))
        assert np.array_equal(got[0], ref2) and got[1] == ct2 and not np.array_equal(ref2, ref)
        # the other sharer's host side is its own too: its update of the same chunk starts from the unmoved vertices
        v3 = v.copy()
        v3[ids] += np.tile(np.array([-0.1, 0.1, 0.2], f32), 3)
        rb.update_mesh_chunk(chunk, v3[ids])
        assert np.array_equal(frame(rb)[0], oracle_frame((v3, a, e))[0])
        assert np.array_equal(frame(ra)[0], ref2)


def test_surfaces_on_one_sharer():
    n = 6400
    mesh = soup(n, 68)
    kind, ior = scenes.soup_surfaces(n, 68, 0.2, 0.2, 1.5)
    ref, ct = oracle_frame(mesh)
    with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb, R.Renderer(0) as rc:
        for r in (ra, rb, rc):
            r.set_mesh(*mesh)
        before = frame(rb)
        assert np.array_equal(before[0], ref) and before[1] == ct
        ra.set_surfaces(kind, ior)
        assert [r.mesh_sharers() for r in (ra, rb, rc)] == [1, 2, 2]
        for r in (rb, rc):
            again = frame(r)
            assert np.array_equal(again[0], before[0]) and again[1] == before[1]
        want = scratch_frame(mesh, after_set=lambda r: r.set_surfaces(kind, ior))
        got = frame(ra)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        assert not np.array_equal(got[0], ref)  # mirrors and glass are in view
        ra.set_surfaces(None)  # Lambert again, but no longer the listed mesh
        assert np.array_equal(frame(ra)[0], ref) and ra.mesh_sharers() == 1
        rb.set_surfaces(kind, ior)
        assert [r.mesh_sharers() for r in (ra, rb, rc)] == [1, 1, 1]
        assert np.array_equal(frame(rb)[0], want[0]) and np.array_equal(frame(rc)[0], ref)


def test_frame_slots_follow_their_context_through_a_detach():
    mesh = soup(5600, 69)
    v2 = moved(mesh[0], 5)
    ref, ref2 = oracle_frame(mesh)[0], oracle_frame((v2, mesh[1], mesh[2]))[0]
    with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb:
        ra.set_mesh(*mesh)
        rb.set_mesh(*mesh)
        for r in (ra, rb):
            r.resize(W, H)
            r.frames_configure(2, r.FRAME_F32)
        prm = ra.pt_params(**VIEW)
        for r in (ra, rb):
            r.frame_submit(0, pt_params=prm)
        ra.refit_mesh_device(tdev(v2))  # while slot 0 of both is in flight
        for r in (ra, rb):
            assert np.array_equal(r.frame_wait(0), ref)
            r.frame_submit(1, pt_params=prm)
            r.frame_submit(0, pt_params=prm)
        for slot in (1, 0):
            assert np.array_equal(ra.frame_wait(slot), ref2)
            assert np.array_equal(rb.frame_wait(slot), ref)
        assert (ra.mesh_sharers(), rb.mesh_sharers()) == (1, 1)


# ---- lifetime ----------------------------------------------------------------------------------------------------------------

def test_mesh_outlives_its_uploader_and_dies_with_the_last_context():
    mesh = soup(6700, 70)
    ref, ct = oracle_frame(mesh)
    with sharing(True):
        ra, rb, rc = R.Renderer(0), R.Renderer(0), R.Renderer(0)
        try:
            for r in (ra, rb, rc):
                r.set_mesh(*mesh)
            first = [frame(r) for r in (rb, rc)]
            ra.close()  # it built and uploaded the mesh
            assert (rb.mesh_sharers(), rc.mesh_sharers()) == (2, 2)
            for r, (rgb, counts) in zip((rb, rc), first):
                again = frame(r)
                assert np.array_equal(again[0], rgb) and np.array_equal(rgb, ref) and again[1] == counts == ct
            rb.close()
            assert rc.mesh_sharers() == 1 and np.array_equal(frame(rc)[0], ref)
            rc.close()
            with R.Renderer(0) as rd:
                rd.set_mesh(*mesh)  # nothing is resident any more: builds again
                assert rd.mesh_sharers() == 1
                assert rd.pt_stats()["bvh_build_ms"] > 0
                assert np.array_equal(frame(rd)[0], ref)
        finally:
            for r in (ra, rb, rc):
                r.close()


@pytest.mark.parametrize("on", [True, False], ids=["sharing", "no_sharing"])
def test_swap_to_another_mesh_and_back(on):
    cornell = scenes.cornell_tri_scene()
    other = soup(3400, 71)
    cref, cct = oracle_frame(cornell, pos=(0, 1, 0))
    oref, oct_ = oracle_frame(other)
    with sharing(on), R.Renderer(0) as keeper, R.Renderer(0) as r:
        keeper.set_mesh(*cornell)
        held = keeper.mesh_sharers()  # other tests' contexts may render the Cornell box too
        for mesh, view, ref, ct, shared in [(cornell, dict(pos=(0, 1, 0)), cref, cct, 1), (other, {}, oref, oct_, 0), (cornell, dict(pos=(0, 1, 0)), cref, cct, 1),
                                            (other, {}, oref, oct_, 0)]:
            r.set_mesh(*mesh)
            assert keeper.mesh_sharers() == (held + shared if on else held)
            assert r.mesh_sharers() == (keeper.mesh_sharers() if on and shared else 1)
            rgb, counts = frame(r, **view)
            assert np.array_equal(rgb, ref) and counts == ct
            rgb, counts = frame(keeper, pos=(0, 1, 0))
            assert np.array_equal(rgb, cref) and counts == cct


def test_two_threads_set_the_same_mesh():
    mesh = soup(30000, 72)
    ref, ct = oracle_frame(mesh)
    for _ in range(3):
        with sharing(True), R.Renderer(0) as ra, R.Renderer(0) as rb:
            gate = threading.Barrier(2)
            errors = []

            def work(r):
                try:
                    gate.wait()
                    r.set_mesh(*mesh)
                except Exception as ex:  # noqa: BLE001
                    errors.append(ex)

            ts = [threading.Thread(target=work, args=(r,)) for r in (ra, rb)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errors, errors
            assert (ra.mesh_sharers(), rb.mesh_sharers()) in ((1, 1), (2, 2))  # one copy, or two complete ones
            for r in (ra, rb):
                rgb, counts = frame(r)
                assert np.array_equal(rgb, ref) and counts == ct
            with R.Renderer(0) as rc:
                rc.set_mesh(*mesh)
                assert rc.mesh_sharers() in (2, 3)
                assert np.array_equal(frame(rc)[0], ref)
