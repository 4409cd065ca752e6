"""Path B's ray queries on the GPU against exact geometry, on every way a tree comes to be.

For each ray family of tests/ray_exact.py ((a)-(j): interior, edge and vertex rays, from near and from 32 M away, a translated and
a small-edged soup, grazing incidence, occlusion segments ending at 0.999 and starting on a plane) rt_trace_rays (closest hit, any
hit) and rt_trace_rays_counted run on the host-built single-level tree, the two-level tree with 64 chunks, the device-built tree,
that tree after an identity refit and after a refit to moved vertices.  Two assertions per run: the answers are the oracle's
brute-force answers bit for bit, and they satisfy the float64 contract on their own (so the test keeps its meaning if the oracle
changes).  The oracle itself is held to the contract in tests/test_ray_contract.py."""
import functools

import numpy as np
import pytest

import oracle as O
import ray_exact as X

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def family_data(name):
    """Per part: the oracle's brute-force answers and the float64 candidates, on the part's mesh and on the moved mesh."""
    out = []
    for part in X.family(name):
        v = X.mesh(part["mesh"])[0]
        vm = X.moved(v)
        out.append(dict(part=part, ref=X.part_reference(part), cand=X.part_candidates(part),
                        moved=vm, ref_moved=X.part_reference(part, verts=vm), cand_moved=X.part_candidates(part, verts=vm)))
    return out


@pytest.fixture(scope="module", params=X.FAMILIES)
def fam(request):
    return request.param, family_data(request.param)


def check_runs(renderer, name, part, ref, cand, what):
    cc, co = cand
    for counted in (False, True):
        got = renderer.trace_rays(part["o"], part["d"], counted=counted)
        t, tri = got[0], got[1]
        assert np.array_equal(tri, ref["tri"]), (name, part["mesh"], what, counted, np.nonzero(tri != ref["tri"])[0][:8])
        assert np.array_equal(t, ref["t"]), (name, part["mesh"], what, counted, np.nonzero(t != ref["t"])[0][:8])  # inf on a miss, both
        if counted:
            assert (got[2][:, 0] > 0).all()  # every ray fetched the root
        if name in X.CLOSEST_FAMILIES:
            ok = cc.check_closest(tri, t)
            assert ok.all(), (name, part["mesh"], what, "closest hit outside the contract", np.nonzero(~ok)[0][:8])
    _, occ = renderer.trace_rays(part["o"], part["seg"], any_hit=True)
    assert np.array_equal(occ.astype(bool), ref["occ"]), (name, part["mesh"], what, np.nonzero(occ.astype(bool) != ref["occ"])[0][:8])
    ok = co.check_occluded(occ)
    assert ok.all(), (name, part["mesh"], what, "occlusion outside the contract", np.nonzero(~ok)[0][:8])


@pytest.mark.parametrize("tree", ["host", "two_level"])
def test_host_built_trees(renderer, fam, tree):
    name, data = fam
    for p in data:
        v, a, e = X.mesh(p["part"]["mesh"])
        if tree == "host":
            renderer.set_mesh(v, a, e)
        else:
            renderer.set_mesh(v, a, e, bvh_levels=2, blas_chunks=64)
        check_runs(renderer, name, p["part"], p["ref"], p["cand"], tree)


def test_device_built_tree_and_refits(renderer, fam):
    import torch

    name, data = fam
    dev = torch.device("cuda", renderer.device)
    for p in data:
        v, a, e = X.mesh(p["part"]["mesh"])
        tv, ta, te = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (v, a, e))
        renderer.set_mesh_device(tv, ta, te)
        check_runs(renderer, name, p["part"], p["ref"], p["cand"], "device build")
        renderer.refit_mesh_device(tv)
        check_runs(renderer, name, p["part"], p["ref"], p["cand"], "identity refit")
        renderer.refit_mesh_device(torch.from_numpy(p["moved"]).to(dev))
        check_runs(renderer, name, p["part"], p["ref_moved"], p["cand_moved"], "refit to moved vertices")
        assert not np.array_equal(p["ref"]["t"], p["ref_moved"]["t"])  # the moved mesh does answer differently


def grazing_view():
    """The flat grid (plane z = 5.3, two paddings thick) seen through a telephoto lens from 31 M away, 0.4 above its plane: every
    camera ray meets it at |cos| of about 2.5e-3, the case the padding-only slab test is tightest for."""
    v, a, e = X.flat_grid(axis=2)
    m = float(np.abs(v).max())
    h = 0.4
    pos = (0.0, -31.0 * m, float(np.float32(5.3)) + h)
    dist = 31.0 * m
    pitch = -float(np.arctan2(h, dist))
    half = 16 * 0.37 / 2
    ratio = (1.15 * half / dist, 1.15 * 0.5 * (h / (dist - half) - h / (dist + half)))
    return (v, a, e), m, pos, O.camera_quat(0.0, pitch), ratio


def test_grazing_telephoto_view_of_a_flat_mesh(renderer):
    """Case (h) through the render kernels: the frame equals the oracle's bit for bit however the camera rays are traced
    (per-lane kernel, and the packet kernel with each of its node tests), as do the ray counts."""
    mesh, m, pos, rot, ratio = grazing_view()
    w, h = 96, 64
    kw = dict(spp=2, bounces=1, seed=3, sky=(0.3, 0.3, 0.4))
    ref, ct = O.TriScene(*mesh).render(w, h, rot=rot, pos=pos, ratio=ratio, **kw)
    assert ct["bounce_rays"] > 0.5 * ct["camera_rays"], "the view must look at the mesh"
    renderer.set_mesh(*mesh)
    renderer.resize(w, h, ratio=ratio)
    try:
        for mode in (1, 2, 3, 4, 5):
            rgb = renderer.render_pt(rot=rot, pos=pos, tune_no_packet=mode, **kw)
            st = renderer.pt_stats()
            assert np.array_equal(rgb, ref), (mode, np.count_nonzero(rgb != ref))
            assert (st["camera_rays"], st["bounce_rays"], st["shadow_rays"]) == (ct["camera_rays"], ct["bounce_rays"], ct["shadow_rays"])
    finally:
        renderer.resize(64, 64)
