"""The device BVH build and the refit against an independent reference tree, byte for byte.

The build (rt_set_mesh_device) is a deterministic function of the mesh, the refit (rt_refit_mesh_device) one of the
tree's topology and the new vertices (section 6.10).  tests/native/lbvh_ref.cpp restates both on the CPU by other means (std::sort, a
recursive radix tree, recursive unions, a queue); rt_read_bvh must equal its output exactly, at the sizes where a mechanism of
csrc/bvh_build_gpu.hip changes and on the mesh families of tests/lbvh_exact.py.  A tree that is merely valid and conservative - another
Morton bit order, an unstable sort pass, another child opened or another tie break in the collapse, a box left too large by the refit -
passes tests/test_gpu_device_bvh.py and tests/test_gpu_refit.py and fails here.  Nothing is rendered or queried."""
import numpy as np
import pytest

import lbvh_exact as LX
from raytracing_engine_amd import scenes
from test_gpu_device_bvh import dev

pytestmark = pytest.mark.gpu
f32 = np.float32


def materials(n, lights):
    a = np.full((n, 3), 0.5, f32)
    e = np.zeros((n, 3), f32)
    e[lights] = 2.0
    return a, e


def build(r, verts, how="device", lights=(0,)):
    mesh = (np.array(verts, f32),) + materials(len(verts), list(lights))  # a copy: the shared cases are read-only, torch wants writable arrays
    if how == "host":
        r.set_mesh(*mesh)
    else:
        r.set_mesh_device(*dev(mesh, r.device))


def refit(r, verts):
    import torch

    r.refit_mesh_device(torch.from_numpy(np.ascontiguousarray(verts, f32).reshape(-1, 9)).to(f"cuda:{r.device}"))


# ---- build ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LX.CASES, ids=[LX.case_id(c) for c in LX.CASES])
def test_device_build_equals_the_reference(renderer, case):
    verts, ref = LX.case(*case)
    build(renderer, verts)
    nodes, leaf = renderer.read_bvh()
    diff = LX.difference(nodes, leaf, ref["nodes"], ref["leaf"])
    assert diff is None, diff
    assert nodes.tobytes() == ref["nodes"].tobytes() and leaf.tobytes() == ref["leaf"].tobytes()
    st = renderer.pt_stats()
    assert (st["n_tris"], st["n_nodes"], st["bvh_depth"], st["stack_need"]) == (ref["n"], ref["n_nodes"], ref["depth"], ref["depth"] + 1)
    assert st["bvh_levels"] == 1
    LX.check_tree(nodes, leaf, verts)


# ---- payload ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [("random", LX.K_SORT_TILE + 1), ("shared_centroids", 16 * LX.K_SORT_TILE + 1)], ids=LX.case_id)
def test_payload_follows_the_leaf_order(renderer, case):
    """rt_read_bvh's leaf order IS word 9 of the leaf-order triangle records (it is gathered from them), so the comparison with the
    reference's leaf order pins that word.  Word 10 (the emission flag) and the light list have no reader in Renderer: they are held to
    n_lights, for lights at the borders of the flag scan's tiles, and no ABI entry is added for more (the frames of
    tests/test_gpu_lights.py depend on both)."""
    verts, ref = LX.case(*case)
    n = len(verts)
    lights = sorted({0, 1, LX.K_THREADS - 1, LX.K_THREADS, LX.K_SORT_TILE - 1, LX.K_SORT_TILE, n - 1} & set(range(n)))
    build(renderer, verts, lights=lights)
    nodes, leaf = renderer.read_bvh()
    assert leaf.tobytes() == ref["leaf"].tobytes() and nodes.tobytes() == ref["nodes"].tobytes()  # the tree does not depend on the materials
    assert renderer.pt_stats()["n_lights"] == len(lights)


# ---- refit ----------------------------------------------------------------------------------------------------------------------------------

def refit_mesh(name):
    if name == "deep":
        return np.ascontiguousarray(scenes.deep_scene()[0], f32).reshape(-1, 9)
    return LX.random_mesh(int(name))


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("name", ["700", "30000", "300000", "deep"])
def test_refit_equals_the_reference_refit(renderer, how, name):
    """700: the whole tree in bvhr_top; 30 000 and 300 000: levels above and below kRefitTopNodes, handed from bvhr_level to bvhr_top; deep: more
    levels than the structure tests' soups have.  Every motion is judged from the tree as it was read BEFORE that refit."""
    verts = refit_mesh(name)
    build(renderer, verts, how)
    first = renderer.read_bvh()
    if how == "device" and name != "deep":
        ref = LX.case("random", len(verts))[1]
        assert LX.difference(first[0], first[1], ref["nodes"], ref["leaf"]) is None
    sizes = np.diff([a for a, _ in LX.level_ranges(first[0])] + [len(first[0])])
    if name == "700":
        assert sizes.max() <= LX.K_REFIT_TOP_NODES and len(sizes) <= LX.K_REFIT_TOP_MAX
    if name in ("30000", "300000"):
        assert sizes.max() > LX.K_REFIT_TOP_NODES
    if (how, name) == ("host", "deep"):
        assert len(sizes) > LX.K_REFIT_TOP_MAX  # levels below the sixteenth are small and still go to bvhr_level
    before = first
    for motion in LX.MOTIONS:
        new = LX.moved(verts, motion)
        want = LX.reference_refit(before[0], before[1], new)
        refit(renderer, new)
        after = renderer.read_bvh()
        diff = LX.difference(after[0], after[1], want["nodes"], want["leaf"])
        assert diff is None, f"{motion}: {diff}"
        assert after[0].tobytes() == want["nodes"].tobytes() and after[1].tobytes() == before[1].tobytes()
        if motion != "back":
            assert after[0].tobytes() != first[0].tobytes(), motion
        before = after
    assert before[0].tobytes() == first[0].tobytes() and before[1].tobytes() == first[1].tobytes(), "back at the original vertices"
