"""pt_shade's load schedule (csrc/path_b.hip): every way through the kernel gives the oracle's frame bit for bit.

The kernel keeps the sampled lights in an LDS table while there are at most kShadeLightTable of them and loads them from
global memory above that; it has an instantiation for meshes with mirror and glass; behind the packet kernel it takes depth 0
without a queue and stores each path's radiance once; on a tile share some of its path slots lie outside the frame.  Each case
here takes one of these ways and compares the frame with np.array_equal and the three ray counters with oracle B's
(oracle.TriScene; with surfaces the test reference of tests/test_pt_surfaces_ref.py, which is the oracle plus section 6.11 and
is compared with the oracle here on the same mesh without surfaces).  The lights carry a colour each
(scenes.light_emission), so a table entry that holds another light's record or emission changes the frame."""
import os
import re

import numpy as np
import pytest

import oracle as O
from raytracing_engine_amd import scenes
from test_pt_surfaces_ref import SurfRef

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("camera_rays", "bounce_rays", "shadow_rays")
W, H = 96, 54
SKY = (0.2, 0.2, 0.25)
VIEW = dict(pos=(0.0, 15.0, 0.0), spp=2, seed=5, sky=SKY)  # inside the soup: x, z in [-10, 10], y in [5, 25]
N_TRIS = 3000


def table_size():
    src = open(os.path.join(ROOT, "raytracing_engine_amd", "csrc", "path_b.hip")).read()
    return int(re.search(r"constexpr uint32_t kShadeLightTable = (\d+);", src).group(1))


TABLE = table_size()


def soup(n_lights):
    """The soup with its first n_lights triangles lit (about 300: every tenth), each with its own colour."""
    base = scenes.soup_scene(N_TRIS, seed=5, edge=1.0)
    if n_lights == 300:
        return scenes.with_lights(base, "every", 10)
    return scenes.with_lights(base, "block", 0, n_lights)


def check(r, want, w=W, h=H, what="", **kw):
    r.resize(w, h)
    rgb = r.render_pt(**kw)
    assert np.isfinite(want[0]).all()
    assert np.array_equal(rgb, want[0]), f"{what}: {np.count_nonzero(rgb != want[0])} of {rgb.size} values differ"
    st = r.pt_stats()
    assert {k: st[k] for k in COUNTS} == {k: want[1][k] for k in COUNTS}, what
    return rgb


@pytest.mark.parametrize("n_lights", [1, 2, TABLE, TABLE + 1, 300])
def test_light_table_sizes(renderer, n_lights):
    assert TABLE in (32, 64)
    mesh = soup(n_lights)
    assert int((mesh[2] > 0).any(1).sum()) == n_lights
    view = dict(VIEW, bounces=2)
    want = O.TriScene(*mesh).render(W, H, threads=16, **view)
    assert want[1]["shadow_rays"] > 1000 and want[1]["bounce_rays"] > 1000
    renderer.set_mesh(*mesh)
    assert renderer.pt_stats()["n_lights"] == n_lights
    check(renderer, want, what=f"{n_lights} lights", **view)


def test_no_lights(renderer):
    mesh = scenes.with_lights(scenes.soup_scene(N_TRIS, seed=5, edge=1.0), "none")
    view = dict(VIEW, bounces=2)
    want = O.TriScene(*mesh).render(W, H, threads=16, **view)
    assert want[1]["shadow_rays"] == 0 and want[1]["bounce_rays"] > 1000
    renderer.set_mesh(*mesh)
    assert renderer.pt_stats()["n_lights"] == 0
    check(renderer, want, what="no lights", **view)


def test_mirror_and_glass_instantiation(renderer):
    mesh = soup(2)
    kind, ior = scenes.soup_surfaces(N_TRIS, 5, 0.1, 0.1, 1.5)
    view = dict(VIEW, bounces=3)
    lambert = O.TriScene(*mesh).render(W, H, threads=16, **view)
    plain = SurfRef(*mesh).render(W, H, threads=16, **view)
    assert np.array_equal(plain[0], lambert[0]) and {k: plain[1][k] for k in COUNTS} == {k: lambert[1][k] for k in COUNTS}
    want = SurfRef(*mesh, kind, ior).render(W, H, threads=16, **view)
    assert not np.array_equal(want[0], lambert[0])
    renderer.set_mesh(*mesh)
    check(renderer, lambert, what="before the surfaces", **view)
    try:
        renderer.set_surfaces(kind, ior)
        check(renderer, want, what="10 % mirror, 10 % glass", **view)
    finally:
        renderer.set_surfaces(None)


@pytest.mark.parametrize("no_packet", [0, 1])
def test_depth_0_with_and_without_the_queue(renderer, no_packet):
    mesh = scenes.cornell_tri_scene()
    view = dict(pos=(0, 1, 0), spp=2, bounces=3, seed=3)
    want = O.TriScene(*mesh).render(64, 64, threads=16, **view)
    assert want[1]["shadow_rays"] > 1000
    renderer.set_mesh(*mesh)
    check(renderer, want, 64, 64, what=f"tune_no_packet={no_packet}", tune_no_packet=no_packet, **view)


def test_tile_share_equals_the_same_tiles_of_the_whole_frame(renderer):
    """Rank 1 of 3 on a frame of 2 x 1 tiles owns the second tile, a third of which lies inside the frame: the other path slots of
    the share belong to no pixel and must neither be shaded nor stored."""
    import torch

    mesh = soup(2)
    view = dict(VIEW, bounces=2)
    pos = view.pop("pos")
    want = O.TriScene(*mesh).render(W, H, threads=16, pos=pos, **view)
    renderer.set_mesh(*mesh)
    full = check(renderer, want, what="whole frame", pos=pos, **view)
    prm = renderer.pt_params(**view)
    try:
        renderer.set_partition(1, 3)
        tx, ty, owned = renderer.tile_info()
        assert (tx, ty, owned) == (2, 1, 1)
        tiles = torch.zeros((owned, 64, 64, 3), dtype=torch.float32, device="cuda")
        renderer.render_pt_device((0, 0, 0, 1), pos, prm, tiles.data_ptr(), tile_major=True)
        renderer.synchronize()
        got = tiles.cpu().numpy()[0]  # tile 1: pixels x = 64 .. 127, y = 0 .. 63
        assert np.array_equal(got[:H, :W - 64], full[:, 64:])
    finally:
        renderer.set_partition(0, 1)
        renderer.resize(64, 64)
