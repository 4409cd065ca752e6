"""GPU tests of the wide packet kernel (pt_trace_packet_wide, tune_no_packet = 6 / 7): two / four camera rays per lane, one tree
walk per 128 / 256 paths.  Every frame must be oracle B's bit for bit and equal the 64-path kernel's (mode 4) of the same build,
with equal ray counts: at frame edges and sample counts that do not tile a wave, for views whose packets mix direction octants,
for a tile share, for a frame split into sample passes, for a deep tree and for the Cornell room.  The walk counters are pinned
too: one walk per 64 R paths, and a wide walk enters no more nodes than the R walks it replaces enter together."""
import numpy as np
import pytest

import oracle as O
import raytracing_engine_amd as R
from raytracing_engine_amd import scenes

pytestmark = pytest.mark.gpu

WIDE = {6: 2, 7: 4}  # tune_no_packet -> rays per lane
SKY = (0.3, 0.3, 0.4)
_ORACLE = {}


def oracle_frame(key, mesh, w, h, **kw):
    """The oracle's (frame, ray counts) for a view, computed once per session and left unchanged."""
    if key not in _ORACLE:
        rgb, ct = O.TriScene(*mesh).render(w, h, threads=16, **kw)
        rgb.setflags(write=False)
        _ORACLE[key] = (rgb, ct)
    return _ORACLE[key]


def n_paths(w, h, spp):
    """Paths of one sample batch: whole 64x64 tiles, spp paths per pixel slot."""
    return -(-w // 64) * -(-h // 64) * 4096 * spp


def check_wide(r, mode, key, mesh, w, h, rot=(0, 0, 0, 1), pos=(0, 0, 0), set_mesh=True, **kw):
    """Mode `mode` renders the oracle's frame with the oracle's ray counts, and mode 4's frame and counts; its walk counters
    are what one walk per 64 R paths gives.  Returns the frame."""
    if set_mesh:
        r.set_mesh(*mesh)
    r.resize(w, h)
    ref, ct = oracle_frame(key, mesh, w, h, rot=rot, pos=pos, **kw)
    narrow = r.render_pt(rot, pos, tune_no_packet=4, **kw)
    st4 = r.pt_stats()
    got = r.render_pt(rot, pos, tune_no_packet=mode, **kw)
    st = r.pt_stats()
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} values differ from the oracle's frame, max {np.abs(got - ref).max()}"
    assert np.array_equal(got, narrow)
    assert st["stack_overflow"] == 0
    for c in ("camera_rays", "bounce_rays", "shadow_rays"):
        assert st[c] == st4[c] == ct[c], c
    r.render_pt(rot, pos, tune_no_packet=4, count_traversal=True, **kw)
    c4 = r.pt_stats()
    counted = r.render_pt(rot, pos, tune_no_packet=mode, count_traversal=True, **kw)
    cw = r.pt_stats()
    assert np.array_equal(counted, ref)
    paths = n_paths(w, h, kw["spp"])
    print(f"mode {mode} {w}x{h} spp {kw['spp']}: packets {cw['packets']} (mode 4: {c4['packets']}), nodes {cw['packet_nodes_fetched']} "
          f"(mode 4: {c4['packet_nodes_fetched']}), triangles {cw['packet_tris_fetched']} (mode 4: {c4['packet_tris_fetched']})")
    assert c4["packets"] == paths // 64
    assert cw["packets"] == -(-paths // (64 * WIDE[mode]))
    assert cw["packet_nodes_fetched"] >= cw["packets"]
    assert cw["packet_nodes_fetched"] <= c4["packet_nodes_fetched"]
    assert cw["stack_overflow"] == 0 and c4["stack_overflow"] == 0
    return got


@pytest.mark.parametrize("mode", [6, 7])
@pytest.mark.parametrize("spp", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", [(70, 50), (96, 54)])
def test_frame_edges_and_odd_sample_counts(renderer, w, h, spp, mode):
    """Frames that are no multiple of a wave's pixel block, sample counts that do not tile a wave (3, 5) or leave a pixel's samples
    in different waves: the wide kernel may assume neither 4 spp nor a power of two."""
    mesh = scenes.soup_scene(2000, seed=3, edge=1.5)
    check_wide(renderer, mode, ("soup2k", w, h, spp), mesh, w, h, spp=spp, bounces=1, seed=5, sky=SKY)


def test_soup_fixture_configuration(renderer, golden_dir):
    """The committed soup frame (96x54, 2 spp) is what the 2-spp case above compares with."""
    import os

    g = np.load(os.path.join(golden_dir, "path_b_soup2k_96x54.npz"))
    mesh = scenes.soup_scene(2000, seed=3, edge=1.5)
    renderer.set_mesh(*mesh)
    renderer.resize(96, 54)
    for mode in WIDE:
        rgb = renderer.render_pt(spp=2, bounces=1, seed=5, sky=SKY, tune_no_packet=mode)
        assert np.array_equal(rgb, g["rgb"]), mode
        st = renderer.pt_stats()
        assert [st["camera_rays"], st["bounce_rays"], st["shadow_rays"]] == list(g["counters"]), mode


@pytest.mark.parametrize("mode", [6, 7])
@pytest.mark.parametrize("name,yaw", [("+Y", 0.0), ("-X", -np.pi / 2)])
def test_octant_straddling_views(renderer, name, yaw, mode):
    """Camera inside the soup looking straight along an axis: the blocks at the image centre hold rays of four direction octants,
    which a wave walks in as many passes."""
    mesh = scenes.soup_scene(20000, seed=17, edge=0.7)
    rot = R.camera_quat(yaw, 0.0)
    check_wide(renderer, mode, ("straddle", name), mesh, 80, 48, rot=rot, pos=(0, 15, 0), spp=4, bounces=1, seed=9, sky=SKY)


@pytest.mark.parametrize("mode", [6, 7])
def test_tile_share(renderer, mode):
    """Rank 1 of 3 on a 200x140 frame (4 x 3 tiles) owns tiles 1, 4, 7 and 10, two of which reach over the frame's edge: the
    tile-major output holds the oracle's pixels of exactly these tiles."""
    import torch

    w, h = 200, 140
    mesh = scenes.soup_scene(2000, seed=3, edge=1.5)
    view = dict(spp=2, bounces=1, seed=11, sky=SKY)
    ref, _ = oracle_frame(("share", w, h), mesh, w, h, **view)
    renderer.set_mesh(*mesh)
    renderer.resize(w, h)
    prm = renderer.pt_params(tune_no_packet=mode, **view)
    try:
        renderer.set_partition(1, 3)
        tx, ty, owned = renderer.tile_info()
        assert (tx, ty, owned) == (4, 3, 4)
        tiles = torch.zeros((owned, 64, 64, 3), dtype=torch.float32, device="cuda")
        renderer.render_pt_device((0, 0, 0, 1), (0, 0, 0), prm, tiles.data_ptr(), tile_major=True)
        renderer.synchronize()
        assert renderer.pt_stats()["stack_overflow"] == 0
        got = tiles.cpu().numpy()
        for k in range(owned):
            tile = 1 + 3 * k
            y0, x0 = (tile // tx) * 64, (tile % tx) * 64
            want = ref[y0:y0 + 64, x0:x0 + 64]
            assert np.array_equal(got[k, :want.shape[0], :want.shape[1]], want), tile
    finally:
        renderer.set_partition(0, 1)
        renderer.resize(64, 64)


@pytest.mark.parametrize("mode", [6, 7])
def test_sample_passes(renderer, mode):
    """8 spp with room for three samples per pixel slot in flight: passes of 3, 3 and 2 samples (192-path pixel blocks of 3
    samples tile no wide wave) add up to the single-pass frame, which is the oracle's."""
    w, h = 70, 50
    mesh = scenes.soup_scene(2000, seed=3, edge=1.5)
    view = dict(spp=8, bounces=1, seed=5, sky=SKY)
    ref, ct = oracle_frame(("passes", w, h), mesh, w, h, **view)
    renderer.set_mesh(*mesh)
    renderer.resize(w, h)
    single = renderer.render_pt(tune_no_packet=mode, **view)
    assert np.array_equal(single, ref)
    split = renderer.render_pt(tune_no_packet=mode, max_paths=3 * n_paths(w, h, 1), count_traversal=True, **view)
    st = renderer.pt_stats()
    assert np.array_equal(split, single)
    assert st["camera_rays"] == ct["camera_rays"] and st["stack_overflow"] == 0
    r = WIDE[mode]
    assert st["packets"] == 2 * -(-n_paths(w, h, 3) // (64 * r)) + -(-n_paths(w, h, 2) // (64 * r))


@pytest.mark.parametrize("mode", [6, 7])
def test_deep_tree(renderer, mode):
    """The deep scene's tree (more than 20 levels, the deepest the builders make from it) through the wide walk's VGPR stack, and
    the rule that sends a tree to the per-lane kernel: when a tree needs more entries than the packet kernels' stack holds, no packet
    is walked; otherwise the wide kernel walks it.  Either way the frame is the oracle's."""
    mesh = scenes.deep_scene()
    view = dict(spp=2, bounces=2, seed=17)
    ref, ct = oracle_frame("deep", mesh, 64, 64, **view)
    for opts in (dict(), dict(bvh_levels=2, blas_chunks=64)):
        renderer.set_mesh(*mesh, **opts)
        renderer.resize(64, 64)
        got = renderer.render_pt(tune_no_packet=mode, count_traversal=True, **view)
        st = renderer.pt_stats()
        assert np.array_equal(got, ref), opts
        assert st["bvh_depth"] >= 20 and st["stack_overflow"] == 0, (opts, st["bvh_depth"])
        assert [st[c] for c in ("camera_rays", "bounce_rays", "shadow_rays")] == [ct[c] for c in ("camera_rays", "bounce_rays", "shadow_rays")]
        assert st["packets"] == (0 if st["stack_need"] > 40 else -(-n_paths(64, 64, 2) // (64 * WIDE[mode]))), (opts, st["stack_need"])


@pytest.mark.parametrize("mode", [6, 7])
def test_cornell_room(renderer, mode):
    """Cornell room, 64x64, 4 spp, 3 bounces (the committed Cornell frame has 2 bounces: the oracle renders this one)."""
    mesh = scenes.cornell_tri_scene()
    check_wide(renderer, mode, "cornell", mesh, 64, 64, pos=(0, 1, 0), spp=4, bounces=3, seed=7)
