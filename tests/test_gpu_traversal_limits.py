"""GPU tests of path B's traversal buffers at their limits: the wave-pooled triangle ring (kPoolRing groups per wave), the
traversal stack (lds_cap entries in LDS, the rest spilled to global memory) and the refit's single-workgroup top levels
(kRefitTopMax).  The everyday scenes never take these near their bounds, so two adversarial scenes do (scenes.py):
- the sliver stack: thousands of parallel triangles whose boxes a ray crosses without hitting them, so every leaf-parent
  node it visits hands it up to 8 leaf hits and its tmax never culls;
- the deep scene: nested clusters that drive the host builder to its binary depth cap and collapse into a tree of more
  than 16 levels.
Every frame must equal the oracle's bit for bit, with equal ray counts; every test asserts the precondition that makes it
bite (triangles tested per ray, tree depth, level count)."""
import numpy as np
import pytest

import oracle as O
from raytracing_engine_amd import scenes
from test_gpu_device_bvh import check_bvh, dev
from test_gpu_path_b import check_pt
from test_gpu_refit import check_frame, tdev

pytestmark = pytest.mark.gpu

# the host builder reaches 25 levels on deep_scene() (tests/test_bvh_build_host.py pins the same bound on the CPU), the device
# builder (LBVH: Morton keys cannot tell the smallest clusters apart) 12
DEEP_MIN_DEPTH, DEEP_DEVICE_MIN_DEPTH = 20, 10
REFIT_TOP_MAX, REFIT_TOP_NODES = 16, 1024  # bvh_build_gpu.hip: kRefitTopMax, kRefitTopNodes


def check_frame_against(r, k, w, h, **knobs):
    """render_pt with `knobs` on the current mesh equals the cached oracle frame k["ref"] bit for bit, with its ray counts."""
    got = r.render_pt(k["rot"], k["pos"], **k["kw"], **knobs)
    st = r.pt_stats()
    assert np.array_equal(got, k["ref"]), f"{np.count_nonzero(got != k['ref'])} values differ from the oracle's frame, max {np.abs(got - k['ref']).max()}"
    assert st["stack_overflow"] == 0
    for c in ("camera_rays", "bounce_rays", "shadow_rays"):
        assert st[c] == k["ct"][c], c
    return st


def levels_of(nodes):
    """Node counts of the breadth-first levels of a tree read back by Renderer.read_bvh() (rt_abi_mesh.hip: level_starts)."""
    n_in = np.array([bin(int(w) >> 24).count("1") for w in nodes[:, 3]])
    sizes, first, count = [], 0, 1
    while count:
        sizes.append(count)
        first, count = first + count, int(n_in[first:first + count].sum())
    assert first == len(nodes)
    return sizes


# ---- 1. the sliver stack: the wave-pooled ring and the other triangle schedules --------------------------------------------

SLIVER_W, SLIVER_H, SLIVER_LAYERS = 64, 64, 2048
_SLIVER = {}


def sliver():
    """The sliver stack and the oracle's frame + ray counts for it (computed once per session)."""
    if not _SLIVER:
        v, a, e = scenes.sliver_stack_scene(SLIVER_LAYERS)
        kw = dict(spp=2, bounces=2, seed=13)
        ref, ct = O.TriScene(v, a, e).render(SLIVER_W, SLIVER_H, **kw)
        _SLIVER.update(mesh=(v, a, e), ref=ref, ct=ct, kw=kw, rot=(0, 0, 0, 1), pos=(0, 0, 0))
    return _SLIVER


def test_sliver_stack_rays_test_every_layer(renderer):
    """Precondition of the sliver tests: camera rays through the open half of the stack that reach the backdrop test (nearly)
    every layer, and rays through the covered half stop at the first layer."""
    k = sliver()
    v, a, e = k["mesh"]
    renderer.set_mesh(v, a, e)
    sc = O.TriScene(v, a, e)
    g = np.linspace(-0.95, 0.95, 24, dtype=np.float32)
    nx, nz = (x.ravel() for x in np.meshgrid(g, g))
    d = np.stack([nx, np.ones_like(nx), nz], 1).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.zeros_like(d)
    t, tri, counts = renderer.trace_rays(o, d, counted=True)
    back = len(v) - 4  # the backdrop's two triangles
    open_half = nx + nz > 0.05
    through = open_half & (tri >= back) & (tri < back + 2)
    assert through.sum() >= 120, through.sum()
    assert (counts[through, 1] >= 0.9 * SLIVER_LAYERS).all(), counts[through, 1].min()
    covered = nx + nz < -0.05
    assert (tri[covered] == 0).all()  # the layer nearest to the camera
    targets = open_half & (tri >= SLIVER_LAYERS) & (tri < back)
    assert targets.sum() >= 20, targets.sum()
    for i in np.flatnonzero(open_half)[::7]:
        assert tri[i] == sc.closest_hit(o[i], d[i])[0], i


@pytest.mark.parametrize("knobs", [dict(), dict(tune_tri_mode=1), dict(tune_tri_mode=2), dict(tune_tri_mode=3), dict(tune_tri_mode=4),
                                   dict(tune_tri_mode=2 | (64 << 8) | (255 << 16)), dict(tune_tri_mode=2 | (1 << 8) | (1 << 16)),
                                   dict(tune_tri_mode=2 | (7 << 8) | (3 << 16), tune_refill_min=1),
                                   dict(tune_no_packet=1), dict(tune_tri_mode=2 | (64 << 8) | (255 << 16), tune_no_packet=1),
                                   dict(tune_tri_mode=2 | (64 << 8) | (255 << 16), tune_no_overlap=0),
                                   dict(tune_tri_mode=2 | (64 << 8) | (255 << 16), tune_no_overlap=1),
                                   dict(tune_tri_mode=2 | (64 << 8) | (255 << 16), tune_no_overlap=2),
                                   dict(tune_tri_mode=3, tune_no_packet=1), dict(tune_tri_mode=4, tune_no_packet=1)])
def test_sliver_stack_schedules_match_the_oracle(renderer, knobs):
    """Every triangle schedule (inline, wave-pooled with the flush rules from eager to the worst case - a flush only at 64
    groups, groups waiting 255 rounds -, postponed, pipelined refill), the per-lane kernel for camera rays and each shadow
    launch overlap, on a scene where most node visits yield a group of several leaf hits: the oracle's frame."""
    k = sliver()
    renderer.set_mesh(*k["mesh"])
    renderer.resize(SLIVER_W, SLIVER_H)
    check_frame_against(renderer, k, SLIVER_W, SLIVER_H, **knobs)


# ---- 2. the deep tree: the spilled traversal stack ---------------------------------------------------------------------------

DEEP_W, DEEP_H = 64, 64
_DEEP = {}


def deep():
    """The deep scene and the oracle's frame + ray counts for it, camera at the clusters' common centre (computed once)."""
    if not _DEEP:
        v, a, e = scenes.deep_scene()
        kw = dict(spp=2, bounces=2, seed=17)
        ref, ct = O.TriScene(v, a, e).render(DEEP_W, DEEP_H, **kw)
        _DEEP.update(mesh=(v, a, e), ref=ref, ct=ct, kw=kw, rot=(0, 0, 0, 1), pos=(0, 0, 0))
    return _DEEP


def test_deep_tree_depth(renderer):
    """Precondition of the deep tests: the host tree is at least DEEP_MIN_DEPTH levels deep and the camera rays walk it down."""
    k = deep()
    renderer.set_mesh(*k["mesh"])
    st = renderer.pt_stats()
    assert st["bvh_depth"] >= DEEP_MIN_DEPTH and st["stack_need"] == st["bvh_depth"] + 1, (st["bvh_depth"], st["stack_need"])
    assert check_bvh(renderer, k["mesh"][0]) == st["bvh_depth"]
    d = np.array([[0.5, 1.0, 0.3]], np.float32) + np.linspace(-0.02, 0.02, 64, dtype=np.float32)[:, None]  # towards the clusters
    _, _, counts = renderer.trace_rays(np.zeros_like(d), d, counted=True)
    assert counts[:, 0].max() >= st["bvh_depth"], counts[:, 0].max()


@pytest.mark.parametrize("knobs", [dict(), dict(tune_lds_stack=1), dict(tune_lds_stack=78),
                                   dict(tune_tri_mode=1, tune_lds_stack=1), dict(tune_tri_mode=2, tune_lds_stack=1),
                                   dict(tune_tri_mode=3, tune_lds_stack=1), dict(tune_tri_mode=4, tune_lds_stack=1),
                                   dict(tune_no_overlap=0, tune_lds_stack=1), dict(tune_no_overlap=1, tune_lds_stack=1),
                                   dict(tune_no_overlap=2, tune_lds_stack=1), dict(tune_no_overlap=1), dict(tune_no_overlap=2),
                                   dict(tune_no_packet=1, tune_lds_stack=1)])
def test_deep_tree_matches_the_oracle(renderer, knobs):
    """The host-built deep tree with the stack in LDS, almost all of it spilled (tune_lds_stack=1: two dozen spilled entries
    per lane, the shadow kernel in the second half of the spill buffer while it overlaps the next closest-hit launch) and
    with the LDS share clamped to the tree's need (78): the oracle's frame under every schedule and launch overlap."""
    k = deep()
    renderer.set_mesh(*k["mesh"])
    renderer.resize(DEEP_W, DEEP_H)
    check_frame_against(renderer, k, DEEP_W, DEEP_H, **knobs)


def test_shallow_deep_shallow_mesh_swaps(renderer):
    """One renderer: a shallow mesh, the deep one (the spill buffer grows between frames), a shallow one again."""
    k = deep()
    check_pt(renderer, scenes.cornell_tri_scene(), 48, 48, pos=(0, 1, 0), spp=2, bounces=2, seed=3, tune_lds_stack=2)
    need0 = renderer.pt_stats()["stack_need"]
    check_pt(renderer, k["mesh"], DEEP_W, DEEP_H, **k["kw"], tune_lds_stack=2)
    assert renderer.pt_stats()["stack_need"] > need0 + 10
    check_pt(renderer, scenes.soup_scene(3000, seed=5, edge=1.0), 48, 48, spp=2, bounces=1, seed=2, sky=(0.1, 0.1, 0.1), tune_lds_stack=2)
    check_pt(renderer, k["mesh"], DEEP_W, DEEP_H, **k["kw"])


def test_device_built_deep_tree(renderer):
    """The same mesh built on the GPU (LBVH): a valid tree and the oracle's frame."""
    k = deep()
    renderer.set_mesh_device(*dev(k["mesh"], renderer.device))
    depth = check_bvh(renderer, k["mesh"][0])
    assert depth >= DEEP_DEVICE_MIN_DEPTH, depth
    renderer.resize(DEEP_W, DEEP_H)
    for knobs in (dict(), dict(tune_lds_stack=1), dict(tune_lds_stack=1, tune_tri_mode=2)):
        check_frame_against(renderer, k, DEEP_W, DEEP_H, **knobs)


# ---- 3. the refit of the deep tree: more levels than the single-workgroup top takes --------------------------------------------

def test_refit_of_the_deep_tree(renderer):
    """The host-built deep tree has more than kRefitTopMax levels of at most kRefitTopNodes nodes, so the refit's single
    workgroup takes the top 16 and the rest go to per-level launches.  An identity refit gives the tree back byte for
    byte; after the vertices move, frames equal the oracle's on the moved mesh."""
    k = deep()
    v, a, e = k["mesh"]
    renderer.set_mesh(v, a, e)
    nodes0, leaf0 = renderer.read_bvh()
    sizes = levels_of(nodes0)
    assert len(sizes) > REFIT_TOP_MAX and max(sizes[:REFIT_TOP_MAX + 1]) <= REFIT_TOP_NODES, sizes
    renderer.refit_mesh_device(tdev(v, renderer.device))
    nodes1, leaf1 = renderer.read_bvh()
    assert nodes0.tobytes() == nodes1.tobytes(), f"{np.count_nonzero((nodes0 != nodes1).any(1))} nodes differ"
    assert leaf0.tobytes() == leaf1.tobytes()
    moved = (v.reshape(-1, 3) * np.array([1.1, 0.95, 1.05], np.float32)).reshape(-1, 9).astype(np.float32)
    renderer.refit_mesh_device(tdev(moved, renderer.device))
    check_bvh(renderer, moved)
    nodes2, _ = renderer.read_bvh()
    assert not np.array_equal(nodes2[:, :4], nodes0[:, :4])
    check_frame(renderer, (moved, a, e), DEEP_W, DEEP_H, **k["kw"], tune_lds_stack=1)
