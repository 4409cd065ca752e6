"""Path B's frames on the GPU, path by path, against a float64 reading of the specification (tests/path_b_exact.py, DESIGN.md
sections 3 and 6.4).  No oracle is imported: every frame of Renderer.render_pt is compared with path_b_exact.expected() alone.

Every pixel that is not ambiguous lies within EPS_RGB of the reference, no case leaves out more than 1 % of its pixels, and the
camera / bounce / shadow ray counts are the predicted ones - for the default schedule on every case of path_b_exact.CASES, for
the per-lane and the wide-packet camera kernels, for a device-built, a two-level and a refitted mesh, for a frame whose samples
are split into passes and for the union of a 2-rank partition.  The constants were measured on the CPU (python
tests/path_b_exact.py); nothing here is measured on a GPU frame.  Power, on the GPU's own frames: the frame of another seed and
the frame of another ray_eps are rejected.
"""
import numpy as np
import pytest

import path_b_exact as X

pytestmark = pytest.mark.gpu
f32 = np.float32


def load(r, s):
    """Mesh s = (verts, albedo, emission, kind, ior) into renderer r, host-built."""
    r.set_mesh(*s[:3])
    if s[3] is not None:
        r.set_surfaces(s[3], s[4])


def frame(r, fr, **tune):
    """(rgb, counts) of the current mesh for Frame fr."""
    r.resize(fr.w, fr.h)
    rgb = r.render_pt(**fr.render_kw(), **tune)
    st = r.pt_stats()
    assert st["stack_overflow"] == 0
    return rgb, {k: st[k] for k in X.COUNTS}


def check(r, name, exp=None, **tune):
    fr = X.case(name)[2]
    exp = X.case_expected(name) if exp is None else exp
    rgb, counts = frame(r, fr, **tune)
    print(f"{name} {tune}: largest excess {X.excess(rgb, exp).max():.3g} (EPS_RGB {X.EPS_RGB:.3g}), left out {X.left_out(exp):.4%}, "
          + ", ".join(f"{k} {counts[k]} / {exp[k]}" for k in X.COUNTS))
    X.check_frame(rgb, exp, counts=counts, bounces=fr.bounces)
    return rgb


@pytest.mark.parametrize("name", list(X.CASES))
def test_frames_lie_within_eps_of_the_specification(renderer, name):
    load(renderer, X.case(name)[0])
    check(renderer, name)


@pytest.mark.parametrize("no_packet", [1, 6, 7])
@pytest.mark.parametrize("name", ["cornell_b1", "cornell_b3", "soup"])
def test_every_camera_ray_kernel(renderer, name, no_packet):
    """tune_no_packet = 1: the per-lane traversal kernel; 6 and 7: the wide packets of two and four rays per lane."""
    load(renderer, X.case(name)[0])
    check(renderer, name, tune_no_packet=no_packet)


def on_device(r, *arrays):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(a, f32)).to(f"cuda:{r.device}") for a in arrays)


def test_a_device_built_mesh(renderer):
    s = X.case("soup_dense")[0]
    renderer.set_mesh_device(*on_device(renderer, s[0].reshape(-1, 9), s[1], s[2]))
    check(renderer, "soup_dense")


def test_a_two_level_mesh(renderer):
    s = X.case("many_lights")[0]
    renderer.set_mesh(*s[:3], bvh_levels=2, blas_chunks=16)
    check(renderer, "many_lights")


def test_a_refitted_mesh_whose_vertices_moved(renderer):
    """The short box of the room is shifted and lifted off the floor, the tall one lifted; the reference is given the moved vertices."""
    s, _, fr = X.case("cornell_b3")
    v = np.asarray(s[0], f32).reshape(-1, 3, 3).copy()
    v[14:26, :, 2] += f32(1.25)
    v[26:38, :, 0] -= f32(1.5)
    v[26:38, :, 2] += f32(0.75)
    moved = v.reshape(-1, 9)
    exp = X.expected(X.Mesh(moved, s[1], s[2]), fr)
    assert np.abs(exp["rgb"] - X.case_expected("cornell_b3")["rgb"]).max() > 0.1, "the move must show"
    renderer.set_mesh_device(*on_device(renderer, s[0].reshape(-1, 9), s[1], s[2]))
    check(renderer, "cornell_b3")
    renderer.refit_mesh_device(*on_device(renderer, moved))
    check(renderer, "cornell_b3", exp=exp)


def test_samples_split_into_passes(renderer):
    """max_paths = 8192 on the 64 x 64 frame at 5 spp: two samples per pass, three passes; the running sum keeps the sample order."""
    load(renderer, X.case("cornell_b2_spp5")[0])
    check(renderer, "cornell_b2_spp5", max_paths=8192)


def test_the_union_of_a_two_rank_partition(renderer):
    import torch

    s, _, fr = X.case("cornell_turned")
    exp = X.case_expected("cornell_turned")
    load(renderer, s)
    renderer.resize(fr.w, fr.h)
    kw = fr.render_kw()
    rot, pos = kw.pop("rot"), kw.pop("pos")
    prm = renderer.pt_params(**kw)
    n_ranks = 2
    tx, ty, _ = renderer.tile_info()
    assert tx * ty >= n_ranks
    per = -(-(tx * ty) // n_ranks)
    gathered = torch.zeros((n_ranks, per, 64, 64, 3), dtype=torch.float32, device=f"cuda:{renderer.device}")
    try:
        for rank in range(n_ranks):
            renderer.set_partition(rank, n_ranks)
            renderer.render_pt_device(rot, pos, prm, gathered[rank].data_ptr(), tile_major=True)
            renderer.synchronize()
        out = torch.empty((fr.h, fr.w, 3), dtype=torch.float32, device=f"cuda:{renderer.device}")
        renderer.detile_device(gathered.data_ptr(), n_ranks, per, out.data_ptr())
        renderer.synchronize()
    finally:
        renderer.set_partition(0, 1)
    X.check_frame(out.cpu().numpy(), exp)


def test_the_frame_of_another_seed_is_rejected(renderer):
    s, _, fr = X.case("cornell_b1")
    exp = X.case_expected("cornell_b1")
    load(renderer, s)
    other = X.Frame(fr.w, fr.h, **dict(X.CASES["cornell_b1"][3], seed=fr.seed + 1))
    rgb, _ = frame(renderer, other)
    share = X.rejected_share(rgb, exp)
    print(f"seed {other.seed} against the reference of seed {fr.seed}: {share:.1%} of the pixels outside {X.REJECT:.0f} EPS_RGB")
    assert share > X.CAP_AMBIGUOUS  # more pixels than a case may leave out
    with pytest.raises(AssertionError):
        X.check_frame(rgb, exp)


def test_the_frame_of_another_ray_eps_is_rejected(renderer):
    """An offset of 2e-3 instead of 1e-3 moves every lit pixel by a few parts in 10^4: several EPS_RGB, rarely 100."""
    s, _, fr = X.case("cornell_b1")
    exp = X.case_expected("cornell_b1")
    load(renderer, s)
    other = X.Frame(fr.w, fr.h, **dict(X.CASES["cornell_b1"][3], ray_eps=2e-3))
    rgb, _ = frame(renderer, other)
    share = X.rejected_share(rgb, exp, 1.0)
    print(f"ray_eps 2e-3 against the reference of 1e-3: {share:.1%} of the pixels outside EPS_RGB")
    assert share > X.CAP_AMBIGUOUS
    with pytest.raises(AssertionError):
        X.check_frame(rgb, exp)
