"""Oracle A's frames against closed-form sphere geometry (tests/path_a_exact.py), and the power of that check.  CPU only.

oracle_a.c and path_a.hip mirror each other line by line, so the bit-exact GPU tests cannot see a misreading the two share.  Here
every level of the oracle's depth pyramid has to lie in the float64 band of its texel and every hit pixel in its RGB interval, for
bands that use none of the oracle's code; tests/test_gpu_path_a_exact.py holds the kernels to the same bands without any oracle.
The mutated frames below are what a shared misreading would produce: each one has to be rejected.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import path_a_exact as X


@pytest.fixture(scope="module")
def frames():
    """Oracle frames, rendered once and never modified (mutants work on copies)."""
    cache = {}

    def get(name, w, h):
        if (name, w, h) not in cache:
            cache[name, w, h] = X.oracle_frame(name, w, h)
        return cache[name, w, h]

    return get


def copy_of(fr, levels=None, rgb=None):
    """fr with other levels or another RGB (a new Frame: the cached one stays as rendered)."""
    scene, view, conf = X.CASES[fr.name][:3]
    out = X.Frame(scene, fr.w, fr.h, levels=fr.levels if levels is None else levels, rgb=fr.rgb if rgb is None else rgb, **view, **conf)
    out.name = fr.name
    return out


@pytest.mark.parametrize("name,w,h", X.FRAMES)
def test_oracle_frames_lie_inside_every_band(frames, name, w, h):
    fr = frames(name, w, h)
    depth, rgb = X.check_frame(fr)
    for i, lv in enumerate(depth):
        print(f"level {i}: {lv}")
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    print(rgb)
    assert rgb["bad"] == 0 and rgb["miss_nonblack"] == 0, rgb
    X.check_caps(name, rgb)
    if name == "all_miss":
        assert rgb["hits"] == 0 and all(lv["hits"] == 0 for lv in depth)
    else:
        assert rgb["hits"] > 0.05 * w * h


def test_the_constants_are_the_measured_ones_and_under_the_bar():
    assert 0 < X.EPS_RGB <= 1e-4 and 0 < X.EPS_DEPTH <= 1e-5


# ---- power: frames a shared misreading would produce ---------------------------------------------------------------------------
POWER = [("startup", 96, 64), ("room_turned", 96, 64), ("startup_turned", 200, 120)]


def finest(fr):
    i = fr.count - 1
    return i, X.check_depth(fr, i)


@pytest.mark.parametrize("name,w,h", POWER)
def test_a_finest_level_rolled_by_one_texel_is_rejected(frames, name, w, h):
    fr = frames(name, w, h)
    levels = list(fr.levels)
    levels[-1] = np.roll(levels[-1], 1, axis=1)
    i, res = finest(copy_of(fr, levels=levels))
    print(res)
    assert finest(fr)[1]["bad"] == 0 and res["bad"] > 0


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name,w,h", POWER)
def test_hit_depths_moved_by_one_cone_radius_are_rejected(frames, name, w, h, sign):
    fr = frames(name, w, h)
    for i in range(fr.count):
        levels = list(fr.levels)
        tau = X.SQRT2_8 * (1 << (fr.count - 1 - i)) / fr.w
        v = levels[i]
        if i == 0:
            len0 = np.ones_like(v)
        else:
            gy, gx = np.mgrid[0:v.shape[0], 0:v.shape[1]]
            len0 = levels[i - 1][gy >> 1, gx >> 1]
        radius = (np.maximum(v - len0, 0.0) + 1.0) * tau  # the cone radius where the march stopped, to first order
        levels[i] = np.where(v < fr.render_dist, np.maximum(v + sign * radius, 0.0), v)
        res = X.check_depth(copy_of(fr, levels=levels), i)
        print(f"level {i}: {res}")
        assert res["bad"] > 0, (i, res)


def cone_level_from(fr, i, parent_of):
    """Level i marched by the oracle's own traceCone from the parent texel parent_of(gx, gy) of the frame's level i - 1."""
    scene, view, conf = X.CASES[fr.name][:3]
    sc = O.scene_from_bytes(scene)
    h, w = fr.levels[i].shape
    gy, gx = (a.ravel() for a in np.mgrid[0:h, 0:w])
    pw = float(1 << (fr.count - 1 - i))
    isx, isy = pw / fr.w, pw / fr.h
    u = X.rays(fr, (2.0 * gx + 1.0) * isx - 1.0, (2.0 * gy + 1.0) * isy - 1.0).astype(np.float32)
    ph, pw_ = fr.levels[i - 1].shape
    qx, qy = parent_of(gx, gy)
    len0 = fr.levels[i - 1][np.minimum(qy, ph - 1), np.minimum(qx, pw_ - 1)].astype(np.float32)
    origin = (fr.pos.astype(np.float32) + len0[:, None] * u).astype(np.float32)
    tau = float(np.float32(X.SQRT2_8 * isx))
    out = np.array([O.trace_cone(sc, origin[k], u[k], tau) for k in range(len(gx))], np.float32)
    return np.maximum(len0 + out, np.float32(0)).reshape(h, w)


@pytest.mark.parametrize("name,w,h", POWER[:2])
def test_a_child_level_marched_from_the_wrong_parent_texel_is_rejected(frames, name, w, h):
    fr = frames(name, w, h)
    i = fr.count - 1
    levels = list(fr.levels)
    levels[i] = cone_level_from(fr, i, lambda gx, gy: (gx >> 1, gy >> 1))
    right = X.check_depth(copy_of(fr, levels=levels), i)
    levels[i] = cone_level_from(fr, i, lambda gx, gy: (gx, gy))
    wrong = X.check_depth(copy_of(fr, levels=levels), i)
    print(right, wrong)
    assert right["bad"] == 0 and wrong["bad"] > 0


@pytest.mark.parametrize("name,w,h", POWER)
def test_rgb_rolled_by_one_pixel_is_rejected(frames, name, w, h):
    fr = frames(name, w, h)
    res = X.check_rgb(copy_of(fr, rgb=np.roll(fr.rgb, 1, axis=1)))
    print(res)
    assert X.check_rgb(fr)["bad"] == 0 and res["bad"] > 0


def rendered_with(fr, edit_scene=None, **conf):
    """The RGB oracle A gives for fr's view with an edited scene / config: what a misreading of the shading would draw."""
    scene, view, base = X.CASES[fr.name][:3]
    sc = O.scene_from_bytes(scene)
    if edit_scene:
        edit_scene(sc)
    cfg = O.default_config()
    for k, v in {**base, **conf}.items():
        setattr(cfg, k, v)
    return O.render_a(sc, fr.w, fr.h, cfg=cfg, want_levels=False, **view)["rgb"]


def swap_materials(sc):
    a, b = bytes(sc.mats[0]), bytes(sc.mats[1])
    C.memmove(C.byref(sc.mats[0]), b, len(b))
    C.memmove(C.byref(sc.mats[1]), a, len(a))


def drop_light(sc):
    sc.lightCount -= 1


@pytest.mark.parametrize("edit", [swap_materials, drop_light])
@pytest.mark.parametrize("name,w,h", POWER)
def test_swapped_materials_and_a_dropped_light_are_rejected(frames, name, w, h, edit):
    fr = frames(name, w, h)
    res = X.check_rgb(copy_of(fr, rgb=rendered_with(fr, edit)))
    print(res)
    assert res["bad"] > 0


def test_exchanged_fall_offs_are_rejected(frames):
    fr = frames("config", 96, 64)
    conf = X.CASES["config"][2]
    assert conf["light_fall_off"] != conf["cam_fall_off"]
    same = X.check_rgb(copy_of(fr, rgb=rendered_with(fr)))
    res = X.check_rgb(copy_of(fr, rgb=rendered_with(fr, light_fall_off=conf["cam_fall_off"], cam_fall_off=conf["light_fall_off"])))
    print(res)
    assert same["bad"] == 0 and res["bad"] > 0


def test_the_shadow_term_is_capped_by_the_distance_to_the_light():
    """The detail a reader of the formula gets wrong: every sampled value is min(end, f), so a light nearer than 1 to the lit point
    dims itself.  One sphere of radius 2 at distance 10 straight ahead, one light 1 in front of it (the march stops a cone radius short of the surface, here 0.4 from that light): at the centre pixel normal,
    light and eye line up, diffuse = specular base = 1, both fall-offs are 1, and rgb = ambient + 2 soft with soft = light_dist =
    depth - 7 (the open space around the segment is wider than that); without the cap it would be ambient + 2."""
    scene = X._pack_scene([(0, 10, 0, 2)], [(1, 1, 1, 1, 0.05)], [((0, 7, 0), (1, 1, 1))])
    ref = O.render_a(O.scene_from_bytes(scene), 65, 65)  # odd: pixel 32 looks straight down the axis
    fr = X.Frame(scene, 65, 65, levels=ref["levels"], rgb=ref["rgb"])
    sb = X.shade_bands(fr)
    centre = (sb["py"] == 32) & (sb["px"] == 32)
    assert X.check_rgb(fr)["bad"] == 0 and sb["pinned"][centre].all()
    depth, got = fr.levels[-1][32, 32], fr.rgb[32, 32]
    assert 7.0 < depth < 7.9
    assert np.abs(got - (0.05 + 2.0 * (depth - 7.0))).max() < 5e-3 and np.abs(sb["hi"][centre] - got).max() <= X.EPS_RGB
