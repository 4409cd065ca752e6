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

    def get(name, w, h, march_algorithm=3):
        if (name, w, h, march_algorithm) not in cache:
            cache[name, w, h, march_algorithm] = X.oracle_frame(name, w, h, march_algorithm=march_algorithm)
        return cache[name, w, h, march_algorithm]

    return get


def copy_of(fr, levels=None, rgb=None, jitter=None, march_algorithm=None):
    """fr with other levels, another RGB, or read with another jitter / march algorithm (a new Frame: the cached one stays as rendered)."""
    scene, view, conf = X.CASES[fr.name][:3]
    out = X.Frame(scene, fr.w, fr.h, levels=fr.levels if levels is None else levels, rgb=fr.rgb if rgb is None else rgb,
                  jitter=fr.jitter if jitter is None else jitter, march_algorithm=fr.alg if march_algorithm is None else march_algorithm, **view, **conf)
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


def test_the_image_hook_is_exported_and_bound():
    import raytracing_engine_amd as R
    from raytracing_engine_amd import _lib

    lib = R.load()
    assert "rt_read_level_image" in _lib.PROTOTYPES
    sample = C.c_uint32(7)
    assert lib.rt_read_level_image(None, 0, 0, None, None, None, C.byref(sample)) == -1 and sample.value == 7  # no context: nothing written
    assert lib.rt_abi_version() == 4


def test_the_jitter_is_the_stratum_centre_in_fp32():
    """n = 1 is exactly the reference's sample; 2 x 2 at 96 x 64: +-0.5 / n pixels = +-(1 / 2) / view in normalised coordinates,
    x fastest; 3 x 3: the middle stratum is the pixel centre again."""
    assert not X.sample_jitter(0, 1, 96, 64).any()
    got = np.array([X.sample_jitter(s, 4, 96, 64) for s in range(4)])
    assert np.array_equal(got, np.array([(-0.5 / 96, -0.5 / 64), (0.5 / 96, -0.5 / 64), (-0.5 / 96, 0.5 / 64), (0.5 / 96, 0.5 / 64)], np.float32))
    nine = np.array([X.sample_jitter(s, 9, 200, 120) for s in range(9)], np.float64)
    assert np.allclose(nine[:, 0] * 200, np.tile([-2 / 3, 0, 2 / 3], 3), atol=1e-6) and np.allclose(nine[:, 1] * 120, np.repeat([-2 / 3, 0, 2 / 3], 3), atol=1e-6)
    assert nine.dtype == np.float64 and X.sample_jitter(4, 9, 200, 120).dtype == np.float32


# ---- multi-sample frames: every sample a full frame with its own jitter, averaged in sample order ------------------------------
@pytest.fixture(scope="module")
def samples():
    """Oracle frames of every sample and their average, rendered once and never modified."""
    cache = {}

    def get(name, w, h, spp):
        if (name, w, h, spp) not in cache:
            cache[name, w, h, spp] = X.oracle_samples(name, w, h, spp)
        return cache[name, w, h, spp]

    return get


@pytest.mark.parametrize("name,w,h,spp", X.SAMPLE_FRAMES)
def test_oracle_multi_sample_frames_lie_inside_every_band(samples, name, w, h, spp):
    frames, rgb = samples(name, w, h, spp)
    assert len({tuple(fr.jitter) for fr in frames}) == spp
    res = X.check_samples(frames, rgb)
    for s, levels in enumerate(res["depth"]):
        for i, lv in enumerate(levels):
            assert lv["bad"] == 0 and lv["far_bad"] == 0, (s, i, lv)
        own = X.check_rgb(frames[s])
        assert own["bad"] == 0 and own["miss_nonblack"] == 0, (s, own)
    print({k: v for k, v in res.items() if k != "depth"})
    assert res["bad"] == 0 and res["miss_nonblack"] == 0, res
    X.check_caps(name, res)
    assert res["hits"] > 0.05 * w * h and res["sample_hits"] >= res["hits"]


POWER_SAMPLES = [("startup", 96, 64, 4), ("room_turned", 96, 64, 9), ("ratio", 200, 120, 4)]
WRONG_JITTER = {
    "zero": lambda fr: fr.jitter * 0.0,
    "x flipped": lambda fr: fr.jitter * (-1.0, 1.0),
    "y flipped": lambda fr: fr.jitter * (1.0, -1.0),
    "doubled": lambda fr: fr.jitter * 2.0,
    "after the ratio": lambda fr: fr.jitter / fr.ratio,  # (n ratio + j) = (n + j / ratio) ratio
}


@pytest.mark.parametrize("wrong", WRONG_JITTER)
@pytest.mark.parametrize("name,w,h,spp", POWER_SAMPLES)
def test_bands_built_with_a_wrong_jitter_reject_the_frame(samples, name, w, h, spp, wrong):
    """The frames are the oracle's, the bands are read with a jitter a misreading would use: the depth bands of the samples'
    finest levels and the averaged RGB intervals each reject it on their own."""
    frames, rgb = samples(name, w, h, spp)
    mutants = [copy_of(fr, jitter=WRONG_JITTER[wrong](fr)) for fr in frames]
    assert any(not np.array_equal(m.jitter, fr.jitter) for m, fr in zip(mutants, frames))
    depth_bad = sum(X.check_depth(m, m.count - 1)["bad"] for m in mutants)
    res = X.check_samples_rgb(mutants, rgb)
    print(f"{wrong}: finest-level texels rejected {depth_bad}, pixels rejected {res['bad']} of {res['hits']}")
    assert depth_bad > 0 and res["bad"] > 0


@pytest.mark.parametrize("name,w,h,spp", POWER_SAMPLES)
def test_jitter_in_the_levels_but_not_in_the_shading_is_rejected(samples, name, w, h, spp):
    """A shade stage that forgot the jitter while the levels have it, on the band side: intervals shaded along the unjittered
    rays from the right levels reject the right frame (the levels themselves are not looked at here)."""
    frames, rgb = samples(name, w, h, spp)
    res = X.check_samples_rgb([copy_of(fr, jitter=(0, 0)) for fr in frames], rgb)
    print(res)
    assert res["bad"] > 0


@pytest.mark.parametrize("name,w,h,spp", POWER_SAMPLES)
def test_exchanged_level_images_are_rejected(samples, name, w, h, spp):
    """Sample 0's levels read as sample 1's and the other way round (an image mapped to the wrong sample index)."""
    frames, rgb = samples(name, w, h, spp)
    mutants = list(frames)
    mutants[0], mutants[1] = copy_of(frames[0], levels=frames[1].levels), copy_of(frames[1], levels=frames[0].levels)
    res = X.check_samples(mutants, rgb)
    bad = [sum(lv["bad"] for lv in levels) for levels in res["depth"]]
    print(bad, res["bad"])
    assert bad[0] > 0 and bad[1] > 0 and not any(bad[2:]) and res["bad"] > 0


@pytest.mark.parametrize("name,w,h,spp", POWER_SAMPLES)
def test_a_wrong_average_is_rejected(samples, name, w, h, spp):
    frames, rgb = samples(name, w, h, spp)
    assert X.check_samples_rgb(frames, rgb)["bad"] == 0
    total = rgb * np.float32(spp)
    by_one_less = X.check_samples_rgb(frames, total / np.float32(spp - 1))
    twice = [fr.rgb for fr in frames]
    twice[1] = twice[0]  # sample 0 counted twice, sample 1 dropped
    dropped = X.check_samples_rgb(frames, X.average(twice))
    print(by_one_less["bad"], dropped["bad"], by_one_less["hits"])
    assert by_one_less["bad"] > 0 and dropped["bad"] > 0


# ---- march algorithm 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", X.ALG1_FRAMES)
def test_oracle_algorithm_1_frames_lie_inside_every_band(frames, name, w, h):
    fr = frames(name, w, h, 1)
    assert fr.alg == 1
    depth, rgb = X.check_frame(fr)
    for i, lv in enumerate(depth):
        print(f"level {i}: {lv}")
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    print(rgb)
    assert rgb["bad"] == 0 and rgb["miss_nonblack"] == 0, rgb
    X.check_caps(name, rgb)
    if name == "all_miss":
        # tau = 0.94 at level 0: f (1 - tau) <= (s + 1) tau stops every march far from any surface, in its band; the finer levels miss
        assert rgb["hits"] == 0 and all(lv["hits"] == 0 for lv in depth[1:])
    else:
        assert rgb["hits"] > 0.05 * w * h


def test_the_coarse_level_of_algorithm_1_is_pinned_to_a_point(frames):
    """tau = 1.33 at level 0 of 17 x 9: the first sample stops the march and the band has no width."""
    fr = frames("startup", 17, 9, 1)
    bd = X.depth_bands(fr, 0)
    assert bd["tau"] >= 1.0 and np.array_equal(bd["lo"], bd["hi"]) and not bd["empty"].any()
    assert X.check_depth(fr, 0)["bad"] == 0


@pytest.mark.parametrize("name,w,h", POWER)
def test_algorithm_1_frames_are_rejected_by_the_bands_of_algorithm_3_and_back(frames, name, w, h):
    one, three = frames(name, w, h, 1), frames(name, w, h, 3)
    as_three = [X.check_depth(copy_of(one, march_algorithm=3), i)["bad"] for i in range(one.count)]
    as_one = [X.check_depth(copy_of(three, march_algorithm=1), i)["bad"] for i in range(one.count)]
    print(as_three, as_one)
    assert as_three[-1] > 0 and as_one[-1] > 0
    assert X.check_rgb(copy_of(one, march_algorithm=3))["bad"] == 0  # the shading bands do not depend on the algorithm


@pytest.mark.parametrize("name,w,h", POWER)
def test_an_algorithm_1_level_rolled_by_one_texel_is_rejected(frames, name, w, h):
    fr = frames(name, w, h, 1)
    levels = list(fr.levels)
    levels[-1] = np.roll(levels[-1], 1, axis=1)
    i, res = finest(copy_of(fr, levels=levels))
    print(res)
    assert finest(fr)[1]["bad"] == 0 and res["bad"] > 0


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name,w,h", POWER)
def test_algorithm_1_depths_moved_by_one_cone_radius_are_rejected(frames, name, w, h, sign):
    """Algorithm 1 takes the radius after the step: a value v stopped at total = (v - len0 + tau) / (1 - tau) with radius (total + 1) tau."""
    fr = frames(name, w, h, 1)
    for i in range(fr.count):
        levels = list(fr.levels)
        tau = X.SQRT2_8 * (1 << (fr.count - 1 - i)) / fr.w
        assert tau < 1.0
        v = levels[i]
        if i == 0:
            len0 = np.ones_like(v)
        else:
            gy, gx = np.mgrid[0:v.shape[0], 0:v.shape[1]]
            len0 = levels[i - 1][gy >> 1, gx >> 1]
        radius = (np.maximum((v - len0 + tau) / (1.0 - tau), 0.0) + 1.0) * tau
        levels[i] = np.where(v < fr.render_dist, np.maximum(v + sign * radius, 0.0), v)
        res = X.check_depth(copy_of(fr, levels=levels), i)
        print(f"level {i}: rejected {res['bad']} of {res['hits']} hit texels ({100.0 * res['bad'] / max(res['hits'], 1):.1f} %)")
        assert res["bad"] > 0, (i, res)


# ---- the mirror and transmission chains: every recorded march judged from the recorded link before it ----------------------------
@pytest.fixture(scope="module")
def chain_frames():
    """Oracle frames with their recorded marches and the right reading's result, rendered once and never modified."""
    cache = {}

    def get(name, w, h):
        if (name, w, h) not in cache:
            fr = X.oracle_chain_frame(name, w, h)
            cache[name, w, h] = (fr, X.check_chains(fr))
        return cache[name, w, h]

    return get


def chain_copy(fr, chains=None, rgb=None):
    scene, view, conf = X.CHAIN_CASES[fr.name][:3]
    out = X.Frame(scene, fr.w, fr.h, levels=fr.levels, rgb=fr.rgb if rgb is None else rgb, chains=fr.chains if chains is None else chains, **view, **conf)
    out.name = fr.name
    return out


def test_the_chain_cases_give_every_surface_its_own_scales():
    for name, (scene, _, conf, _) in X.CHAIN_CASES.items():
        sc = X.parse_scene(scene)
        for key in ("diffuse", "specular"):
            v = sc[key]
            assert len(set(v.tolist())) == len(v) and (v > 0).all() and (v < 1).all(), (name, key, v)
        assert conf["reflections"] + conf["transmissions"] > 0 and 0 < conf["reflectivity"] < 1 and 0 < conf["transparency"] < 1


@pytest.mark.parametrize("name,w,h", X.CHAIN_FRAMES)
def test_oracle_chains_lie_inside_every_band(chain_frames, name, w, h):
    """The pyramid and the primary colour are those of a frame without chains (check_frame's depth part; the RGB now holds the
    secondary light, so it is judged by the chain check alone); every recorded march against the link before it; the caps, the
    coverage conditions and the counter identities."""
    fr, res = chain_frames(name, w, h)
    for i in range(fr.count):
        lv = X.check_depth(fr, i)
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    print(res)
    X.assert_chains(fr, res, fr.counters)
    assert res["hits"] > 0.05 * w * h


def test_the_chain_rows_hold_what_render_a_returns_without_them():
    """want_chains changes nothing else: levels, RGB and counters are those of the plain call; mirror rows first."""
    scene, view, conf = X.CHAIN_CASES["room_turned_r2_t2_n1.5"][:3]
    cfg = O.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    plain = O.render_a(O.scene_from_bytes(scene), 96, 64, cfg=cfg, **view)
    rec = O.render_a(O.scene_from_bytes(scene), 96, 64, cfg=cfg, want_chains=True, **view)
    assert "chains" not in plain and rec["chains"].shape == (64, 96, 4, 7)
    assert np.array_equal(plain["rgb"], rec["rgb"]) and plain["counters"] == rec["counters"]
    assert all(np.array_equal(a, b) for a, b in zip(plain["levels"], rec["levels"]))
    ran = ~np.isnan(rec["chains"][..., 6])
    assert ran[..., 0].sum() == (rec["levels"][-1][:64, :96] < cfg.render_dist).sum()  # every hit pixel marches its first mirror ray
    assert not (ran[..., 1] & ~ran[..., 0]).any() and not (ran[..., 3] & ~ran[..., 2]).any()  # a later link only behind an earlier one
    assert (ran[..., 2] & ~ran[..., 1]).any()  # the transmission chain does not wait for the mirror chain


def test_the_chain_constants_are_the_measured_ones_and_under_the_bar():
    """Lengths, positions and directions under 1e-5 relative to their magnitude, RGB under 1e-4; the guards are widths of the same
    kind (a difference of two evaluations of one formula) and far below the 1 % they may cost."""
    assert 0 < X.EPS_CHAIN_EYE <= 1e-5 and 0 < X.EPS_CHAIN_DIR <= 1e-5 and 0 < X.EPS_CHAIN_LEN <= 1e-5 and 0 < X.EPS_CHAIN_RGB <= 1e-4
    assert 0 < X.GUARD_K <= 1e-5 and 0 < X.GUARD_DISC <= 1e-5 and X.CHAIN_COVERED == 0.10


def test_the_chain_constants_are_four_times_the_measurement(chain_frames):
    """Over the CPU cases (the 512 x 288 frame of `python tests/path_a_exact.py` is not rendered here, so: at most the constant / 4)."""
    worst = {}
    for name, w, h in X.CHAIN_FRAMES:
        fr, _ = chain_frames(name, w, h)
        res = X.check_chains(fr, 0.0, 0.0, 0.0, 0.0)
        for k in ("eye", "dir", "len", "rgb", "guard_k", "guard_disc"):
            worst[k] = max(worst.get(k, 0.0), res[k])
    print(worst)
    for k, c in (("eye", X.EPS_CHAIN_EYE), ("dir", X.EPS_CHAIN_DIR), ("len", X.EPS_CHAIN_LEN), ("rgb", X.EPS_CHAIN_RGB), ("guard_k", X.GUARD_K), ("guard_disc", X.GUARD_DISC)):
        assert 0.5 * c / 4 <= worst[k] <= c / 4 * (1 + 1e-3), (k, worst[k], c)


@pytest.mark.parametrize("wrong", X.WRONG_CHAINS)
@pytest.mark.parametrize("name,w,h", X.CHAIN_FRAMES)
def test_a_wrong_reading_of_the_chains_is_rejected(chain_frames, name, w, h, wrong):
    """The recordings are the oracle's, the reference is what a misreading of rt_abi.h would compute: it has to reject them on every
    case where the two readings differ (X.wrong_applies)."""
    fr, right = chain_frames(name, w, h)
    assert right["bad"] == 0
    if not X.wrong_applies(wrong, fr, right):
        if wrong == "cam_fall from the camera" and fr.reflections + fr.transmissions:
            a, b = X.chain_bands(fr), X.chain_bands(fr, wrong)
            assert np.array_equal(a["lo"], b["lo"]) and np.array_equal(a["hi"], b["hi"])  # clamped fall-off: the same intervals
        return
    res = X.check_chains(fr, wrong=wrong)
    print(f"{wrong}: {res['bad']} of {res['hits']} hit pixels reject it (nan {res['bad_nan']}, eye {res['bad_eye']}, dir {res['bad_dir']}, len {res['bad_len']}, rgb {res['bad_rgb']})")
    assert res["bad"] > 0, res


def test_every_wrong_reading_is_tried_on_some_case(chain_frames):
    for wrong in X.WRONG_CHAINS:
        assert sum(X.wrong_applies(wrong, *chain_frames(name, w, h)) for name, w, h in X.CHAIN_FRAMES) >= 2, wrong


@pytest.mark.parametrize("name,w,h", X.CHAIN_FRAMES)
def test_exchanged_recordings_are_rejected(chain_frames, name, w, h):
    """Two hit pixels' recordings exchanged (a row written to the wrong pixel): both pixels reject theirs."""
    fr, right = chain_frames(name, w, h)
    cb = X.chain_bands(fr)
    k = len(cb["py"])
    a, b = (cb["py"][k // 3], cb["px"][k // 3]), (cb["py"][2 * k // 3], cb["px"][2 * k // 3])
    chains = fr.chains.copy()
    chains[a], chains[b] = fr.chains[b], fr.chains[a]
    res = X.check_chains(chain_copy(fr, chains=chains))
    print(f"{res['bad']} of {res['hits']} hit pixels reject the exchange")
    assert right["bad"] == 0 and res["bad"] == 2, res


@pytest.mark.parametrize("name,w,h", X.CHAIN_FRAMES)
def test_edited_recordings_are_rejected(chain_frames, name, w, h):
    """The first link of every pixel rolled by one pixel, moved by one cone radius along the ray, and erased."""
    fr, right = chain_frames(name, w, h)
    rolled = fr.chains.copy()
    rolled[:, :, 0] = np.roll(fr.chains[:, :, 0], 1, axis=1)
    moved = fr.chains.copy()
    moved[:, :, 0, 6] = np.where(moved[:, :, 0, 6] < fr.render_dist, moved[:, :, 0, 6] * (1.0 + fr.ray_radius) + fr.ray_radius, moved[:, :, 0, 6])
    erased = fr.chains.copy()
    erased[:, :, 0] = np.nan
    for label, chains in (("rolled", rolled), ("moved", moved), ("erased", erased)):
        res = X.check_chains(chain_copy(fr, chains=chains))
        print(f"{label}: {res['bad']} of {res['hits']} hit pixels reject it")
        assert res["bad"] > 0.02 * res["hits"], (label, res)


def test_the_chain_hook_is_exported_and_bound(tmp_path):
    import abi_boundary as AB

    AB.exports(AB.CHAIN_HOOK)
    AB.null_context(AB.CHAIN_HOOK)
    import raytracing_engine_amd as R

    out = np.full(7, 7.0, np.float32)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    assert R.load().rt_render_chains(None, p, p, p, p, p) == -1 and (out == 7.0).all()  # no context: nothing written
