"""Path A's kernels against closed-form sphere geometry: no oracle, no fixture; every expected value comes from tests/path_a_exact.py.

tests/test_gpu_path_a.py holds the kernels bit-exact to oracle A, which mirrors them line by line; a misreading the two share (the
pixel-centre mapping, the cone radius taken from the relative length, the parent texel, the nearest-sphere rule, the fall-offs, the
cap of the shadow term) passes there.  Here every level of the depth pyramid lies in the float64 band of its texel, every hit pixel
in its RGB interval (EPS_DEPTH / EPS_RGB were measured on the CPU, never on a GPU frame), misses are exactly black, and the caps that
keep the intervals meaningful hold; both launch schedules, padded levels, a non-default config and ratio.  What the bands decide and
what they leave open (grazing rays, penumbrae), and the power of the check: tests/test_path_a_exact_host.py, DESIGN.md section 3.

Multi-sample frames are what the benchmark renders: batched level launches (grid.y = sample, the jitter recomputed in the kernel) and
the SP shade kernel (four lanes per pixel) for batches of a multiple of four.  Every image of the batch is read back
(rt_read_level_image), mapped to its sample by the index the hook reports, and held to the bands of that sample's jitter; the
averaged frame to the averaged intervals; 4 (SP), 9 (in-thread loop) and 16 spp (four SP rounds).  March algorithm 1 against its own
bands.  Without any band: the batched schedule and the one-sample-per-launch schedule give the same frame bit for bit at 4, 9, 16,
25 (16 SP + 9 continuing the sum) and 36 spp (16 + 16 + 4), at widths that are no multiple of 4 or 64; SP with tile-major output and
a partition de-tiles to the single frame; a frame slot at 16 spp delivers the synchronous frame.

The mirror and transmission chains (X.CHAIN_FRAMES): rt_render_chains returns what every secondary march did, and every link is
held to the closed forms from the recorded link before it (X.chain_bands), with the NaN pattern, the summed RGB and the counters;
its RGB and depth are rt_render's bit for bit, and the batched schedule it does not enter is tied to it bit for bit at 4 and 16 spp.
"""
import numpy as np
import pytest

import path_a_exact as X

pytestmark = pytest.mark.gpu


def setup(r, name, w, h, fused=0, march_algorithm=0):
    """Config, scene and size of case `name` on the renderer -> (scene, view, conf, rot, pos).  The caller resets the config."""
    scene, view, conf = X.CASES[name][:3]
    cfg = r.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    cfg.fuse_levels = int(fused)
    cfg.march_algorithm = int(march_algorithm)
    r.set_config(cfg)
    r.set_scene(scene)
    r.resize(w, h, view.get("ratio"))
    return scene, view, conf, view.get("rot", (0, 0, 0, 1)), view.get("pos", (0, 0, 0))


def gpu_frame(r, name, w, h, fused, march_algorithm=0):
    scene, view, conf, rot, pos = setup(r, name, w, h, fused, march_algorithm)
    rgb, depth = r.render(rot, pos, want_depth=True)
    levels = [r.read_level(i) for i in range(len(r.level_info()))]
    assert np.array_equal(depth, levels[-1])
    fr = X.Frame(scene, w, h, levels=levels, rgb=rgb, march_algorithm=march_algorithm or 3, **view, **conf)
    fr.hit_pixels = r.stats()["hit_pixels"]
    return fr


def read_batch(r, n_images):
    """{sample index: [levels]} of the last batch's images, each mapped through the sample index the hook reports."""
    out = {}
    for image in range(n_images):
        levels = []
        for i in range(len(r.level_info())):
            lv, sample = r.read_level(i, image)
            levels.append(lv)
            assert sample == r.read_level(0, image)[1]
        out[sample] = levels
    return out


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("name,w,h", X.FRAMES + X.GPU_ONLY_FRAMES)
def test_frames_lie_inside_every_band(renderer, name, w, h, fused):
    """Only texels with on-screen descendants count (the fused schedule computes no others; nothing reads them)."""
    try:
        fr = gpu_frame(renderer, name, w, h, fused)
    finally:
        renderer.set_config(renderer.default_config())
    depth, rgb = X.check_frame(fr)
    for i, lv in enumerate(depth):
        print(f"level {i}: {lv}")
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    print(rgb)
    assert rgb["bad"] == 0 and rgb["miss_nonblack"] == 0, rgb
    X.check_caps(name, rgb)
    if name == "all_miss":
        assert rgb["hits"] == 0 and not fr.rgb.any()
    else:
        assert rgb["hits"] > 0.05 * w * h
        assert fr.hit_pixels == rgb["hits"]


@pytest.mark.parametrize("name,w,h", X.ALG1_FRAMES)
def test_algorithm_1_frames_lie_inside_every_band(renderer, name, w, h):
    """March algorithm 1 (every SDF every step, radius after the step) against its own closed-form bands; per-level schedule
    (the sketched algorithms have no fused launch)."""
    try:
        fr = gpu_frame(renderer, name, w, h, 0, march_algorithm=1)
    finally:
        renderer.set_config(renderer.default_config())
    depth, rgb = X.check_frame(fr)
    for i, lv in enumerate(depth):
        print(f"level {i}: {lv}")
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    print(rgb)
    assert rgb["bad"] == 0 and rgb["miss_nonblack"] == 0, rgb
    X.check_caps(name, rgb)
    if name == "all_miss":
        assert rgb["hits"] == 0 and not fr.rgb.any() and all(lv["hits"] == 0 for lv in depth[1:])
    else:
        assert rgb["hits"] > 0.05 * w * h
        assert fr.hit_pixels == rgb["hits"]


# ---- multi-sample frames: the batched level launches and the SP shade kernel -------------------------------------------------------
@pytest.mark.parametrize("name,w,h,spp", X.SAMPLE_FRAMES + X.GPU_ONLY_SAMPLE_FRAMES)
def test_multi_sample_frames_lie_inside_every_band(renderer, name, w, h, spp):
    """Per-level schedule, one batch (spp <= 16): every image of the batch is read back, mapped to its sample through the index the
    hook reports, and held to the bands of that sample's jitter; the averaged frame to the averaged intervals."""
    try:
        scene, view, conf, rot, pos = setup(renderer, name, w, h)
        rgb = renderer.render(rot, pos, spp=spp)
        hit_pixels = renderer.stats()["hit_pixels"]
        batch = read_batch(renderer, spp)
    finally:
        renderer.set_config(renderer.default_config())
    assert sorted(batch) == list(range(spp))
    frames = [X.Frame(scene, w, h, levels=batch[s], jitter=X.sample_jitter(s, spp, w, h), **view, **conf) for s in range(spp)]
    res = X.check_samples(frames, rgb)
    for s, levels in enumerate(res["depth"]):
        for i, lv in enumerate(levels):
            assert lv["bad"] == 0 and lv["far_bad"] == 0, (s, i, lv)
    print({k: v for k, v in res.items() if k != "depth"})
    assert res["bad"] == 0 and res["miss_nonblack"] == 0, res
    X.check_caps(name, res)
    assert res["hits"] > 0.05 * w * h
    assert hit_pixels == res["sample_hits"]


@pytest.mark.parametrize("name,w,h,spp", X.SAMPLE_FRAMES)
def test_the_last_sample_of_a_fused_multi_sample_frame_lies_inside_its_bands(renderer, name, w, h, spp):
    """fuse_levels = 1 renders one sample per launch, so only the last sample's levels can be read: image 0 = sample spp - 1."""
    try:
        scene, view, conf, rot, pos = setup(renderer, name, w, h, fused=1)
        renderer.render(rot, pos, spp=spp)
        batch = read_batch(renderer, 1)
    finally:
        renderer.set_config(renderer.default_config())
    assert list(batch) == [spp - 1]
    fr = X.Frame(scene, w, h, levels=batch[spp - 1], jitter=X.sample_jitter(spp - 1, spp, w, h), **view, **conf)
    for i in range(fr.count):
        lv = X.check_depth(fr, i)
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)


def test_the_hook_reads_the_images_of_the_last_batch_only(renderer):
    import raytracing_engine_amd as R

    try:
        scene, view, conf, rot, pos = setup(renderer, "startup", 70, 66)
        renderer.render(rot, pos, spp=25)  # batches of 16 and 9
        top = len(renderer.level_info()) - 1
        assert [renderer.read_level(top, k)[1] for k in range(9)] == list(range(16, 25))
        assert np.array_equal(renderer.read_level(top), renderer.read_level(top, 8)[0])
        for bad in (9, 15, 16, 2 ** 32 - 1):
            with pytest.raises(R.RtError) as e:
                renderer.read_level(top, bad)
            assert e.value.code == -1
        renderer.render(rot, pos, spp=4)
        assert [renderer.read_level(0, k)[1] for k in range(4)] == [0, 1, 2, 3]
        with pytest.raises(R.RtError):
            renderer.read_level(0, 4)  # allocated (the pyramid keeps 16 images) but not of the last batch
        setup(renderer, "startup", 70, 66, fused=1)
        renderer.render(rot, pos, spp=9)
        assert renderer.read_level(top, 0)[1] == 8
        with pytest.raises(R.RtError):
            renderer.read_level(top, 1)
    finally:
        renderer.set_config(renderer.default_config())


# ---- the two schedules give the same frame, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [4, 9, 16, 25, 36])
@pytest.mark.parametrize("w,h", [(17, 9), (70, 66), (200, 120)])
@pytest.mark.parametrize("name", ["startup", "room"])
def test_batched_and_one_sample_per_launch_frames_are_bit_identical(renderer, name, w, h, spp):
    """the per-level schedule renders batches of up to 16 samples (the SP shade kernel when the batch is a
    multiple of four: 4, 16, the 16 of 25, 16 + 16 + 4 of 36; the in-thread loop for 9 and the 9 of 25, continuing the running
    sum), the fused schedule one sample per launch and never SP.  Both state ((s0 + s1) + s2) + ..., / spp, so the frames are equal
    bit for bit, and so is the last sample's finest level on the texels inside the frame (the fused launch writes no others)."""
    try:
        scene, view, conf, rot, pos = setup(renderer, name, w, h, fused=0)
        batched = renderer.render(rot, pos, spp=spp)
        top = len(renderer.level_info()) - 1
        last = spp - 1 - (spp - 1) // 16 * 16  # image of the last batch that holds sample spp - 1
        level, sample = renderer.read_level(top, last)
        hits = renderer.stats()["hit_pixels"]
        setup(renderer, name, w, h, fused=1)
        single = renderer.render(rot, pos, spp=spp)
        level1, sample1 = renderer.read_level(top, 0)
        hits1 = renderer.stats()["hit_pixels"]
    finally:
        renderer.set_config(renderer.default_config())
    assert sample == sample1 == spp - 1
    assert np.array_equal(level[:h, :w], level1[:h, :w])
    diff = np.flatnonzero((batched != single).any(-1))
    assert not len(diff), (len(diff), np.abs(batched - single).max())
    assert hits == hits1 and batched.any()


# ---- SP with partitions and frame slots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [4, 25])
@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("name,w,h", [("room", 200, 120), ("startup", 200, 120), ("room", 70, 66), ("startup", 70, 66)])
def test_tile_major_multi_sample_partitions_unite_to_the_single_frame(renderer, name, w, h, n_ranks, spp):
    """The SP shade kernel (4 spp; the batch of 16 in 25 spp) with tile-major output and a partition: every rank renders only its
    64 x 64 tiles, de-tiled they are the single-context frame bit for bit."""
    import torch

    try:
        scene, view, conf, rot, pos = setup(renderer, name, w, h)
        renderer.set_partition(0, 1)
        full = renderer.render(rot, pos, spp=spp)
        tx, ty, _ = renderer.tile_info()
        tiles_per_rank = -(-(tx * ty) // n_ranks)
        gathered = torch.zeros((n_ranks, tiles_per_rank, 64, 64, 3), dtype=torch.float32, device="cuda")
        for rank in range(n_ranks):
            renderer.set_partition(rank, n_ranks)
            renderer.render_device(rot, pos, spp, gathered[rank].data_ptr(), tile_major=True)
            renderer.synchronize()
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        renderer.detile_device(gathered.data_ptr(), n_ranks, tiles_per_rank, out.data_ptr())
        renderer.synchronize()
    finally:
        renderer.set_partition(0, 1)
        renderer.set_config(renderer.default_config())
    assert full.any() and np.array_equal(out.cpu().numpy(), full)


def test_a_frame_slot_at_16_spp_delivers_the_synchronous_frame(renderer):
    try:
        scene, view, conf, rot, pos = setup(renderer, "room", 200, 120)
        want = renderer.render(rot, pos, spp=16)
        renderer.frames_configure(1, renderer.FRAME_F32)
        renderer.frame_submit(0, rot, pos, spp=16)
        got = renderer.frame_wait(0)
    finally:
        renderer.resize(64, 64)  # releases the slot
        renderer.set_config(renderer.default_config())
    assert want.any() and np.array_equal(got, want)


# ---- the mirror and transmission chains: rt_render_chains returns every secondary march, each judged from the link before it -------
def setup_chain(r, name, w, h, fused=0, chains=True):
    """Config, scene and size of chain case `name` (chains = False: the same frame with both counts 0) -> (scene, view, conf, rot, pos)."""
    scene, view, conf = X.CHAIN_CASES[name][:3]
    cfg = r.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    if not chains:
        cfg.reflections = cfg.transmissions = 0
    cfg.fuse_levels = int(fused)
    r.set_config(cfg)
    r.set_scene(scene)
    r.resize(w, h, view.get("ratio"))
    return scene, view, conf, view.get("rot", (0, 0, 0, 1)), view.get("pos", (0, 0, 0))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("name,w,h", X.CHAIN_FRAMES + X.GPU_ONLY_CHAIN_FRAMES)
def test_chain_frames_lie_inside_every_band(renderer, name, w, h, fused):
    """The frame without chains passes check_frame (pyramid and primary colour); with them, rt_render_chains returns the RGB and
    depth of rt_render bit for bit, the pyramid is the same, and every recorded march, the summed RGB, the NaN pattern, the caps,
    the coverage conditions and the counters are what X.chain_bands derives link by link (constants measured on the CPU)."""
    try:
        scene, view, conf, rot, pos = setup_chain(renderer, name, w, h, fused, chains=False)
        rgb0, depth0 = renderer.render(rot, pos, want_depth=True)
        levels0 = [renderer.read_level(i) for i in range(len(renderer.level_info()))]
        setup_chain(renderer, name, w, h, fused)
        rgb1, depth1 = renderer.render(rot, pos, want_depth=True)
        stats1 = renderer.stats()
        rgb, depth, chains = renderer.render_chains(rot, pos)
        stats = renderer.stats()
        levels = [renderer.read_level(i) for i in range(len(renderer.level_info()))]
    finally:
        renderer.set_config(renderer.default_config())
    assert np.array_equal(rgb, rgb1) and np.array_equal(depth, depth1) and np.array_equal(depth, levels[-1])
    assert all(np.array_equal(a, b) for a, b in zip(levels, levels0))
    for k in ("hit_pixels", "shadow_rays", "reflection_rays", "transmission_rays"):
        assert stats[k] == stats1[k], k
    plain = X.Frame(scene, w, h, levels=levels0, rgb=rgb0, **view, **{k: v for k, v in conf.items() if k in X.OTHER_CONFIG})
    depth_res, rgb_res = X.check_frame(plain)
    for i, lv in enumerate(depth_res):
        assert lv["bad"] == 0 and lv["far_bad"] == 0, (i, lv)
    assert rgb_res["bad"] == 0 and rgb_res["miss_nonblack"] == 0 and rgb_res["ambiguous"] <= X.CAP_AMBIGUOUS, rgb_res
    assert chains.shape == (h, w, conf["reflections"] + conf["transmissions"], 7)
    fr = X.Frame(scene, w, h, levels=levels, rgb=rgb, chains=chains, **view, **conf)
    res = X.check_chains(fr)
    print(res)
    X.assert_chains(fr, res, stats)
    assert res["hits"] > 0.05 * w * h


def test_the_chain_hook_refuses_and_writes_nothing(renderer):
    """NULL outputs (RT_ERR_INVALID), both counts 0 and a partition of more than one rank (RT_ERR_STATE): sentinels stay."""
    import ctypes as C

    import raytracing_engine_amd as R

    def sentinels(rows):
        return np.full((64, 96, 3), 7.0, np.float32), np.full(renderer.level_info()[-1][::-1], 7.0, np.float32), np.full((64, 96, rows, 7), 7.0, np.float32)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))

    try:
        scene, view, conf, rot, pos = setup_chain(renderer, "room_turned_r2_t2_n1.5", 96, 64)
        rot, pos = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(pos, np.float32)
        lib = R.load()
        for missing in range(3):
            outs = sentinels(4)
            args = [None if k == missing else a for k, a in enumerate(outs)]
            assert lib.rt_render_chains(renderer._ctx, ptr(rot), ptr(pos), *[ptr(a) for a in args]) == -1
            assert all((a == 7.0).all() for a in outs)
        renderer.set_partition(1, 2)
        outs = sentinels(4)
        assert lib.rt_render_chains(renderer._ctx, ptr(rot), ptr(pos), *[ptr(a) for a in outs]) == -4
        assert all((a == 7.0).all() for a in outs)
        with pytest.raises(R.RtError) as e:
            renderer.render_chains(rot, pos)
        assert e.value.code == -4
        renderer.set_partition(0, 1)
        setup_chain(renderer, "room_turned_r2_t2_n1.5", 96, 64, chains=False)
        outs = sentinels(1)
        assert lib.rt_render_chains(renderer._ctx, ptr(rot), ptr(pos), *[ptr(a) for a in outs]) == -4
        assert all((a == 7.0).all() for a in outs)
        with pytest.raises(R.RtError) as e:
            renderer.render_chains(rot, pos)
        assert e.value.code == -4
        # and the context renders on: the hook right after the refusals
        setup_chain(renderer, "room_turned_r2_t2_n1.5", 96, 64)
        rgb, depth, chains = renderer.render_chains(rot, pos)
        assert rgb.any() and not np.isnan(chains[..., 0, :]).all()
    finally:
        renderer.set_partition(0, 1)
        renderer.set_config(renderer.default_config())


@pytest.mark.parametrize("spp", [4, 16])
def test_batched_and_one_sample_per_launch_chain_frames_are_bit_identical(renderer, spp):
    """test_batched_and_one_sample_per_launch_frames_are_bit_identical with both chains on (reflections 2, transmissions 2, index
    1.5, the room): the batched launches, which rt_render_chains does not enter, give bit for bit the average of the one-sample
    launches that it pins."""
    name, w, h = "room_r2_t2_n1.5", 200, 120
    try:
        scene, view, conf, rot, pos = setup_chain(renderer, name, w, h, fused=0)
        batched = renderer.render(rot, pos, spp=spp)
        top = len(renderer.level_info()) - 1
        level, sample = renderer.read_level(top, spp - 1)
        stats = renderer.stats()
        setup_chain(renderer, name, w, h, fused=1)
        single = renderer.render(rot, pos, spp=spp)
        level1, sample1 = renderer.read_level(top, 0)
        stats1 = renderer.stats()
    finally:
        renderer.set_config(renderer.default_config())
    assert sample == sample1 == spp - 1
    assert np.array_equal(level[:h, :w], level1[:h, :w])
    diff = np.flatnonzero((batched != single).any(-1))
    assert not len(diff), (len(diff), np.abs(batched - single).max())
    for k in ("hit_pixels", "shadow_rays", "reflection_rays", "transmission_rays"):
        assert stats[k] == stats1[k] and stats[k] > 0, k
    assert batched.any()
