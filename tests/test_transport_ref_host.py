"""CPU tests of the float64 transport reference (tests/native/pt_transport_ref.cpp, tests/transport_ref.py; DESIGN.md sections 3, 6.4).

(i) the reference meets closed forms within five of its own standard errors; (ii) the committed fixtures are reproducible and a run
does not depend on the thread count; (iii) oracle B, and tests/native/pt_surfaces_ref.c where there are mirrors and glass, meet the
fixtures through compare() at a budget of a few seconds per scene, and compare() fails on frames that are 1 % too bright and on a
mesh whose mirror and glass are painted Lambert.  The GPU leg, thirty times the samples, is tests/test_gpu_transport.py."""
import functools
import math
import os

import numpy as np
import pytest

import transport_ref as TR
from test_oracle_lights import CAM as LIGHT_CAM, reference as irradiance_reference
from test_pt_surfaces_ref import join, wall
from raytracing_engine_amd import scenes

GLASS, MIRROR = scenes.SURFACE_GLASS, scenes.SURFACE_MIRROR
SMALL = dict(batches=64, spp=16)  # 2^18 paths, a fraction of a second


def within(r, want, sigmas=5.0):
    """Every cell and the frame of reference result r within `sigmas` of its own standard errors of `want` per channel
    (1e-12 relative for rounding, which is all a deterministic answer leaves)."""
    want = np.asarray(want, np.float64)
    for mean, se in ((r["mean"], r["se"]), (r["frame_mean"], r["frame_se"])):
        assert (np.abs(mean - want) <= sigmas * se + 1e-12 * np.abs(want)).all(), (mean, se, want)


# ---- (i) closed forms -----------------------------------------------------------------------------------------------------------------

def test_plane_under_a_uniform_sky_is_albedo_times_sky():
    alb, sky = (0.25, 0.5, 0.75), (2.0, 1.0, 0.5)
    r = TR.reference(wall(20.0, 1e4, alb), bounces=1, sky=sky, seed=3, **SMALL)
    within(r, np.multiply(alb, sky))
    assert (r["by_depth"][[0, 2]] == 0).all()  # everything is gathered by the miss at depth 1
    deeper = TR.reference(wall(20.0, 1e4, alb), bounces=4, sky=sky, seed=3, **SMALL)  # a plane cannot see itself
    within(deeper, np.multiply(alb, sky))
    none = TR.reference(wall(20.0, 1e4, alb), bounces=0, sky=sky, seed=3, **SMALL)  # the specification traces no ray from depth B on
    assert (none["frame_mean"] == 0).all()


def test_mirror_filling_the_view_reflects_the_sky():
    alb, sky = (0.8, 0.5, 0.25), (0.3, 0.6, 0.9)
    r = TR.reference(wall(5.0, 100.0, alb), [MIRROR] * 2, bounces=1, sky=sky, seed=4, **SMALL)
    within(r, np.float32(alb).astype(np.float64) * sky)  # the mesh holds the albedo in fp32
    ends = TR.reference(wall(5.0, 100.0, alb), [MIRROR] * 2, bounces=0, sky=sky, seed=4, **SMALL)  # a delta vertex at depth B adds nothing
    assert (ends["frame_mean"] == 0).all()


def test_clear_pane_passes_the_sky():
    sky = (0.3, 0.6, 0.9)
    r = TR.reference(wall(5.0, 100.0, (1, 1, 1)), [GLASS] * 2, [1.5, 1.5], bounces=1, sky=sky, seed=5, **SMALL)
    within(r, sky)


def test_irradiance_under_the_rectangle_light():
    """The floor under tests/test_oracle_lights.py's light through its narrow camera, against that file's float64 closed form: without
    next-event estimation the value is albedo Le times the fraction of cosine-distributed directions that meet the light."""
    want, err = irradiance_reference()
    rot = TR.DOWN
    for bounces in (0, 2):  # a plane cannot see itself: more bounces add nothing
        r = TR.reference(scenes.tessellated_light_scene(8, 1.6), bounces=bounces, rot=rot, seed=6, batches=64, spp=64, **LIGHT_CAM)
        assert (np.abs(r["frame_mean"] - want) <= 5.0 * r["frame_se"] + err).all() and (r["frame_se"] > 0).all() and (r["frame_se"] < 0.005 * want).all()
        assert (np.abs(r["mean"] - want) <= 5.0 * r["se"] + err).all()


@pytest.mark.parametrize("eta", [1.5, 2.4])
def test_fresnel_at_normal_incidence(eta):
    """A glass interface straight ahead, seen through a narrow camera, a large light behind the camera and a black sky: the reflected
    part sees the light, the refracted part leaves: F Le with F = ((eta - 1) / (eta + 1))^2, from outside and from inside."""
    le = (5.0, 7.0, 11.0)
    want = ((eta - 1.0) / (eta + 1.0)) ** 2 * np.asarray(le)
    pane = wall(5.0, 10.0, (1, 1, 1))  # e1 x e2 points to -y, towards the camera: the ray enters
    back = (np.ascontiguousarray(pane[0].reshape(2, 3, 3)[:, ::-1].reshape(2, 9)), pane[1], pane[2])  # wound the other way: the ray leaves
    for mesh in (pane, back):
        r = TR.reference(join(mesh, wall(-5.0, 1000.0, (0, 0, 0), le)), [GLASS, GLASS, 0, 0], [eta, eta, 1, 1], bounces=1, ratio=(1e-4, 1e-4), seed=7,
                         batches=64, spp=64)
        within(r, want)
        assert (r["frame_se"] > 0).all() and (r["frame_se"] < 0.02 * want).all()


# ---- (ii) reproducible ------------------------------------------------------------------------------------------------------------

def test_a_run_depends_on_the_seed_and_not_on_the_thread_count():
    s = TR.scene("surfaces")
    runs = [TR.reference(s["mesh"], s["kind"], s["ior"], seed=seed, threads=threads, batches=64, spp=4, **s["view"]) for seed, threads in ((9, 1), (9, 7), (10, 7))]
    for key in ("mean", "se", "sd", "frame_mean", "by_depth"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    assert not np.array_equal(runs[0]["mean"], runs[2]["mean"])
    assert np.allclose(runs[0]["by_depth"].sum(axis=0), runs[0]["frame_mean"], rtol=1e-12)
    one = TR.reference(s["mesh"], s["kind"], s["ior"], seed=9, only_depth=2, batches=64, spp=4, **s["view"])
    assert np.allclose(one["frame_mean"], runs[0]["by_depth"][2], rtol=1e-12)


@pytest.mark.parametrize("name", TR.SCENES)
def test_fixture_is_reproducible(name):
    """A small run with the committed seed meets the committed means within five sigma of the small run, the scene in the file is the
    scene of transport_ref.scene(), and the file records that the reference met its conditions."""
    g = TR.golden(name)
    s = TR.scene(name)
    mesh, kind, ior, view = TR.golden_scene(g)
    for got, want in zip(mesh, s["mesh"]):
        assert np.array_equal(got, np.asarray(want, np.float32).reshape(got.shape))
    assert (kind is None) == (s["kind"] is None) and (kind is None or (np.array_equal(kind, s["kind"]) and np.array_equal(ior, s["ior"])))
    assert set(view) == set(s["view"]) and all(np.array_equal(np.float32(view[k]), np.float32(s["view"][k])) for k in view)
    assert int(g["paths"]) == 256 * int(g["ref_batches"]) * int(g["ref_spp"]) and int(g["ref_batches"]) >= 64
    frame, cell = TR.reference_conditions(g)
    assert frame == float(g["frame_rel_se"]) <= TR.FRAME_REL_SE and cell == float(g["cell_rel_se"]) <= TR.CELL_REL_SE
    r = TR.reference(mesh, kind, ior, seed=int(g["ref_seed"]), batches=64, spp=32, **view)
    z = np.abs(TR._z(r["mean"] - g["mean"], np.hypot(r["se"], g["se"])))
    zf = np.abs(TR._z(r["frame_mean"] - g["frame_mean"], np.hypot(r["frame_se"], g["frame_se"])))
    print(f"{name}: small run of {r['paths']} paths, max |z| cell {z.max():.2f} frame {zf.max():.2f}")
    assert z.max() <= 5.0 and zf.max() <= 5.0
    assert np.allclose(g["by_depth"].sum(axis=0), g["frame_mean"], rtol=1e-9)


def test_reference_program_is_clean_under_sanitizers():
    """The stand-alone program built with -fsanitize=address,undefined, on the scene with every surface kind."""
    s = TR.scene("surfaces")
    a = TR.reference(s["mesh"], s["kind"], s["ior"], seed=9, threads=4, batches=64, spp=1, sanitized=True, **s["view"])
    b = TR.reference(s["mesh"], s["kind"], s["ior"], seed=9, threads=4, batches=64, spp=1, **s["view"])
    assert np.allclose(a["mean"], b["mean"], rtol=1e-12, atol=1e-15)


# ---- (iii) oracle B and pt_surfaces_ref against the fixtures ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cpu_frames(name):
    mesh, kind, ior, view = TR.golden_scene(TR.golden(name))
    return TR.cpu_frames(mesh, kind, ior, view, TR.CPU_SPP[name], threads=min(16, os.cpu_count() or 1))


@pytest.mark.parametrize("name", TR.SCENES)
def test_oracle_meets_the_float64_transport(name):
    g = TR.golden(name)
    report = TR.compare(cpu_frames(name), g, TR.CPU_SPP[name], check=False)
    print(f"{name}: {TR.summary(report)}")
    assert not report["failures"], "\n".join(report["failures"])


@pytest.mark.parametrize("name", ["cornell", "surfaces", "tess_light"])
def test_compare_fails_on_frames_one_percent_too_bright(name):
    g = TR.golden(name)
    frames = {s: (f * np.float32(1.01)).astype(np.float32) for s, f in cpu_frames(name).items()}
    with pytest.raises(AssertionError, match="frame"):
        TR.compare(frames, g, TR.CPU_SPP[name])
    report = TR.compare(frames, g, TR.CPU_SPP[name], check=False)
    assert np.abs(report["z_frame"]).max() > TR.Z_MAX  # the frame mean alone names it


def test_compare_fails_on_the_surfaces_mesh_painted_lambert():
    g = TR.golden("surfaces")
    mesh, kind, ior, view = TR.golden_scene(g)
    assert kind is not None and (kind == MIRROR).any() and (kind == GLASS).any()
    frames = TR.cpu_frames(mesh, None, None, view, TR.CPU_SPP["surfaces"], threads=min(16, os.cpu_count() or 1))
    with pytest.raises(AssertionError, match="cell"):
        TR.compare(frames, g, TR.CPU_SPP["surfaces"])


def test_compare_fails_on_an_estimator_that_is_noisier_than_the_cap():
    """Frames whose seed-to-seed scatter is four times the brute-force estimator's would widen their own tolerance: the cap names them
    (four times: the deviation of 32 seeds scatters by 13 %, so every cell stays above 1.5)."""
    g = TR.golden("sky_room")
    spp = 64
    rng = np.random.default_rng(1)
    sd = 4.0 * np.repeat(np.repeat(g["sd"], 4, axis=0), 4, axis=1) / math.sqrt(spp)  # per pixel value of a frame
    mean = np.repeat(np.repeat(g["mean"], 4, axis=0), 4, axis=1)
    frames = {s: mean + sd * rng.standard_normal(mean.shape) for s in range(TR.K_SEEDS)}
    report = TR.compare(frames, g, spp, check=False)
    assert report["failures"] and all("sigma_path" in f for f in report["failures"]) and (report["cap"] > TR.SE_CAP).all()


# what DESIGN.md section 6.4 states, in per cent: scene -> (frame mean, worst bright cell)
STATED_DETECTABLE = {"cornell": (0.39, 3.1), "surfaces": (0.38, 2.9), "sky_room": (0.31, 1.8), "tess_light": (0.42, 2.2), "cornell_b0": (0.46, 5.5),
                     "cornell_b1": (0.42, 3.8)}


def test_detectable_bias_comes_from_the_recorded_errors():
    """The smallest bias the GPU leg (32 frames of 4096 paths per pixel) is certain to flag is computed from the committed standard errors
    and per-path deviations, and DESIGN.md states these figures: below half a per cent of the frame mean on every scene."""
    for name in TR.SCENES:
        frame, cell = TR.detectable_bias(TR.golden(name), 4096)
        print(f"{name}: frame {frame:.3%} cell {cell:.3%}")
        assert (round(100 * frame, 2), round(100 * cell, 1)) == STATED_DETECTABLE[name] and frame < 0.005
