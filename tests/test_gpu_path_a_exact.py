"""Path A's kernels against closed-form sphere geometry: no oracle, no fixture; every expected value comes from tests/path_a_exact.py.

tests/test_gpu_path_a.py holds the kernels bit-exact to oracle A, which mirrors them line by line; a misreading the two share (the
pixel-centre mapping, the cone radius taken from the relative length, the parent texel, the nearest-sphere rule, the fall-offs, the
cap of the shadow term) passes there.  Here every level of the depth pyramid lies in the float64 band of its texel, every hit pixel
in its RGB interval (EPS_DEPTH / EPS_RGB were measured on the CPU, never on a GPU frame), misses are exactly black, and the caps that
keep the intervals meaningful hold; both launch schedules, padded levels, a non-default config and ratio.  What the bands decide and
what they leave open (grazing rays, penumbrae), and the power of the check: tests/test_path_a_exact_host.py, DESIGN.md section 3.
"""
import numpy as np
import pytest

import path_a_exact as X

pytestmark = pytest.mark.gpu


def gpu_frame(r, name, w, h, fused):
    scene, view, conf = X.CASES[name][:3]
    cfg = r.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    cfg.fuse_levels = int(fused)
    r.set_config(cfg)
    r.set_scene(scene)
    r.resize(w, h, view.get("ratio"))
    rgb, depth = r.render(view.get("rot", (0, 0, 0, 1)), view.get("pos", (0, 0, 0)), want_depth=True)
    levels = [r.read_level(i) for i in range(len(r.level_info()))]
    assert np.array_equal(depth, levels[-1])
    fr = X.Frame(scene, w, h, levels=levels, rgb=rgb, **view, **conf)
    fr.hit_pixels = r.stats()["hit_pixels"]
    return fr


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
