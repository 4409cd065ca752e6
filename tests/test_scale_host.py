"""Path B's answers across coordinate scale, on the CPU references (tests/scale_exact.py).

Every other comparison of path B is made at one scale, between 1e-3 and 1e4.  Here the whole problem is multiplied by 2^k - which is
exact in fp32 - and the references' answers must be the transformed k = 0 answers bit for bit: over the recorded range of every
family, and no further than recorded (the first k on each side where equality breaks is part of the record).  At the tested scales
the float64 contracts hold on the scaled problem with their constants unchanged.  The library's coordinate limit lies inside every
measured range, and frames are finite at every scale, also where they are no longer covariant.  tests/test_gpu_scale.py holds the
kernels to the same."""
import os
import re

import numpy as np
import pytest

import scale_exact as S

f32 = np.float32


scales_of = S.host_scales  # k = 0, +-1, +-12, both ends of the family's range and one step inside, and the GPU tests' scales


# ---- the helper's self-check ---------------------------------------------------------------------------------------------------
def test_power_of_two_scaling_is_exact_and_anything_else_is_seen(monkeypatch):
    x = np.array([1.1, -0.37, 3e-3, 0.0, -0.0, np.inf, 25.84], f32)
    for k in (-60, -1, 0, 1, 60):
        q = S.scaled_problem(k, verts=x, d=x)
        assert q["exact"] and q["d"] is x and np.array_equal(q["verts"].astype(np.float64), x.astype(np.float64) * 2.0 ** k)
    with pytest.raises(AssertionError):
        S.scaled_problem(-140, verts=x)  # 3e-3 * 2^-140 is subnormal: mantissa bits are lost
    assert not S.scaled_problem(125, check=False, verts=x)["exact"]  # 25.84 * 2^125 overflows
    with pytest.raises(KeyError):
        S.scaled_problem(1, vertices=x)
    # a factor that is no power of two: the self-check refuses it, and the answers are NOT the transformed ones - the bit-equality
    # of the other tests is not vacuous
    monkeypatch.setattr(S, "SCALE", lambda a, k: (a * f32(1.5) ** f32(k)).astype(f32))
    with pytest.raises(AssertionError):
        S.scaled_problem(1, verts=x)
    got = S.closest_hit(1, check=False)  # (not through the cache)
    assert not got["exact"].any()
    bad = S.differing(got, S.transformed(S.answers("closest_hit", 0), 1))
    assert "t*" in bad and "exact" in bad, bad
    hit = got["tri"] >= 0
    assert (got["t*"][hit].view(np.uint32) != S.transformed(S.answers("closest_hit", 0), 1)["t*"][hit].view(np.uint32)).mean() > 0.2


def test_the_cases_are_not_vacuous():
    rays, points = S.ray_cases(), S.point_cases()
    assert sum(len(c["o"]) for c in rays) == S.N == sum(len(c["p"]) for c in points)
    a = S.answers("hit_attr", 0)
    assert (a["tri"] >= 0).mean() > 0.3 and (a["tri"] == -1).mean() > 0.2  # hits, and misses (the halved limits among them)
    occ = S.answers("occlusion", 0)["occluded"]
    assert 0.05 < occ.mean() < 0.95
    h = S.answers("all_hits", 0)
    assert h["count"].max() >= 3 and len(h["tri"]) > S.N // 2
    nb = S.answers("neighbors", 0)
    assert nb["count"].max() >= 8 and (nb["count"] >= 1).mean() > 0.9
    s = S.answers("sides", 0)
    assert 0.1 < (s["inside"] == 1).mean() < 0.9 and (s["sdist*"] < 0).any() and (s["sdist*"] > 0).any()
    for family in S.FRAME_FAMILIES:
        for name, rgb in S.answers(family, 0).items():
            if name != "exact":
                assert rgb.shape == (32, 48, 3) and (rgb > 0).mean() > 0.5 and len(np.unique(rgb)) > 100, name  # (most of the soup's frame is sky)


# ---- the ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_answers_are_the_transformed_answers_over_the_recorded_range_and_no_further(family):
    lo, hi = S.RANGES[family]
    assert lo < -12 and hi > 12
    # every ray, point and pixel at each scale, none left out; the scales: the tested ones and every fourth of the range (measure()
    # walked all of them, outward from 0, and stopped at the first that failed)
    for k in sorted(set(range(lo, hi + 1, 4)) | set(scales_of(family))):
        ok, bad = S.holds_at(family, k)
        assert ok, (family, k, bad)
    for k in (lo - 1, hi + 1):
        ok, bad = S.holds_at(family, k)
        assert not ok, (family, k, "the recorded range ends here, but the answers still hold")


@pytest.mark.parametrize("family", [f for f in S.FAMILIES if f not in S.FRAME_FAMILIES])
def test_float64_contracts_hold_at_every_tested_scale(family):
    for k in scales_of(family):
        assert S.contract_failures(family, k) == 0, (family, k)


def test_the_contract_check_is_not_vacuous():
    """An answer of the neighbouring ray, and a distance off by 2^-12 of itself, miss the contracts at a scaled problem too."""
    k = S.RANGES["closest_hit"][0] + 1
    a = dict(S.answers("closest_hit", k))
    a["tri"] = np.roll(a["tri"], 1)
    assert S.contract_failures("closest_hit", k, a) > S.N // 4
    k = S.RANGES["closest_point"][1] - 1
    a = dict(S.answers("closest_point", k))
    a["dist*"] = (a["dist*"] * f32(1 + 2.0 ** -12)).astype(f32)
    assert S.contract_failures("closest_point", k, a) > S.N // 4


# ---- the limit -----------------------------------------------------------------------------------------------------------------
def test_the_coordinate_limit_lies_inside_every_measured_range():
    """2^L <= M0 * 2^k_hi: the largest mesh the library takes has been seen to give covariant answers in every family."""
    header = open(os.path.join(S.ROOT, "include", "rt_abi.h")).read()
    assert int(re.search(r"#define RT_PT_MAX_COORD_LOG2 (\d+)", header).group(1)) == S.COORD_LIMIT_LOG2
    assert int(re.search(r"#define RT_PT_MIN_FEATURE_LOG2 \((-\d+)\)", header).group(1)) == S.FEATURE_MIN_LOG2
    for family, (lo, hi) in S.RANGES.items():
        assert S.COORD_LIMIT_LOG2 <= hi + int(np.floor(np.log2(S.m0(family)))), (family, hi, S.m0(family))
    for family in S.FAMILIES:
        assert S.gpu_scales(family)[-1] == min(S.RANGES[family][1], S.k_limit(family))


def test_the_documented_feature_size_lies_inside_every_measured_range():
    """The smallest feature of each case at k = 0, times 2^k_lo, is below 2^FEATURE_MIN_LOG2: covariance has been seen down to it."""
    for family, (lo, hi) in S.RANGES.items():
        assert np.log2(S.feature0(family)) + lo <= S.FEATURE_MIN_LOG2, (family, lo, S.feature0(family))


# ---- finiteness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FRAME_FAMILIES)
def test_frames_are_finite_at_every_scale(family):
    """From 2^-75 of the scenes' size up to the library's limit: no non-finite pixel.  NONFINITE_BEFORE
    are the scales at which the references gave some before the light weight's denominator was guarded."""
    assert set(S.NONFINITE_BEFORE[family]) <= set(range(-S.K_SCAN, 0))
    for k in range(-S.K_SCAN, S.k_limit(family) + 1):  # every scale, none left out
        assert S.frames_finite(family, k), (family, k)
