"""Oracle B's frames, path by path, against a float64 reading of the specification (tests/path_b_exact.py), and the power of that
check.  CPU only.

oracle_b.c and path_b.hip mirror each other line by line, so the bit-exact GPU tests cannot see a misreading of DESIGN.md section 6
that the two share.  Here every pixel of the oracle's frame that is not ambiguous has to lie within EPS_RGB of a reference that uses
none of the oracle's code (meshes with surfaces: tests/native/pt_surfaces_ref.c, which the GPU frames equal bit for bit), the ray
counts have to agree, and no case may leave out more than 1 % of its pixels; tests/test_gpu_path_b_exact.py holds the kernels to the
same reference without any oracle.

The wrong readings (path_b_exact.WRONG) are what a shared misreading would produce: for each, the oracle's frame must have pixels
outside 100 EPS_RGB of the reference that reads the specification that way.  Share of the pixels that are not ambiguous which lie
outside, on the case named in MUTATIONS (printed by the tests, recorded here):

  pixel_centre           cornell_turned  23.2 %     cl_without_abs         cornell_turned  98.1 %
  jitter_after_ratio     cornell_turned  21.6 %     offset_unflipped       soup_dense      41.6 %
  swap_dims_3_4          cornell_turned  85.7 %     t_without_albedo       cornell_turned  97.9 %
  bounce_dims_3_4        cornell_turned  96.5 %     emitter_after_lambert  cornell_turned   2.8 %
  pick_ceil              cornell_turned  63.5 %     emitter_after_lambert  surfaces         6.8 %
  weight_without_nl      cornell_turned  97.8 %     swap_b1_b2             cornell_turned  95.4 %
  refract_entry_side     surfaces        13.8 %     fresnel_without_half   surfaces         2.6 %

(every wall of the room faces the room, so nothing is flipped there: offset_unflipped is held against the dense soup.)  Each share
has to exceed the 1 % of its pixels that a case may leave out.

Indistinguishable, reported and asserted to be so (INDISTINGUISHABLE):
  pick_no_clamp      rnd < 1, so floor(rnd N_L) <= N_L - 1 in exact arithmetic: the clamp acts only where fp32 rounds rnd N_L up to N_L,
                     at most one sample in 2^24, and then the pixel is ambiguous by the pick guard.  The reference never clamps.
  divide_before_sum  on the 5 spp frame sum(x / 5) and sum(x) / 5 differ by rounding alone (float64: 1e-16; fp32: 1e-7, inside EPS_RGB).
"""
import numpy as np
import pytest

import path_b_exact as X

MUTATIONS = [(w, "cornell_turned") for w in ("pixel_centre", "jitter_after_ratio", "swap_dims_3_4", "bounce_dims_3_4", "pick_ceil", "weight_without_nl",
                                              "cl_without_abs", "t_without_albedo", "emitter_after_lambert", "swap_b1_b2")]
MUTATIONS += [("offset_unflipped", "soup_dense")]  # every wall of the room faces the room: nothing is flipped there
MUTATIONS += [(w, "surfaces") for w in ("refract_entry_side", "fresnel_without_half", "emitter_after_lambert")]
INDISTINGUISHABLE = [("pick_no_clamp", "many_lights"), ("pick_no_clamp", "cornell_turned"), ("divide_before_sum", "cornell_b2_spp5")]


@pytest.fixture(scope="module")
def frames():
    """Oracle frames and counts, rendered once and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            s, _, fr = X.case(name)
            cache[name] = X.oracle_frame(s, fr)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(X.CASES))
def test_oracle_frames_lie_within_eps_of_the_specification(frames, name):
    rgb, counts = frames(name)
    exp = X.case_expected(name)
    fr = X.case(name)[2]
    print(f"{name}: largest excess {X.excess(rgb, exp).max():.3g} (EPS_RGB {X.EPS_RGB:.3g}), left out {X.left_out(exp):.4%}, "
          + ", ".join(f"{k} {counts[k]} / {exp[k]}" for k in X.COUNTS))
    worst, share = X.check_frame(rgb, exp, counts=counts, bounces=fr.bounces)
    assert share <= X.CAP_AMBIGUOUS
    assert abs(share - X.LEFT_OUT[name]) < 1e-6, "the recorded share is stale"
    assert np.abs(exp["rgb"]).max() > 0.1, "a black frame proves nothing"


def test_the_cases_are_the_ones_asked_for():
    for name, (scene, w, h, kw) in X.CASES.items():
        assert w <= 96 and h <= 64 and len(X.scene(scene)[0]) <= 2000, name
    assert len(X.Mesh(*X.scene("many_lights")).lights) > 32
    assert {X.CASES[n][3]["bounces"] for n in ("cornell_b0", "cornell_b1", "cornell_b3", "cornell_b8")} == {0, 1, 3, 8}
    assert X.CASES["cornell_b2_spp4"][3]["spp"] == 4 and X.CASES["cornell_b2_spp5"][3]["spp"] == 5
    assert X.CASES["surfaces"][3]["bounces"] == 6 and X.scene("surfaces")[3].any()


def test_the_constants_are_under_the_bar():
    assert 0 < X.EPS_RGB <= 1e-4
    assert all(0 < g < 16 for k, g in X.GUARDS.items() if k != "pick") and 0 < X.GUARD_PICK < 1e-6
    assert X.REJECT * X.EPS_RGB < 0.01


def test_every_wrong_reading_is_listed():
    assert {w for w, _ in MUTATIONS + INDISTINGUISHABLE} == set(X.WRONG)


@pytest.mark.parametrize("wrong,name", MUTATIONS)
def test_a_wrong_reading_is_rejected(frames, wrong, name):
    rgb, counts = frames(name)
    _, mesh, fr = X.case(name)
    exp = X.expected(mesh, fr, wrong=wrong)
    share = X.rejected_share(rgb, exp)
    print(f"{wrong} on {name}: {share:.1%} of the pixels outside {X.REJECT:.0f} EPS_RGB; {X.WRONG[wrong]}")
    assert share > X.CAP_AMBIGUOUS, f"the oracle's frame passes for the reading '{X.WRONG[wrong]}'"
    with pytest.raises(AssertionError):
        X.check_frame(rgb, exp)


@pytest.mark.parametrize("wrong,name", INDISTINGUISHABLE)
def test_an_indistinguishable_reading_is_reported(frames, wrong, name):
    """These move nothing: the reading cannot be told from the specification's on any frame, which is stated, not passed over."""
    _, mesh, fr = X.case(name)
    exp, right = X.expected(mesh, fr, wrong=wrong), X.case_expected(name)
    moved = float(np.abs(exp["rgb"] - right["rgb"]).max() / (1.0 + np.abs(right["rgb"]).max()))
    print(f"{wrong} on {name}: moves the reference by {moved:.3g}")
    assert moved < 1e-12
    assert all(exp[k] == right[k] for k in X.COUNTS)
    X.check_frame(frames(name)[0], exp)


def test_a_frame_of_another_seed_or_offset_is_rejected(frames):
    """The power checks the GPU tests make on the kernels' frames, here on the oracle's.  Another seed is another frame; an offset of
    2e-3 instead of 1e-3 moves every lit pixel by a few parts in 10^4, several EPS_RGB, and only a few by 100 EPS_RGB."""
    s, mesh, fr = X.case("cornell_b1")
    exp = X.case_expected("cornell_b1")
    kw = dict(X.CASES["cornell_b1"][3])
    for change, factor in ((dict(seed=kw["seed"] + 1), X.REJECT), (dict(ray_eps=2e-3), 1.0)):
        other = X.Frame(fr.w, fr.h, **dict(kw, **change))
        rgb, _ = X.oracle_frame(s, other)
        share = X.rejected_share(rgb, exp, factor)
        print(change, f"{share:.1%} of the pixels outside {factor:.0f} EPS_RGB")
        assert share > X.CAP_AMBIGUOUS, change  # more pixels than a case may leave out
        with pytest.raises(AssertionError):
            X.check_frame(rgb, exp)
