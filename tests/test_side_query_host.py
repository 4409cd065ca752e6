"""CPU tests of the inside/outside query (rt_query_sides_device / rt_query_signed_distance_device, Renderer.query_sides /
query_signed_distance): the boundary (exports, bindings, NULL contexts, struct layouts, defaults, the wrappers'
refusals), and the arithmetic of csrc/ray_parity.h through the native reference tests/native/side_query_ref.cpp - clean under ASan +
UBSan; its BVH8 walk with the kernels' slab test counts the crossings its brute force counts on every family and mesh (tree
independence: no GPU needed); its restated triangle test returns the oracle's brute-force closest hits bit for bit; the majority of
three parities satisfies the float64 contract of tests/sign_exact.py where one parity alone fails it.  The kernel itself is tested on
the GPU (tests/test_gpu_side_query.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_boundary as AB
import ray_exact as RX
import sign_exact as SX
import raytracing_engine_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rt_default_side_query_params", "rt_query_sides_device", "rt_query_signed_distance_device", "rt_get_side_query_stats")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS, methods=("query_sides", "query_signed_distance", "side_query_stats"), params="SideQueryParams", stats="SideQueryStats",
               params_c="rt_side_query_params", stats_c="rt_side_query_stats", params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
               stats_fields=["points", "invalid_points", "skipped_points", "walks", "third_walks", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
               default="rt_default_side_query_params",
               null_calls=(("rt_query_sides_device", (None, 0, None, None, None, None)),
                           ("rt_query_sides_device", (V, 1, C.byref(R.SideQueryParams()), V, V, V)),
                           ("rt_query_signed_distance_device", (None, None, 0, None, None, None, None, None, None)),
                           ("rt_query_signed_distance_device", (V, V, 1, C.byref(R.PointQueryParams()), C.byref(R.SideQueryParams()), V, V, V, V)),
                           ("rt_get_side_query_stats", (C.byref(R.SideQueryStats()),)), ("rt_default_side_query_params", ())))
ALL = SX.CLOSED + SX.OPEN


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    AB.struct_layout(KIND, tmp_path)


def test_default_params_are_zeros():
    AB.default_params(KIND)


def test_the_wrappers_check_their_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    for bad in (a, good, good.double(), torch.zeros(3, 4).t(), torch.zeros(4, 4)):
        for call in (r.query_sides, r.query_signed_distance, lambda x: r.query_sides(x, want_crossings=True), lambda x: r.query_signed_distance(x, want_points=False)):
            with pytest.raises(ValueError):
                call(bad)


def test_the_wrappers_compare_lengths_and_shapes():
    """The refusals past the device check (a renderer that takes CPU tensors for its device's)."""
    torch = pytest.importorskip("torch")

    r = AB.cpu_renderer()
    p = torch.zeros(4, 3)
    i, x = torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32)
    d, c = torch.zeros(4), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="points"):
        r.query_sides(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="inside"):
        r.query_sides(p, out=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="inside"):
        r.query_sides(p, out=d)  # float32 where int32 is due
    with pytest.raises(ValueError, match="out"):
        r.query_sides(p, out=(i, x))  # a pair without want_crossings
    with pytest.raises(ValueError, match="out"):
        r.query_sides(p, out=i, want_crossings=True)
    with pytest.raises(ValueError, match="crossings"):
        r.query_sides(p, out=(i, torch.zeros(4, 2, dtype=torch.int32)), want_crossings=True)
    with pytest.raises(ValueError, match="crossings"):
        r.query_sides(p, out=(i, torch.zeros(5, 3, dtype=torch.int32)), want_crossings=True)
    with pytest.raises(ValueError, match="crossings"):
        r.query_sides(p, out=(i, c), want_crossings=True)
    with pytest.raises(TypeError, match="query_sides"):
        r.query_sides(p, tune_nothing=1)
    for bad_rmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1)):
        with pytest.raises(ValueError, match="rmax"):
            r.query_signed_distance(p, rmax=bad_rmax)
    with pytest.raises(ValueError, match="out"):
        r.query_signed_distance(p, out=(d, i))  # want_points=True fills three
    with pytest.raises(ValueError, match="out"):
        r.query_signed_distance(p, out=(d, i, c), want_points=False)
    with pytest.raises(ValueError, match="sdist"):
        r.query_signed_distance(p, out=(torch.zeros(5), i, c))
    with pytest.raises(ValueError, match="tri"):
        r.query_signed_distance(p, out=(d, torch.zeros(4), c))
    with pytest.raises(ValueError, match="point"):
        r.query_signed_distance(p, out=(d, i, torch.zeros(5, 3)))
    with pytest.raises(TypeError, match="query_signed_distance"):
        r.query_signed_distance(p, count_traversal=True)  # each step has its own switch in C; the wrapper exposes the tuning only
    # the old methods accept and refuse what they did
    with pytest.raises(TypeError, match=r"query_points\(\) got an unexpected keyword argument 'tune_nothing'"):
        r.query_points(p, tune_nothing=1)


# ---- the native reference ------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.view(np.uint32).tolist() == b.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist() == b.tolist()


def test_the_meshes_are_what_they_are_called():
    for name in SX.CLOSED:
        v = SX.mesh(name)
        assert SX.is_closed(v) and 700 <= len(v) <= 2000, (name, len(v))
    for name in SX.OPEN:
        assert not SX.is_closed(SX.mesh(name))
    # the directions: no small component, pairwise |cos| <= 0.6, unit length to the digits given
    d = SX.D.astype(np.float64)
    assert (np.abs(d) >= 0.3).all() and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-4)
    assert all(abs(d[i] @ d[j]) <= 0.6 for i in range(3) for j in range(i))


def test_the_reference_is_clean_under_sanitizers():
    """ASan + UBSan build of the stand-alone program on a slice of every family of every mesh, invalid points and a ray file included;
    its answers are the plain build's."""
    for name in ALL:
        c = SX.case(name)
        p = np.concatenate([c["p"][r][-12:] for r in c["rows"].values()]).copy()  # the tails: family c's points at the reach
        p[0, 1] = np.nan
        p[1, 2] = np.inf
        p[2, 0] = np.nextafter(np.float32(32.0) * max(np.float32(1.0), np.abs(c["verts"]).max()), np.float32(np.inf))
        rays = (p[3:40], np.tile(SX.D, (13, 1))[:37])
        plain = SX.reference(c["verts"], p, rays)
        checked = SX.reference(c["verts"], p, rays, sanitized=True)
        for key in ("inside", "third", "brute", "walk", "t", "tri", "ray_t", "ray_tri"):
            assert same_bits(plain[key].ravel(), checked[key].ravel()), (name, key)
        assert (plain["nodes"], plain["tris"], plain["thirds"]) == (checked["nodes"], checked["tris"], checked["thirds"])
        assert plain["inside"][:3].tolist() == [SX.INVALID] * 3 and (plain["inside"][3:] >= 0).all()


@pytest.mark.parametrize("name", ALL)
def test_the_walk_counts_what_brute_force_counts(name):
    """Tree independence: (b), the BVH8 walk with the kernels' slab test and tmax = +inf, counts under the boxes it enters exactly the
    crossings that (a) counts over all triangles, for all three directions, on every family - family c's points at the reach limit
    too - and does prune."""
    c = SX.case(name)
    ref = c["ref"]
    assert (ref["inside"] >= 0).all()
    for f, r in c["rows"].items():
        assert np.array_equal(ref["brute"][r], ref["walk"][r]), (name, f, int((ref["brute"][r] != ref["walk"][r]).sum()))
    per_walk = ref["tris"] / (3 * len(c["p"]))
    print(f"{name}: {per_walk:.2f} triangles and {ref['nodes'] / (3 * len(c['p'])):.2f} nodes per walk; brute force {len(c['verts'])}")
    assert per_walk < len(c["verts"]) / 8


def test_the_restated_triangle_test_is_the_oracles():
    """(c): the closest accepted triangle (t, index) of csrc/ray_parity.h's test over all triangles equals the oracle's brute-force
    closest_hit bit for bit - along the three directions from family a on every mesh, and on ray_exact's families a - c (aimed at
    interiors, edges and vertices from arbitrary directions)."""
    import oracle as O

    for name in ALL:
        c = SX.case(name)
        p = c["p"][c["rows"]["a"]]
        sc = O.TriScene(*RX._with_surface(c["verts"]))
        for k in range(3):
            t, tri, _ = RX.oracle_answers(sc, p, np.broadcast_to(SX.D[k], p.shape), None, use_bvh=False)
            assert same_bits(c["ref"]["t"][c["rows"]["a"], k], t) and c["ref"]["tri"][c["rows"]["a"], k].tolist() == tri.tolist(), (name, k)
        assert (c["ref"]["tri"][c["rows"]["a"]] >= 0).any() or name in SX.OPEN
    hits = 0
    for fam in ("a", "b", "c"):
        for part in RX.family(fam, 600):
            want = RX.part_reference(part)
            got = SX.reference(RX.mesh(part["mesh"])[0], np.zeros((0, 3), np.float32), rays=(part["o"], part["d"]))
            assert same_bits(got["ray_t"], want["t"]) and got["ray_tri"].tolist() == want["tri"].tolist(), (fam, part["mesh"])
            hits += int((want["tri"] >= 0).sum())
    assert hits > 900


def test_the_lazy_rule_is_the_majority(tmp_path):
    """par0 == par1 ? par0 : par2 against the 2-of-3 majority on all eight parity triples (and on counts, whose low bit is the parity),
    straight from csrc/ray_parity.h; and on every point of every case."""
    prog = tmp_path / "lazy.cpp"
    prog.write_text("#include <cstdio>\n#include \"ray_parity.h\"\nint main() {\n    for (unsigned a = 0; a < 4; a++) for (unsigned b = 0; b < 4; b++) for (unsigned c = 0; c < 4; c++)\n"
                    "        std::printf(\"%u %u %u %u %d\\n\", a, b, c, rt::side_of_parities(a, b, c), (int)rt::needs_third_parity(a, b));\n    return 0;\n}\n")
    exe = tmp_path / "lazy"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "raytracing_engine_amd", "csrc"), str(prog), "-o", str(exe)], check=True)
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(rows) == 64 and {(a & 1, b & 1, c & 1) for a, b, c, _, _ in rows} == {(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    for a, b, c, side, third in rows:
        assert side == int((a & 1) + (b & 1) + (c & 1) >= 2), (a, b, c)
        assert third == int((a & 1) != (b & 1))
    for name in ALL:
        ref = SX.case(name)["ref"]
        par = ref["brute"] & 1
        assert np.array_equal(ref["inside"], (par.sum(1) >= 2).astype(np.int32)), name
        assert np.array_equal(ref["third"], (par[:, 0] != par[:, 1]).astype(np.int32)) and ref["thirds"] == int(ref["third"].sum())


@pytest.mark.parametrize("name", SX.CLOSED)
def test_the_majority_satisfies_the_contract_where_one_ray_fails_it(name):
    """The contract: outside the distance band (which no family enters: share 0) and outside the two-rays-near-an-edge exclusion (at
    most 0.1 % per family; 0 expected) the majority of three parities is the exact winding number's answer for every point.  The
    power: direction k alone is wrong for at least 5 % of the families aimed along it, and for no point of the others."""
    c, ex = SX.case(name), SX.exact_case(name)
    ref = c["ref"]
    assert ex["frac"] < 2e-6  # the winding number is an integer there, as far as float64 tells
    both = set(ex["inside"][c["rows"]["a"]].tolist()) | set(ex["inside"][c["rows"]["b"]].tolist())
    assert both == {0, 1}
    verdict = SX.judge(name, ref["inside"])
    print(name, "majority (wrong, in the distance band, two rays near an edge, points):", verdict, "thirds:", {f: int(ref["third"][r].sum()) for f, r in c["rows"].items()})
    for f, (wrong, band, two, n) in verdict.items():
        assert band == 0, (name, f, band)
        assert two <= n // 1000, (name, f, two)
        assert wrong == 0, (name, f, wrong)
    for k in range(3):
        single = SX.judge(name, ref["brute"][:, k] & 1)
        print(name, f"direction {k} alone, wrong:", {f: v[0] for f, v in single.items()})
        for f, (wrong, _, _, n) in single.items():
            if f in ("d%d" % k, "e%d" % k):
                assert wrong >= n // 20, (name, k, f, wrong)
            else:
                assert wrong == 0, (name, k, f, wrong)
    # the third walk is needed where the first two rays are aimed, and nowhere else
    for f, r in c["rows"].items():
        assert (ref["third"][r].sum() > 0) == (f in ("d0", "e0", "d1", "e1")), (name, f)


def test_the_cavity_of_the_shell_is_outside():
    v = SX.mesh("shell")
    p = np.array([[0.02, 0.1, -0.04], [0.9, 0.0, 0.0], [3.0, 0.0, 0.0]], np.float32)  # in the cavity, between the spheres, outside both
    assert SX.exact_inside(v, p)[0].tolist() == [0, 1, 0]
    assert SX.reference(v, p)["inside"].tolist() == [0, 1, 0]
