"""CPU tests of the test reference for mirror and glass surfaces on path B (tests/native/pt_surfaces_ref.c).

The reference reuses oracle B's closest hit, occlusion, RNG and cosine lobe and restates only the camera ray and the path loop
with surfaces.  It is pinned here: with every triangle Lambert it IS oracle B (bit for bit, equal ray counts); mirrors and
glass give analytic known answers; its Fresnel and refraction helpers obey the physics they stand for.  The GPU kernels are
checked against it in tests/test_gpu_surfaces.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle as O
from raytracing_engine_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native", "pt_surfaces_ref.c")
LAMBERT, MIRROR, GLASS = scenes.SURFACE_LAMBERT, scenes.SURFACE_MIRROR, scenes.SURFACE_GLASS
f32 = np.float32
_REF = None


def ref_lib():
    """Compile the reference with oracle B's arithmetic flags against oracle/_build/liboracle.so (once per process)."""
    global _REF
    if _REF is None:
        so = O.build()
        O.lib()  # loaded first: the reference's orb_* symbols resolve against this copy
        out = os.path.join(tempfile.mkdtemp(prefix="pt_surfaces_ref_"), "libpt_surfaces_ref.so")
        odir = os.path.dirname(so)
        subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2", "-fopenmp",
                        "-Wall", "-Wextra", "-o", out, NATIVE, "-L" + odir, "-loracle", "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(out)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        L.prs_scene_create.argtypes = [fp, fp, fp, u32p, fp, C.c_uint32]
        L.prs_scene_create.restype = C.c_void_p
        L.prs_scene_destroy.argtypes = [C.c_void_p]
        L.prs_render_rows.argtypes = [C.c_void_p, C.POINTER(O.PtParams), C.c_uint32, C.c_uint32, fp, C.POINTER(C.c_uint64), C.c_int]
        L.prs_render_rows.restype = C.c_int
        L.prs_fresnel.argtypes = [C.c_float, C.c_float]
        L.prs_fresnel.restype = C.c_float
        L.prs_delta_dir.argtypes = [fp, fp, C.c_float, C.c_int, C.c_float, fp, C.POINTER(C.c_int)]
        _REF = L
    return _REF


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class SurfRef:
    """A mesh with surfaces in the test reference; render() mirrors oracle.TriScene.render."""

    def __init__(self, verts, albedo, emission, kind=None, ior=None):
        L = ref_lib()
        self.verts = np.ascontiguousarray(verts, f32).reshape(-1, 9)
        self.albedo = np.ascontiguousarray(albedo, f32).reshape(-1, 3)
        self.emission = np.ascontiguousarray(emission, f32).reshape(-1, 3)
        n = len(self.verts)
        self.kind = None if kind is None else np.ascontiguousarray(kind, np.uint32)
        self.ior = np.ascontiguousarray(np.ones(n, f32) if ior is None else ior, f32)
        assert self.albedo.shape[0] == n == self.emission.shape[0] == len(self.ior) and (self.kind is None or len(self.kind) == n)
        kp = None if self.kind is None else self.kind.ctypes.data_as(C.POINTER(C.c_uint32))
        self._h = L.prs_scene_create(_fp(self.verts), _fp(self.albedo), _fp(self.emission), kp, _fp(self.ior), n)
        if not self._h:
            raise RuntimeError("prs_scene_create failed")

    def __del__(self):
        if getattr(self, "_h", None):
            ref_lib().prs_scene_destroy(self._h)
            self._h = None

    def render(self, width, height, spp=1, bounces=1, seed=1, rot=(0, 0, 0, 1), pos=(0, 0, 0), ratio=None, sky=(0.0, 0.0, 0.0),
               ray_eps=1e-3, threads=0, rows=None):
        p = O.PtParams()
        p.width, p.height, p.spp, p.bounces, p.seed = width, height, spp, bounces, seed
        if ratio is None:
            ratio = (1.0, f32(1.0) * f32(height) / f32(width))
        p.ratio[:] = [float(f32(x)) for x in ratio]
        p.rot[:] = [float(f32(x)) for x in rot]
        p.pos[:] = [float(f32(x)) for x in pos]
        p.sky[:] = [float(f32(x)) for x in sky]
        p.ray_eps = ray_eps
        row0, row1 = rows if rows is not None else (0, height)
        rgb = np.zeros((row1 - row0, width, 3), f32)
        ct = (C.c_uint64 * 3)()
        if ref_lib().prs_render_rows(self._h, C.byref(p), row0, row1, _fp(rgb), ct, threads):
            raise RuntimeError("prs_render_rows failed")
        return rgb, {"camera_rays": int(ct[0]), "bounce_rays": int(ct[1]), "shadow_rays": int(ct[2])}


def fresnel(c, eta):
    return float(ref_lib().prs_fresnel(c, eta))


def delta_dir(d, n, w, flipped, u):
    d_, n_ = np.ascontiguousarray(d, f32), np.ascontiguousarray(n, f32)
    out, below = np.zeros(3, f32), C.c_int()
    ref_lib().prs_delta_dir(_fp(d_), _fp(n_), w, int(flipped), u, _fp(out), C.byref(below))
    return out, bool(below.value)


def quad(p0, p1, p2, p3):
    p = [np.asarray(x, f32) for x in (p0, p1, p2, p3)]
    return [np.concatenate([p[0], p[1], p[2]]), np.concatenate([p[0], p[2], p[3]])]


def wall(y, half, albedo, emission=(0, 0, 0)):
    """A square of two triangles in the plane y = const, x and z in [-half, half]."""
    v = np.array(quad((-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)), f32)
    return v, np.tile(np.asarray(albedo, f32), (2, 1)), np.tile(np.asarray(emission, f32), (2, 1))


def join(*meshes):
    return tuple(np.concatenate([m[k] for m in meshes]) for k in range(3))


# ---- all Lambert: the reference is oracle B --------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["cornell", "soup2k"])
def test_all_lambert_equals_oracle_b(which):
    if which == "cornell":
        mesh, w, h, view = scenes.cornell_tri_scene(), 48, 32, dict(pos=(0, 1, 0))
    else:
        mesh, w, h, view = scenes.soup_scene(2000, seed=2), 64, 36, dict(sky=(0.2, 0.2, 0.25))
    oracle = O.TriScene(*mesh)
    n = len(mesh[0])
    refs = [SurfRef(*mesh), SurfRef(*mesh, kind=np.zeros(n, np.uint32))]
    for bounces in (0, 1, 3):
        for spp in (1, 4):
            for seed in (1, 7):
                want, wct = oracle.render(w, h, spp=spp, bounces=bounces, seed=seed, **view)
                for ref in refs:
                    got, ct = ref.render(w, h, spp=spp, bounces=bounces, seed=seed, **view)
                    assert np.array_equal(got, want), (which, bounces, spp, seed)
                    assert ct == {k: wct[k] for k in ("camera_rays", "bounce_rays", "shadow_rays")}


# ---- known answers ----------------------------------------------------------------------------------------------------------

def test_mirror_filling_the_view_reflects_the_sky():
    alb, sky = (0.8, 0.5, 0.25), (0.3, 0.6, 0.9)
    mesh = wall(5.0, 100.0, alb)
    ref = SurfRef(*mesh, kind=[MIRROR, MIRROR])
    want = (np.asarray(alb, f32) * np.asarray(sky, f32)).astype(f32)
    for spp in (1, 2):
        rgb, ct = ref.render(24, 16, spp=spp, bounces=1, sky=sky)
        assert (rgb == want).all()
        assert ct == {"camera_rays": 24 * 16 * spp, "bounce_rays": 24 * 16 * spp, "shadow_rays": 0}
    rgb, ct = ref.render(24, 16, spp=2, bounces=0, sky=sky)  # the path ends at the mirror: nothing is added
    assert (rgb == 0).all() and ct["bounce_rays"] == 0


def test_clear_glass_pane_passes_the_sky():
    sky = (0.3, 0.6, 0.9)
    mesh = wall(5.0, 100.0, (1, 1, 1))
    ref = SurfRef(*mesh, kind=[GLASS, GLASS], ior=[1.5, 1.5])
    for spp in (1, 2, 4):
        rgb, _ = ref.render(24, 16, spp=spp, bounces=2, seed=3, sky=sky)
        assert (rgb == np.asarray(sky, f32)).all()
    rgb, _ = ref.render(24, 16, spp=2, bounces=0, sky=sky)
    assert (rgb == 0).all()


def test_light_seen_in_a_mirror():
    """A small mirror straight ahead and a large light behind the camera: the pixels that see the mirror see the light."""
    alb, le = (0.9, 0.6, 0.3), (5.0, 7.0, 11.0)
    mirror = wall(5.0, 1.0, alb)
    light = wall(-5.0, 100.0, (0, 0, 0), le)
    ref = SurfRef(*join(mirror, light), kind=[MIRROR, MIRROR, LAMBERT, LAMBERT])
    rgb, _ = ref.render(32, 32, spp=2, bounces=1, ratio=(1, 1))
    want = (np.asarray(alb, f32) * np.asarray(le, f32)).astype(f32)
    assert (rgb[13:19, 13:19] == want).all()  # |ndc| < 0.2 for every jitter: inside the mirror's silhouette
    assert (rgb[:4] == 0).all()
    rgb, _ = ref.render(32, 32, spp=2, bounces=0, ratio=(1, 1))
    assert (rgb == 0).all()


# ---- Fresnel and refraction ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", [1.0, 1.33, 1.5, 2.4, 4.0])
def test_fresnel_normal_incidence_and_grazing(eta):
    assert fresnel(1.0, 1.0 / eta) == pytest.approx(((eta - 1) / (eta + 1)) ** 2, rel=1e-5, abs=1e-7)
    assert fresnel(1.0, eta) == pytest.approx(((eta - 1) / (eta + 1)) ** 2, rel=1e-5, abs=1e-7)
    cs = np.linspace(1.0, 0.0, 201, dtype=f32)
    F = np.array([fresnel(float(c), 1.0 / eta) for c in cs])
    if eta > 1:  # entering: from Brewster's angle on (rp = 0 there) F rises monotonically to 1 at grazing incidence
        beyond = cs <= 1 / np.sqrt(1 + eta * eta)
        assert (np.diff(F[beyond]) > 0).all() and (F[beyond] > F[0] - 0.05).all()
    assert F[-1] == 1.0


@pytest.mark.parametrize("eta", [1.33, 1.5, 2.4])
def test_fresnel_reciprocity_and_total_internal_reflection(eta):
    for ci in np.linspace(0.05, 1.0, 40):
        ct = np.sqrt(1 - (1 / eta) ** 2 * (1 - ci * ci))
        # within rounding: fp32 inputs; dF/dcos grows like 1/cos towards grazing incidence
        assert fresnel(float(ci), 1 / eta) == pytest.approx(fresnel(float(ct), eta), abs=1e-6 / ci)
    crit = np.sqrt(1 - 1 / eta ** 2)  # cos of arcsin(1/eta)
    for ci in np.linspace(0.0, crit * 0.999, 20):  # inside the glass beyond the critical angle: everything is reflected
        assert fresnel(float(ci), eta) == 1.0
        d = np.array([np.sqrt(1 - ci * ci), 0.0, -ci], f32)
        out, below = delta_dir(d, (0, 0, 1), eta, True, 0.999999)
        assert not below
        np.testing.assert_allclose(out, [d[0], 0, ci], atol=1e-6)
    assert fresnel(float(crit * 1.01), eta) < 1.0


@pytest.mark.parametrize("eta", [1.33, 1.5, 2.4])
def test_refracted_direction_obeys_snell(eta):
    rng = np.random.default_rng(5)
    n = np.array([0.0, 0.0, 1.0], f32)
    for _ in range(200):
        d = rng.normal(size=3)
        d[2] = -abs(d[2]) - 0.05
        d = (d / np.linalg.norm(d)).astype(f32)
        for flipped, eta_r in ((False, 1 / eta), (True, eta)):
            ci = -float(d[2])
            si = np.sqrt(max(0.0, 1 - ci * ci))
            if eta_r * si >= 0.999:
                continue
            t, below = delta_dir(d, n, eta, flipped, 0.999999)
            assert below
            assert abs(np.linalg.norm(t.astype(np.float64)) - 1) <= 1e-6
            assert t[2] < 0
            st = np.linalg.norm(np.cross(t.astype(np.float64), n))
            assert st == pytest.approx(eta_r * si, rel=2e-5, abs=1e-6)
        r, below = delta_dir(d, n, -1.0, False, 0.0)  # mirror
        assert not below
        np.testing.assert_allclose(r, [d[0], d[1], -d[2]], atol=1e-6)


# ---- scenes ---------------------------------------------------------------------------------------------------------------

def test_cornell_surfaces_glass_box_is_wound_outward():
    v, a, e, kind, ior = scenes.cornell_surfaces_scene()
    assert len(v) == len(kind) == len(ior) == 38
    assert (kind[14:26] == MIRROR).all() and (kind[26:38] == GLASS).all() and (kind[:14] == LAMBERT).all()
    assert (ior[26:38] == f32(1.5)).all() and (a[26:38] == 1).all()
    for box in (slice(14, 26), slice(26, 38)):
        t = v[box].reshape(-1, 3, 3).astype(np.float64)
        centre = t.reshape(-1, 3).mean(0)
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        assert (np.einsum("ij,ij->i", nrm, t.mean(1) - centre) > 0).all()


def test_soup_surfaces_fractions():
    kind, ior = scenes.soup_surfaces(100000, seed=1, mirror_frac=0.1, glass_frac=0.2, ior=1.7)
    assert kind.dtype == np.uint32 and ior.dtype == f32 and (ior == f32(1.7)).all()
    assert abs((kind == MIRROR).mean() - 0.1) < 0.01 and abs((kind == GLASS).mean() - 0.2) < 0.01
    assert (kind[-2:] == LAMBERT).all()
    assert np.array_equal(kind, scenes.soup_surfaces(100000, seed=1, mirror_frac=0.1, glass_frac=0.2, ior=1.7)[0])
    assert not np.array_equal(kind, scenes.soup_surfaces(100000, seed=2, mirror_frac=0.1, glass_frac=0.2)[0])


def test_surfaces_change_the_frame():
    """The surfaces of cornell_surfaces_scene are visible: the frame differs from the all-Lambert one, and a mirror box seen
    from the camera reflects light (the reference adds emission behind delta vertices)."""
    v, a, e, kind, ior = scenes.cornell_surfaces_scene()
    lam, _ = SurfRef(v, a, e).render(48, 32, spp=2, bounces=3, pos=(0, 1, 0))
    srf, ct = SurfRef(v, a, e, kind, ior).render(48, 32, spp=2, bounces=3, pos=(0, 1, 0))
    assert not np.array_equal(lam, srf) and np.isfinite(srf).all() and (srf >= 0).all()
    assert ct["bounce_rays"] > 0
