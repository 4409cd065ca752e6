"""Closed-form float64 sphere geometry that path A's depth pyramid and shading are held to, with none of the march loops.

Test helper (imported by tests/test_path_a_exact_host.py and tests/test_gpu_path_a_exact.py); not a conftest, no fixtures.
numpy float64 only: nothing from `oracle`, nothing from librt_amd at module level.  Written from the specification (include/rt_abi.h,
oracle/oracle.h, DESIGN.md sections 4-5), not from oracle_a.c / path_a.hip, which mirror each other line by line and would share any
misreading.  It covers the reference as shipped (march algorithm 3, 1 spp, jitter 0), multi-sample frames (every sample a full frame
with its own jitter, averaged in sample order), march algorithm 1, and the mirror and transmission chains (CHAINS below); no repeat(),
no algorithm 2, no camera inside a sphere under algorithm 1 or with chains.
There is no stepping loop over a ray anywhere in this file: the scene is at most 8 spheres, so what the marches approximate has a
closed form, and what they leave open (WHERE a march samples) is held in an interval.

DEPTH, depth_bands(frame, i).  Texel (gx, gy) of level i looks along u = normalize(rotate(rot, ((2gx+1) isx - 1) ratio_x, 1,
((2gy+1) isy - 1) ratio_y)), isx, isy = 2^(count-1-i) / view, starts at o = pos + len0 u with len0 = 1 at level 0 and the frame's OWN
parent texel (gx>>1, gy>>1) above, and marches the relative distance t >= 0 with f(t) = min_k |o + t u - c_k| - r_k against the cone
radius rho(t) = (t + 1) tau, tau = sqrt2 * 8 * isx (x only; relative t, both as the reference has them).  The cached distances of
algorithm 3 are lower bounds of a 1-Lipschitz function and a cached value at or below the radius is refreshed, hence exact, so:
    the march stops at the first SAMPLED s with f(s) <= rho(s), it never steps across a surface (f >= 0 on [0, s)), and returns
    max(len0 + g(s), 0),  g(s) = s + max(f(s), 0) - rho(s);   otherwise it runs out at a relative length >= render_dist.
Where it samples is not decided here.  Per sphere {t : f_k <= rho} is one quadratic, (1 - tau^2) t^2 + 2 (oc.u - tau (r + tau)) t
+ |oc|^2 - (r + tau)^2 <= 0; the feasible set F is the union of those touch sets cut at the first surface crossing a (the usual
ray/sphere root; 0 when o is inside a sphere) and at render_dist.  The band is [len0 + min_F g, len0 + max_F g], clamped at 0: g is
sampled at N_SAMPLE points of every interval of F and widened by its Lipschitz constant (2 + tau) times half the spacing, and cut by
two closed forms that hold on any interval I of sphere k: g >= s - rho(s) (linear) and g <= s - rho(s) + max(f_k(s), 0) (convex, so
its maximum is at an end of I).  A texel is right when
    it reports a hit (< render_dist) and lies in the band;  or it reports a miss (>= render_dist) and either lies in the band or the
    centre line crosses no surface before render_dist AND the value is >= len0 + render_dist (a march that ran out);
so an empty F forces a miss, a crossed surface forbids one, and a grazing ray whose cone touches while its centre line misses may
report either.  In every tested scene a texel whose parent missed stays a miss (`far_bad` counts the others); the tests assert that too.

ALGORITHM 1 (Frame(march_algorithm=1); oracle.h, rt_abi.h: every SDF every step, the radius taken AFTER the step).  The march samples
s_0 = 0, s_{j+1} = s_j + f(s_j), so it never crosses a surface either, stops at the first sampled s with f(s) <= (s + f(s) + 1) tau and
returns max(len0 + g1(s), 0), g1(s) = (s + f(s)) (1 - tau) - tau.  For tau < 1 the stop condition is f(s) <= (s + 1) tau', tau' = tau /
(1 - tau): the touch sets are the same quadratic with tau' for tau, cut the same way, g1 has the Lipschitz constant 2 (1 - tau), and the
two closed forms are g1 with 0 and with max(f_k, 0) for f.  For tau >= 1 (level 0 of 17 x 9) f(0) (1 - tau) <= 0 <= tau: the first sample
stops the march and the band is the one point len0 + f(0) (1 - tau) - tau, clamped at 0.  The miss rules are the same; so is the colour,
which only reads the finest level.  A camera inside a sphere is not covered under algorithm 1.

SAMPLES.  Sample s of spp = n x n adds the fp32 offset sample_jitter(s, spp, w, h) = ((2i + 1) / n - 1) / view, i = s % n in x and s // n
in y, to the normalised coordinates of every level's texels and of the pixel, BEFORE the ratio (rays()).  check_samples(frames, rgb):
every level of every sample in the bands of its own jitter; per pixel the average lies in [sum lo_s, sum hi_s] / spp, a sample that
missed adding exactly 0; a pixel is left out when one of its hit samples is ambiguous, pinned when all of them are, and exactly black
when every sample missed.

COLOUR, shade_bands(frame).  Pixel (px, py) with own finest-level depth d < render_dist: step through ((px + 0.5) 2 / view - 1) ratio,
P = pos + d step, nearest sphere by strict '<' (first wins), then DESIGN.md section 5's formula in float64: cam_fall, normal,
normal_fall, per light light_dir, light_dist, light_fall, diffuse, reflect, pow (0 for a base <= 0).  Where the two smallest SDFs at P
differ by less than AMBIGUOUS the pixel is ambiguous and left out.  The shadow factor is not marched.  The shadow march walks
o' = P + light_dir along light_dir over t in [0, end), end = light_dist (THE CAP: every sampled value is min(end, f), which a reader
of the formula alone gets wrong for a light nearer than 1 to open space), always samples t = 0, exactly, and steps by at most
f + ray_radius.  So with m* = min of f over the segment (per sphere the closest approach clamped to the segment) and f0 = f(0):
    min(end, f0) <= ray_radius                                            soft = 0    (the first sample already stops it)
    the segment crosses a surface at some a <= end - 2 ray_radius         soft = 0    (a sample lands in [a, a + ray_radius], f <= ray_radius)
    otherwise   soft in [lo, hi],  hi = min(1, end, max(f0, 0)),  lo = min(m*, end, 1) if m* > ray_radius else 0.
RGB is monotone in every soft, so the pixel lies between RGB(lo) and RGB(hi) component-wise; it is PINNED when that interval is
narrower than PINNED_WIDTH (every light blocked, or its minimum attained at t = 0, or >= end or 1).

THE CONSTANTS are measured on the CPU against oracle A, never on a GPU frame:  python tests/path_a_exact.py  renders every frame of
the two test files (FRAMES, ALG1_FRAMES, SAMPLE_FRAMES and the GPU_ONLY lists below; multi-sample frames per sample and averaged) with
the oracle and prints, with no tolerance at all, the largest distance of an oracle texel / pixel outside its band.  Measured by that command:
    depth, relative to 1 + depth:  5.922e-07  (room_turned 96 x 64, algorithm 1, finest level: its bands are narrow next to a wall of radius
                                               50, where the fp32 |p - c| - r is a few ulps of 50 off; algorithm 3 alone: 3.109e-07, room_turned
                                               200 x 120; jittered samples: 2.57e-07)
    rgb:                           9.342e-06  (random_8_8 96 x 64 under algorithm 1: shine 30, eight lights; algorithm 3: 5.471e-06; one
                                               jittered sample: 6.73e-06, same scene; an averaged frame: 2.48e-06)
Constants = four times the measurement, to cover powf and the fp32 position the kernels shade at:
    EPS_DEPTH = 2.369e-06      EPS_RGB = 3.737e-05   (under the project's 1e-5 / 1e-4 bars)
A roll by one texel, a depth moved by one cone radius, a wrong parent, swapped materials, a dropped light or exchanged fall-offs move
a frame by 1e-2 and more (tests/test_path_a_exact_host.py shows each rejected), so the margin costs no power.
Shares of the hit pixels, same command: ambiguous 0 - 0.37 %; pinned 57 - 100 % in the open scenes and 24 - 49 % in the room; median
width of the room's RGB intervals 0.0004 - 0.045.  Averaged frames (4, 9, 16 spp; shares of the pixels some sample hit): ambiguous
0 - 0.68 % (17 x 9) and <= 0.38 % elsewhere, every hit sample pinned 53 - 94 % (open) and 24 - 33 % (rooms), room median width 0.012 - 0.0451.
Algorithm 1: ambiguous <= 0.37 %, pinned 55 - 100 % / 25 - 31 %, room median width 0.017 - 0.047.

CHAINS, chain_bands(frame) (rt_config.reflections / transmissions in include/rt_abi.h, ora_config in oracle/oracle.h).  A chain cannot
be judged end to end from the primary depth: an fp32 rounding of 1e-6 in a hit point on a sphere of radius r is 2 L / r times that in
the next hit.  The frame therefore carries what every secondary march did (Frame.chains: rt_render_chains / ora_render_a_chains;
(h, w, reflections + transmissions, 7) = eye[3], dir[3], len per possible march, mirror bounces first, NaN where none ran), and every
link is computed from the RECORDED values of the link before it, so nothing is carried across links.  For every hit pixel, from the
frame's own depth: step, P0 = pos + d step, nearest sphere, n0.
    mirror bounce j:   H_{j-1} = eye_{j-1} + dir_{j-1} max(len_{j-1}, 0)  (H_{-1} = P0, dir_{-1} = step); its nearest sphere gives n,
        specular; expected eye_j = H_{j-1}, dir_j = reflect(dir_{j-1}, n), w_j = w_{j-1} reflectivity specular
    transmission pass j:  starts again at P0, step, w = 1; T = I or normalize(refract(I, n, 1 / index)); oc = P - c, b = oc.T,
        disc = b^2 - (oc.oc - r^2), t = max(disc > 0 ? sqrt(disc) - b : 0, 0), Q = P + T t, n2 = normalize(oc + T t), D = T or
        normalize(refract(T, -n2, index)); expected eye_j = Q, dir_j = D, w_j = w_{j-1} transparency diffuse; k < 0 or k2 < 0 ends it
    either:  len_j in ray_band(o = eye_j + dir_j, u = dir_j, len0 = 1, tau = ray_radius) under the hit / miss rules of a level texel;
        len_j < render_dist adds w_j shade_point(H_j, eye = eye_j, view = dir_j) and the chain goes on, otherwise it ends and every
        later row is NaN
The pixel's RGB interval is the primary one plus the weighted secondary ones; the NaN pattern is the walk's; reflection_rays /
transmission_rays = the non-NaN rows, shadow_rays = lightCount (hit pixels + rows with len < render_dist).  The silhouette ring where
only the cone touched the sphere is predicted, not left out: disc <= 0, t = 0, Q = P.  Left out: a shaded chain point with its two
smallest SDFs closer than AMBIGUOUS, and a branch decided inside a guard (|disc| < GUARD_DISC r^2, |k| or |k2| < GUARD_K).
Measured by the same command over CHAIN_FRAMES + GPU_ONLY_CHAIN_FRAMES (oracle A on the CPU), constants = four times:
    guards: the formula in fp32 against float64 from the same recorded inputs:  k, k2 1.697e-06 -> GUARD_K = 6.788e-06;
            disc / r^2 6.815e-07 -> GUARD_DISC = 2.726e-06;  left out 0 - 0.59 % of the hit pixels (cap 1 %)
    eye, relative to 1 + |eye|:       1.805e-07 -> EPS_CHAIN_EYE = 7.218e-07
    dir, relative to 1 + |eye| / r:   9.854e-07 -> EPS_CHAIN_DIR = 3.941e-06   (a normal is a position over a radius: half an ulp of the
                                      fp32 hit point is eps |eye| / r in dir; measured plainly 3.05e-06 on the room's radius-1 ball)
    len outside its band, / (1 + len): 1.141e-06 -> EPS_CHAIN_LEN = 4.562e-06
    rgb:                              5.104e-06 -> EPS_CHAIN_RGB = 2.042e-05
disc cancels (b^2 against oc.oc - r^2), so fp32 holds it to GUARD_DISC r^2 at best and t = sqrt(disc) - b, hence Q, only to
GUARD_DISC r^2 / (2 sqrt(disc)) (4e-5 of |Q| measured near grazing incidence); through n2 and sqrt(k2) the same reaches D near the
critical angle (1.7e-4).  Those first-order bounds are taken off the eye / dir differences before the constants apply (chain_bands,
t_allow / dir_allow); nothing is taken off for t = 0 or a straight ray, and the next link starts from the recorded values anyway.
Every case (CHAIN_CASES) gives each sphere its own diffuse and specular in (0, 1), has secondary light above 100 EPS_RGB on >= 10 % of
its hit pixels (10.9 - 98.3 %) and a march of each kind that ends by a miss.  WRONG_CHAINS are the misreadings whose references must
reject the right recordings (tests/test_path_a_exact_host.py).
"""
import sys

import numpy as np

SQRT2_8 = float(np.float32(1.4142135)) * 8.0  # compute.glsl:75 as the fp32 code holds it
N_SAMPLE = 33
AMBIGUOUS = 1e-3
PINNED_WIDTH = 1e-6
# python tests/path_a_exact.py  (see the module docstring)
EPS_DEPTH = 2.369e-06
EPS_RGB = 3.737e-05
# the chains (CHAINS in the module docstring): four times the largest excursion of oracle A's recordings over CHAIN_FRAMES + GPU_ONLY_CHAIN_FRAMES
EPS_CHAIN_EYE = 7.218e-07 # recorded eye against the expected one, relative to 1 + |eye|
EPS_CHAIN_DIR = 3.941e-06 # recorded dir against the expected one, relative to 1 + |eye| / r (the normal is a position over a radius)
EPS_CHAIN_LEN = 4.562e-06 # recorded len outside its band, relative to 1 + len
EPS_CHAIN_RGB = 2.042e-05 # RGB outside the summed interval
# A branch decided inside these widths is one fp32 cannot decide and the pixel is left out: four times the largest difference between
# the formula evaluated in fp32 and in float64 from the same recorded inputs, same command
GUARD_K = 6.788e-06       # k and k2 of the two refractions against 0
GUARD_DISC = 2.726e-06   # disc of the crossing against 0, relative to r^2
CHAIN_COVERED = 0.10    # share of a case's hit pixels that must receive a secondary contribution above 100 EPS_RGB


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def level_count(width):
    """floor(log2(width / 8)) + 1, at least 1, at most 9."""
    q = int(width) // 8
    return min(max(q.bit_length(), 1), 9)


def level_dims(width, height, count, level):
    """(w, h) of pyramid level `level`: ceil(res * 2^level / (4 << count)) * 8."""
    den = 4 << count
    return -(-(width << level) // den) * 8, -(-(height << level) // den) * 8


def parse_scene(raw):
    """The 656-byte scene -> float64 arrays of the live objects, their materials (material i belongs to object i) and lights."""
    raw = bytes(raw)
    assert len(raw) == 656
    n_mat, n_obj, n_light, _ = np.frombuffer(raw, np.uint32, 4)
    mats = np.frombuffer(raw, np.float32, 64, 16).reshape(8, 8).astype(np.float64)
    objs = np.frombuffer(raw, np.float32, 32, 16 + 256).reshape(8, 4).astype(np.float64)
    lights = np.frombuffer(raw, np.float32, 64, 16 + 256 + 128).reshape(8, 8).astype(np.float64)
    n_obj, n_light = int(n_obj), int(n_light)
    return dict(c=objs[:n_obj, :3], r=objs[:n_obj, 3], color=mats[:n_obj, :3], shine=mats[:n_obj, 5], ambient=mats[:n_obj, 6],
                diffuse=mats[:n_obj, 3], specular=mats[:n_obj, 4], lpos=lights[:n_light, :3], lcol=lights[:n_light, 4:7])


class Frame:
    """Everything the two band functions read: the scene, the view, the config scalars, and the frame's own levels and RGB."""

    def __init__(self, scene, width, height, rot=(0, 0, 0, 1), pos=(0, 0, 0), ratio=None, render_dist=1000.0, cam_fall_off=0.01,
                 light_fall_off=0.01, ray_radius=0.01, levels=None, rgb=None, jitter=(0, 0), march_algorithm=3, reflections=0, reflectivity=0.5,
                 transmissions=0, transparency=0.5, refraction_index=1.0, chains=None):
        self.scene = parse_scene(scene)
        # the chains (chain_bands): the config scalars as fp32 holds them, and the recorded marches (h, w, reflections + transmissions, 7)
        self.reflections, self.transmissions = int(reflections), int(transmissions)
        self.reflectivity, self.transparency, self.refraction_index = (float(np.float32(v)) for v in (reflectivity, transparency, refraction_index))
        self.chains = None if chains is None else np.asarray(chains, np.float64)
        if self.chains is not None:
            assert self.chains.shape == (int(height), int(width), self.reflections + self.transmissions, 7)
        self.jitter = np.asarray(jitter, np.float32).astype(np.float64)  # added to the normalised coordinates, before the ratio
        assert march_algorithm in (1, 3)
        self.alg = int(march_algorithm)
        self.w, self.h = int(width), int(height)
        f32 = np.float32
        if ratio is None:
            ratio = (1.0, f32(1.0) * f32(height) / f32(width))
        self.ratio = np.asarray(ratio, np.float32).astype(np.float64)
        self.rot = np.asarray(rot, np.float32).astype(np.float64)
        self.pos = np.asarray(pos, np.float32).astype(np.float64)
        self.render_dist, self.cam_fall_off, self.light_fall_off, self.ray_radius = (float(f32(v)) for v in (render_dist, cam_fall_off, light_fall_off, ray_radius))
        self.count = level_count(self.w)
        self.levels = None if levels is None else [np.asarray(lv, np.float64) for lv in levels]
        self.rgb = None if rgb is None else np.asarray(rgb, np.float64)
        if self.levels is not None:
            assert [lv.shape[::-1] for lv in self.levels] == [level_dims(self.w, self.h, self.count, i) for i in range(self.count)]

    def on_screen(self, i):
        """Texels of level i with a descendant inside the frame: the others are padding nothing reads."""
        w, h = level_dims(self.w, self.h, self.count, i)
        s = self.count - 1 - i
        gy, gx = np.mgrid[0:h, 0:w]
        return ((gx << s) < self.w) & ((gy << s) < self.h)


def rotate(q, v):
    """utilities.glsl:26-29: t = cross(q.xyz, v) + q.w v; v + 2 cross(q.xyz, t)."""
    t = np.cross(q[:3], v) + q[3] * v
    return v + 2.0 * np.cross(q[:3], t)


def sample_jitter(s, spp, width, height):
    """The offset of sample s of spp = n x n stratified samples (include/rt_abi.h at rt_render_spp):
    ((2i + 1) / n - 1) / view with i = s % n for x and s // n for y, every operation in fp32; the fp32 pair."""
    n = int(round(spp ** 0.5))
    assert n * n == spp and 0 <= s < spp
    f32 = np.float32
    return np.array([(f32(2 * (s % n) + 1) / f32(n) - f32(1)) / f32(width), (f32(2 * (s // n) + 1) / f32(n) - f32(1)) / f32(height)], np.float32)


def rays(fr, nx, ny):
    """Unit directions through the normalised coordinates (nx, ny), to which the sample's jitter is added first:
    normalize(rotate(rot, ((nx + jx) ratio_x, 1, (ny + jy) ratio_y)))."""
    nx, ny = nx + fr.jitter[0], ny + fr.jitter[1]
    v = np.stack([nx * fr.ratio[0], np.ones_like(nx), ny * fr.ratio[1]], -1)
    d = rotate(fr.rot, v)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- depth ---------------------------------------------------------------------------------------------------------------------
def _touch_intervals(A, B, Cq):
    """{t : A t^2 + 2 B t + Cq <= 0} as two intervals (lo, hi)[..., 2]; an empty one has lo > hi."""
    inf = np.inf
    D = B * B - A * Cq
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.maximum(D, 0.0))
        r1, r2 = (-B - sq) / A, (-B + sq) / A
        lin = -Cq / (2.0 * B)
    lo = np.full(A.shape + (2,), inf)
    hi = np.full(A.shape + (2,), -inf)
    pos, neg, zero = (A > 0) & (D >= 0), A < 0, A == 0
    lo[..., 0] = np.where(pos, r1, lo[..., 0])
    hi[..., 0] = np.where(pos, r2, hi[..., 0])
    # A < 0: everything when there is no real root, otherwise outside the roots (r2 <= r1 there, dividing by a negative A)
    every = neg & (D < 0)
    out = neg & (D >= 0)
    lo[..., 0] = np.where(every | out, -inf, lo[..., 0])
    hi[..., 0] = np.where(every, inf, np.where(out, r2, hi[..., 0]))
    lo[..., 1] = np.where(out, r1, lo[..., 1])
    hi[..., 1] = np.where(out, inf, hi[..., 1])
    # A == 0: 2 B t + Cq <= 0
    zl = zero & (B > 0)
    zg = zero & (B < 0)
    ze = zero & (B == 0) & (Cq <= 0)
    lo[..., 0] = np.where(zl | ze, -inf, np.where(zg, lin, lo[..., 0]))
    hi[..., 0] = np.where(zl, lin, np.where(zg | ze, inf, hi[..., 0]))
    return lo, hi


def depth_bands(fr, i, texels=None, chunk=4096):
    """depth_bands_chunk over blocks of `chunk` texels (bounds the working set)."""
    w, h = level_dims(fr.w, fr.h, fr.count, i)
    gy, gx = (a.ravel() for a in np.mgrid[0:h, 0:w]) if texels is None else texels
    parts = [depth_bands_chunk(fr, i, (gy[k:k + chunk], gx[k:k + chunk])) for k in range(0, max(len(gy), 1), chunk)]
    return {key: (np.concatenate([p[key] for p in parts]) if key != "tau" else parts[0]["tau"]) for key in parts[0]}


def depth_bands_chunk(fr, i, texels):
    """Bands of level i of fr (which carries its own levels).  texels: (gy, gx) index arrays.
    Returns a dict of flat arrays over those texels: lo, hi (nan where F is empty), empty (F empty), crossed (the centre line crosses a
    surface before render_dist), len0."""
    gy, gx = texels
    pw = float(1 << (fr.count - 1 - i))
    isx, isy = pw / fr.w, pw / fr.h
    tau = SQRT2_8 * isx
    u = rays(fr, (2.0 * gx + 1.0) * isx - 1.0, (2.0 * gy + 1.0) * isy - 1.0)
    len0 = np.ones(len(gx)) if i == 0 else fr.levels[i - 1][gy >> 1, gx >> 1]
    o = fr.pos + len0[:, None] * u
    out = ray_band(o, u, len0, tau, fr.scene, fr.render_dist, fr.alg)
    out.update(gy=gy, gx=gx, tau=tau)
    return out


def ray_band(o, u, len0, tau, scene, render_dist, alg=3):
    """The band of ANY cone march: origin o (T, 3), unit direction u (T, 3), the length len0 (T,) its result is added to, cone factor
    tau; what the module docstring says under DEPTH, for algorithm `alg`.  A level texel marches o = pos + len0 u with its level's
    tau; a mirror or transmitted ray marches o = eye + dir with len0 = 1 and tau = ray_radius (chain_bands).
    Returns dict(lo, hi (nan where F is empty), empty, crossed (the centre line crosses a surface before render_dist), len0)."""
    n_rays = len(len0)
    c, r = scene["c"], scene["r"]
    RD = render_dist
    oc = o[:, None, :] - c[None]                    # (T, n, 3)
    b = (oc * u[:, None, :]).sum(-1)                # (T, n)
    cc = (oc * oc).sum(-1)

    # first surface crossing of the centre line
    disc = b * b - (cc - r * r)
    with np.errstate(invalid="ignore"):
        root = -b - np.sqrt(np.maximum(disc, 0.0))
    a_k = np.where(cc <= r * r, 0.0, np.where((disc >= 0) & (root >= 0), root, np.inf))
    a = a_k.min(1)
    cut = np.minimum(a, RD)

    if alg == 1 and tau >= 1.0:
        # f(0) (1 - tau) <= 0 <= tau: the first sample stops the march, the band is one point
        f0 = (np.sqrt(cc) - r).min(1)
        assert (f0 >= 0.0).all(), "algorithm 1 from inside a sphere is not covered"
        point = np.maximum(len0 + f0 * (1.0 - tau) - tau, 0.0)
        return dict(lo=point, hi=point.copy(), empty=np.zeros(n_rays, bool), crossed=a < RD, len0=len0)
    # the radius factor of the touch sets {f_k <= (t + 1) tq}; algorithm 1 stops on f (1 - tau) <= (s + 1) tau
    tq = tau if alg == 3 else tau / (1.0 - tau)
    lo_k, hi_k = _touch_intervals(np.full_like(b, 1.0 - tq * tq), b - tq * (r + tq), cc - (r + tq) ** 2)
    lo_k = np.maximum(lo_k, 0.0)
    hi_k = np.minimum(hi_k, cut[:, None, None])

    def f_at(idx, s):  # min_k |o + s u - c_k| - r_k for texels idx at relative distances s (len(idx), m)
        p = oc[idx][:, None, :, :] + s[:, :, None, None] * u[idx][:, None, None, :]
        return (np.sqrt((p * p).sum(-1)) - r).min(-1)

    if alg == 3:
        lipschitz = 2.0 + tau

        def g_of(s, f):  # what a march that stops at s returns, relative to len0
            return s + np.maximum(f, 0.0) - (s + 1.0) * tau
    else:
        lipschitz = 2.0 * (1.0 - tau)

        def g_of(s, f):  # f >= 0 on F, the march never crosses a surface: the clamp only takes the rounding at the cut
            return (s + np.maximum(f, 0.0)) * (1.0 - tau) - tau

    gmin = np.full(n_rays, np.inf)
    gmax = np.full(n_rays, -np.inf)
    frac = np.linspace(0.0, 1.0, N_SAMPLE)
    for k in range(len(r)):
        for j in range(2):
            idx = np.nonzero(lo_k[:, k, j] <= hi_k[:, k, j])[0]
            if not len(idx):
                continue
            l, hgh = lo_k[idx, k, j], hi_k[idx, k, j]
            s = l[:, None] + (hgh - l)[:, None] * frac
            g = g_of(s, f_at(idx, s))
            slack = lipschitz * (hgh - l) / (2.0 * (N_SAMPLE - 1))
            # closed forms on this interval: g >= g with f = 0 (linear, rising); g <= g with max(f_k, 0) for f (convex in s)
            ends = np.stack([l, hgh], 1)
            pk = oc[idx, k][:, None, :] + ends[:, :, None] * u[idx][:, None, :]
            fk = np.sqrt((pk * pk).sum(-1)) - r[k]
            g_lo = np.maximum(g.min(1) - slack, g_of(ends, 0.0).min(1))
            g_hi = np.minimum(g.max(1) + slack, g_of(ends, np.maximum(fk, 0.0)).max(1))
            np.minimum.at(gmin, idx, g_lo)
            np.maximum.at(gmax, idx, g_hi)
    empty = ~np.isfinite(gmin)
    with np.errstate(invalid="ignore"):
        lo = np.where(empty, np.nan, np.maximum(len0 + gmin, 0.0))
        hi = np.where(empty, np.nan, np.maximum(len0 + gmax, 0.0))
    return dict(lo=lo, hi=hi, empty=empty, crossed=a < RD, len0=len0)


def march_rules(v, bd, render_dist, eps):
    """The hit and miss rules of the module docstring for marched values v against their ray_band bd.  Returns (ok, excursion, miss):
    excursion = the distance outside the band relative to 1 + v, 0 where a rule holds, inf for a rule with no distance."""
    with np.errstate(invalid="ignore"):
        out = np.maximum(np.maximum(bd["lo"] - v, v - bd["hi"]), 0.0) / (1.0 + v)  # nan where F is empty
    in_band = ~bd["empty"] & (out <= eps)
    miss = v >= render_dist
    # a march that ran out left the loop at a relative fp32 length >= render_dist; the one rounding of len0 + length is monotone
    ran_out = miss & ~bd["crossed"] & (v >= (bd["len0"] + render_dist) * (1.0 - 2.0 ** -23))
    ok = np.where(miss, in_band | ran_out, in_band)
    return ok, np.where(ok, 0.0, np.where(np.isfinite(out), out, np.inf)), miss


def check_depth(fr, i, eps=None, texels=None, bands=None):
    """Level i of fr against its bands, over the on-screen texels (or `texels`).  Returns dict(n, bad, excursion, far_bad, hits):
    bad = texels that break a rule by more than eps (1 + depth); excursion = the largest distance outside a band relative to
    1 + depth (inf for a rule with no distance: a forbidden or a forced miss); far_bad = texels whose parent missed and that do not."""
    eps = EPS_DEPTH if eps is None else eps
    if texels is None:
        gy, gx = np.nonzero(fr.on_screen(i))
    else:
        gy, gx = texels
    bd = bands if bands is not None else depth_bands(fr, i, (gy, gx))
    v = fr.levels[i][gy, gx]
    RD = fr.render_dist
    ok, exc, miss = march_rules(v, bd, RD, eps)
    far = bd["len0"] >= RD
    return dict(n=len(v), bad=int(np.count_nonzero(~ok)), excursion=float(exc.max()) if len(v) else 0.0,
                far_bad=int(np.count_nonzero(far & ~miss)), hits=int(np.count_nonzero(~miss)))


def sample_texels(fr, i, limit=100_000, n=20_000, seed=1):
    """The on-screen texels of level i, or a fixed-seed sample of n of them when there are more than `limit`."""
    gy, gx = np.nonzero(fr.on_screen(i))
    if len(gy) > limit:
        pick = np.sort(np.random.default_rng(seed + i).choice(len(gy), n, replace=False))
        gy, gx = gy[pick], gx[pick]
    return gy, gx


# ---- colour --------------------------------------------------------------------------------------------------------------------
def _segment_min(o, d, end, c, r):
    """min over t in [0, end] and spheres of |o + t d - c_k| - r_k for unit d: per sphere the closest approach clamped to the segment.
    Also the first t in [0, end] with f <= 0 (inf when there is none).  o, d (P, 3); end (P,)."""
    oc = o[:, None, :] - c[None]
    b = (oc * d[:, None, :]).sum(-1)
    cc = (oc * oc).sum(-1)
    t = np.clip(-b, 0.0, end[:, None])
    p = oc + t[..., None] * d[:, None, :]
    m = (np.sqrt((p * p).sum(-1)) - r).min(1)
    disc = b * b - (cc - r * r)
    with np.errstate(invalid="ignore"):
        root = -b - np.sqrt(np.maximum(disc, 0.0))
    a = np.where(cc <= r * r, 0.0, np.where((disc >= 0) & (root >= 0), root, np.inf)).min(1)
    f0 = (np.sqrt(cc) - r).min(1)
    return m, np.where(a <= end, a, np.inf), f0


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


def _nearest(fr, P):
    """(nearest sphere by strict '<', first wins; outward normal there; two smallest SDFs closer than AMBIGUOUS) at points P (n, 3)."""
    sc = fr.scene
    sdf = np.linalg.norm(P[:, None, :] - sc["c"][None], axis=-1) - sc["r"]
    best = sdf.argmin(1)
    if sdf.shape[1] > 1:
        two = np.partition(sdf, 1, axis=1)
        amb = (two[:, 1] - two[:, 0]) < AMBIGUOUS
    else:
        amb = np.zeros(len(P), bool)
    return best, _unit(P - sc["c"][best]), amb


def shade_point(fr, P, eye, view):
    """RGB interval of surface points P (n, 3) seen from `eye` (n, 3) along the unit directions `view` (n, 3): the camera ray has
    eye = pos and view = step, a mirror ray eye = the previous hit, a transmitted ray eye = Q.  Returns dict(lo, hi (n, 3); best (n,) =
    the nearest sphere, strict '<', first wins; normal (n, 3); ambiguous (n,) = the two smallest SDFs at P closer than AMBIGUOUS)."""
    sc = fr.scene
    best, normal, ambiguous = _nearest(fr, P)
    cam_dist = np.linalg.norm(P - eye, axis=-1)
    cam_fall = np.maximum(fr.cam_fall_off * (cam_dist * cam_dist + 1.0), 1.0)
    cam_dir = -view
    normal_fall = np.maximum((normal * cam_dir).sum(-1), 0.0)
    color, shine, ambient = sc["color"][best], sc["shine"][best], sc["ambient"][best]
    rr = fr.ray_radius
    lo = np.zeros((len(P), 3))
    hi = np.zeros((len(P), 3))
    for lp, lc in zip(sc["lpos"], sc["lcol"]):
        to = lp - P
        light_dist = np.linalg.norm(to, axis=-1)
        light_dir = to / light_dist[:, None]
        light_fall = np.maximum(fr.light_fall_off * light_dist * light_dist, 1.0)
        diffuse = np.maximum((normal * light_dir).sum(-1), 0.0)
        inc = -light_dir
        refl = inc - 2.0 * (normal * inc).sum(-1)[:, None] * normal
        base = (refl * cam_dir).sum(-1)
        with np.errstate(invalid="ignore"):
            spec = np.where(base > 0, np.maximum(diffuse * np.power(np.maximum(base, 0.0), shine), 0.0), 0.0)
        s = np.maximum(diffuse + spec, 0.0)
        end = light_dist
        m, a, f0 = _segment_min(P + light_dir, light_dir, end, sc["c"], sc["r"])
        blocked = (np.minimum(end, f0) <= rr) | (a <= end - 2.0 * rr)
        s_hi = np.where(blocked, 0.0, np.minimum(np.minimum(1.0, end), np.maximum(f0, 0.0)))
        s_lo = np.where(blocked | (m <= rr), 0.0, np.minimum(np.minimum(m, end), 1.0))
        for soft, acc in ((s_lo, lo), (s_hi, hi)):
            direct = (s[:, None] * lc[None] / light_fall[:, None]) * soft[:, None]
            acc += (ambient[:, None] + direct) / cam_fall[:, None] * normal_fall[:, None] * color
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    return dict(lo=lo, hi=hi, best=best, normal=normal, ambiguous=ambiguous)


def shade_bands(fr, pixels=None):
    """RGB intervals of the pixels whose own finest-level depth is < render_dist.  Returns dict(py, px: the hit pixels; lo, hi (n, 3);
    ambiguous, pinned (n,) bool; width (n,) = the largest component of hi - lo; and of the primary hit: step, P, best, normal)."""
    depth = fr.levels[-1][:fr.h, :fr.w]
    if pixels is None:
        py, px = np.nonzero(depth < fr.render_dist)
    else:
        py, px = pixels
        keep = depth[py, px] < fr.render_dist
        py, px = py[keep], px[keep]
    d = depth[py, px]
    step = rays(fr, (px + 0.5) * 2.0 / fr.w - 1.0, (py + 0.5) * 2.0 / fr.h - 1.0)
    P = fr.pos + d[:, None] * step
    sp = shade_point(fr, P, np.broadcast_to(fr.pos, P.shape), step)
    lo, hi, ambiguous = sp["lo"], sp["hi"], sp["ambiguous"]
    width = (hi - lo).max(1) if len(d) else np.zeros(0)
    return dict(py=py, px=px, lo=lo, hi=hi, ambiguous=ambiguous, pinned=~ambiguous & (width < PINNED_WIDTH), width=width,
                step=step, P=P, best=sp["best"], normal=sp["normal"])


def check_rgb(fr, eps=None, bands=None):
    """fr.rgb against its intervals.  Returns dict(hits, bad, excursion, ambiguous, pinned (shares of the hit pixels), median_width,
    miss_nonblack (miss pixels that are not exactly black))."""
    eps = EPS_RGB if eps is None else eps
    sb = bands if bands is not None else shade_bands(fr)
    got = fr.rgb[sb["py"], sb["px"]]
    keep = ~sb["ambiguous"]
    out = np.maximum(np.maximum(sb["lo"] - got, got - sb["hi"]), 0.0).max(1) if len(got) else np.zeros(0)
    out = np.where(np.isfinite(out), out, np.inf)[keep]
    n = len(got)
    missed = fr.levels[-1][:fr.h, :fr.w] >= fr.render_dist
    return dict(hits=n, bad=int(np.count_nonzero(out > eps)), excursion=float(out.max()) if len(out) else 0.0,
                ambiguous=float(np.count_nonzero(sb["ambiguous"])) / max(n, 1), pinned=float(np.count_nonzero(sb["pinned"])) / max(n, 1),
                median_width=float(np.median(sb["width"][keep])) if keep.any() else 0.0,
                miss_nonblack=int(np.count_nonzero(fr.rgb[missed])))


def check_frame(fr, eps_depth=None, eps_rgb=None, limit=100_000):
    """Every level and the RGB of fr.  Returns (list of check_depth results, check_rgb result)."""
    depth = [check_depth(fr, i, eps_depth, sample_texels(fr, i, limit)) for i in range(fr.count)]
    return depth, check_rgb(fr, eps_rgb)


def sample_bands(frames):
    """Intervals of the average of the per-sample frames (each with its own jitter and levels): per pixel [sum lo_s, sum hi_s] / spp,
    a sample that missed adding exactly 0.  Returns dict(lo, hi (h, w, 3); hit (a sample hit), ambiguous (a hit sample is
    ambiguous), pinned (every hit sample is pinned) (h, w) bool; sample_hits = the (pixel, sample) pairs that hit)."""
    h, w, n = frames[0].h, frames[0].w, len(frames)
    lo, hi = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    hit, ambiguous, pinned = np.zeros((h, w), bool), np.zeros((h, w), bool), np.ones((h, w), bool)
    sample_hits = 0
    for fr in frames:
        assert (fr.w, fr.h) == (w, h)
        sb = shade_bands(fr)
        py, px = sb["py"], sb["px"]  # every pixel at most once
        lo[py, px] += sb["lo"]
        hi[py, px] += sb["hi"]
        hit[py, px] = True
        ambiguous[py, px] |= sb["ambiguous"]
        pinned[py, px] &= sb["pinned"]
        sample_hits += len(py)
    return dict(lo=lo / n, hi=hi / n, hit=hit, ambiguous=ambiguous, pinned=pinned & hit, sample_hits=sample_hits)


def check_samples_rgb(frames, rgb, eps=None, bands=None):
    """The averaged frame `rgb` against sample_bands(frames).  check_rgb's keys, the shares being of the pixels some sample hit
    (ambiguous pixels are left out of bad / excursion / median_width), and sample_hits."""
    eps = EPS_RGB if eps is None else eps
    sb = bands if bands is not None else sample_bands(frames)
    rgb = np.asarray(rgb, np.float64)
    hit, keep = sb["hit"], sb["hit"] & ~sb["ambiguous"]
    out = np.maximum(np.maximum(sb["lo"] - rgb, rgb - sb["hi"]), 0.0).max(-1)
    out = np.where(np.isfinite(out), out, np.inf)[keep]
    n = int(np.count_nonzero(hit))
    width = (sb["hi"] - sb["lo"]).max(-1)
    return dict(hits=n, bad=int(np.count_nonzero(out > eps)), excursion=float(out.max()) if len(out) else 0.0,
                ambiguous=float(np.count_nonzero(sb["ambiguous"])) / max(n, 1), pinned=float(np.count_nonzero(sb["pinned"])) / max(n, 1),
                median_width=float(np.median(width[keep])) if keep.any() else 0.0, miss_nonblack=int(np.count_nonzero(rgb[~hit])),
                sample_hits=sb["sample_hits"])


def check_samples(frames, rgb, eps_depth=None, eps_rgb=None, limit=100_000):
    """A multi-sample frame: `frames` are the per-sample Frames (own jitter, own levels), `rgb` their average as rendered.  Every
    level of every sample against its bands, and the average against the averaged intervals.  Returns check_samples_rgb's dict (so
    check_caps applies) with depth = [sample][level] check_depth results."""
    res = check_samples_rgb(frames, rgb, eps_rgb)
    res["depth"] = [[check_depth(fr, i, eps_depth, sample_texels(fr, i, limit)) for i in range(fr.count)] for fr in frames]
    return res


# ---- the mirror and transmission chains ----------------------------------------------------------------------------------------
def reflect(i, n):
    """GLSL reflect(I, N) = I - 2 dot(N, I) N."""
    return i - 2.0 * _dot(n, i)[:, None] * n


def refract(i, n, eta):
    """GLSL refract(I, N, eta): k = 1 - eta^2 (1 - dot(N, I)^2); eta I - (eta dot(N, I) + sqrt(k)) N for k >= 0.  Returns (vector, k)."""
    ci = _dot(n, i)
    k = 1.0 - eta * eta * (1.0 - ci * ci)
    return eta * i - (eta * ci + np.sqrt(np.maximum(k, 0.0)))[:, None] * n, k


def _trans_branches(P, I, c, rad, index, dt):
    """The three quantities that decide a branch of the transmission formula, evaluated in the number format dt from the same
    inputs: k of the entry refraction, disc / r^2 of the crossing, k2 of the exit refraction (k = k2 = 1 for index 1)."""
    P, I, c, rad, index = (np.asarray(a, np.float64).astype(dt) for a in (P, I, c, rad, index))
    one = dt(1.0)
    oc = P - c
    nrm = oc / np.sqrt((oc * oc).sum(-1))[:, None]
    k = np.ones(len(P), dt)
    Tdir = I
    if index != one:
        eta = one / index
        ci = (nrm * I).sum(-1)
        k = one - eta * eta * (one - ci * ci)
        v = eta * I - (eta * ci + np.sqrt(np.maximum(k, dt(0))))[:, None] * nrm
        Tdir = v / np.sqrt((v * v).sum(-1))[:, None]
    b = (oc * Tdir).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - rad * rad)
    t = np.maximum(np.where(disc > 0, np.sqrt(np.maximum(disc, dt(0))) - b, dt(0)), dt(0))
    k2 = np.ones(len(P), dt)
    if index != one:
        e = oc + Tdir * t[:, None]
        n2 = e / np.sqrt((e * e).sum(-1))[:, None]
        ce = (n2 * Tdir).sum(-1)
        k2 = one - index * index * (one - ce * ce)
    return k, disc / (rad * rad), k2


# What a wrong reading of the specification would compute: chain_bands(fr, wrong=<one of these>) is that reading's reference, which
# has to REJECT the right recordings (tests/test_path_a_exact_host.py).  "mirror" / "trans": the chain kind it needs; 2: at least two
# links of that kind; "both": both chains; "bend": refraction_index != 1.
WRONG_CHAINS = {
    "reflect sign flipped": "mirror",          # I + 2 dot(N, I) N
    "index and 1/index exchanged": "bend",
    "exit normal not negated": "bend",         # refract(T, n2, index)
    "weight from the surface hit": "any",      # the surface the ray arrives at instead of the one it leaves
    "weight from the surface before": "any2",  # the surface left one link earlier
    "weight not accumulated": "any2",
    "cam_fall from the camera": "any",
    "transmission from the mirror chain's end": "both",
    "near root": "trans",                      # -sqrt(disc) - b
    "finest level's tau": "any",
    "len0 = 0": "any",
    "started at eye": "any",
    "first contribution dropped": "any",
    "first contribution twice": "any",
}


def wrong_applies(wrong, fr, res):
    """Does the wrong reading differ from the right one on this frame?  res: check_chains(fr) of the right reading.  A weight that
    depends on an earlier link needs a second or later link of a chain that found a surface (later_hits); measuring cam_fall from
    the camera changes nothing where the fall-off is clamped to 1 for either eye, that is where every shaded point lies within
    sqrt(1 / cam_fall_off - 1) of both (CAM_FALL_FLAT; the test asserts that the two readings' intervals are then the same)."""
    need = WRONG_CHAINS[wrong]
    r, t = fr.reflections, fr.transmissions
    if wrong == "cam_fall from the camera" and getattr(fr, "name", None) in CAM_FALL_FLAT:
        return False
    return {"mirror": r > 0, "trans": t > 0, "bend": t > 0 and fr.refraction_index != 1.0, "any": r + t > 0,
            "any2": max(r, t) >= 2 and res["later_hits"] > 0, "both": r > 0 and t > 0}[need]


CAM_FALL_FLAT = ("mirror_r2",)  # both spheres within 9.95 = sqrt(1 / 0.01 - 1) of the camera and of each other


def chain_bands(fr, wrong=None):
    """What the recorded secondary marches of fr (fr.chains) and its RGB have to be, link by link; see CHAINS in the module docstring.
    Every expected value of link j is computed from the RECORDED values of link j - 1 (and the frame's own depth for link 0), so no
    rounding is carried from one link to the next.  Over the hit pixels (shade_bands' order) returns dict(py, px; lo, hi (n, 3): the
    RGB interval, primary plus the weighted secondary intervals; secondary (n,): the largest component of the summed lower ends of
    the secondary intervals; left_out (n,): ambiguous at some shaded point, or a branch of the formula decided inside a guard;
    nan_bad (n,): recordings where the walk predicts none, or none where it predicts one; eye_exc, dir_exc, len_exc (n,): the largest
    excursions of the pixel's recorded eye (relative to 1 + |eye|), dir and len (outside its band, relative to 1 + len; inf for a
    forbidden or forced miss); n_mirror, n_trans, n_points: non-NaN mirror / transmission recordings and those with len <
    render_dist, over the hit pixels; miss_mirror, miss_trans: recorded marches that ended by a miss; later_hits: second and later
    links of a chain that found a surface; guard_k, guard_disc: the largest fp32 - float64 differences of the branch quantities;
    miss_recorded: values that are not NaN at miss pixels)."""
    assert wrong is None or wrong in WRONG_CHAINS
    sb = shade_bands(fr)
    py, px = sb["py"], sb["px"]
    n = len(py)
    sc, RD = fr.scene, fr.render_dist
    R, T = fr.reflections, fr.transmissions
    rec = fr.chains[py, px]                      # (n, R + T, 7)
    lo, hi = sb["lo"].copy(), sb["hi"].copy()
    sec_lo = np.zeros((n, 3))
    left_out = sb["ambiguous"].copy()
    nan_bad = np.zeros(n, bool)
    eye_exc, dir_exc, len_exc = np.zeros(n), np.zeros(n), np.zeros(n)
    counts = dict(n_mirror=0, n_trans=0, n_points=0, miss_mirror=0, miss_trans=0, later_hits=0, guard_k=0.0, guard_disc=0.0)
    tau = fr.ray_radius
    if wrong == "finest level's tau":
        tau = SQRT2_8 / fr.w
    pos_all = np.broadcast_to(fr.pos, (n, 3))

    def link(row, alive, eye_x, dir_x, weight, kind, first, radius, eye_allow=None, dir_allow=None):
        """One recorded march: rows `row` of the pixels `alive` against the expected eye / dir, its band, and its weighted shading.
        radius: of the sphere whose normal made dir; eye_allow, dir_allow: what the conditioning of the crossing and of the exit
        refraction leaves open (absolute, taken off the differences first).  Returns (hit: the march ran and found a surface, H: the recorded hit point, the recorded dir)."""
        r7 = rec[:, row]
        has = ~np.isnan(r7).any(1)
        nan_bad[:] |= (has != alive) | (np.isnan(r7).any(1) != np.isnan(r7).all(1))
        idx = np.nonzero(alive & has)[0]
        hit = np.zeros(n, bool)
        H = np.full((n, 3), np.nan)
        if not len(idx):
            return hit, H, r7[:, 3:6]
        eye, dr, ln = r7[idx, 0:3], r7[idx, 3:6], r7[idx, 6]
        counts["n_" + kind] += len(idx)
        size = np.linalg.norm(eye_x[idx], axis=1)
        ea = 0.0 if eye_allow is None else eye_allow[idx]
        da = 0.0 if dir_allow is None else dir_allow[idx]
        np.maximum.at(eye_exc, idx, np.maximum(np.abs(eye - eye_x[idx]).max(1) - ea, 0.0) / (1.0 + size))
        np.maximum.at(dir_exc, idx, np.maximum(np.abs(dr - dir_x[idx]).max(1) - da, 0.0) / (1.0 + size / radius[idx]))
        u = _unit(dr)
        if wrong == "len0 = 0":
            bd = ray_band(eye + dr, u, np.zeros(len(idx)), tau, sc, RD)
        elif wrong == "started at eye":
            bd = ray_band(eye, u, np.zeros(len(idx)), tau, sc, RD)
        else:
            bd = ray_band(eye + dr, u, np.ones(len(idx)), tau, sc, RD)
        ok, exc, miss = march_rules(ln, bd, RD, 0.0)
        np.maximum.at(len_exc, idx, exc)
        counts["miss_" + kind] += int(np.count_nonzero(miss))
        h = idx[~miss]
        hit[h] = True
        counts["n_points"] += len(h)
        if not first:
            counts["later_hits"] += len(h)
        H[h] = r7[h, 0:3] + r7[h, 3:6] * np.maximum(r7[h, 6], 0.0)[:, None]
        if len(h):
            sp = shade_point(fr, H[h], pos_all[h] if wrong == "cam_fall from the camera" else r7[h, 0:3], _unit(r7[h, 3:6]))
            left_out[h] |= sp["ambiguous"]
            w = weight[h]
            if wrong == "weight from the surface hit":  # this link's factor (weight_factor, scale, per_surface: the calling loop's) retaken at H
                w = w / weight_factor[h] * scale * per_surface[sp["best"]]
            times = {"first contribution dropped": 0.0, "first contribution twice": 2.0}.get(wrong, 1.0) if first else 1.0
            lo[h] += times * w[:, None] * sp["lo"]
            hi[h] += times * w[:, None] * sp["hi"]
            sec_lo[h] += w[:, None] * sp["lo"]
        return hit, H, r7[:, 3:6]

    first = True
    last_mirror = None  # (alive, H, dir) where the mirror chain's last link hit
    # ---- mirror bounces: r = reflect(dir, n), eye = the previous hit, weight prod(reflectivity * specular) over the surfaces left
    scale, per_surface = fr.reflectivity, sc["specular"]
    alive = np.ones(n, bool)
    H, dprev = sb["P"], sb["step"]
    weight = np.ones(n)
    factors = []
    for j in range(R):
        safe = np.where(np.isnan(H).any(1)[:, None], 0.0, H)
        best, nrm, amb = _nearest(fr, safe)
        left_out |= alive & amb
        weight_factor = scale * per_surface[best]
        factors.append(weight_factor)
        if wrong == "weight not accumulated":
            weight = weight_factor.copy()
        elif wrong == "weight from the surface before" and j > 0:
            weight = weight * factors[j - 1]
        else:
            weight = weight * weight_factor
        d_in = _unit(np.where(np.isnan(dprev).any(1)[:, None], 1.0, dprev))
        dir_x = reflect(d_in, nrm) if wrong != "reflect sign flipped" else d_in + 2.0 * _dot(nrm, d_in)[:, None] * nrm
        hit, Hn, dn = link(j, alive, safe, dir_x, weight, "mirror", first, sc["r"][best])
        first = False
        alive = hit
        if alive.any():
            last_mirror = (alive.copy(), Hn.copy(), dn.copy())
        H, dprev = Hn, dn
    # ---- transmission passes: again from the camera ray's hit, weight prod(transparency * diffuse) over the surfaces left
    scale, per_surface = fr.transparency, sc["diffuse"]
    idxr = fr.refraction_index
    bend = idxr != 1.0
    alive = np.ones(n, bool)
    H, dprev = sb["P"], sb["step"]
    if wrong == "transmission from the mirror chain's end" and last_mirror is not None:
        m_alive, m_H, m_d = last_mirror
        H = np.where(m_alive[:, None], m_H, H)
        dprev = np.where(m_alive[:, None], m_d, dprev)
    weight = np.ones(n)
    factors = []
    first = True
    for j in range(T):
        P = np.where(np.isnan(H).any(1)[:, None], 0.0, H)
        I = _unit(np.where(np.isnan(dprev).any(1)[:, None], 1.0, dprev))
        best, nrm, amb = _nearest(fr, P)
        left_out |= alive & amb
        weight_factor = scale * per_surface[best]
        factors.append(weight_factor)
        if wrong == "weight not accumulated":
            weight = weight_factor.copy()
        elif wrong == "weight from the surface before" and j > 0:
            weight = weight * factors[j - 1]
        else:
            weight = weight * weight_factor
        eta_in, eta_out = (1.0 / idxr, idxr) if wrong != "index and 1/index exchanged" else (idxr, 1.0 / idxr)
        Tdir = I
        if bend:
            v, k = refract(I, nrm, eta_in)
            left_out |= alive & (np.abs(k) < GUARD_K)
            alive = alive & (k >= 0.0)
            Tdir = _unit(np.where((k >= 0.0)[:, None], v, I))
        c, rad = sc["c"][best], sc["r"][best]
        if alive.any():  # what fp32 makes of the three deciding quantities, for the guards' measurement
            q32, q64 = _trans_branches(P, I, c, rad, idxr, np.float32), _trans_branches(P, I, c, rad, idxr, np.float64)
            for key, a32, a64 in zip(("guard_k", "guard_disc", "guard_k"), q32, q64):
                counts[key] = max(counts[key], float(np.abs(a32.astype(np.float64) - a64)[alive].max()))
        oc = P - c
        b = _dot(oc, Tdir)
        disc = b * b - (_dot(oc, oc) - rad * rad)
        left_out |= alive & (np.abs(disc) < GUARD_DISC * rad * rad)
        root = np.sqrt(np.maximum(disc, 0.0))
        t = np.maximum(np.where(disc > 0.0, (root if wrong != "near root" else -root) - b, 0.0), 0.0)
        Q = P + Tdir * t[:, None]
        # fp32 holds disc only to GUARD_DISC r^2, so t = sqrt(disc) - b and Q only to that over 2 sqrt(disc) (nothing for t = 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_allow = np.where((disc > 0.0) & (t > 0.0), GUARD_DISC * rad * rad / (2.0 * root), 0.0)
        D = Tdir
        dir_allow = np.zeros(n)
        if bend:
            n2 = _unit(oc + Tdir * t[:, None])
            v, k2 = refract(Tdir, -n2 if wrong != "exit normal not negated" else n2, eta_out)
            left_out |= alive & (np.abs(k2) < GUARD_K)
            alive = alive & (k2 >= 0.0)
            D = _unit(np.where((k2 >= 0.0)[:, None], v, Tdir))
            # n2 moves by t_allow / r, k2 = 1 - index^2 (1 - ce^2) by GUARD_K + 2 index^2 |ce| dn2, sqrt(k2) by that over 2 sqrt(k2);
            # D = index T + (sqrt(k2) - index ce) n2
            ce = np.abs(_dot(n2, Tdir))
            dn2 = t_allow / rad
            with np.errstate(divide="ignore", invalid="ignore"):
                sq = np.sqrt(np.maximum(k2, 0.0))
                dir_allow = np.where(k2 > 0.0, (GUARD_K + 2.0 * eta_out * eta_out * ce * dn2) / (2.0 * sq) + (sq + 2.0 * eta_out * ce) * dn2, 0.0)
        hit, Hn, dn = link(R + j, alive, Q, D, weight, "trans", first, rad, t_allow, dir_allow)
        first = False
        alive = hit
        H, dprev = Hn, dn
    missed = fr.levels[-1][:fr.h, :fr.w] >= RD
    out = dict(py=py, px=px, lo=lo, hi=hi, secondary=sec_lo.max(1) if n else np.zeros(0), left_out=left_out, nan_bad=nan_bad,
               eye_exc=eye_exc, dir_exc=dir_exc, len_exc=len_exc, miss_recorded=int(np.count_nonzero(~np.isnan(fr.chains[missed]))))
    out.update(counts)
    return out


def check_chains(fr, eps_eye=None, eps_dir=None, eps_len=None, eps_rgb=None, wrong=None):
    """fr's recorded marches and RGB against chain_bands.  Returns dict(hits; bad_nan, bad_eye, bad_dir, bad_len, bad_rgb: pixels that
    break that rule by more than its tolerance, left-out pixels not counted (what their guard leaves open includes whether a march
    runs at all); bad = pixels that break any; eye, dir, len, rgb: the largest excursions;
    left_out (share of the hit pixels); covered = share of the hit pixels whose secondary contribution exceeds 100 EPS_RGB;
    miss_nonblack, miss_recorded; the counters of chain_bands)."""
    eps_eye = EPS_CHAIN_EYE if eps_eye is None else eps_eye
    eps_dir = EPS_CHAIN_DIR if eps_dir is None else eps_dir
    eps_len = EPS_CHAIN_LEN if eps_len is None else eps_len
    eps_rgb = EPS_CHAIN_RGB if eps_rgb is None else eps_rgb
    cb = chain_bands(fr, wrong)
    n = len(cb["py"])
    keep = ~cb["left_out"]
    got = fr.rgb[cb["py"], cb["px"]]
    rgb_exc = np.maximum(np.maximum(cb["lo"] - got, got - cb["hi"]), 0.0).max(1) if n else np.zeros(0)
    rgb_exc = np.where(np.isfinite(rgb_exc), rgb_exc, np.inf)
    bad = {"nan": cb["nan_bad"] & keep, "eye": (cb["eye_exc"] > eps_eye) & keep, "dir": (cb["dir_exc"] > eps_dir) & keep,
           "len": (cb["len_exc"] > eps_len) & keep, "rgb": (rgb_exc > eps_rgb) & keep}
    any_bad = np.zeros(n, bool)
    for v in bad.values():
        any_bad |= v
    missed = fr.levels[-1][:fr.h, :fr.w] >= fr.render_dist

    def worst(a):
        return float(a[keep].max()) if keep.any() else 0.0

    res = dict(hits=n, bad=int(np.count_nonzero(any_bad)), eye=worst(cb["eye_exc"]), dir=worst(cb["dir_exc"]), len=worst(cb["len_exc"]), rgb=worst(rgb_exc),
               left_out=float(np.count_nonzero(cb["left_out"])) / max(n, 1), covered=float(np.count_nonzero(cb["secondary"] > 100.0 * EPS_RGB)) / max(n, 1),
               miss_nonblack=int(np.count_nonzero(fr.rgb[missed])))
    res.update({"bad_" + k: int(np.count_nonzero(v)) for k, v in bad.items()})
    res.update({k: cb[k] for k in ("n_mirror", "n_trans", "n_points", "miss_mirror", "miss_trans", "miss_recorded", "later_hits", "guard_k", "guard_disc")})
    return res


def assert_chains(fr, res, counters=None):
    """What every chain case asserts of a check_chains result (and of the frame's counters: hit_pixels, shadow_rays,
    reflection_rays, transmission_rays)."""
    assert res["bad"] == 0 and res["miss_nonblack"] == 0 and res["miss_recorded"] == 0, res
    assert res["left_out"] <= CAP_AMBIGUOUS, res
    assert res["covered"] >= CHAIN_COVERED, res
    assert (res["miss_mirror"] > 0 or not fr.reflections) and (res["miss_trans"] > 0 or not fr.transmissions), res
    if counters is not None:
        n_light = len(fr.scene["lpos"])
        assert counters["hit_pixels"] == res["hits"], (counters, res)
        assert counters["reflection_rays"] == res["n_mirror"] and counters["transmission_rays"] == res["n_trans"], (counters, res)
        assert counters["shadow_rays"] == n_light * (res["hits"] + res["n_points"]), (counters, res)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------
def _pack_scene(spheres, mats, lights):
    """The 656-byte scene image: spheres [(x, y, z, r)], mats [(r, g, b, shine, ambient)], lights [((x, y, z), (r, g, b))]."""
    head = np.array([len(mats), len(spheres), len(lights), 0], np.uint32)
    m = np.zeros((8, 8), np.float32)
    o = np.zeros((8, 4), np.float32)
    li = np.zeros((8, 8), np.float32)
    for k, (r, g, b, shine, ambient) in enumerate(mats):
        m[k, :7] = (r, g, b, 1.0, 1.0, shine, ambient)
    for k, s in enumerate(spheres):
        o[k] = s
    for k, (p, c) in enumerate(lights):
        li[k, :3], li[k, 4:7] = p, c
    return head.tobytes() + m.tobytes() + o.tobytes() + li.tobytes()


def startup_scene():
    """The reference's start-up scene (src/main.rs:524-591)."""
    return _pack_scene([(5, 5, -1, 3), (5, 4, 10, 6), (-3, 3, -3, 1), (4, -1, 0, 2)],
                       [(0.2, 0.2, 1.0, 1, 0.05), (0.1, 1.0, 0.1, 10, 0.05), (1.0, 1.0, 0.1, 1, 0.05), (1.0, 0.1, 0.1, 1, 0.05)],
                       [((-1, 0, -3), (0.1, 0.5, 0.6)), ((8, -5, 10), (1.2, 0.2, 0.3))])


def room_scene():
    """The eight-sphere room of BASELINE.json configs[0]/[1]: five wall spheres of radius 50, three balls, one light."""
    return _pack_scene([(-56, 10, 0, 50), (56, 10, 0, 50), (0, 10, -56, 50), (0, 10, 56, 50), (0, 72, 0, 50), (-2.5, 14, -4, 2), (2.5, 11, -3, 3), (0, 8, -5, 1)],
                       [(0.75, 0.15, 0.15, 1, 0.05), (0.15, 0.75, 0.15, 1, 0.05), (0.75, 0.75, 0.75, 1, 0.05), (0.75, 0.75, 0.75, 1, 0.05),
                        (0.75, 0.75, 0.75, 1, 0.05), (0.9, 0.9, 0.2, 10, 0.05), (0.2, 0.4, 0.9, 30, 0.05), (0.9, 0.5, 0.2, 4, 0.05)],
                       [((0, 10, 5), (1.0, 1.0, 1.0))])


def random_scene(n_obj, n_light):
    """Drawn as tests/test_gpu_path_a.py::test_object_and_light_counts draws its scenes."""
    rng = np.random.default_rng(n_obj * 16 + n_light)
    spheres = [(rng.uniform(-8, 8), rng.uniform(6, 25), rng.uniform(-6, 6), rng.uniform(0.5, 3)) for _ in range(n_obj)]
    mats = [(*rng.uniform(0.1, 1, 3), float(rng.choice([1, 2, 10, 30])), 0.05) for _ in range(n_obj)]
    lights = [(tuple(rng.uniform(-10, 10, 3)), tuple(rng.uniform(0.1, 1.5, 3))) for _ in range(n_light)]
    return _pack_scene(spheres, mats, lights)


def camera_quat(yaw, pitch):
    """Rz(-yaw) * Rx(pitch) as [x, y, z, w], fp32 (src/main.rs:402-404)."""
    hz, hx = np.float32(-yaw) * np.float32(0.5), np.float32(pitch) * np.float32(0.5)
    zs, zc, xs, xc = np.sin(hz), np.cos(hz), np.sin(hx), np.cos(hx)
    return np.array([zc * xs, zs * xs, zs * xc, zc * xc], np.float32)


TURNED = dict(rot=camera_quat(0.6, -0.2), pos=(1.0, -2.0, 0.5))
OTHER_CONFIG = dict(render_dist=40.0, cam_fall_off=0.02, light_fall_off=0.005, ray_radius=0.02)
SMALL, MID, PADDED = (17, 9), (96, 64), (200, 120)  # tau = 0.67 at the finest level of two; four levels; five levels padded to multiples of 8
# name -> (scene, view keywords, config keywords, kind, sizes); kind "open" and "room" carry the caps on the pinned share.
# The caps below are conditions on (scene, view, size), asserted for every frame listed here; a frame that misses one is not listed.
# The room seen straight on misses the width cap below 200 x 120 (median width 0.056 at 17 x 9, where 3.3 % of its pixels are ambiguous
# as well, and 0.059 at 96 x 64: the cone radius lifts P off the walls and every shadow segment ends one unit past the light, next to
# the ceiling), so it runs at 200 x 120 (and 512 x 288 on the GPU) and the turned room carries the small sizes.
CASES = {
    "startup": (startup_scene(), {}, {}, "open", [(12, 10), SMALL, MID, PADDED]),
    "startup_turned": (startup_scene(), TURNED, {}, "open", [SMALL, MID, PADDED]),
    "room": (room_scene(), {}, {}, "room", [PADDED]),
    "room_turned": (room_scene(), TURNED, {}, "room", [SMALL, MID, PADDED]),
    "random_5_2": (random_scene(5, 2), {}, {}, "open", [MID, PADDED]),
    "random_8_8": (random_scene(8, 8), {}, {}, "open", [MID, PADDED]),
    # inside a sphere, off its centre (at the centre the normal is 0 / 0, outside the arithmetic contract)
    "inside": (_pack_scene([(0.5, 1.0, -0.25, 5)], [(1, 1, 1, 1, 0.05)], [((0, 1, 0), (1, 1, 1))]), {}, {}, None, [SMALL, MID]),
    "all_miss": (_pack_scene([(0, -50, 0, 1)], [(1, 1, 1, 1, 0.05)], [((0, 1, 0), (1, 1, 1))]), {}, {}, None, [MID]),
    "config": (startup_scene(), {}, OTHER_CONFIG, None, [MID, PADDED]),
    "ratio": (startup_scene(), dict(ratio=(0.7, 0.9)), {}, None, [MID, PADDED]),
}
FRAMES = [(name, w, h) for name, case in CASES.items() for w, h in case[4]]
GPU_ONLY_FRAMES = [("startup", 512, 288), ("room", 512, 288)]  # 7 levels, tau = 0.022: the tight bands; sampled above 100 000 texels a level
# (name, w, h, spp): spp = n x n stratified samples, each a full frame with its own jitter; the caps are asserted on the averaged frame.
# 4 = one SP batch; 9 = a batch that is no multiple of four; 16 = four SP rounds.  Sizes follow FRAMES (the room only at 200 x 120).
SAMPLE_FRAMES = [(name, w, h, spp) for spp in (4, 9) for name, w, h in
                 [("startup",) + SMALL, ("startup",) + MID, ("startup_turned",) + PADDED, ("room_turned",) + MID, ("random_8_8",) + MID,
                  ("room",) + PADDED, ("ratio",) + PADDED]] + [("startup",) + MID + (16,), ("room_turned",) + MID + (16,)]
GPU_ONLY_SAMPLE_FRAMES = [("startup", 512, 288, 4)]
# march algorithm 1 at 1 spp (17 x 9: tau = 1.33 at level 0, the one-point band); no camera inside a sphere
ALG1_FRAMES = [("startup",) + SMALL, ("startup",) + MID, ("startup_turned",) + PADDED, ("room_turned",) + MID, ("room",) + PADDED,
               ("random_8_8",) + MID, ("random_5_2",) + PADDED, ("all_miss",) + MID, ("config",) + MID]
# ---- chain cases: name -> (scene, view keywords, config keywords, sizes) ----------------------------------------------------------
# mat.diffuse / mat.specular (the per-material scales of the transmission / mirror weights; 1 in every scene above) pairwise different
# and strictly between 0 and 1, so that a weight taken from the wrong surface shows
SURFACES = [(0.9, 0.35), (0.8, 0.45), (0.7, 0.55), (0.6, 0.65), (0.5, 0.75), (0.4, 0.85), (0.3, 0.95), (0.95, 0.25)]


def with_surfaces(scene, pairs=SURFACES):
    """The scene image with (mat.diffuse, mat.specular) of material k set to pairs[k]."""
    raw = bytearray(scene)
    for k, pair in enumerate(pairs):
        raw[16 + 32 * k + 12:16 + 32 * k + 20] = np.array(pair, np.float32).tobytes()
    return bytes(raw)


def mirror_scene():
    """tests/test_oracle_a.py::test_mirror_reflection_known_answers: a grey sphere facing a lit red one, the red one larger and nearer
    (radius 4 at (7, 4, 0) for 2 at (6, 6, 0)): as drawn there only 6.8 % of the hit pixels show the other sphere (CHAIN_COVERED)."""
    return with_surfaces(_pack_scene([(0, 10, 0, 4), (7, 4, 0, 4)], [(0.9, 0.9, 0.9, 4, 0.05), (1.0, 0.2, 0.2, 4, 0.05)], [((0, 0, 12), (2, 2, 2))]))


def lens_scene():
    """tests/test_oracle_a.py::test_transmission_known_answers: a clear sphere in front of a lit red one, a ball lens."""
    return with_surfaces(_pack_scene([(0, 10, 0, 3), (0, 24, 0, 5)], [(0.9, 0.9, 0.9, 4, 0.05), (1.0, 0.2, 0.2, 4, 0.05)], [((0, 14, 14), (2, 2, 2))]))


def _chain(reflections=0, transmissions=0, index=1.0, **other):
    return dict(reflections=reflections, reflectivity=0.75, transmissions=transmissions, transparency=0.625, refraction_index=index, **other)


CHAIN_CASES = {
    "mirror_r2": (mirror_scene(), {}, _chain(2), [MID]),
    "lens_t2_n1.5": (lens_scene(), {}, _chain(0, 2, 1.5), [MID]),
    "lens_t1_n1": (lens_scene(), {}, _chain(0, 1, 1.0), [MID]),
    "room_r1": (with_surfaces(room_scene()), {}, _chain(1), [PADDED]),
    "room_turned_r2": (with_surfaces(room_scene()), TURNED, _chain(2), [MID]),
    "room_turned_r4": (with_surfaces(room_scene()), TURNED, _chain(4), [MID, PADDED]),
    "room_t1_n1": (with_surfaces(room_scene()), {}, _chain(0, 1, 1.0), [PADDED]),
    "room_turned_t2_n1.33": (with_surfaces(room_scene()), TURNED, _chain(0, 2, 1.33), [MID]),
    "room_turned_t3_n1.5": (with_surfaces(room_scene()), TURNED, _chain(0, 3, 1.5), [MID, PADDED]),
    "room_turned_r2_t2_n1.5": (with_surfaces(room_scene()), TURNED, _chain(2, 2, 1.5), [MID]),
    "room_r2_t2_n1.5": (with_surfaces(room_scene()), {}, _chain(2, 2, 1.5), [PADDED]),
    # from the origin 4.9 % of the hit pixels show another sphere; from (2, 8, 1), among the spheres and outside every one, 10.9 %
    "random_8_8_r2": (with_surfaces(random_scene(8, 8)), dict(pos=(2.0, 8.0, 1.0)), _chain(2), [MID]),
    "config_r1_t1_n1.33": (with_surfaces(startup_scene()), {}, _chain(1, 1, 1.33, **OTHER_CONFIG), [MID]),  # ray_radius 0.02
}
CHAIN_FRAMES = [(name, w, h) for name, case in CHAIN_CASES.items() for w, h in case[3]]
GPU_ONLY_CHAIN_FRAMES = [("room_r2_t2_n1.5", 512, 288)]
CAP_AMBIGUOUS = 0.01
CAP_PINNED ={"open": 0.50, "room": 0.20}
CAP_ROOM_MEDIAN_WIDTH = 0.05


def check_caps(name, rgb):
    """The caps as assertions on a check_rgb result of case `name`."""
    kind = CASES[name][3]
    assert rgb["ambiguous"] <= CAP_AMBIGUOUS, rgb
    if kind:
        assert rgb["pinned"] >= CAP_PINNED[kind], rgb
    if kind == "room":
        assert rgb["median_width"] <= CAP_ROOM_MEDIAN_WIDTH, rgb


# ---- measurement ---------------------------------------------------------------------------------------------------------------
def oracle_frame(name, w, h, jitter=(0, 0), march_algorithm=3):
    """The case rendered by oracle A (CPU), at one sample's jitter and with one of the march algorithms."""
    import oracle as O

    scene, view, conf = CASES[name][:3]
    cfg = O.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    cfg.march_algorithm = march_algorithm
    ref = O.render_a(O.scene_from_bytes(scene), w, h, cfg=cfg, jitter=jitter, **view)
    fr = Frame(scene, w, h, levels=ref["levels"], rgb=ref["rgb"], jitter=jitter, march_algorithm=march_algorithm, **view, **conf)
    fr.name = name
    return fr


def oracle_chain_frame(name, w, h):
    """The chain case rendered by oracle A (CPU) with its recorded marches; fr.counters = the oracle's counters."""
    import oracle as O

    scene, view, conf = CHAIN_CASES[name][:3]
    cfg = O.default_config()
    for k, v in conf.items():
        setattr(cfg, k, v)
    ref = O.render_a(O.scene_from_bytes(scene), w, h, cfg=cfg, want_chains=True, **view)
    fr = Frame(scene, w, h, levels=ref["levels"], rgb=ref["rgb"], chains=ref["chains"], **view, **conf)
    fr.name, fr.counters = name, ref["counters"]
    return fr


def measure_chains(out=sys.stdout):
    """Largest excursions of oracle A's recorded marches and chain RGB over every chain case, with no tolerance, and the largest
    fp32-against-float64 differences of the branch quantities (the guards are not applied to themselves: they are measured over all
    pixels; the excursions over the pixels the committed guards keep)."""
    worst = dict(eye=0.0, dir=0.0, len=0.0, rgb=0.0, guard_k=0.0, guard_disc=0.0)
    for name, w, h in CHAIN_FRAMES + GPU_ONLY_CHAIN_FRAMES:
        fr = oracle_chain_frame(name, w, h)
        res = check_chains(fr, 0.0, 0.0, 0.0, 0.0)
        for k in worst:
            worst[k] = max(worst[k], res[k])
        print(f"{name} {w}x{h}: eye {res['eye']:.3g} dir {res['dir']:.3g} len {res['len']:.3g} rgb {res['rgb']:.3g} | NaN pattern wrong {res['bad_nan']} | "
              f"left out {100 * res['left_out']:.2f} %, secondary light on {100 * res['covered']:.1f} % of {res['hits']} hit pixels | marches: mirror "
              f"{res['n_mirror']} ({res['miss_mirror']} missed), transmitted {res['n_trans']} ({res['miss_trans']} missed) | fp32 - float64: k {res['guard_k']:.3g}, "
              f"disc / r^2 {res['guard_disc']:.3g}", file=out)
    for k, label in (("eye", "EPS_CHAIN_EYE"), ("dir", "EPS_CHAIN_DIR"), ("len", "EPS_CHAIN_LEN"), ("rgb", "EPS_CHAIN_RGB"), ("guard_k", "GUARD_K"), ("guard_disc", "GUARD_DISC")):
        print(f"chains: largest {k} = {worst[k]:.4g}  -> {label} = {4 * worst[k]:.4g}", file=out)
    return worst


def average(rgbs):
    """fp32 frames added in index order, ((s0 + s1) + s2) + ..., then divided by their number."""
    acc = np.asarray(rgbs[0], np.float32)
    for f in rgbs[1:]:
        acc = acc + np.asarray(f, np.float32)
    return acc / np.float32(len(rgbs))


def oracle_samples(name, w, h, spp):
    """The spp per-sample frames of the case by oracle A, and their average."""
    frames = [oracle_frame(name, w, h, jitter=sample_jitter(s, spp, w, h)) for s in range(spp)]
    return frames, average([fr.rgb for fr in frames])


def measure(out=sys.stdout):
    """Largest excursions of oracle A's frames from the bands, every frame of both test files, with no tolerance."""
    worst_d = worst_c = 0.0

    def line(label, depth, rgb):
        nonlocal worst_d, worst_c
        ed = max(x["excursion"] for x in depth)
        worst_d, worst_c = max(worst_d, ed), max(worst_c, rgb["excursion"])
        print(f"{label:28s} depth: {sum(x['bad'] for x in depth):5d} of {sum(x['n'] for x in depth):6d} outside, worst {ed:.3g}, "
              f"parent missed and child hit {sum(x['far_bad'] for x in depth)} | rgb: {rgb['bad']:5d} of {rgb['hits']:6d} outside, worst {rgb['excursion']:.3g}, "
              f"ambiguous {100 * rgb['ambiguous']:.2f} %, pinned {100 * rgb['pinned']:.1f} %, median width {rgb['median_width']:.3g}", file=out)

    for name, w, h in FRAMES + GPU_ONLY_FRAMES:
        line(f"{name} {w}x{h}", *check_frame(oracle_frame(name, w, h), 0.0, 0.0))
    for name, w, h in ALG1_FRAMES:
        line(f"{name} {w}x{h} alg 1", *check_frame(oracle_frame(name, w, h, march_algorithm=1), 0.0, 0.0))
    for name, w, h, spp in SAMPLE_FRAMES + GPU_ONLY_SAMPLE_FRAMES:
        frames, rgb = oracle_samples(name, w, h, spp)
        per_sample = [check_rgb(fr, 0.0) for fr in frames]
        res = check_samples(frames, rgb, 0.0, 0.0)
        worst_c = max(worst_c, max(x["excursion"] for x in per_sample))
        print(f"{name} {w}x{h} {spp} spp: largest rgb excursion of one sample {max(x['excursion'] for x in per_sample):.3g}, of all samples' "
              f"depth {max(x['excursion'] for lv in res['depth'] for x in lv):.3g}; averaged:", file=out)
        line("", [x for lv in res["depth"] for x in lv], res)
    print(f"largest depth excursion / (1 + depth) = {worst_d:.4g}  -> EPS_DEPTH = {4 * worst_d:.4g}", file=out)
    print(f"largest rgb excursion = {worst_c:.4g}  -> EPS_RGB = {4 * worst_c:.4g}", file=out)
    return worst_d, worst_c


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["chains"]:  # `chains`: only the new measurements
        measure()
    measure_chains()
