"""Synthetic triangle scenes for path B (BASELINE.json configs[2..4]).  The
reference has no triangle scenes: these are build-defined inputs, generated from a counter hash so
they are identical on every host and numpy version."""
import numpy as np


def _hash32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _uniform(seed, stream, n):
    """n floats in [0,1) on a 2^-24 grid: hash32(i + hash32(seed*0x9e3779b9 + stream))."""
    with np.errstate(over="ignore"):
        base = _hash32(np.uint32((seed * 0x9E3779B9 + stream) & 0xFFFFFFFF))
        h = _hash32(np.arange(n, dtype=np.uint32) + base)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _quad(p0, p1, p2, p3):
    return [np.concatenate([p0, p1, p2]), np.concatenate([p0, p2, p3])]


def soup_scene(n_tris, seed=1, edge=0.25, light_emission=(30.0, 30.0, 30.0)):
    """n_tris random triangles: v0 ~ U([-10,10] x [5,25] x [-10,10]), edges ~ U(-edge,edge)^3,
    albedo ~ U(0.2,0.9); the last two triangles are replaced by one emissive quad overhead
    (z = 12, facing down).  Returns (verts[n,9], albedo[n,3], emission[n,3]) float32."""
    n = int(n_tris)
    assert n >= 3
    u = [_uniform(seed, k, n) for k in range(12)]
    v0 = np.stack([u[0] * 20 - 10, u[1] * 20 + 5, u[2] * 20 - 10], 1).astype(np.float32)
    e1 = (np.stack(u[3:6], 1) * 2 - 1).astype(np.float32) * np.float32(edge)
    e2 = (np.stack(u[6:9], 1) * 2 - 1).astype(np.float32) * np.float32(edge)
    verts = np.concatenate([v0, v0 + e1, v0 + e2], 1).astype(np.float32)
    albedo = (np.stack(u[9:12], 1) * np.float32(0.7) + np.float32(0.2)).astype(np.float32)
    emission = np.zeros((n, 3), np.float32)
    f = np.float32
    quad = _quad(np.array([-4, 11, 12], f), np.array([4, 11, 12], f), np.array([4, 19, 12], f), np.array([-4, 19, 12], f))
    verts[n - 2], verts[n - 1] = quad
    albedo[n - 2:] = 0.0
    emission[n - 2:] = np.asarray(light_emission, f)
    return verts, albedo, emission


def cornell_tri_scene():
    """A small closed room (x,z in [-6,6], y in [0,22]) with a ceiling light and two boxes: 7 quads
    + 2 boxes = 38 triangles.  Camera at (0,1,0) looking +Y sees the whole room."""
    f = np.float32
    tris, alb, emi = [], [], []

    def add(q, a, e=(0, 0, 0)):
        for t in _quad(*[np.array(p, f) for p in q]):
            tris.append(t)
            alb.append(a)
            emi.append(e)

    X, Z, Y0, Y1 = 6.0, 6.0, 0.0, 22.0
    white, red, green = (0.75, 0.75, 0.75), (0.75, 0.15, 0.15), (0.15, 0.75, 0.15)
    add([(-X, Y0, -Z), (X, Y0, -Z), (X, Y1, -Z), (-X, Y1, -Z)], white)  # floor
    add([(-X, Y0, Z), (-X, Y1, Z), (X, Y1, Z), (X, Y0, Z)], white)      # ceiling
    add([(-X, Y1, -Z), (X, Y1, -Z), (X, Y1, Z), (-X, Y1, Z)], white)    # back wall
    add([(-X, Y0, -Z), (-X, Y1, -Z), (-X, Y1, Z), (-X, Y0, Z)], red)    # left
    add([(X, Y0, -Z), (X, Y0, Z), (X, Y1, Z), (X, Y1, -Z)], green)      # right
    add([(-X, Y0, -Z), (-X, Y0, Z), (X, Y0, Z), (X, Y0, -Z)], white)    # wall behind the camera
    add([(-2, 9, Z - 0.01), (-2, 13, Z - 0.01), (2, 13, Z - 0.01), (2, 9, Z - 0.01)], (0, 0, 0), (15, 15, 15))  # light

    def box(cx, cy, cz, sx, sy, sz, a):
        x0, x1, y0, y1, z0, z1 = cx - sx, cx + sx, cy - sy, cy + sy, cz - sz, cz + sz
        add([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], a)
        add([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)], a)
        add([(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)], a)
        add([(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)], a)
        add([(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], a)
        add([(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], a)

    box(-2.5, 14, -3.0, 1.8, 1.8, 3.0, (0.7, 0.7, 0.3))
    box(2.5, 10, -4.5, 1.5, 1.5, 1.5, (0.3, 0.5, 0.8))
    return np.array(tris, f), np.array(alb, f), np.array(emi, f)


SURFACE_LAMBERT, SURFACE_MIRROR, SURFACE_GLASS = 0, 1, 2  # rt_set_mesh_surfaces kinds


def cornell_surfaces_scene(ior=1.5):
    """cornell_tri_scene with a mirror box and a glass box: the tall box (triangles 14-25) is a mirror
    tinted 0.9, the short box (26-37) clear glass (albedo 1) of index `ior`; both are wound outward, as glass needs.
    Returns (verts, albedo, emission, kind[n] uint32, ior[n] float32)."""
    v, a, e = cornell_tri_scene()
    n = len(v)
    kind = np.full(n, SURFACE_LAMBERT, np.uint32)
    eta = np.ones(n, np.float32)
    kind[14:26] = SURFACE_MIRROR
    a[14:26] = 0.9
    kind[26:38] = SURFACE_GLASS
    a[26:38] = 1.0
    eta[26:38] = ior
    return v, a, e, kind, eta


def soup_surfaces(n_tris, seed=1, mirror_frac=0.1, glass_frac=0.1, ior=1.5):
    """Surface kinds for soup_scene(n_tris, seed): with u = stream 12 of the counter hash (soup_scene uses 0-11), triangle i
    is a mirror if u_i < mirror_frac, glass if u_i < mirror_frac + glass_frac (fp32 sum), Lambert otherwise; the light quad
    stays Lambert.  Returns (kind[n] uint32, ior[n] float32, `ior` everywhere)."""
    n = int(n_tris)
    u = _uniform(seed, 12, n)
    m = np.float32(mirror_frac)
    g = np.float32(m + np.float32(glass_frac))
    kind = np.where(u < m, SURFACE_MIRROR, np.where(u < g, SURFACE_GLASS, SURFACE_LAMBERT)).astype(np.uint32)
    kind[n - 2:] = SURFACE_LAMBERT
    return kind, np.full(n, np.float32(ior), np.float32)


def terrain_scene(grid=708, seed=1, light_emission=(6.0, 6.0, 6.0)):
    """A closed-surface scene for context (the soup is a participating-medium-like worst case): a
    height field of grid x grid cells = 2*grid^2 triangles over x in [-30,30], y in [2,62] (the camera at
    the origin looks along +Y and slightly down onto it), heights from three octaves of hashed value
    noise, plus the same emissive quad overhead.  grid=708 gives 1 002 528 + 2 triangles."""
    f = np.float32
    n = int(grid)

    def lattice(cells, stream):
        return _uniform(seed, stream, (cells + 1) * (cells + 1)).reshape(cells + 1, cells + 1)

    def value_noise(cells, stream):
        lat = lattice(cells, stream)
        t = np.linspace(0, cells, n + 1, dtype=np.float64)
        i = np.minimum(t.astype(np.int64), cells - 1)
        fr = (t - i)
        fr = fr * fr * (3 - 2 * fr)
        a = lat[i][:, i] * (1 - fr)[None, :] + lat[i][:, i + 1] * fr[None, :]
        b = lat[i + 1][:, i] * (1 - fr)[None, :] + lat[i + 1][:, i + 1] * fr[None, :]
        return a * (1 - fr)[:, None] + b * fr[:, None]

    hgt = (6.0 * value_noise(6, 20) + 2.0 * value_noise(24, 21) + 0.5 * value_noise(96, 22)).astype(f) - f(9.0)
    xs = np.linspace(-30, 30, n + 1, dtype=f)
    ys = np.linspace(2, 62, n + 1, dtype=f)
    X, Y = np.meshgrid(xs, ys)
    P = np.stack([X, Y, hgt], -1)  # (n+1, n+1, 3)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t1 = np.concatenate([p00, p10, p11], -1).reshape(-1, 9)
    t2 = np.concatenate([p00, p11, p01], -1).reshape(-1, 9)
    verts = np.concatenate([t1, t2]).astype(f)
    m = len(verts)
    u = [_uniform(seed, 30 + k, m) for k in range(3)]
    albedo = (np.stack(u, 1) * f(0.4) + f(0.4)).astype(f)
    emission = np.zeros((m, 3), f)
    quad = _quad(np.array([-6, 20, 14], f), np.array([6, 20, 14], f), np.array([6, 32, 14], f), np.array([-6, 32, 14], f))
    verts = np.concatenate([verts, np.array(quad, f)])
    albedo = np.concatenate([albedo, np.zeros((2, 3), f)])
    emission = np.concatenate([emission, np.tile(np.asarray(light_emission, f), (2, 1))])
    return verts, albedo, emission


def planet_scene(n_tris=1000000, seed=1, radius=10.0, centre=(0.0, 20.0, 0.0), relief=0.12, light_emission=(6.0, 6.0, 6.0)):
    """A CLOSED surface (terrain_scene is an open height field): a UV sphere of `stacks` x 2 `stacks` cells, stacks =
    round(sqrt(n_tris / 4)), whose vertices are pushed along their directions by three octaves of hashed 3-D value noise (radius x
    (1 +- relief)), so that the surface has hills and hollows at several scales and still bounds a volume: every edge is shared by
    exactly two triangles, bit for bit (vertices are shared by index, the poles are single vertices), and all triangles are wound
    outward.  4 stacks (stacks - 1) triangles: 1 000 000 gives stacks = 500 and 998 000.  The last triangle is emissive (the mesh
    needs one light and stays closed).  Returns (verts[n,9], albedo[n,3], emission[n,3]) float32."""
    f = np.float32
    stacks = max(3, int(round((int(n_tris) / 4.0) ** 0.5)))
    slices = 2 * stacks

    def value_noise3(q, cells, stream):  # q in [-1, 1]^3
        lat = _uniform(seed, stream, (cells + 1) ** 3).astype(np.float64).reshape(cells + 1, cells + 1, cells + 1)
        t = (q + 1.0) * (0.5 * cells)
        i = np.minimum(t.astype(np.int64), cells - 1)
        fr = t - i
        fr = fr * fr * (3 - 2 * fr)
        out = 0.0
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    w = np.where(dx, fr[..., 0], 1 - fr[..., 0]) * np.where(dy, fr[..., 1], 1 - fr[..., 1]) * np.where(dz, fr[..., 2], 1 - fr[..., 2])
                    out = out + w * lat[i[..., 0] + dx, i[..., 1] + dy, i[..., 2] + dz]
        return out

    th = np.pi * np.arange(1, stacks, dtype=np.float64) / stacks
    ph = 2 * np.pi * np.arange(slices, dtype=np.float64) / slices
    dirs = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.cos(th)[:, None] * np.ones_like(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :]], -1)
    dirs = np.concatenate([dirs.reshape(-1, 3), [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]])  # the rings, then the two poles
    h = (4.0 * value_noise3(dirs, 3, 90) + 2.0 * value_noise3(dirs, 12, 91) + 1.0 * value_noise3(dirs, 48, 92)) / 7.0  # in [0, 1)
    P = (np.asarray(centre, np.float64) + dirs * (radius * (1.0 + relief * (2.0 * h - 1.0)))[:, None]).astype(f)
    ring = np.arange((stacks - 1) * slices).reshape(stacks - 1, slices)
    north, south = (stacks - 1) * slices, (stacks - 1) * slices + 1
    nxt = np.roll(ring, -1, axis=1)  # the vertex one slice on, wrapping
    a, b, c, d = ring[:-1], ring[1:], nxt[:-1], nxt[1:]  # (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)
    idx = np.concatenate([np.stack([a, d, b], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3),
                          np.stack([np.full(slices, north), nxt[0], ring[0]], -1), np.stack([np.full(slices, south), ring[-1], nxt[-1]], -1)])
    verts = P[idx].reshape(-1, 9)
    m = len(verts)
    u = [_uniform(seed, 93 + k, m) for k in range(3)]
    albedo = (np.stack(u, 1) * f(0.4) + f(0.4)).astype(f)
    emission = np.zeros((m, 3), f)
    albedo[m - 1] = 0.0
    emission[m - 1] = np.asarray(light_emission, f)
    return np.ascontiguousarray(verts, f), albedo, emission


def sliver_stack_scene(n_layers=2048, n_targets=48, seed=1):
    """Adversarial scene for the traversal's leaf-hit buffers: n_layers parallel triangles stacked along the view axis (y in [4, 6]),
    every one covering the half x + z < 0 of the square x, z in [-8, 8].  A ray through the other half passes through every
    layer's box and hits none, so every leaf-parent node it visits hands it up to 8 leaf hits and its tmax never culls.
    n_targets small rectangles (two triangles each) at hashed depths inside the stack, in the half x + z > 0, give such rays
    different closest hits; a backdrop at y = 10 and an emitter between the camera and the stack (out of a 90-degree view from
    the origin) send bounce and shadow rays back through it.  Camera at the origin looking +Y.
    Returns (verts[n,9], albedo[n,3], emission[n,3]) float32."""
    f = np.float32
    n = int(n_layers)
    ys = (np.float64(4.0) + 2.0 * (np.arange(n, dtype=np.float64) + 0.5) / n).astype(f)
    layers = np.zeros((n, 9), f)
    layers[:, 0], layers[:, 2] = -8.0, -8.0  # (x, z) = (-8, -8), (8, -8), (-8, 8)
    layers[:, 3], layers[:, 5] = 8.0, -8.0
    layers[:, 6], layers[:, 8] = -8.0, 8.0
    layers[:, 1] = layers[:, 4] = layers[:, 7] = ys
    u = [_uniform(seed, 40 + k, n_targets) for k in range(6)]
    tris = [layers]
    for i in range(n_targets):  # centre in the miss half, 0.4 .. 1.6 wide, depth strictly inside the stack
        cx, cz = f(u[0][i] * 7.0 - 0.5), f(u[1][i] * 7.0 - 0.5)
        cx, cz = (cx, cz) if cx + cz > 1.0 else (f(cx + 2.0), f(cz + 2.0))
        hx, hz = f(0.2 + 0.6 * u[2][i]), f(0.2 + 0.6 * u[3][i])
        y = f(4.05 + 1.9 * u[4][i])
        tris.append(np.array(_quad(np.array([cx - hx, y, cz - hz], f), np.array([cx + hx, y, cz - hz], f),
                                   np.array([cx + hx, y, cz + hz], f), np.array([cx - hx, y, cz + hz], f)), f))
    back = _quad(np.array([-20, 10, -20], f), np.array([20, 10, -20], f), np.array([20, 10, 20], f), np.array([-20, 10, 20], f))
    light = _quad(np.array([2, 1, 2], f), np.array([2, 1, 5], f), np.array([5, 1, 5], f), np.array([5, 1, 2], f))
    tris += [np.array(back, f), np.array(light, f)]
    verts = np.concatenate(tris).astype(f)
    m = len(verts)
    albedo = np.empty((m, 3), f)
    albedo[:n] = (0.7, 0.7, 0.7)
    tu = [_uniform(seed, 50 + k, m - n - 4) for k in range(3)]
    albedo[n:m - 4] = np.stack(tu, 1) * f(0.7) + f(0.2)
    albedo[m - 4:m - 2] = (0.6, 0.6, 0.6)
    albedo[m - 2:] = 0.0
    emission = np.zeros((m, 3), f)
    emission[m - 2:] = (20.0, 20.0, 20.0)
    return verts, albedo, emission


def deep_scene(n_clusters=48, per_cluster=24, ratio=0.45, spread=0.2, scale=4.0, seed=1):
    """Adversarial scene for the traversal stack and the BVH's depth: n_clusters clusters of per_cluster small triangles at
    geometrically shrinking sizes and distances from the origin (cluster k: centre ratio^k * scale * (0.5, 1, 0.3), triangles
    within spread * ratio^k * scale of it).  Binary SAH splits peel one cluster per level, down to the builder's depth cap, and
    the 8-wide collapse spends a node's slots on the big peeled cluster rather than on the small rest, so the compressed tree
    is about as deep as the binary one.  A backdrop at y = 3 * scale and an emitter above close the scene; a camera at the
    origin looking +Y starts inside every deep box.  Returns (verts[n,9], albedo[n,3], emission[n,3]) float32."""
    f = np.float32
    m = int(n_clusters) * int(per_cluster)
    k = np.repeat(np.arange(n_clusters, dtype=np.float64), per_cluster)
    s = (ratio ** k * scale)[:, None]
    u = [_uniform(seed, 60 + j, m).astype(np.float64) * 2.0 - 1.0 for j in range(9)]
    v0 = np.array([0.5, 1.0, 0.3]) * s + np.stack(u[0:3], 1) * spread * s
    v1 = v0 + np.stack(u[3:6], 1) * spread * s
    v2 = v0 + np.stack(u[6:9], 1) * spread * s
    verts = np.concatenate([v0, v1, v2], 1).astype(f)
    a = [_uniform(seed, 70 + j, m) for j in range(3)]
    albedo = (np.stack(a, 1) * f(0.6) + f(0.3)).astype(f)
    S, Y = f(4.0 * scale), f(3.0 * scale)
    back = _quad(np.array([-S, Y, -S], f), np.array([S, Y, -S], f), np.array([S, Y, S], f), np.array([-S, Y, S], f))
    light = _quad(np.array([-1, 1, 1.5], f) * f(scale), np.array([-1, 2, 1.5], f) * f(scale), np.array([1, 2, 1.5], f) * f(scale),
                  np.array([1, 1, 1.5], f) * f(scale))
    verts = np.concatenate([verts, np.array(back + light, f)])
    albedo = np.concatenate([albedo, np.array([[0.6, 0.6, 0.6]] * 2 + [[0, 0, 0]] * 2, f)])
    emission = np.zeros((m + 4, 3), f)
    emission[m + 2:] = (12.0, 12.0, 12.0)
    return verts, albedo, emission


# ---- many-light meshes (one light per Lambert vertex is picked uniformly from the light list) ---------------------

LIGHT_PATTERNS = ("none", "all", "first", "last", "every", "indices", "block", "random")


def light_mask(n_tris, pattern, *args):
    """Which of n_tris triangles (original indices) a named pattern lights, as a bool array: "none", "all", "first", "last",
    ("every", step): 0, step, 2 step, ...; ("indices", list); ("block", lo, hi): lo <= i < hi; ("random", frac, seed): triangle i
    is lit if u_i < frac (fp32), u = stream 80 of the counter hash."""
    n = int(n_tris)
    m = np.zeros(n, bool)
    if pattern == "none":
        assert not args
    elif pattern == "all":
        assert not args
        m[:] = True
    elif pattern == "first":
        assert not args
        m[0] = True
    elif pattern == "last":
        assert not args
        m[n - 1] = True
    elif pattern == "every":
        (step,) = args
        assert int(step) >= 1
        m[::int(step)] = True
    elif pattern == "indices":
        (ids,) = args
        ids = np.asarray(ids, np.int64)
        assert ids.size == 0 or (0 <= ids.min() and ids.max() < n)
        m[ids] = True
    elif pattern == "block":
        lo, hi = args
        assert 0 <= lo <= hi <= n
        m[int(lo):int(hi)] = True
    elif pattern == "random":
        frac, seed = args
        m = _uniform(int(seed), 80, n) < np.float32(frac)
    else:
        raise ValueError(f"unknown light pattern {pattern!r} (one of {LIGHT_PATTERNS})")
    return m


def light_emission(n_tris, level=6.0):
    """The emission triangle i has when a pattern lights it: level * (0.25 + 1.5 u_i) per channel, u = streams 81-83 of the
    counter hash with seed 0, so it depends on the original index alone and no two lights of a mesh share a colour.  A frame
    therefore changes when a light list holds the right set in another order or an emission is gathered from another triangle."""
    u = np.stack([_uniform(0, 81 + k, int(n_tris)) for k in range(3)], 1)
    return (np.float32(level) * (np.float32(0.25) + np.float32(1.5) * u)).astype(np.float32)


def with_lights(mesh, pattern, *args, level=6.0):
    """A copy of mesh = (verts, albedo, emission) whose emission array is light_emission(n, level) on the triangles that
    light_mask(n, pattern, *args) names and zero elsewhere (lights the mesh had before are put out).
    Returns (verts[n,9], albedo[n,3], emission[n,3]) float32."""
    v = np.ascontiguousarray(mesh[0], np.float32).reshape(-1, 9).copy()
    a = np.ascontiguousarray(mesh[1], np.float32).reshape(-1, 3).copy()
    m = light_mask(len(v), pattern, *args)
    e = np.where(m[:, None], light_emission(len(v), level), np.float32(0.0)).astype(np.float32)
    return v, a, e


TESS_LIGHT = dict(x=(-2.0, 2.0), y=(8.0, 12.0), z=3.0, radiance=40.0, floor_z=-2.0, floor_albedo=0.8)  # tessellated_light_scene's geometry


def tessellated_light_scene(k, ratio=1.0):
    """A diffuse floor (z = -2, albedo 0.8, x in [-50, 50], y in [0, 100]) under a rectangular light (x in [-2, 2], y in [8, 12],
    z = 3, radiance 40) cut along x into k strips whose widths form a geometric series with quotient `ratio`, two triangles per
    strip: 2 k lights whose areas span ratio^(k-1), the same emitter for every (k, ratio).  Neighbouring strips share their
    fp32 edge, and the outer edges are exactly -2 and 2.  Returns (verts[2+2k,9], albedo, emission) float32; the floor is
    triangles 0 and 1."""
    f = np.float32
    k = int(k)
    assert k >= 1 and ratio > 0
    g = TESS_LIGHT
    w = np.float64(ratio) ** np.arange(k, dtype=np.float64)
    x0, x1 = g["x"]
    edges = np.concatenate([[x0], x0 + (x1 - x0) * np.cumsum(w) / w.sum()]).astype(f)
    edges[-1] = x1
    assert (np.diff(edges) > 0).all(), "a strip is narrower than fp32 resolves"
    y0, y1, z, fz = f(g["y"][0]), f(g["y"][1]), f(g["z"]), f(g["floor_z"])
    tris = _quad(np.array([-50, 0, fz], f), np.array([50, 0, fz], f), np.array([50, 100, fz], f), np.array([-50, 100, fz], f))
    for j in range(k):
        a, b = edges[j], edges[j + 1]
        tris += _quad(np.array([a, y0, z], f), np.array([b, y0, z], f), np.array([b, y1, z], f), np.array([a, y1, z], f))
    n = 2 + 2 * k
    albedo = np.zeros((n, 3), f)
    albedo[:2] = g["floor_albedo"]
    emission = np.zeros((n, 3), f)
    emission[2:] = g["radiance"]
    return np.array(tris, f), albedo, emission
