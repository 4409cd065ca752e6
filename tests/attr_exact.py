"""Reference of path B's hit attributes, the float64 contract they are held to, and how its constants were set.

Test helper (imported by tests/test_hit_attr_host.py and tests/test_gpu_hit_attr.py); a sibling of tests/ray_exact.py and
tests/point_exact.py, whose meshes, families and float64 geometry it uses; not a conftest, no fixtures.

THE REFERENCE.  tests/native/hit_attr_ref.cpp: for every ray the brute-force winner over all triangles and csrc/hit_attr.h's barycentrics
and normal of it; for given triangles the normal alone.  The kernels must give its answers bit for bit.

THE CONTRACT, per hit, in float64 on the caller's three fp32 VERTICES V0, V1, V2 (not the fp32 edges the records hold):
  barycentrics  P = (1 - ub - vb) V0 + ub V1 + vb V2 lies within Kuv * unit of the exact ray / plane point Q = o + t_exact d of
                ray_exact.exact_pairs, the difference measured perpendicular to d (along d the two differ by the error of t, which is
                Kt's business, and for a grazing ray by 1 / |cos| times as much); unit = 2^-24 * S as in ray_exact.py, S = the largest
                |coordinate| among the origin, the triangle's vertices and Q.
  normal        | n - N | <= Kn * nunit, N = the float64 unit normal (V1 - V0) x (V2 - V0) / |..|, nunit = 2^-24 * max(1, S_tri / h):
                S_tri = the largest |coordinate| of the triangle's vertices, h = its smallest altitude.  The record's edges are
                fp32(V1 - V0), fp32(V2 - V0): each is off by up to 2^-24 S_tri, which tilts a triangle of altitude h by 2^-24 S_tri / h;
                the arithmetic after that (cross, dot, sqrt, three divisions) adds a few 2^-24.
                Triangles whose float64 doubled area is below 2^-63 are excluded: there the fp32 |n|^2 is subnormal or zero and the
                normal is defined as zero, or has lost its precision.  None of the ray families' meshes has one.

THE CONSTANTS.  measure() (python tests/attr_exact.py [rays per family]) finds the smallest Kuv and Kn for which the NATIVE BRUTE-FORCE
REFERENCE - never the kernel - satisfies the contract on all ten ray families.  Largest values found with 20 000 rays per family:
    Kuv_measured = 64162.4 (family g; a 5626.4, i 2567.8, f 1880.8, d 1785.0, b 1009.4, c 311.1, j 20.4, h 5.6, e 1.5)
    Kn_measured  = 0.406 (families a, b, c, d, i alike; g, j 0.177; f 0.005; e, h 0.000)
    excluded from the normal's contract: 0 in every family
Why Kuv is so much larger than K and Kt: ub and vb are quotients by det = -(d . n) |e1 x e2|, which the fp32 test forms as a sum of
products that cancel down to |cos| of their size, so det - and with it the offset of P from v0, in whatever direction that lies - is
good to 2^-24 / |cos| only.  Family (g) grazes at |cos| down to 1e-5; (a)'s tail are its few rays that happen to graze; the grazing
rays of (h) hit a grid whose offset from v0 is short against S.  A caller who needs the position at a grazing hit to fp32 accuracy
takes o + t d; the barycentrics are for interpolating what lives on the vertices.
Constants = four times the measurement, rounded up to a power of two (ray_exact.pow2_margin: the rule by which K and Kt were set):
    Kuv = 262144      Kn = 2
A swapped (ub, vb), barycentrics applied to the neighbouring triangle and a normal with one sign flipped are off by a fraction of a
triangle or of a unit vector, thousands of units: tests/test_hit_attr_host.py shows that the contract rejects them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_ref as NR  # noqa: E402
import ray_exact as RX  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
KUV = 262144.0
KN = 2.0
AREA2_MIN = 2.0 ** -63
f32 = np.float32


# ---- the native reference ------------------------------------------------------------------------------------------------------


def build_reference(sanitized=False, where=None):
    """Compiles tests/native/hit_attr_ref.cpp (once per process and flavour); returns the program's path."""
    return NR.build("hit_attr_ref", (), sanitized, where)


def reference(verts, o, d, tmax=None, tris=None, sanitized=False):
    """The native reference on mesh `verts` and rays (o, d).  Returns dict(t, tri, ub, vb, uvd (n, 3): u, v, det as the test forms
    them, normal (n, 3)[, tri_normals (len(tris), 3): the unit normals of the triangles `tris`, NaN rows for negative indices])."""
    o = np.ascontiguousarray(o, f32).reshape(-1, 3)
    d = np.ascontiguousarray(d, f32).reshape(-1, 3)
    n = len(o)
    inputs = dict(mesh=np.asarray(verts, f32), rays=np.concatenate([o, d], 1).astype(f32, copy=False), out=NR.OUT, tmax=None if tmax is None else np.asarray(tmax, f32))
    if tris is not None:
        inputs["tris"] = np.asarray(tris, np.int32)
    m = 0 if tris is None else inputs["tris"].size
    head, out = NR.unpack(NR.run(build_reference(sanitized), inputs), 1, (("t", f32, n), ("tri", np.int32, n), ("ub", f32, n), ("vb", f32, n), ("uvd", f32, 3 * n),
                                                                           ("normal", f32, 3 * n), ("tri_normals", f32, 3 * m)))
    assert head[0] == n
    out["uvd"], out["normal"], out["tri_normals"] = out["uvd"].reshape(n, 3), out["normal"].reshape(n, 3), out["tri_normals"].reshape(m, 3)
    if tris is None:
        del out["tri_normals"]
    return out


# ---- the float64 contract ------------------------------------------------------------------------------------------------------
def bary_point(em, tri, ub, vb):
    """P = (1 - ub - vb) V0 + ub V1 + vb V2 in float64 on the caller's vertices (em: ray_exact.ExactMesh)."""
    ub, vb = np.asarray(ub, np.float64)[:, None], np.asarray(vb, np.float64)[:, None]
    v = em.v[tri]
    return (1.0 - ub - vb) * v[:, 0] + ub * v[:, 1] + vb * v[:, 2]


def uv_needs(em, o, d, tri, ub, vb, point=None):
    """The Kuv each hit needs (0 for rows with tri < 0): the distance of P (or of `point`) from the exact ray / plane point, perpendicular to d, in units."""
    tri = np.asarray(tri)
    hit = tri >= 0
    tt = np.where(hit, tri, 0)
    o64, d64 = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    t, _, _ = RX.exact_pairs(np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3), em, tt)
    with np.errstate(invalid="ignore", over="ignore"):
        Q = o64 + t[:, None] * d64
        P = bary_point(em, tt, np.where(hit, ub, 0.0), np.where(hit, vb, 0.0)) if point is None else np.asarray(point, np.float64)
        diff = P - Q
        dh = d64 / np.sqrt((d64 * d64).sum(1, keepdims=True))
        perp = diff - (diff * dh).sum(1, keepdims=True) * dh
        S = np.maximum(np.maximum(np.abs(o64).max(1), em.vmax[tt]), np.abs(Q).max(1))
        need = np.sqrt((perp * perp).sum(1)) / (U * S)
    return np.where(hit, np.where(np.isnan(need), np.inf, need), 0.0)


def normal_unit(em, tri):
    """nunit of the triangles tri, and which of them the contract covers (float64 doubled area >= 2^-63)."""
    v = em.v[tri]
    edges = np.stack([np.linalg.norm(v[:, (k + 1) % 3] - v[:, k], axis=1) for k in range(3)], 1)
    area2 = em.area2[tri]
    covered = area2 >= AREA2_MIN
    with np.errstate(invalid="ignore", divide="ignore"):
        h = area2 / edges.max(1)
        unit = U * np.maximum(1.0, em.vmax[tri] / h)
    return unit, covered


def normal_needs(em, tri, normal):
    """(the Kn each hit needs - 0 for tri < 0 and for triangles the contract excludes -, the number of excluded hits)."""
    tri = np.asarray(tri)
    hit = tri >= 0
    tt = np.where(hit, tri, 0)
    unit, covered = normal_unit(em, tt)
    with np.errstate(invalid="ignore"):
        need = np.linalg.norm(np.asarray(normal, np.float64).reshape(-1, 3) - em.n[tt], axis=1) / unit
    use = hit & covered
    return np.where(use, np.where(np.isnan(need), np.inf, need), 0.0), int((hit & ~covered).sum())


def check_uv(em, o, d, tri, ub, vb, Kuv=None, point=None):
    return uv_needs(em, o, d, tri, ub, vb, point) <= (KUV if Kuv is None else Kuv)


def check_normal(em, tri, normal, Kn=None):
    return normal_needs(em, tri, normal)[0] <= (KN if Kn is None else Kn)


# ---- measuring the constants ---------------------------------------------------------------------------------------------------
def measure(n=20000, out=sys.stdout):
    """Smallest Kuv and Kn for which the native brute-force reference satisfies the contract, family by family."""
    worst_uv, worst_n = (0.0, None), (0.0, None)
    for name in RX.FAMILIES:
        k_uv, k_n, excluded, hits = 0.0, 0.0, 0, 0
        for part in RX.family(name, n):
            verts = RX.mesh(part["mesh"])[0]
            em = RX.ExactMesh(verts)
            ref = reference(verts, part["o"], part["d"])
            hits += int((ref["tri"] >= 0).sum())
            k_uv = max(k_uv, float(uv_needs(em, part["o"], part["d"], ref["tri"], ref["ub"], ref["vb"]).max()))
            need, ex = normal_needs(em, ref["tri"], ref["normal"])
            k_n, excluded = max(k_n, float(need.max())), excluded + ex
        print(f"family {name}: {hits:6d} hits   Kuv needed {k_uv:8.3f}   Kn needed {k_n:8.3f}   excluded from Kn {excluded}", file=out, flush=True)
        if k_uv > worst_uv[0]:
            worst_uv = (k_uv, name)
        if k_n > worst_n[0]:
            worst_n = (k_n, name)
    print(f"Kuv_measured = {worst_uv[0]:.3f} (family {worst_uv[1]}) -> Kuv = {RX.pow2_margin(worst_uv[0]):g}", file=out)
    print(f"Kn_measured = {worst_n[0]:.3f} (family {worst_n[1]}) -> Kn = {RX.pow2_margin(worst_n[0]):g}", file=out)
    return worst_uv, worst_n


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    measure(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
