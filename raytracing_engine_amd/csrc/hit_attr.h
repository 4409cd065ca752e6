// hit_attr.h — the arithmetic of path B's hit attributes: where in the winning triangle a closest hit or a closest
// point lies, and which way the triangle faces.  Defined once for the kernels (the ATTR instantiations of pt_query_rays, pt_trace.hip,
// and of pt_query_points, pt_point_query.hip) and for the tests' reference (tests/native/hit_attr_ref.cpp).  Compiled by plain g++ and
// by hipcc; every function is host + device under hipcc.  fp32 only, after DESIGN.md §4: every fused multiply-add is an explicit
// __builtin_fmaf, dot() and cross() in §4's order (p3_dot, p3_cross of point_tri.h), correctly rounded / and sqrt, no contraction
// (-ffp-contract=off on both sides).  The same operations in the same order on both sides, so the two agree bit for bit.
//
// RAY BARYCENTRICS of a triangle record (v0, e1, e2):  ub = u / det,  vb = v / det  with u, v, det exactly the values that §6.3's
// ray / triangle test forms (tri_test / tri_inside_mask of pt_traverse.h, ray_tri_t of ray_parity.h: the same operations in the same
// order, ray_tri_uvdet below).  The hit point is v0 + ub e1 + vb e2; the weights of the caller's three vertices are
// (1 - ub - vb, ub, vb).  What the accept test implies for a triangle it accepted (ray_uvdet_accepted):
// (for finite u, v, det: products that overflow into inf - inf = NaN pass every comparison of the test, and nothing is claimed for them)
//   ub >= 0 and vb >= 0, as comparisons.  det > 0: the test passed !(u < 0), so u > 0 or u = +-0, and a correctly rounded quotient of
//     such a number by a positive one is > 0 or +-0.  det < 0: u <= 0 over det < 0, likewise.  So -0.0 can occur (u = -0 over det > 0,
//     u = +0 over det < 0); it compares equal to 0.
//   ub + vb <= 1 + 2^-22, the sum taken exactly.  Take det > 0 (det < 0: negate u, v, det).  The test passed !(fl(u + v) > det), so
//     fl(u + v) <= det, and fl(u + v) >= (u + v)(1 - 2^-24), so  u + v <= det / (1 - 2^-24).  Each quotient is correctly rounded:
//     ub <= (u / det)(1 + 2^-24), vb likewise (a quotient that underflows is off by at most 2^-150 absolutely, which the slack below
//     swallows), so  ub + vb <= (1 + 2^-24) / (1 - 2^-24) < 1 + 2^-23 + 2^-46 < 1 + 2^-22.
//
// UNIT GEOMETRIC NORMAL.  n = p3_cross(e1, e2), nn = p3_dot(n, n); for 0 < nn < inf the result is n / sqrt(nn), one correctly
// rounded square root and three correctly rounded divisions; otherwise - a triangle without area, or one so small or so large that
// nn underflows to 0 or overflows - three zeros.  Each component is off by at most 1.5 ulp of itself relative to n / |n| for the
// computed n (sqrt: 2^-25 from nn's rounding, half of 3 x 2^-24, plus its own 2^-24; the division 2^-24), so | |result|^2 - 1 | <=
// 2^-21 with room.  The orientation is that of the caller's winding, (v1 - v0) x (v2 - v0); it is never turned towards the ray or
// the point.
//
// POINT BARYCENTRICS are ClosestTri::u, v of the winning triangle exactly as closest_on_tri (point_tri.h) returns them: no new
// arithmetic.
#pragma once
#include "point_tri.h"

namespace rt {

struct RayUvDet {
    float u, v, det;
};
// u, v, det of §6.3's test for the ray (o, d) and the record (v0, e1, e2): tri_test's operations in tri_test's order
RT_HD RayUvDet ray_tri_uvdet(P3 o, P3 d, P3 v0, P3 e1, P3 e2) {
    const P3 pvec = p3_cross(d, e2);
    const float det = p3_dot(e1, pvec);
    const P3 tvec = p3_sub(o, v0);
    const float u = p3_dot(tvec, pvec);
    const P3 qvec = p3_cross(tvec, e1);
    const float v = p3_dot(d, qvec);
    return RayUvDet{u, v, det};
}
// tri_test's verdict on them (without the t > 0 that its callers add)
RT_HD bool ray_uvdet_accepted(RayUvDet a) {
    if (a.det == 0.0f) return false;
    if (a.det > 0.0f) return !(a.u < 0.0f || a.v < 0.0f || a.u + a.v > a.det);
    return !(a.u > 0.0f || a.v > 0.0f || a.u + a.v < a.det);
}

struct Bary {
    float u, v;
};
RT_HD Bary ray_bary(P3 o, P3 d, P3 v0, P3 e1, P3 e2) {
    const RayUvDet a = ray_tri_uvdet(o, d, v0, e1, e2);
    return Bary{a.u / a.det, a.v / a.det};
}

RT_HD P3 unit_normal(P3 e1, P3 e2) {
    const P3 n = p3_cross(e1, e2);
    const float nn = p3_dot(n, n);
    if (!(nn > 0.0f && nn < __builtin_inff())) return P3{0.0f, 0.0f, 0.0f};
    const float len = __builtin_sqrtf(nn);
    return P3{n.x / len, n.y / len, n.z / len};
}

// Row i of the two attribute arrays (n x 2 and n x 3), each only where the caller asked for it; without a winner - a miss, an
// invalid ray or point - every element is NaN
RT_HD void write_attr(float* uv_out, float* normal_out, size_t i, float u, float v, P3 n) {
    if (uv_out) {
        uv_out[2 * i] = u;
        uv_out[2 * i + 1] = v;
    }
    if (normal_out) {
        normal_out[3 * i] = n.x;
        normal_out[3 * i + 1] = n.y;
        normal_out[3 * i + 2] = n.z;
    }
}
RT_HD void write_no_attr(float* uv_out, float* normal_out, size_t i) {
    const float nan = __builtin_nanf("");
    write_attr(uv_out, normal_out, i, nan, nan, P3{nan, nan, nan});
}

}  // namespace rt
