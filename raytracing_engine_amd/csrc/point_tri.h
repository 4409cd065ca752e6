// point_tri.h — the arithmetic of path B's closest-point query, defined once for the kernel (pt_query_points,
// pt_point_query.hip) and for the tests' reference (tests/native/point_query_ref.cpp).  Compiled by plain g++ and by hipcc; every function is
// host + device under hipcc.  fp32 only, after DESIGN.md §4: every fused multiply-add is an explicit __builtin_fmaf, dot() in §4's
// order, correctly rounded / (and sqrt at the callers), no contraction (-ffp-contract=off on both sides).  The same operations in
// the same order on both sides, so the two agree bit for bit.
//
// THE ANSWER, without a tree: the lexicographic minimum of (d2, original triangle index) over all triangles whose d2 < limit2,
// d2 = closest_on_tri(...).d2, limit2 = rmax * rmax as one fp32 product (+inf without a limit).  A walk of the BVH8 may skip a
// child box or a leaf only when child_lb2(...) > the best d2 it holds (strictly: a tie must reach the index comparison); §6.14
// shows that then  child_lb2 <= d2  holds in fp32 for every triangle under the box, with no slack term, so a walk returns the
// tree-free answer whatever its order.
#pragma once
#include "bvh_node.h"

namespace rt {

struct P3 {
    float x, y, z;
};
RT_HD P3 p3_sub(P3 a, P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_HD float p3_dot(P3 a, P3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }  // §4's order
RT_HD P3 p3_cross(P3 a, P3 b) {
    return P3{__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x))};
}

// ---- closest point on a triangle --------------------------------------------------------------------------------------------------
// The point of the triangle at (u, v):  c = v0 + e1 u + e2 v, two fmas per component
RT_HD P3 tri_point(P3 v0, P3 e1, P3 e2, float u, float v) {
    return P3{__builtin_fmaf(e2.x, v, __builtin_fmaf(e1.x, u, v0.x)), __builtin_fmaf(e2.y, v, __builtin_fmaf(e1.y, u, v0.y)),
              __builtin_fmaf(e2.z, v, __builtin_fmaf(e1.z, u, v0.z))};
}
RT_HD float tri_point_d2(P3 p, P3 v0, P3 e1, P3 e2, float u, float v) {
    const P3 d = p3_sub(p, tri_point(v0, e1, e2, u, v));
    return p3_dot(d, d);
}
// parameter of the point of the segment a + t e, 0 <= t <= 1, nearest to a + ap.  A segment without length (ee = 0, or so short
// that ee underflows) gives 0; a NaN quotient (inf / inf after an overflow) gives 0 as well: both comparisons are false for it.
RT_HD float segment_param(P3 ap, P3 e) {
    const float ee = p3_dot(e, e);
    float t = ee > 0.0f ? p3_dot(ap, e) / ee : 0.0f;
    t = t > 0.0f ? t : 0.0f;
    return t < 1.0f ? t : 1.0f;
}

struct ClosestTri {
    float d2, u, v;
};
// p against the triangle record's v0, e1, e2 - the words the kernels fetch.  Returns the squared distance to c = tri_point(u, v) and
// (u, v) itself, with u >= 0, v >= 0 and u + v <= 1 up to one rounding (u + v <= 1 + 2^-24), so that c is a point of the triangle up
// to the rounding of its own evaluation and d2 can undershoot the exact squared distance only by that, however thin the triangle.
//
// Method: the minimum over (at most) four candidates that all lie in the closed triangle - the nearest point of each of the three
// edge segments, and the foot of the perpendicular when it falls inside.  It is Ericson's region method (Real-Time Collision
// Detection §5.1.5) with the region chosen by the distances themselves and not by the signs of six dot products: the signs of
// d1 d4 - d3 d2 and its kin cancel catastrophically for needles, and a wrong region is a wrong answer by the needle's length, while a
// candidate that is merely evaluated inexactly is still a point of the triangle.  A triangle without area (collinear or equal
// vertices: n = 0, or nn underflows) has no fourth candidate and is the segments, or the point, it consists of; no division by
// zero, no NaN: a NaN foot (overflow) fails `inside`.  Candidates replace one another only when strictly nearer, in the order below.
RT_HD ClosestTri closest_on_tri(P3 p, P3 v0, P3 e1, P3 e2) {
    const P3 ap = p3_sub(p, v0);
    ClosestTri best;
    best.u = segment_param(ap, e1);  // edge v0 -> v0 + e1
    best.v = 0.0f;
    best.d2 = tri_point_d2(p, v0, e1, e2, best.u, 0.0f);
    {
        const float t = segment_param(ap, e2);  // edge v0 -> v0 + e2
        const float d2 = tri_point_d2(p, v0, e1, e2, 0.0f, t);
        if (d2 < best.d2) best = ClosestTri{d2, 0.0f, t};
    }
    {
        const float t = segment_param(p3_sub(ap, e1), p3_sub(e2, e1));  // edge v0 + e1 -> v0 + e2
        const float u = 1.0f - t;
        const float d2 = tri_point_d2(p, v0, e1, e2, u, t);
        if (d2 < best.d2) best = ClosestTri{d2, u, t};
    }
    const P3 n = p3_cross(e1, e2);
    const float nn = p3_dot(n, n);
    if (nn > 0.0f) {  // p = v0 + u e1 + v e2 + w n:  (ap x e2) . n = u nn,  (e1 x ap) . n = v nn
        const float u = p3_dot(p3_cross(ap, e2), n) / nn, v = p3_dot(p3_cross(e1, ap), n) / nn;
        if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f) {
            const float d2 = tri_point_d2(p, v0, e1, e2, u, v);
            if (d2 < best.d2) best = ClosestTri{d2, u, v};
        }
    }
    return best;
}

// (d2, id) against the best so far: nearer, or as near with the lower original index
RT_HD bool nearer(float d2, uint32_t id, float best_d2, uint32_t best_id) { return d2 < best_d2 || (d2 == best_d2 && id < best_id); }

// ---- lower bound of a child box -------------------------------------------------------------------------------------------------
// One axis: the planes as the node stores them (q = the plane's byte as a float, exact), decoded with one fma each, and how far p lies
// outside the slab between them.  (max of finite numbers: fmax is std::max here.)
RT_HD float axis_gap(float p, float origin, float scale, float qlo, float qhi) {
    const float lo = __builtin_fmaf(qlo, scale, origin), hi = __builtin_fmaf(qhi, scale, origin);
    return __builtin_fmaxf(__builtin_fmaxf(lo - p, p - hi), 0.0f);
}
RT_HD float gap_lb2(float gx, float gy, float gz) { return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx)); }  // dot(gap, gap)
// No slack: the derivation (§6.14) needs none.  lb2 <= d2 follows from  lo <= c <= hi  as fp32 numbers on every axis (the padding
// of 2e-5 M is 37 times the rounding of c plus that of the decoded plane) and from the monotonicity of rounded -, * and fma.

// child slot s of the node words w (bvh_node.h): squared distance from p to its box, 0 inside
RT_HD float child_lb2(const uint32_t* w, uint32_t s, P3 p) {
    const float pc[3] = {p.x, p.y, p.z};
    float g[3];
    for (int a = 0; a < 3; a++) {
        const uint32_t qlo = (w[8 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu, qhi = (w[14 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu;
        g[a] = axis_gap(pc[a], node_origin(w, a), node_scale(w, a), (float)qlo, (float)qhi);
    }
    return gap_lb2(g[0], g[1], g[2]);
}

// ---- limits and validity --------------------------------------------------------------------------------------------------------
// rmax -> the bound on d2 (hit when d2 < limit2, strictly).  An rmax so small that its square underflows to 0 admits nothing.
RT_HD float point_limit2(float rmax) { return rmax * rmax; }
// a point the query answers: finite and within reach = 32 x max(1, largest |vertex coordinate|) on every axis (false for a NaN)
RT_HD bool point_in_reach(P3 p, float reach) { return __builtin_fabsf(p.x) <= reach && __builtin_fabsf(p.y) <= reach && __builtin_fabsf(p.z) <= reach; }

}  // namespace rt
