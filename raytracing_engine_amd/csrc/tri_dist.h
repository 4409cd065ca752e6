// tri_dist.h — the arithmetic of path B's clearance query, defined once for the kernel (pt_query_clearance,
// pt_clearance_query.hip) and for the tests' reference (tests/native/clearance_query_ref.cpp).  Compiled by plain g++ and by hipcc;
// every function is host + device under hipcc.  fp32 only, after DESIGN.md §4: every fused multiply-add is an explicit __builtin_fmaf,
// p3_dot's order, correctly rounded / (and sqrt at the callers), no contraction.  The same operations in the same order on both
// sides, so the two agree bit for bit.
//
// THE ANSWER, without a tree.  Query triangle i has the vertices A0, A1, A2 as the caller gave them; F1 = A1 - A0, F2 = A2 - A0 (one
// fp32 subtraction per component); Q = query_box.  Mesh triangle T has the record words v0, e1, e2.  A pair's answer is
// (d2, uq, vq, um, vm) with  a = tri_point(A0, F1, F2, uq, vq),  c = tri_point(v0, e1, e2, um, vm),  d2 = p3_dot(a - c, a - c):
// the minimum of d2 over up to twenty-one candidates, every one a pair of barycentrics in the two closed triangles; a candidate
// replaces the best only when strictly nearer, in this order:
//     0 - 5   only where overlap_cand(Q, T): bit b of overlap_mask(i, T) (tri_overlap.h, the same six tests on the same arguments,
//             seg_pierce below).  Where the test accepts, the point at t on the edge and the point at (u / det, v / det), clamped, in the
//             pierced triangle - for two triangles that intersect this pair is the pierce point twice and d2 is its rounding, 0 or
//             a few 2^-48 S^2.  The test PROPOSES a pair; what counts is the d2 the pair evaluates to, like every other candidate's.
//     6 - 8   corner k of the query triangle ((0,0), (1,0), (0,1) through tri_point: an evaluated point) against T by closest_on_tri
//     9 - 11  corner k of T, likewise evaluated, against (A0, F1, F2) by closest_on_tri
//     12 - 20 edge j of the query triangle against edge k of T, j-major: the closest points of two clamped segments (seg_seg_params);
//             edge k of a triangle (p0, g1, g2) is  p0 -> p0 + g1,  p0 + g1 -> p0 + g2,  p0 + g2 -> p0  and its parameter s is
//             (u, v) = (s, 0), (1 - s, s), (0, 1 - s)
// §6.14's principle: a candidate that is placed inexactly is still a point of both triangles, and no region is chosen by cancelling
// signs.  That is why an accepted segment test does not set d2 = 0 by itself: on a query triangle without area (a segment, a point)
// or a needle its determinant is rounding noise, it accepts pairs that are far apart, and a verdict taken at its word would
// answer 0 for them (§6.22 has the case that was found); the pair it proposes then simply loses against the other candidates.
// The query's answer is the lexicographic minimum of (d2, original triangle index) over all mesh triangles with d2 < limit2,
// limit2 = point_limit2(rmax); dist = sqrt(d2); the winner's barycentrics are recomputed at retire with the same function.
// A walk of the BVH8 may skip a child box or a leaf only when box_lb2(...) > the best d2 it holds, strictly; §6.22 shows
// box_lb2 <= d2 in fp32 for every triangle under the box, with no slack term.
#pragma once
#include "tri_section.h"

namespace rt {

struct TriDist {
    float d2, uq, vq, um, vm;
    int cand;  // which candidate won (0 .. 20): for the tests; the kernel does not read it
};

// x clamped to [0, 1]; a NaN gives 0 (both comparisons are false for it), as in segment_param
RT_HD float clamp01(float x) {
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}

// corner k of a triangle in its barycentrics
RT_HD float corner_u(int k) { return k == 1 ? 1.0f : 0.0f; }
RT_HD float corner_v(int k) { return k == 2 ? 1.0f : 0.0f; }

// edge k of the triangle (p0, g1, g2): where it starts (an evaluated corner: tri_point at that corner is this sum) and its direction
RT_HD void tri_edge(P3 p0, P3 g1, P3 g2, int k, P3& o, P3& d) {
    if (k == 0) {
        o = p0;
        d = g1;
    } else if (k == 1) {
        o = P3{p0.x + g1.x, p0.y + g1.y, p0.z + g1.z};
        d = p3_sub(g2, g1);
    } else {
        o = P3{p0.x + g2.x, p0.y + g2.y, p0.z + g2.z};
        d = P3{-g2.x, -g2.y, -g2.z};
    }
}
RT_HD void edge_uv(int k, float s, float& u, float& v) {
    u = k == 0 ? s : k == 1 ? 1.0f - s : 0.0f;
    v = k == 0 ? 0.0f : k == 1 ? s : 1.0f - s;
}

// Closest points of the segments p1 + s d1 and p2 + t d2, 0 <= s, t <= 1 (Ericson, Real-Time Collision Detection §5.1.9).
//   a = d1.d1, e = d2.d2, b = d1.d2, c = d1.r, f = d2.r, r = p1 - p2
//   s = clamp((b f - c e) / (a e - b b)), or 0 where the denominator is not positive (parallel, or a segment without length)
//   t = clamp((b s + f) / e), 0 where e is not positive; where t is 0 or 1 (it left the segment, or e = 0), s is taken again for
//   that end: s = clamp((t b - c) / a), 0 where a is not positive.
// A NaN quotient gives parameter 0.  Whatever the roundings do, (s, t) are parameters of the two closed segments.
RT_HD void seg_seg_params(P3 p1, P3 d1, P3 p2, P3 d2, float& s, float& t) {
    const P3 r = p3_sub(p1, p2);
    const float a = p3_dot(d1, d1), e = p3_dot(d2, d2), b = p3_dot(d1, d2), c = p3_dot(d1, r), f = p3_dot(d2, r);
    const float den = __builtin_fmaf(a, e, -(b * b));
    s = den > 0.0f ? clamp01(__builtin_fmaf(b, f, -(c * e)) / den) : 0.0f;
    t = e > 0.0f ? clamp01(__builtin_fmaf(b, s, f) / e) : 0.0f;
    if (!(t > 0.0f && t < 1.0f)) {
        const float num = t > 0.0f ? b - c : -c;
        s = a > 0.0f ? clamp01(num / a) : 0.0f;
    }
}

// d2 of a pair of barycentrics
RT_HD float pair_d2(P3 a0, P3 f1, P3 f2, float uq, float vq, P3 v0, P3 e1, P3 e2, float um, float vm) {
    const P3 d = p3_sub(tri_point(a0, f1, f2, uq, vq), tri_point(v0, e1, e2, um, vm));
    return p3_dot(d, d);
}

// tri_overlap.h's seg_crosses (ray_tri_t of ray_parity.h restated operation for operation, then 0 < t < 1) that also says where:
// t along the segment and (u, v) = (u / det, v / det), clamped, in the triangle (w0, g1, g2).  u + v <= 1 up to the roundings of the two
// quotients, as closest_on_tri's foot.
RT_HD bool seg_pierce(P3 o, P3 d, P3 w0, P3 g1, P3 g2, float& t, float& u, float& v) {
    const P3 pvec = p3_cross(d, g2);
    const float det = p3_dot(g1, pvec);
    if (det == 0.0f) return false;
    const P3 tvec = p3_sub(o, w0);
    const float un = p3_dot(tvec, pvec);
    const P3 qvec = p3_cross(tvec, g1);
    const float vn = p3_dot(d, qvec);
    if (det > 0.0f) {
        if (un < 0.0f || vn < 0.0f || un + vn > det) return false;
    } else {
        if (un > 0.0f || vn > 0.0f || un + vn < det) return false;
    }
    t = p3_dot(g2, qvec) / det;
    if (!(0.0f < t && t < 1.0f)) return false;
    u = clamp01(un / det);
    v = clamp01(vn / det);
    return true;
}

// The pair's answer.  (closest_on_tri's d2 of a mesh corner against the query triangle is p3_dot(c - a, c - a): the components
// are the exact negatives of a - c, their products and fmas the same numbers, so it is pair_d2 bit for bit.)
// The three-trip loops are kept rolled on the device: k is uniform, its selects are scalar, and the code stays a third as long.
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_TRI_DIST_ROLLED _Pragma("unroll 1")
#else
#define RT_TRI_DIST_ROLLED
#endif
RT_HD TriDist tri_dist(const QueryTri& A, const Box& Q, P3 v0, P3 e1, P3 e2) {
    const P3 f1 = p3_sub(A.a1, A.a0), f2 = p3_sub(A.a2, A.a0);
    TriDist best{std::numeric_limits<float>::infinity(), 0.0f, 0.0f, 0.0f, 0.0f, -1};
    if (overlap_cand(Q, v0, e1, e2)) {  // overlap_mask's six tests, argument for argument
        float t, u, v;
        RT_TRI_DIST_ROLLED
        for (int k = 0; k < 3; k++) {  // bits 0 - 2: the query's edge A_k -> A_k+1 through T
            const P3 o = k == 0 ? A.a0 : k == 1 ? A.a1 : A.a2, to = k == 0 ? A.a1 : k == 1 ? A.a2 : A.a0;
            if (seg_pierce(o, p3_sub(to, o), v0, e1, e2, t, u, v)) {
                float uq, vq;
                edge_uv(k, t, uq, vq);
                const float dd = pair_d2(A.a0, f1, f2, uq, vq, v0, e1, e2, u, v);
                if (dd < best.d2) best = TriDist{dd, uq, vq, u, v, k};
            }
        }
        const P3 v1{v0.x + e1.x, v0.y + e1.y, v0.z + e1.z};
        RT_TRI_DIST_ROLLED
        for (int k = 0; k < 3; k++) {  // bits 3 - 5: T's edges v0 -> v1, v1 -> v2, v0 -> v2 through the query triangle
            const P3 o = k == 1 ? v1 : v0, d = k == 0 ? e1 : k == 1 ? p3_sub(e2, e1) : e2;
            if (seg_pierce(o, d, A.a0, f1, f2, t, u, v)) {
                const float um = k == 0 ? t : k == 1 ? 1.0f - t : 0.0f, vm = k == 0 ? 0.0f : t;
                const float dd = pair_d2(A.a0, f1, f2, u, v, v0, e1, e2, um, vm);
                if (dd < best.d2) best = TriDist{dd, u, v, um, vm, 3 + k};
            }
        }
    }
    RT_TRI_DIST_ROLLED
    for (int k = 0; k < 3; k++) {
        const float u = corner_u(k), v = corner_v(k);
        const ClosestTri ct = closest_on_tri(tri_point(A.a0, f1, f2, u, v), v0, e1, e2);
        if (ct.d2 < best.d2) best = TriDist{ct.d2, u, v, ct.u, ct.v, 6 + k};
    }
    RT_TRI_DIST_ROLLED
    for (int k = 0; k < 3; k++) {
        const float u = corner_u(k), v = corner_v(k);
        const ClosestTri ct = closest_on_tri(tri_point(v0, e1, e2, u, v), A.a0, f1, f2);
        if (ct.d2 < best.d2) best = TriDist{ct.d2, ct.u, ct.v, u, v, 9 + k};
    }
    RT_TRI_DIST_ROLLED
    for (int j = 0; j < 3; j++) {
        P3 p1, d1;
        tri_edge(A.a0, f1, f2, j, p1, d1);
        RT_TRI_DIST_ROLLED
        for (int k = 0; k < 3; k++) {
            P3 p2, d2;
            tri_edge(v0, e1, e2, k, p2, d2);
            float s, t, uq, vq, um, vm;
            seg_seg_params(p1, d1, p2, d2, s, t);
            edge_uv(j, s, uq, vq);
            edge_uv(k, t, um, vm);
            const float dd = pair_d2(A.a0, f1, f2, uq, vq, v0, e1, e2, um, vm);
            if (dd < best.d2) best = TriDist{dd, uq, vq, um, vm, 12 + 3 * j + k};
        }
    }
    return best;
}
#undef RT_TRI_DIST_ROLLED

// The two reported points of a pair's answer
RT_HD void tri_dist_points(const QueryTri& A, P3 v0, P3 e1, P3 e2, const TriDist& td, P3& on_query, P3& on_mesh) {
    on_query = tri_point(A.a0, p3_sub(A.a1, A.a0), p3_sub(A.a2, A.a0), td.uq, td.vq);
    on_mesh = tri_point(v0, e1, e2, td.um, td.vm);
}

// ---- lower bound of a child box -------------------------------------------------------------------------------------------------
// Qp: Q grown outward by 2e-5 x max(1, largest |coordinate| of the query triangle) - the mesh's own rule for its boxes - so that every
// evaluated point a of the query triangle has Qp.lo <= a <= Qp.hi as fp32 numbers (§6.22: a leaves Q by less than 12 x 2^-24 of that).
RT_HD float query_maxabs(const QueryTri& q) {
    const float mx = max3f(__builtin_fabsf(q.a0.x), __builtin_fabsf(q.a1.x), __builtin_fabsf(q.a2.x));
    const float my = max3f(__builtin_fabsf(q.a0.y), __builtin_fabsf(q.a1.y), __builtin_fabsf(q.a2.y));
    const float mz = max3f(__builtin_fabsf(q.a0.z), __builtin_fabsf(q.a1.z), __builtin_fabsf(q.a2.z));
    return max3f(mx, my, mz);
}
RT_HD Box padded_query_box(const QueryTri& q) {
    Box b = query_box(q);
    const float pad = 2e-5f * std::max(1.0f, query_maxabs(q));
    for (int a = 0; a < 3; a++) b.lo[a] -= pad, b.hi[a] += pad;
    return b;
}
// One axis: the planes as the node stores them, decoded as axis_gap decodes them (one fma each), and how far the two slabs are apart
RT_HD float axis_box_gap(float qlo_p, float qhi_p, float origin, float scale, float qlo, float qhi) {
    const float lo = __builtin_fmaf(qlo, scale, origin), hi = __builtin_fmaf(qhi, scale, origin);
    return __builtin_fmaxf(__builtin_fmaxf(lo - qhi_p, qlo_p - hi), 0.0f);
}
// child slot s of the node words w (bvh_node.h): squared distance from Qp to its box, 0 where they overlap
RT_HD float box_lb2(const uint32_t* w, uint32_t s, const Box& Qp) {
    float g[3];
    for (int a = 0; a < 3; a++) {
        const uint32_t qlo = (w[8 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu, qhi = (w[14 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu;
        g[a] = axis_box_gap(Qp.lo[a], Qp.hi[a], node_origin(w, a), node_scale(w, a), (float)qlo, (float)qhi);
    }
    return gap_lb2(g[0], g[1], g[2]);
}

}  // namespace rt
