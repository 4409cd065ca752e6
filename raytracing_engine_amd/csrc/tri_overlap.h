// tri_overlap.h — the arithmetic of path B's overlap query, defined once for the kernel (pt_query_overlaps,
// pt_overlap_query.hip) and for the tests' reference (tests/native/overlap_query_ref.cpp).  Compiled by plain g++ and by hipcc; every
// function is host + device under hipcc.  fp32 only, after DESIGN.md §4: the segment / triangle test is ray_parity.h's ray_tri_t
// (explicit fmas, §4's dot and cross, a correctly rounded division, no contraction), everything else here is one fp32 subtraction or
// addition per component and plain comparisons.  The same operations in the same order on both sides: the two agree bit for bit.
//
// THE ANSWER, without a tree.  Query triangle i has the vertices A0, A1, A2 as the caller gave them; F1 = A1 - A0, F2 = A2 - A0;
// Q = the per-axis minimum and maximum of the three vertices.  Mesh triangle T has the record words v0, e1, e2;
// B = tri_box(v0, e1, e2, 0) of bvh_node.h: the box of v0, fl(v0 + e1), fl(v0 + e2), no padding.
//   cand(i, T)  = Q.lo[a] <= B.hi[a] && B.lo[a] <= Q.hi[a] on all three axes (closed, plain fp32 comparisons)
//   seg(o, d, w0, g1, g2) = ray_tri_t(o, d, w0, g1, g2, t) && 0 < t && t < 1    (strict at both ends)
//   mask(i, T)  bit 0: seg(A0, A1 - A0, v0, e1, e2)        bit 3: seg(v0, e1, A0, F1, F2)
//               bit 1: seg(A1, A2 - A1, v0, e1, e2)        bit 4: seg(fl(v0 + e1), e2 - e1, A0, F1, F2)
//               bit 2: seg(A2, A0 - A2, v0, e1, e2)        bit 5: seg(v0, e2, A0, F1, F2)
//   overlaps(i) = { T : cand(i, T) and mask(i, T) != 0 }, ascending by original triangle index, each with its mask.
// cand is part of the definition, so that a walk needs no slack: it skips a child whose decoded box is disjoint from Q on some axis
// (box_overlaps below on the planes fma(q, scale, origin)), that box contains B of every triangle below it (§6.14: lo <= c <= hi for
// every evaluated point of such a triangle, its vertices included), so a skipped subtree holds only triangles with cand false.
#pragma once
#include "ray_parity.h"

namespace rt {

// the query triangle as a lane keeps it: the nine coordinates (and, beside them, its box)
struct QueryTri {
    P3 a0, a1, a2;
};

RT_HD float min3f(float a, float b, float c) { return std::min(a, std::min(b, c)); }
RT_HD float max3f(float a, float b, float c) { return std::max(a, std::max(b, c)); }

// Q: the per-axis minimum and maximum of the three vertices
RT_HD Box query_box(const QueryTri& q) {
    Box b;
    b.lo[0] = min3f(q.a0.x, q.a1.x, q.a2.x), b.hi[0] = max3f(q.a0.x, q.a1.x, q.a2.x);
    b.lo[1] = min3f(q.a0.y, q.a1.y, q.a2.y), b.hi[1] = max3f(q.a0.y, q.a1.y, q.a2.y);
    b.lo[2] = min3f(q.a0.z, q.a1.z, q.a2.z), b.hi[2] = max3f(q.a0.z, q.a1.z, q.a2.z);
    return b;
}

// closed overlap of two boxes given plane by plane (false where a NaN is compared)
RT_HD bool box_overlaps(const Box& q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    return q.lo[0] <= hix && lox <= q.hi[0] && q.lo[1] <= hiy && loy <= q.hi[1] && q.lo[2] <= hiz && loz <= q.hi[2];
}

// cand(i, T) on the record's own words
RT_HD bool overlap_cand(const Box& q, P3 v0, P3 e1, P3 e2) {
    const float p0[3] = {v0.x, v0.y, v0.z}, f1[3] = {e1.x, e1.y, e1.z}, f2[3] = {e2.x, e2.y, e2.z};
    const Box b = tri_box(p0, f1, f2, 0.0f);
    return box_overlaps(q, b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
}

// the segment o .. o + d against the triangle (w0, g1, g2), both ends excluded
RT_HD bool seg_crosses(P3 o, P3 d, P3 w0, P3 g1, P3 g2) {
    float t;
    return ray_tri_t(o, d, w0, g1, g2, t) && 0.0f < t && t < 1.0f;
}

// mask(i, T): all six tests, no early-out - the mask is part of the answer
RT_HD uint32_t overlap_mask(const QueryTri& q, P3 v0, P3 e1, P3 e2) {
    uint32_t m = 0u;
    m |= seg_crosses(q.a0, p3_sub(q.a1, q.a0), v0, e1, e2) ? 1u : 0u;
    m |= seg_crosses(q.a1, p3_sub(q.a2, q.a1), v0, e1, e2) ? 2u : 0u;
    m |= seg_crosses(q.a2, p3_sub(q.a0, q.a2), v0, e1, e2) ? 4u : 0u;
    const P3 f1 = p3_sub(q.a1, q.a0), f2 = p3_sub(q.a2, q.a0);
    const P3 v1{v0.x + e1.x, v0.y + e1.y, v0.z + e1.z};
    m |= seg_crosses(v0, e1, q.a0, f1, f2) ? 8u : 0u;
    m |= seg_crosses(v1, p3_sub(e2, e1), q.a0, f1, f2) ? 16u : 0u;
    m |= seg_crosses(v0, e2, q.a0, f1, f2) ? 32u : 0u;
    return m;
}

// child slot s of the node words w (bvh_node.h): does its decoded box overlap q?  The decode is child_lb2's (point_tri.h): the
// plane's byte as a float, one fma.  Empty slots hold an inverted box that a wide q can still "overlap": callers mask by imask / leafmask.
RT_HD bool child_overlaps(const uint32_t* w, uint32_t s, const Box& q) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        const uint32_t qlo = (w[8 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu, qhi = (w[14 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu;
        lo[a] = __builtin_fmaf((float)qlo, node_scale(w, a), node_origin(w, a));
        hi[a] = __builtin_fmaf((float)qhi, node_scale(w, a), node_origin(w, a));
    }
    return box_overlaps(q, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
}

// a query triangle the query answers: every coordinate finite and within reach = 32 x max(1, largest |vertex coordinate|) (false for a NaN)
RT_HD bool tri_in_reach(const QueryTri& q, float reach) { return point_in_reach(q.a0, reach) && point_in_reach(q.a1, reach) && point_in_reach(q.a2, reach); }

}  // namespace rt
