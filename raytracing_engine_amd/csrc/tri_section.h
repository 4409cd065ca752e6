// tri_section.h — the arithmetic of path B's overlap segments, defined once for the kernel (pt_overlap_segments,
// pt_overlap_segments.hip) and for the tests' reference (tests/native/overlap_segment_ref.cpp).  Compiled by plain g++ and by hipcc;
// every function is host + device under hipcc.  fp32 only, after DESIGN.md §4: the six tests are tri_overlap.h's, argument for
// argument, a pierce point is three explicit fmas, a squared length is p3_dot of one fp32 subtraction per component; no contraction.
// The same operations in the same order on both sides: the two agree bit for bit.
//
// THE ANSWER, without a tree.  An entry (i, T) of an overlap list: query triangle i with the vertices A0, A1, A2 as the caller gave
// them, mesh triangle T with the record words v0, e1, e2.
//   m      = cand(i, T) ? mask(i, T) : 0     (tri_overlap.h; recomputed, the stored mask is not an input)
//   for each set bit b of m, with (o, d, w0, g1, g2) the five arguments overlap_mask hands to seg_crosses for that bit:
//   t_b    = ray_tri_t's t_out,   P_b = (fma(t_b, d.x, o.x), fma(t_b, d.y, o.y), fma(t_b, d.z, o.z))
//   one bit set:   both endpoints are P_b (a touch), ends = b | (b << 3)
//   two or more:   the pair b < c of set bits with the largest d2 = p3_dot(P_c - P_b, P_c - P_b); ties go to the first pair in
//                  lexicographic (b, c) order; the segment is (P_b, P_c) in that order, ends = b | (c << 3)
//   m == 0:        (only on a list the library did not write) six NaNs, ends = -1
// In exact arithmetic two non-coplanar triangles that intersect do so in one segment whose two ends are pierce points, and every
// pierce point lies on it: the farthest pair is the segment, and a third bit - a crossing through a vertex, where two edges pierce at
// almost the same place - cannot shorten it.
#pragma once
#include "tri_overlap.h"

namespace rt {

struct Section {
    P3 p0, p1;      // the endpoints, in the order of their bits
    int32_t ends;   // b | (c << 3); -1: no bit set
    uint32_t mask;  // m
};

constexpr int kSectionPairs = 15;  // pairs b < c of six bits, lexicographic: (0,1) (0,2) .. (0,5) (1,2) .. (4,5)

// seg_crosses with its t (0 where the test refuses): the same call, the same comparisons
RT_HD bool seg_crosses_t(P3 o, P3 d, P3 w0, P3 g1, P3 g2, float& t) {
    t = 0.0f;
    return ray_tri_t(o, d, w0, g1, g2, t) && 0.0f < t && t < 1.0f;
}

RT_HD P3 seg_point(P3 o, P3 d, float t) { return P3{__builtin_fmaf(t, d.x, o.x), __builtin_fmaf(t, d.y, o.y), __builtin_fmaf(t, d.z, o.z)}; }

// The six tests of overlap_mask, argument for argument, each with its pierce point: returns the mask, p[b] is P_b where bit b is set
// (and seg_point at t = 0 or at the refused t elsewhere: never read).  No early-out.
RT_HD uint32_t section_points(const QueryTri& q, P3 v0, P3 e1, P3 e2, P3 p[6]) {
    uint32_t m = 0u;
    float t;
    const P3 d0 = p3_sub(q.a1, q.a0), d1 = p3_sub(q.a2, q.a1), d2 = p3_sub(q.a0, q.a2);
    m |= seg_crosses_t(q.a0, d0, v0, e1, e2, t) ? 1u : 0u;
    p[0] = seg_point(q.a0, d0, t);
    m |= seg_crosses_t(q.a1, d1, v0, e1, e2, t) ? 2u : 0u;
    p[1] = seg_point(q.a1, d1, t);
    m |= seg_crosses_t(q.a2, d2, v0, e1, e2, t) ? 4u : 0u;
    p[2] = seg_point(q.a2, d2, t);
    const P3 f1 = p3_sub(q.a1, q.a0), f2 = p3_sub(q.a2, q.a0);
    const P3 v1{v0.x + e1.x, v0.y + e1.y, v0.z + e1.z};
    const P3 d4 = p3_sub(e2, e1);
    m |= seg_crosses_t(v0, e1, q.a0, f1, f2, t) ? 8u : 0u;
    p[3] = seg_point(v0, e1, t);
    m |= seg_crosses_t(v1, d4, q.a0, f1, f2, t) ? 16u : 0u;
    p[4] = seg_point(v1, d4, t);
    m |= seg_crosses_t(v0, e2, q.a0, f1, f2, t) ? 32u : 0u;
    p[5] = seg_point(v0, e2, t);
    return m;
}

RT_HD float section_d2(P3 pb, P3 pc) {
    const P3 w = p3_sub(pc, pb);
    return p3_dot(w, w);
}

RT_HD Section section_none() {
    const float nan = __builtin_nanf("");
    return Section{P3{nan, nan, nan}, P3{nan, nan, nan}, -1, 0u};
}

// The selection rule on the mask m and its points.  d2_out (kSectionPairs floats, or nullptr: the kernel): d2 of every pair of set
// bits in lexicographic order, NaN for the others - what the tests hold the choice to.
RT_HD Section section_select(uint32_t m, const P3 p[6], float* d2_out) {
    Section s = section_none();
    s.mask = m;
    float best = 0.0f;
    bool have = false;
    int pair = 0;
    for (int b = 0; b < 6; b++) {
        if (!have && ((m >> b) & 1u)) s.p0 = p[b], s.p1 = p[b], s.ends = b | (b << 3);  // the lowest set bit: the touch, until a pair is met
        for (int c = b + 1; c < 6; c++, pair++) {
            const bool both = ((m >> b) & 1u) && ((m >> c) & 1u);
            const float d2 = section_d2(p[b], p[c]);
            if (d2_out) d2_out[pair] = both ? d2 : __builtin_nanf("");
            if (both && (!have || d2 > best)) {  // strictly larger: a tie keeps the earlier pair
                best = d2;
                have = true;
                s.p0 = p[b], s.p1 = p[c], s.ends = b | (c << 3);
            }
        }
    }
    return s;
}

// The answer of an entry whose query triangle has the box Q
RT_HD Section overlap_section(const QueryTri& q, const Box& Q, P3 v0, P3 e1, P3 e2, float* d2_out = nullptr) {
    P3 p[6];
    const uint32_t m = section_points(q, v0, e1, e2, p);  // (computed before cand: no branch round the six tests)
    if (!overlap_cand(Q, v0, e1, e2)) {
        if (d2_out)
            for (int k = 0; k < kSectionPairs; k++) d2_out[k] = __builtin_nanf("");
        return section_none();
    }
    return section_select(m, p, d2_out);
}

}  // namespace rt
