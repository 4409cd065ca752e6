// ray_parity.h — the arithmetic of path B's inside/outside query, defined once for the kernel (pt_query_sides,
// pt_side_query.hip) and for the tests' reference (tests/native/side_query_ref.cpp).  Compiled by plain g++ and by hipcc; every
// function is host + device under hipcc.  fp32 only, after DESIGN.md §4: every fused multiply-add is an explicit __builtin_fmaf,
// dot() and cross() in §4's order (p3_dot, p3_cross of point_tri.h), a correctly rounded division, no contraction.
//
// THE ANSWER, without a tree.  crossings(p, k) = the number of triangles that §6.3's ray / triangle test (ray_tri_t below, tri_test
// of pt_traverse.h restated operation for operation) accepts with t > 0 for the ray from p along kParityDir[k], with no upper limit on
// t.  Every triangle lies under exactly one leaf and the box test is conservative for origins within reach (§6.3), so a walk of
// the BVH8 that never shrinks its tmax tests every triangle the ray can cross exactly once and returns this count whatever the
// tree.  inside(p) = the majority of the three parities crossings(p, k) & 1, evaluated lazily (side_of_parities): when the first
// two agree the third cannot change the majority and is not walked.
// The answer is DEFINED ON ANY MESH as this parity of crossings.  It MEANS "inside" on closed meshes (every edge shared by two
// triangles, no self-intersection): there an exact ray crosses the surface an odd number of times exactly when it starts inside.
// On an open mesh (a height field, a soup) it is still deterministic and tree-independent, and still what the three rays cross.
//
// WHY THREE RAYS.  The test is not watertight (§6.3): a ray through a shared edge or a vertex may be accepted by both neighbours, or
// by neither, or by any number of the triangles round a vertex, so one parity is wrong where a ray passes within a few units of
// an edge.  Three fixed directions, no component smaller than 0.3 (no ray lies in an axis-aligned or 45-degree plane of a
// regular grid) and pairwise |cos| <= 0.6 (an edge or vertex that one ray grazes is well off the other two), make two wrong
// parities at one point a coincidence of two independent near-edge passes; tests/sign_exact.py aims each ray through vertices and
// edges and measures it.
#pragma once
#include "point_tri.h"

namespace rt {

constexpr int kParityDirs = 3;
// the directions (unit length up to the four digits given), their reciprocals (constants: no division per walk) and 7 - octant
// (bit 2: x >= 0, bit 1: y >= 0, bit 0: z >= 0, octant_inv of pt_traverse.h)
struct ParityDir {
    P3 d, inv;
    uint32_t oct_inv;
};
RT_HD ParityDir parity_dir(uint32_t k) {
    constexpr float x0 = 0.6350f, y0 = 0.5127f, z0 = 0.5779f;
    constexpr float x1 = -0.4382f, y1 = 0.7561f, z1 = -0.4861f;
    constexpr float x2 = 0.3097f, y2 = -0.4203f, z2 = -0.8529f;
    // (selects, not a table: three constants per component in registers, no constant-memory fetch in the kernel)
    ParityDir r;
    r.d = P3{k == 0u ? x0 : k == 1u ? x1 : x2, k == 0u ? y0 : k == 1u ? y1 : y2, k == 0u ? z0 : k == 1u ? z1 : z2};
    r.inv = P3{k == 0u ? 1.0f / x0 : k == 1u ? 1.0f / x1 : 1.0f / x2, k == 0u ? 1.0f / y0 : k == 1u ? 1.0f / y1 : 1.0f / y2,
               k == 0u ? 1.0f / z0 : k == 1u ? 1.0f / z1 : 1.0f / z2};
    r.oct_inv = k == 0u ? 7u : k == 1u ? 2u : 4u;
    return r;
}

// DESIGN.md §6.3, Moeller-Trumbore with the division deferred: tri_test of pt_traverse.h, the same operations in the same order on
// the record's v0, e1, e2.  true: the ray's line passes through the triangle, t_out = the distance along d (any sign).
RT_HD bool ray_tri_t(P3 o, P3 d, P3 v0, P3 e1, P3 e2, float& t_out) {
    const P3 pvec = p3_cross(d, e2);
    const float det = p3_dot(e1, pvec);
    if (det == 0.0f) return false;
    const P3 tvec = p3_sub(o, v0);
    const float u = p3_dot(tvec, pvec);
    const P3 qvec = p3_cross(tvec, e1);
    const float v = p3_dot(d, qvec);
    if (det > 0.0f) {
        if (u < 0.0f || v < 0.0f || u + v > det) return false;
    } else {
        if (u > 0.0f || v > 0.0f || u + v < det) return false;
    }
    t_out = p3_dot(e2, qvec) / det;
    return true;
}
// one crossing: accepted, in front of the origin
RT_HD bool ray_crosses(P3 o, P3 d, P3 v0, P3 e1, P3 e2) {
    float t;
    return ray_tri_t(o, d, v0, e1, e2, t) && t > 0.0f;
}

// The majority of three parities from the first two where they agree: par0 == par1 ? par0 : par2 equals the 2-of-3 majority on
// all eight triples (tests/test_side_query_host.py), and the third walk is needed only where the first two disagree.
RT_HD bool needs_third_parity(uint32_t par0, uint32_t par1) { return ((par0 ^ par1) & 1u) != 0u; }
RT_HD uint32_t side_of_parities(uint32_t par0, uint32_t par1, uint32_t par2) { return needs_third_parity(par0, par1) ? (par2 & 1u) : (par0 & 1u); }

}  // namespace rt
