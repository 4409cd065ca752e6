// sweep_tri.h — the arithmetic of path B's sphere-cast query, defined once for the kernel (pt_query_sweeps,
// pt_sweep_query.hip) and for the tests' reference (tests/native/sweep_query_ref.cpp).  Compiled by plain g++ and by hipcc; every
// function is host + device under hipcc.  fp32 only, after DESIGN.md §4: every fused multiply-add is an explicit __builtin_fmaf,
// p3_dot's order, correctly rounded / and sqrt, no contraction.  The same operations in the same order on both sides, so the two
// agree bit for bit.
//
// THE ANSWER, without a tree.  Item i is a sphere of radius r whose centre moves along  c(t) = o + t d,  each component ONE fma
// (sweep_centre).  For a triangle T with the record words v0, e1, e2:
//     toi(T) = 0                                 when closest_on_tri(o, T).d2 <= r * r (one fp32 product): the start touches;
//     toi(T) = the smallest ACCEPTED candidate   otherwise; no accepted candidate: T is not touched.
// The candidates are the entry times into the seven features of the sphere-swept triangle, each only where the centre approaches
// the feature: the plane of T offset by r towards the origin's side, the three cylinders of radius r about the edges' lines, the
// three spheres of radius r about the vertices.  A candidate that comes out at or below 0 (the start is within a rounding of
// touching) is raised to kSweepTiny.  A candidate t is ACCEPTED when
//     closest_on_tri(c(t), T).d2 <= (r + kSweepTol S)^2,   S = max(|o|_inf, r, |v0|_inf + max(|e1|_inf, |e2|_inf))
// - §6.14's principle: a feature only PROPOSES a time; what counts is the distance the centre evaluates to at that time, with the
// function whose every candidate is a point of the closed triangle.  This one test is the face's "foot inside the triangle" and
// the cylinders' "parameter in [0, 1]" (which is kept as a filter in front of it), and it cannot be fooled by a needle, whose normal
// and whose short edge are rounding noise: a proposal from noise evaluates to a distance that is not r and is dropped.  A triangle
// without area has no face, an edge without length no cylinder: it is the capsules and spheres it consists of.  A zero direction
// approaches nothing and touches only at t = 0.  r = 0 is a ray against the closed triangle.  A NaN candidate fails every
// comparison and is never accepted.
// The batch answer is the lexicographic minimum of (toi, original triangle index) over the triangles with toi < tmax (strictly)
// and toi <= FLT_MAX; the contact point is closest_on_tri + tri_point of c(toi) against the winner.
// `tcut` lets a walk skip the evaluation of candidates that cannot win: sweep_toi(.., tcut) returns toi(T) whenever toi(T) <= tcut,
// and otherwise either "not touched" or a time above tcut - which loses against the holder of tcut either way.
//
// A walk of the BVH8 may skip a child box or a leaf only when sweep_child_bound(...) > the best t it holds, strictly (a tie must
// reach the index comparison), or when the bound is +inf (the path misses the inflated box); §6.24 shows  bound <= toi(T)  in fp32
// for every triangle under the box.
#pragma once
#include "point_tri.h"

namespace rt {

constexpr float kSweepTol = 0x1p-21f;     // 8 x 2^-24: the acceptance slack in units of S
constexpr float kSweepInflate = 0x1p-19f;  // 32 x 2^-24: what the inflated box has over r, in units of sweep_scale (§6.24)
constexpr float kSweepTiny = 0x1p-126f;    // the smallest positive time: a candidate at or below 0
constexpr float kSweepTmaxCap = 3.402823466e+38f;  // FLT_MAX: a time of impact is finite
constexpr uint32_t kSweepFace = 1u, kSweepEdges = 2u, kSweepVertices = 4u, kSweepFaceUnchecked = 8u;  // `features`: what a mutated reference withholds
constexpr uint32_t kSweepAll = kSweepFace | kSweepEdges | kSweepVertices;

struct Sweep {
    P3 o, d;
    float r;
};

RT_HD float p3_maxabs(P3 a) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z)); }
RT_HD P3 sweep_centre(P3 o, P3 d, float t) { return P3{__builtin_fmaf(t, d.x, o.x), __builtin_fmaf(t, d.y, o.y), __builtin_fmaf(t, d.z, o.z)}; }
RT_HD P3 p3_fma(float k, P3 a, P3 b) { return P3{__builtin_fmaf(k, a.x, b.x), __builtin_fmaf(k, a.y, b.y), __builtin_fmaf(k, a.z, b.z)}; }

// (r + kSweepTol S)^2: what an accepted candidate's evaluated d2 may be
RT_HD float sweep_accept2(const Sweep& s, P3 v0, P3 e1, P3 e2) {
    const float S = __builtin_fmaxf(__builtin_fmaxf(p3_maxabs(s.o), s.r), p3_maxabs(v0) + __builtin_fmaxf(p3_maxabs(e1), p3_maxabs(e2)));
    const float ra = __builtin_fmaf(kSweepTol, S, s.r);
    return ra * ra;
}

struct SweepToi {
    float t;
    bool hit;
};

// One candidate: raised to kSweepTiny, evaluated only where it can still win, accepted by the distance it evaluates to
RT_HD void sweep_offer(const Sweep& s, P3 v0, P3 e1, P3 e2, float lim2, float t, SweepToi& best, bool unchecked = false) {
    if (!(t == t)) return;
    t = t > kSweepTiny ? t : kSweepTiny;
    if (!(best.hit ? t < best.t : t <= best.t)) return;
    if (unchecked || closest_on_tri(sweep_centre(s.o, s.d, t), v0, e1, e2).d2 <= lim2) best = SweepToi{t, true};
}

// Entry time of the point m + t d into the ball of radius r about 0, d restricted to where it approaches (m . d < 0): the time of
// closest approach t0 = -(m . d) / (d . d), the residual p0 = m + t0 d formed with one fma per component, so that its length g is
// good to a few units of |m|'s rounding however far away the start is, then t0 - sqrt((r^2 - g^2) / (d . d)).  NaN: no entry.
RT_HD float ball_entry(P3 m, P3 d, float rr) {
    const float nan = __builtin_nanf("");
    const float b = p3_dot(m, d), dd = p3_dot(d, d);
    if (!(b < 0.0f) || !(dd > 0.0f)) return nan;
    const float t0 = -b / dd;
    const P3 p0 = p3_fma(t0, d, m);
    const float h2 = (rr - p3_dot(p0, p0)) / dd;
    if (!(h2 >= 0.0f)) return nan;
    return t0 - __builtin_sqrtf(h2);
}

// Entry time into the cylinder of radius r about the line (m = start relative to a point of it, axis e), where the contact
// parameter lies in [0, 1]: ball_entry on the components across the axis.
RT_HD float cylinder_entry(P3 m, P3 d, P3 e, float rr) {
    const float nan = __builtin_nanf("");
    const float ee = p3_dot(e, e);
    if (!(ee > 0.0f)) return nan;
    const float km = p3_dot(m, e) / ee, kd = p3_dot(d, e) / ee;
    const float t = ball_entry(p3_fma(-km, e, m), p3_fma(-kd, e, d), rr);
    const float at = __builtin_fmaf(t > 0.0f ? t : 0.0f, kd, km);
    return (at >= 0.0f && at <= 1.0f) ? t : nan;
}

// toi(T), see above.  features: kSweepAll everywhere but in the mutated references of the tests.
RT_HD SweepToi sweep_toi(const Sweep& s, P3 v0, P3 e1, P3 e2, float tcut, uint32_t features = kSweepAll) {
    const float rr = s.r * s.r;
    if (closest_on_tri(s.o, v0, e1, e2).d2 <= rr) return SweepToi{0.0f, true};
    const float lim2 = sweep_accept2(s, v0, e1, e2);
    const P3 ap = p3_sub(s.o, v0);
    SweepToi best{tcut, false};
    if (features & kSweepFace) {
        const P3 n = p3_cross(e1, e2);
        const float nn = p3_dot(n, n);
        if (nn > 0.0f) {
            const float h = p3_dot(ap, n), dn = p3_dot(s.d, n);
            if ((h > 0.0f && dn < 0.0f) || (h < 0.0f && dn > 0.0f))
                sweep_offer(s, v0, e1, e2, lim2, __builtin_fmaf(-s.r, __builtin_sqrtf(nn), __builtin_fabsf(h)) / __builtin_fabsf(dn), best,
                            (features & kSweepFaceUnchecked) != 0u);
        }
    }
    const P3 b1 = p3_sub(ap, e1), b2 = p3_sub(ap, e2);  // the start relative to the other two vertices
    if (features & kSweepEdges) {
        sweep_offer(s, v0, e1, e2, lim2, cylinder_entry(ap, s.d, e1, rr), best);
        sweep_offer(s, v0, e1, e2, lim2, cylinder_entry(ap, s.d, e2, rr), best);
        sweep_offer(s, v0, e1, e2, lim2, cylinder_entry(b1, s.d, p3_sub(e2, e1), rr), best);
    }
    if (features & kSweepVertices) {
        sweep_offer(s, v0, e1, e2, lim2, ball_entry(ap, s.d, rr), best);
        sweep_offer(s, v0, e1, e2, lim2, ball_entry(b1, s.d, rr), best);
        sweep_offer(s, v0, e1, e2, lim2, ball_entry(b2, s.d, rr), best);
    }
    return best;
}

// ---- validity and limits -----------------------------------------------------------------------------------------------------------
// An item the query answers: o within reach on every axis, d finite, 0 <= r <= reach, tmax not a NaN (every comparison is false
// for a NaN, so non-finite components fail)
RT_HD bool sweep_valid(const Sweep& s, float tmax, float reach) {
    const float inf = __builtin_inff();
    return point_in_reach(s.o, reach) && __builtin_fabsf(s.d.x) < inf && __builtin_fabsf(s.d.y) < inf && __builtin_fabsf(s.d.z) < inf && s.r >= 0.0f && s.r <= reach &&
           tmax == tmax;
}
// where the best time starts: tmax, and finite (a box the path misses has the bound +inf, which must lie above it)
RT_HD float sweep_start_bound(float tmax) { return tmax < kSweepTmaxCap ? tmax : kSweepTmaxCap; }

// ---- lower bound of a child box --------------------------------------------------------------------------------------------------
// What the walk holds of an item beside o: 1 / d per axis (0 where d is 0: the path does not move on that axis) and the inflation
// R = r + kSweepInflate max(|o|_inf, r, reach / 8).  reach / 8 = 4 max(1, M) bounds the S of every triangle of the mesh.
struct SweepSlabs {
    P3 inv;
    float R;
};
RT_HD SweepSlabs sweep_slabs(const Sweep& s, float reach) {
    const float S = __builtin_fmaxf(__builtin_fmaxf(p3_maxabs(s.o), s.r), 0.125f * reach);
    return SweepSlabs{P3{s.d.x != 0.0f ? 1.0f / s.d.x : 0.0f, s.d.y != 0.0f ? 1.0f / s.d.y : 0.0f, s.d.z != 0.0f ? 1.0f / s.d.z : 0.0f},
                      __builtin_fmaf(kSweepInflate, S, s.r)};
}
// One axis: the planes as the node stores them, decoded with one fma each and moved outward by R; [tn, tf] shrinks to where the
// path lies between them.  An axis on which the path does not move keeps the interval or empties it.
RT_HD void axis_slab(float o, float inv, float R, float origin, float scale, float qlo, float qhi, float& tn, float& tf) {
    const float lo = __builtin_fmaf(qlo, scale, origin) - R, hi = __builtin_fmaf(qhi, scale, origin) + R;
    const float a = (lo - o) * inv, b = (hi - o) * inv;
    const bool still = inv == 0.0f;
    const float n = still ? ((o < lo || o > hi) ? __builtin_inff() : -__builtin_inff()) : __builtin_fminf(a, b);
    const float f = still ? __builtin_inff() : __builtin_fmaxf(a, b);
    tn = __builtin_fmaxf(tn, n);
    tf = __builtin_fminf(tf, f);
}
// The entry time, clamped at 0 and taken down by 8 x 2^-24 of itself, or +inf where the path misses the box (the exit time taken
// up by as much lies below it)
RT_HD float slab_bound(float tn, float tf) {
    const float entry = __builtin_fmaxf(tn, 0.0f) * (1.0f - 0x1p-21f), exit = tf * (1.0f + 0x1p-21f);
    return entry <= exit ? entry : __builtin_inff();
}

// child slot s of the node words w (bvh_node.h): the time at which the path enters its box inflated by R
RT_HD float sweep_child_bound(const uint32_t* w, uint32_t s, const Sweep& sw, const SweepSlabs& sl) {
    const float oc[3] = {sw.o.x, sw.o.y, sw.o.z}, ic[3] = {sl.inv.x, sl.inv.y, sl.inv.z};
    float tn = -__builtin_inff(), tf = __builtin_inff();
    for (int a = 0; a < 3; a++) {
        const uint32_t qlo = (w[8 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu, qhi = (w[14 + 2 * a + (s >> 2)] >> (8 * (s & 3u))) & 0xffu;
        axis_slab(oc[a], ic[a], sl.R, node_origin(w, a), node_scale(w, a), (float)qlo, (float)qhi, tn, tf);
    }
    return slab_bound(tn, tf);
}

}  // namespace rt
