// bvh_node.h — the compressed 8-wide BVH node and the leaf-order triangle record of path B, defined once for everything that
// produces or rewrites them: the host builder (bvh_build.cpp), the two-level flatten (bvh_two_level.cpp), the mesh upload
// (rt_abi_mesh.hip) and the GPU build and refit (bvh_build_gpu.hip).  Compiled by plain g++ and by hipcc: standard library
// only, and every function is host + device under hipcc.  The traversal kernels decode nodes in hand-scheduled code of their own (pt_traverse.h: node_step for the
// ray walks, NodeRec / fetch_node for the other query walks; pt_packet.hip; point_node_step of pt_point_query.hip); the tests' decoders (tests/native/bvh_check.cpp, bvh8_walk.cpp) are independent on purpose.
//
// Node = 80 bytes = 5 x 16-byte fetches for 8 children (20 little-endian words):
//   w0..w2  p.xyz (f32)        origin of the node's quantisation frame (= box minimum)
//   w3      ex | ey<<8 | ez<<16 | imask<<24    per-axis scale = 2^(e-127) as a float exponent byte;
//                                               imask bit s = child slot s is an inner node
//   w4      child_base         index of the first inner child; inner child in slot s lives at
//                              child_base + popcount(imask & ((1<<s)-1))
//   w5      tri_base           leaf-order index of the node's first leaf triangle
//   w6      leafmask           bit s (0..7) = child slot s is a leaf.  A leaf is exactly ONE triangle, the one at
//                              tri_base + popcount(leafmask & ((1<<s)-1)); a slot in neither imask nor leafmask is empty
//   w7      0                  reserved
//   w8..w19 qlo.x[8] qlo.y[8] qlo.z[8] qhi.x[8] qhi.y[8] qhi.z[8]   child boxes, 8 bits per plane,
//                              box = p + q * scale, rounded outward (conservative); empty slots hold an inverted box
//                              (lo 255, hi 0) that no ray hits
// One-triangle leaves: with a quantised box per triangle the traversal's hit bits ARE the work lists (inner children
// to enter = hits & imask, triangles to test = hits & leafmask), no per-child count / offset decoding in the node step;
// on the 1 M-triangle soup the optimal-cut collapse chose single-triangle leaves for 98 % of the leaves anyway.
// Child slots are assigned so that slot ^ (7 - ray octant) enumerates children roughly front to back.
//
// Triangle record = 48 bytes (12 words), one per leaf position: v0.xyz, e1.xyz, e2.xyz (edges formed once, in fp32),
// w9 = original triangle index, w10 = 1 if the triangle is emissive (a light), w11 = 0.
//
// min / max: std::min / std::max everywhere (the second operand only if it is strictly smaller / larger).  fmin / fmax differ
// from them for NaN alone, which validated input (finite vertices) cannot bring here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#ifdef __HIPCC__
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

namespace rt {

constexpr uint32_t kNodeWords = 20;  // 80 bytes
constexpr uint32_t kTriWords = 12;   // 48 bytes
constexpr uint32_t kTriIdWord = 9, kTriLightWord = 10;

// ---- reading a node's words ---------------------------------------------------------------------------------------------
template <class W>
RT_HD W* node_at(W* nodes, size_t k) {
    return nodes + k * kNodeWords;
}
RT_HD uint32_t node_imask(const uint32_t* w) { return w[3] >> 24; }
RT_HD uint32_t node_leafmask(const uint32_t* w) { return w[6] & 0xffu; }
RT_HD uint32_t node_child_base(const uint32_t* w) { return w[4]; }
RT_HD uint32_t node_tri_base(const uint32_t* w) { return w[5]; }
RT_HD uint32_t node_inner_count(const uint32_t* w) { return (uint32_t)__builtin_popcount(node_imask(w)); }
RT_HD uint32_t rank_below(uint32_t mask, uint32_t s) { return (uint32_t)__builtin_popcount(mask & ((1u << s) - 1u)); }
RT_HD uint32_t node_inner_child(const uint32_t* w, uint32_t s) { return node_child_base(w) + rank_below(node_imask(w), s); }  // slot s is in imask
RT_HD uint32_t node_leaf_tri(const uint32_t* w, uint32_t s) { return node_tri_base(w) + rank_below(node_leafmask(w), s); }   // slot s is in leafmask
RT_HD float node_origin(const uint32_t* w, int axis) {
    float p;
    __builtin_memcpy(&p, &w[axis], 4);
    return p;
}
RT_HD float node_scale(const uint32_t* w, int axis) {  // 2^(e - 127): the exponent byte is a float's exponent field
    const uint32_t bits = ((w[3] >> (8 * axis)) & 0xffu) << 23;
    float s;
    __builtin_memcpy(&s, &bits, 4);
    return s;
}

// ---- writing the words that quantise() leaves alone ------------------------------------------------------------------------
RT_HD void node_set_topology(uint32_t* w, uint32_t imask, uint32_t child_base, uint32_t tri_base, uint32_t leafmask) {
    w[3] = (w[3] & 0x00ffffffu) | (imask << 24);
    w[4] = child_base;
    w[5] = tri_base;
    w[6] = leafmask;
    w[7] = 0;
}
// the flatten of two levels into one array: a copied node's children and triangles live elsewhere ...
RT_HD void node_relocate(uint32_t* w, uint32_t child_base, uint32_t tri_base) {
    w[4] = child_base;
    w[5] = tri_base;
}
// ... and a top-level node's leaves (chunks) become inner children (the chunks' roots), consecutive with its inner children in slot order
RT_HD void node_leaves_to_inner(uint32_t* w, uint32_t child_base) { node_set_topology(w, node_imask(w) | node_leafmask(w), child_base, 0u, 0u); }

// ---- boxes ------------------------------------------------------------------------------------------------------------------
struct Box {
    float lo[3], hi[3];
    RT_HD static Box empty() {
        Box b;
        for (int a = 0; a < 3; a++) {
            b.lo[a] = std::numeric_limits<float>::infinity();
            b.hi[a] = -std::numeric_limits<float>::infinity();
        }
        return b;
    }
    RT_HD void grow(const Box& b) {
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], b.lo[a]);
            hi[a] = std::max(hi[a], b.hi[a]);
        }
    }
    RT_HD float half_area() const {
        const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
};

// ---- triangles ------------------------------------------------------------------------------------------------------------------
// box of the vertices p0, p0 + e1, p0 + e2, each formed in fp32, grown by pad on every side
RT_HD Box tri_box(const float p0[3], const float e1[3], const float e2[3], float pad) {
    Box b;
    for (int a = 0; a < 3; a++) {
        const float p1 = p0[a] + e1[a], p2 = p0[a] + e2[a];
        b.lo[a] = std::min(p0[a], std::min(p1, p2)) - pad;
        b.hi[a] = std::max(p0[a], std::max(p1, p2)) + pad;
    }
    return b;
}

RT_HD bool is_emissive(const float emission[3]) { return emission[0] > 0.0f || emission[1] > 0.0f || emission[2] > 0.0f; }

// word 10: pt_shade reads the record anyway (normal) and skips the 16-byte emission gather for the triangles that are not
// lights - all but a handful
RT_HD void pack_tri_record(const float v0[3], const float e1[3], const float e2[3], uint32_t id, bool emissive, float out[kTriWords]) {
    for (int a = 0; a < 3; a++) {
        out[a] = v0[a];
        out[3 + a] = e1[a];
        out[6 + a] = e2[a];
    }
    const uint32_t light = emissive ? 1u : 0u;
    __builtin_memcpy(&out[kTriIdWord], &id, 4);
    __builtin_memcpy(&out[kTriLightWord], &light, 4);
    out[11] = 0.0f;
}

// ---- quantisation ---------------------------------------------------------------------------------------------------------------
// Frame origin nb.lo, a power-of-two scale per axis with 255 * scale >= extent, the planes of child slot s (cb[s], read only if
// bit s of occ is set) floor / ceil outward in double, clamped to [0, 255]; a slot not in occ gets the inverted box (lo 255, hi 0).
// Writes w[0..2] (origin), w[3] (exponent bytes; bits 24-31, imask, are left 0) and w[8..19] (planes); w[4..7] are not touched
RT_HD void quantise(const Box& nb, const Box* cb, uint32_t occ, uint32_t* w) {
    uint32_t e_byte[3];
    double scale[3];
    for (int a = 0; a < 3; a++) {
        const double ext = (double)nb.hi[a] - (double)nb.lo[a];
        int e = ext > 0.0 ? (int)std::ceil(std::log2(ext / 255.0)) : -126;
        e = std::min(std::max(e, -126), 127);
        while (e < 127 && std::ldexp(255.0, e) < ext) e++;
        e_byte[a] = (uint32_t)(e + 127);
        scale[a] = std::ldexp(1.0, e);
    }
    uint8_t q[6][8];
    for (int s = 0; s < 8; s++) {
        for (int a = 0; a < 6; a++) q[a][s] = a < 3 ? 255 : 0;  // empty slot: inverted box
        if (!((occ >> s) & 1u)) continue;
        for (int a = 0; a < 3; a++) {
            double ql = std::floor(((double)cb[s].lo[a] - (double)nb.lo[a]) / scale[a]);
            double qh = std::ceil(((double)cb[s].hi[a] - (double)nb.lo[a]) / scale[a]);
            ql = std::min(std::max(ql, 0.0), 255.0);
            qh = std::min(std::max(qh, 0.0), 255.0);
            q[a][s] = (uint8_t)ql;
            q[3 + a][s] = (uint8_t)qh;
        }
    }
    __builtin_memcpy(w, nb.lo, 12);
    w[3] = e_byte[0] | (e_byte[1] << 8) | (e_byte[2] << 16);
    for (int a = 0; a < 6; a++) {
        w[8 + 2 * a] = q[a][0] | (q[a][1] << 8) | (q[a][2] << 16) | ((uint32_t)q[a][3] << 24);
        w[9 + 2 * a] = q[a][4] | (q[a][5] << 8) | (q[a][6] << 16) | ((uint32_t)q[a][7] << 24);
    }
}

// ---- slot assignment ------------------------------------------------------------------------------------------------------------
// Slot bits (x, y, z) = which side of the node centre the child sits on, so that slot ^ (7 - ray octant) orders children front to
// back: greedy on dot(child centre - node centre, slot direction).  child_in[s] = the child (0 .. k - 1) in slot s, -1 = empty;
// every child gets a slot of its own
RT_HD void assign_slots(const Box* cb, int k, const Box& nb, int child_in[8]) {
    float score[8][8];
    for (int i = 0; i < k; i++) {
        float off[3];
        for (int a = 0; a < 3; a++) off[a] = 0.5f * (cb[i].lo[a] + cb[i].hi[a]) - 0.5f * (nb.lo[a] + nb.hi[a]);
        for (int s = 0; s < 8; s++) {
            float c = 0.0f;
            for (int a = 0; a < 3; a++) c += ((s >> (2 - a)) & 1) ? off[a] : -off[a];
            score[i][s] = c;
        }
    }
    int slot_of[8];
    for (int i = 0; i < 8; i++) slot_of[i] = child_in[i] = -1;
    for (int round = 0; round < k; round++) {
        float best = -std::numeric_limits<float>::infinity();
        int bi = -1, bs = -1;
        for (int i = 0; i < k; i++) {
            if (slot_of[i] >= 0) continue;
            for (int s = 0; s < 8; s++) {
                if (child_in[s] >= 0) continue;
                if (score[i][s] > best) {
                    best = score[i][s];
                    bi = i;
                    bs = s;
                }
            }
        }
        if (bi < 0) {  // only with non-finite scores (not for finite input): first free child into the first free slot
            bi = bs = 0;
            while (slot_of[bi] >= 0) bi++;
            while (child_in[bs] >= 0) bs++;
        }
        slot_of[bi] = bs;
        child_in[bs] = bi;
    }
}

}  // namespace rt
