// pt_traverse.h — path B, device side: what one lane needs to walk the compressed 8-wide BVH (bvh_node.h) with a ray.  The ray /
// triangle tests, the ray in traversal form, the work items (node and triangle groups), the per-lane stack, the node step, the
// triangle step and the round that the persistent loops repeat.  Used by the per-lane trace kernels, the test hook
// and the ray queries (pt_trace.hip), for the triangle tests and the ray set-up by the packet kernels (pt_packet.hip), for the stack,
// the work items and the unpacked node record (NodeRec) by the other query kernels (pt_query_loop.h and the pt_*_query.hip units).
// Only __device__ __forceinline__ functions, structs and constants: every unit that includes this compiles its own copy into its
// kernels, and the Makefile gives all of them the same flags so that the copies are the same code.
#pragma once
#include "rt_device_math.h"
#include "rt_internal.h"

namespace rt {
using namespace rtk;

constexpr float kShadowTmax = 0.999f;
constexpr int kTrisPerRound = 1;  // triangle tests per round of the inline schedules, unless tune_refill_min says otherwise (tris_per_round_of, pt_queue.h)
// waves per SIMD the kernels around the inline schedule are compiled for (pt_trace / pt_trace_fused with TRI_INLINE, pt_query_rays)
constexpr int kInlineWaves = 8;  // (7 = 72 VGPRs compiles to the same instruction count)

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---- spec §6.3: ray / triangle -------------------------------------------------------------------
__device__ __forceinline__ bool tri_test(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float& t_out) {
    const v3 pvec = cross(d, e2);
    const float det = dot(e1, pvec);
    if (det == 0.0f) return false;
    const v3 tvec = o - v0;
    const float u = dot(tvec, pvec);
    const v3 qvec = cross(tvec, e1);
    const float v = dot(d, qvec);
    if (det > 0.0f) {
        if (u < 0.0f || v < 0.0f || u + v > det) return false;
    } else {
        if (u > 0.0f || v > 0.0f || u + v < det) return false;
    }
    t_out = dot(e2, qvec) / det;
    return true;
}

// tri_test() up to its division, for a whole wave as straight-line code: the same operations in the same order, the per-lane early
// returns (about sixty scalar instructions per triangle in exec-mask bookkeeping) replaced by lane masks.  Returns the lanes of `lanes`
// whose ray passes through the triangle; their t is  dot(e2, qvec) / det.
__device__ __forceinline__ unsigned long long tri_inside_mask(v3 o, v3 d, v3 v0, v3 e1, v3 e2, unsigned long long lanes, float& det, v3& qvec) {
    const v3 pvec = cross(d, e2);
    det = dot(e1, pvec);
    const v3 tvec = o - v0;
    const float u = dot(tvec, pvec);
    qvec = cross(tvec, e1);
    const float v = dot(d, qvec);
    const float uv = u + v;
    // (ballots, combined as 64-bit scalars: boolean expressions come back as branches or through v_cndmask + v_cmp)
    const unsigned long long m_pos = __builtin_amdgcn_ballot_w64(det > 0.0f), m_nz = __builtin_amdgcn_ballot_w64(det != 0.0f);
    const unsigned long long out_pos = __builtin_amdgcn_ballot_w64(u < 0.0f) | __builtin_amdgcn_ballot_w64(v < 0.0f) | __builtin_amdgcn_ballot_w64(uv > det);
    const unsigned long long out_neg = __builtin_amdgcn_ballot_w64(u > 0.0f) | __builtin_amdgcn_ballot_w64(v > 0.0f) | __builtin_amdgcn_ballot_w64(uv < det);
    return lanes & m_nz & ((m_pos & ~out_pos) | (~m_pos & ~out_neg));
}

// tri_test() for the lanes of a wave that hold a triangle: ONE wave-uniform way out before the division.
__device__ __forceinline__ bool tri_test_flat(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float& t_out) {
    float det;
    v3 qvec;
    const unsigned long long inside = tri_inside_mask(o, d, v0, e1, e2, ~0ull, det, qvec);  // (ballots hold the active lanes only)
    if (inside == 0ull) return false;
    t_out = dot(e2, qvec) / det;
    return __builtin_amdgcn_inverse_ballot_w64(inside);
}

__device__ __forceinline__ v3 safe_inv(v3 d) {
    const float x = __builtin_fabsf(d.x) > 1e-20f ? d.x : __builtin_copysignf(1e-20f, d.x);
    const float y = __builtin_fabsf(d.y) > 1e-20f ? d.y : __builtin_copysignf(1e-20f, d.y);
    const float z = __builtin_fabsf(d.z) > 1e-20f ? d.z : __builtin_copysignf(1e-20f, d.z);
    return mk(1.0f / x, 1.0f / y, 1.0f / z);
}

// A ray in traversal form.  The slab test uses t = plane*inv - o*inv (one fma per plane); boxes are
// padded at build time and quantised outward, so this test only has to be conservative, not
// bit-identical to anything (results do not depend on which boxes are visited).
struct TRay {
    v3 o, d, inv, noi;  // noi = -(o * inv)
    float tmax;
    uint32_t oct_inv;   // 7 - octant: slot ^ oct_inv enumerates a node's children front to back
};
// 7 - octant of a direction, by sign BIT, like safe_inv's copysign: a -0.0 component has a negative reciprocal and must take the far plane first
__device__ __forceinline__ uint32_t octant_inv(v3 d) {
    return ((__float_as_uint(d.x) >> 31) ? 0u : 4u) | ((__float_as_uint(d.y) >> 31) ? 0u : 2u) | ((__float_as_uint(d.z) >> 31) ? 0u : 1u);
}
__device__ __forceinline__ TRay make_tray(v3 o, v3 d, float tmax) {
    TRay r;
    r.o = o;
    r.d = d;
    r.inv = safe_inv(d);
    r.noi = mk(-(o.x * r.inv.x), -(o.y * r.inv.y), -(o.z * r.inv.z));
    r.tmax = tmax;
    r.oct_inv = octant_inv(d);
    return r;
}

struct Hit {
    float t;
    int li;       // leaf-order triangle index, -1 = none
    uint32_t id;  // original triangle index (tie-break)
};

struct TravCounters {
    uint32_t nodes, tris, overflow;
    uint32_t flushes = 0;  // TRI_POOL, COUNT: pool_test passes of this wave (wave-uniform)
};

// A traversal work item (Ylitie et al. 2017): either a node group  x = child_base,
// y = hit bits of inner children in 31..24 (bit 24 + (slot ^ oct_inv): front to back) | the parent's imask in 7..0;
// or a triangle group  x = tri_base, y = hit leaf slots in 7..0 | the node's leafmask in 15..8
// (the triangle of leaf slot s is tri_base + popcount(leafmask below s), bvh_node.h).
struct Group {
    uint32_t x, y;
};
__device__ __forceinline__ bool has_nodes(const Group& g) { return g.y > 0x00ffffffu; }
__device__ __forceinline__ bool has_tris(const Group& t) { return (t.y & 0xffu) != 0u; }

typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef float f4v __attribute__((ext_vector_type(4)));  // native vector: HIP's float4 class has no address-space-qualified members
typedef __attribute__((address_space(3))) f4v lds_f4;

// Per-lane traversal stack of 8-byte groups.  The first `lds_cap` entries live in LDS (column of
// this thread, stride 256 entries: conflict-free); the tree pushes at most one pending sibling
// group per level, the builder reports the depth and the host sizes lds_cap + spill_cap to it;
// entries beyond lds_cap spill to a global column (entry-major, coalesced across a wave).
struct TravStack {
    // The LDS part is an address-space-qualified pointer on purpose: with two generic pointers the compiler folds pop()'s two
    // loads into ONE flat_load on a selected address - the flat path, both address computations and a vmcnt(0) + lgkmcnt(0) wait
    // for every pop, even when nothing ever spills.
    lds_u64* lds;
    unsigned long long* spill;
    size_t spill_stride;
    int lds_cap, spill_cap;
    int sp;
    __device__ __forceinline__ void push(Group g, uint32_t& overflow) {
        const unsigned long long v = ((unsigned long long)g.y << 32) | g.x;
        if (sp < lds_cap) lds[sp * 256] = v;
        else if (sp - lds_cap < spill_cap) spill[(size_t)(sp - lds_cap) * spill_stride] = v;
        else {
            overflow = 1;
            return;
        }
        sp++;
    }
    __device__ __forceinline__ Group pop() {  // caller checks sp > 0
        --sp;
        unsigned long long v;
        if (sp < lds_cap) v = lds[sp * 256];
        else v = spill[(size_t)(sp - lds_cap) * spill_stride];
        return Group{(uint32_t)v, (uint32_t)(v >> 32)};
    }
};

__device__ __forceinline__ float ubyte_f32(uint32_t w, int byte) {  // v_cvt_f32_ubyteN
    return (float)((w >> (8 * byte)) & 0xffu);
}

// An 80-byte node record (bvh_node.h) fetched and unpacked once, for the walks of the queries (pt_query_loop.h and the kernels around
// it): five 16-byte loads, the origin, the three scales from their exponent bytes, the masks, the bases and the twelve plane words.
// node_step below keeps its own hand-scheduled decode: the render kernels are compiled from it.
struct NodeRec {
    float ox, oy, oz, sx, sy, sz;
    uint32_t imask, leafmask, child_base, tri_base;
    uint32_t lx[2], ly[2], lz[2], hx[2], hy[2], hz[2];
    // node index of the inner child in slot s, leaf-order index of the triangle in leaf slot s: the slot's rank under its mask
    __device__ __forceinline__ uint32_t child(uint32_t s) const { return child_base + (uint32_t)__builtin_popcount(imask & ~(0xffffffffu << s)); }
    __device__ __forceinline__ uint32_t leaf_tri(uint32_t s) const { return tri_base + (uint32_t)__builtin_popcount(leafmask & ~(0xffffffffu << s)); }
};
__device__ __forceinline__ float plane_q(const uint32_t (&w)[2], int slot) { return ubyte_f32(w[slot >> 2], slot & 3); }  // a plane's byte, exact
template <bool COUNT>
__device__ __forceinline__ NodeRec fetch_node(const float4* __restrict__ nodes, uint32_t index, TravCounters& tc) {
    const float4* nd = nodes + (size_t)index * 5;
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3], n4 = nd[4];
    if (COUNT) tc.nodes++;
    const uint32_t w3 = __float_as_uint(n0.w);
    return NodeRec{n0.x, n0.y, n0.z, __uint_as_float((w3 & 0xffu) << 23), __uint_as_float(((w3 >> 8) & 0xffu) << 23), __uint_as_float(((w3 >> 16) & 0xffu) << 23),
                   w3 >> 24, __float_as_uint(n1.z) & 0xffu, __float_as_uint(n1.x), __float_as_uint(n1.y),
                   {__float_as_uint(n2.x), __float_as_uint(n2.y)}, {__float_as_uint(n2.z), __float_as_uint(n2.w)}, {__float_as_uint(n3.x), __float_as_uint(n3.y)},
                   {__float_as_uint(n3.z), __float_as_uint(n3.w)}, {__float_as_uint(n4.x), __float_as_uint(n4.y)}, {__float_as_uint(n4.z), __float_as_uint(n4.w)}};
}

// Visit the nearest pending inner child of node group G: fetch its 80-byte record (five 16-byte
// loads for eight children), slab-test the eight quantised boxes and turn the hits into a new node
// group (inner children, ordered by ray octant) and a triangle group (leaf triangles).
template <bool COUNT, bool UNORDERED = false>
__device__ __forceinline__ void node_step(const float4* __restrict__ nodes, const uint8_t* perm_lut, const TRay& r, Group& G, Group& T, TravStack& stk, TravCounters& tc) {
    const uint32_t hits = G.y;
    const uint32_t bit = 31u - (uint32_t)__builtin_clz(hits);
    G.y &= ~(1u << bit);
    if (has_nodes(G)) stk.push(G, tc.overflow);  // remaining siblings
    const uint32_t slot = UNORDERED ? bit - 24u : (bit - 24u) ^ r.oct_inv;  // UNORDERED (any-hit rays of an all-shadow launch): children in slot order, no re-keying
    const uint32_t rel = (uint32_t)__builtin_popcount(hits & ~(0xffffffffu << slot));  // low byte of hits = imask
    const float4* nd = nodes + (size_t)(G.x + rel) * 5;
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3], n4 = nd[4];
    if (COUNT) tc.nodes++;

    const uint32_t w3 = __float_as_uint(n0.w);
    const float sx = __uint_as_float((w3 & 0xffu) << 23), sy = __uint_as_float(((w3 >> 8) & 0xffu) << 23), sz = __uint_as_float(((w3 >> 16) & 0xffu) << 23);
    const uint32_t imask = w3 >> 24;
    // plane t = (p + q*s - o) * inv = q * (s*inv) + (p*inv - o*inv)
    const float ax = sx * r.inv.x, ay = sy * r.inv.y, az = sz * r.inv.z;
    const float bx = __builtin_fmaf(n0.x, r.inv.x, r.noi.x), by = __builtin_fmaf(n0.y, r.inv.y, r.noi.y), bz = __builtin_fmaf(n0.z, r.inv.z, r.noi.z);
    // entry / exit planes per axis are chosen once per node from the ray octant (no per-child min/max)
    const bool px = (r.oct_inv & 4u) != 0u, py = (r.oct_inv & 2u) != 0u, pz = (r.oct_inv & 1u) != 0u;  // direction >= 0
    const uint32_t lx[2] = {__float_as_uint(n2.x), __float_as_uint(n2.y)}, ly[2] = {__float_as_uint(n2.z), __float_as_uint(n2.w)};
    const uint32_t lz[2] = {__float_as_uint(n3.x), __float_as_uint(n3.y)}, hx[2] = {__float_as_uint(n3.z), __float_as_uint(n3.w)};
    const uint32_t hy[2] = {__float_as_uint(n4.x), __float_as_uint(n4.y)}, hz[2] = {__float_as_uint(n4.z), __float_as_uint(n4.w)};
    const uint32_t nx[2] = {px ? lx[0] : hx[0], px ? lx[1] : hx[1]}, fx[2] = {px ? hx[0] : lx[0], px ? hx[1] : lx[1]};
    const uint32_t ny[2] = {py ? ly[0] : hy[0], py ? ly[1] : hy[1]}, fy[2] = {py ? hy[0] : ly[0], py ? hy[1] : ly[1]};
    const uint32_t nz[2] = {pz ? lz[0] : hz[0], pz ? lz[1] : hz[1]}, fz[2] = {pz ? hz[0] : lz[0], pz ? hz[1] : lz[1]};
    // No relative slack on the comparison: the build pads every box by 2e-5 * M (M = largest |coordinate|), at least five
    // times the rounding error of these fmas for ray origins within 32 M (render_pt_common checks the camera), so a box
    // that holds the ray's hit - or a (t, id) tie - always passes tn <= tf and tn <= tmax.
    const float tlim = r.tmax;
    // The eight results are collected as SIGN BITS: miss = (miss << 1) | sign(tf - tn), one v_alignbit_b32 behind one
    // subtraction per child (instead of compare + select + or), children 7 .. 0 so that slot s ends in bit s.  tf - tn < 0 is
    // tn > tf except where tf = -0 meets tn = +0 (a box that ends exactly at the ray's origin and holds no hit with t > 0:
    // missing it is as good as entering it, results do not depend on which boxes are visited); no NaN reaches this point
    // (finite planes, |inv| <= 1e20, tmax = +inf only as the last argument of a minimum).  Empty slots hold inverted boxes.
    uint32_t miss = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const int w = i >> 2, bsel = i & 3;
        const float tnx = __builtin_fmaf(ubyte_f32(nx[w], bsel), ax, bx), tfx = __builtin_fmaf(ubyte_f32(fx[w], bsel), ax, bx);
        const float tny = __builtin_fmaf(ubyte_f32(ny[w], bsel), ay, by), tfy = __builtin_fmaf(ubyte_f32(fy[w], bsel), ay, by);
        const float tnz = __builtin_fmaf(ubyte_f32(nz[w], bsel), az, bz), tfz = __builtin_fmaf(ubyte_f32(fz[w], bsel), az, bz);
        const float tn = fmax_(fmax_(tnx, tny), fmax_(tnz, 0.0f));
        const float tf = fmin_(fmin_(tfx, tfy), fmin_(tfz, tlim));
        miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(tf - tn), 31u);
    }
    const uint32_t h8 = ~miss & 0xffu;  // bit s: the box in child slot s is hit
    // the hit bits are the work lists: inner children to enter, re-keyed front to back (bit slot -> bit slot ^ oct_inv,
    // one byte from a 2 KiB LDS table), and the leaf slots whose single triangle is to be tested
    const uint32_t leafmask = __float_as_uint(n1.z) & 0xffu;
    const uint32_t keyed = UNORDERED ? (h8 & imask) : perm_lut[r.oct_inv * 256u + (h8 & imask)];
    G.x = __float_as_uint(n1.x);
    G.y = (keyed << 24) | imask;
    T.x = __float_as_uint(n1.y);
    T.y = (h8 & leafmask) | (leafmask << 8);
}

// perm_lut[o * 256 + m] = the byte m with bit s moved to bit s ^ o (8 octants x 256 masks), built once per workgroup
__device__ __forceinline__ void build_perm_lut(uint8_t* lut) {
    for (uint32_t i = threadIdx.x; i < 2048u; i += blockDim.x) {
        const uint32_t o = i >> 8, m = i & 0xffu;
        uint32_t out = 0;
#pragma unroll
        for (uint32_t sl = 0; sl < 8; sl++) out |= ((m >> sl) & 1u) << (sl ^ o);
        lut[i] = (uint8_t)out;
    }
    __syncthreads();
}

// Test the next pending triangle of triangle group T.  is_any: what a hit means to this lane's ray - a compile-time constant where a
// kernel traces one kind of ray, a per-lane flag in the loop that carries both.  Returns true when an any-hit ray found an occluder.
// any_tmax: where an any-hit ray's segment ends - the constant of the shadow rays in the render kernels, a per-ray value in a ray query.
template <bool COUNT>
__device__ __forceinline__ bool tri_step(const float4* __restrict__ tris, TRay& r, Hit& best, Group& T, TravCounters& tc, bool is_any,
                                         float any_tmax = kShadowTmax) {
    const uint32_t bit = (uint32_t)__builtin_ctz(T.y);  // lowest pending leaf slot (caller checked has_tris)
    T.y &= T.y - 1u;
    const uint32_t li = T.x + (uint32_t)__builtin_popcount((T.y >> 8) & ~(0xffffffffu << bit));  // rank of the slot among the node's leaves
    const float4* tp = tris + (size_t)li * 3;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    if (COUNT) tc.tris++;
    float t;
    if (tri_test_flat(r.o, r.d, mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, c.x), t) && t > 0.0f) {
        if (is_any) return t < any_tmax;
        const uint32_t id = __float_as_uint(c.y);
        if (t < best.t || (t == best.t && id < best.id)) {
            best.t = t;
            best.li = (int)li;
            best.id = id;
            r.tmax = t;
        }
    }
    return false;
}
template <bool ANY, bool COUNT>
__device__ __forceinline__ bool tri_step(const float4* __restrict__ tris, TRay& r, Hit& best, Group& T, TravCounters& tc) { return tri_step<COUNT>(tris, r, best, T, tc, ANY); }

__device__ __forceinline__ Group root_group() { return Group{0u, 0x80000000u}; }  // "child 0 of nothing" = node 0

// Put a ray into a lane: traversal form, no hit yet, at the root with an empty stack.
__device__ __forceinline__ void start_ray(bool is_any, v3 o, v3 d, TRay& r, Hit& best, Group& G, Group& T, TravStack& stk) {
    r = make_tray(o, d, is_any ? kShadowTmax : __builtin_inff());
    if (!is_any) best = Hit{__builtin_inff(), -1, 0xffffffffu};
    G = root_group();
    T = Group{0u, 0u};
    stk.sp = 0;
}

// One round of the inline schedule: lanes without pending triangles visit their next node, then every lane that holds a leaf hit
// tests up to tris_per_round triangles.  alive: the lane has traversal work; returns whether it still has.  occluded: set when its
// any-hit ray found an occluder.  UNORDERED: see node_step.
// (alive goes in and out by value: a flag that the loops carry from round to round through a reference stays a byte in a vector
// register, with an and + compare wherever a branch needs it as a lane mask)
template <bool COUNT, bool UNORDERED>
__device__ __forceinline__ bool inline_round(const PtScene& sc, const uint8_t* perm_lut, TRay& r, Hit& best, Group& G, Group& T, TravStack& stk, TravCounters& tc,
                                             bool alive, bool& occluded, bool is_any, int tris_per_round, float any_tmax = kShadowTmax) {
    // node phase
    if (alive && !has_tris(T)) {
        if (!has_nodes(G)) {
            if (stk.sp) G = stk.pop();
            else alive = false;
        }
        if (alive) node_step<COUNT, UNORDERED>(sc.nodes, perm_lut, r, G, T, stk, tc);
    }
    // triangle phase: one test, then what a hit means to this lane's kind of ray
#pragma unroll 1
    for (int it = 0; it < tris_per_round; it++) {
        if (alive && has_tris(T)) {
            if (tri_step<COUNT>(sc.tris, r, best, T, tc, is_any, any_tmax)) {
                occluded = true;
                alive = false;
            }
        }
    }
    return alive;
}

// Whole-ray traversal for one lane (used by the rt_trace_rays test hook; the render kernels drive the same rounds from a refilling
// persistent loop).  Returns true when an any-hit ray found an occluder.
template <bool ANY, bool COUNT>
__device__ __forceinline__ bool traverse(const PtScene& sc, const uint8_t* perm_lut, v3 o, v3 d, TravStack& stk, Hit& best, TravCounters& tc) {
    TRay r;
    Group G, T;
    start_ray(ANY, o, d, r, best, G, T, stk);
    bool alive = true, occluded = false;
    while (alive) alive = inline_round<COUNT, false>(sc, perm_lut, r, best, G, T, stk, tc, alive, occluded, ANY, 1);
    return occluded;
}

// This thread's traversal stack: column threadIdx.x of the workgroup's dynamic LDS (sk.lds_cap x 256 entries), then its spill column
__device__ __forceinline__ TravStack make_trav_stack(unsigned long long* lds_stack, const StackCfg& sk) {
    const size_t gtid = (size_t)blockIdx.x * 256u + threadIdx.x;
    return TravStack{(lds_u64*)&lds_stack[threadIdx.x], sk.spill + gtid, sk.spill_stride, sk.lds_cap, sk.spill_cap, 0};
}

}  // namespace rt
