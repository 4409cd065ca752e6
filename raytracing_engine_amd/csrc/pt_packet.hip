// pt_packet.hip — path B: the packet kernels for camera rays, pt_trace_packet (per-ray slab tests of all eight children) and
// pt_trace_packet_ia (interval test for the pass first) and pt_trace_packet_wide (the interval test alone, two or four rays per lane: the
// default), with the generate stage fused (stage map: path_b.hip).  A whole wave walks
// the tree together, so nothing of the per-lane node step or queue is used: from pt_traverse.h only the triangle tests, safe_inv,
// octant_inv and Hit; the camera ray is pt_camera.h's.
#include "pt_camera.h"
#include "pt_launch.h"
#include "pt_traverse.h"

namespace rt {
using namespace rtk;

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// ---- packet trace (camera rays) ---------------------------------------------------------------------
// Camera rays share their origin and the 64 paths of a wave cover a 4x4-pixel block (Morton slots), so the
// whole wave walks the tree TOGETHER: one wave-uniform traversal (stack of node groups in LDS, node header and
// triangle records through scalar loads), the 48 quantised planes of a node decoded ONCE per wave - lane k
// converts plane k and parks it in LDS, ordered near / far for the packet's direction octant - and every
// lane then only runs the six slab fmas per child against planes broadcast from LDS.  A child is entered
// when ANY lane's ray hits its box, a leaf's triangles are tested by all lanes (testing more boxes or
// triangles than a ray needs never changes its (t, id)-minimal hit).  Per node step
// this costs about 100 vector instructions and one 48-byte vector load for 64 rays, against about 300
// instructions and 64 x 5 sixteen-byte gathers in pt_trace.  Lanes whose octant differs from the packet
// leader's (blocks that straddle a sign change of the direction) are walked in a further pass.
constexpr int kPkStack = (int)kPacketStackEntries;  // one pending sibling group per tree level; render_pt_common sends trees whose stack_need exceeds it
                                                   // (single-level: depth <= kBvhMaxDepth / 3 + 2; a flattened two-level tree adds its top level) to the per-lane kernel

// What both packet kernels do first - the generate stage, fused: the kernel makes the camera rays it traces (pt_shade(0) needs only
// the direction) - and last.  Returns whether path pid exists.
struct PacketRays {
    v3 o;  // wave-uniform
    v3 d, inv, noi;
    uint32_t oct_inv;
};
__device__ __forceinline__ bool packet_camera_ray(const PtFrame& f, const PtState& st, uint32_t pid, PacketRays& p) {
    bool alive = false;
    p.d = mk(0.0f, 1.0f, 0.0f);
    if (pid < f.n_paths) {
        const uint32_t slot = pid / f.spp_batch;
        uint32_t px, py, lx, ly, k;
        alive = slot_pixel(f, slot, px, py, lx, ly, k);
        if (alive) {
            p.d = camera_dir(f, px, py, f.sample0 + (pid - slot * f.spp_batch));
            st.ray_d[pid] = make_float4(p.d.x, p.d.y, p.d.z, 0.0f);
        }
    }
    p.o = mk(f.cam.pos[0], f.cam.pos[1], f.cam.pos[2]);
    p.inv = safe_inv(p.d);
    p.noi = mk(-(p.o.x * p.inv.x), -(p.o.y * p.inv.y), -(p.o.z * p.inv.z));
    p.oct_inv = octant_inv(p.d);
    return alive;
}
template <bool COUNT>
__device__ __forceinline__ void packet_finish(const PtState& st, unsigned long long* __restrict__ stats, uint32_t pid, uint32_t lane, bool alive, const Hit& best,
                                              uint32_t n_nodes, uint32_t n_tris, uint32_t overflow /* the last three wave-uniform */) {
    if (alive) st.hit[pid] = make_float2(best.t, __int_as_float(best.li));
    if (COUNT && lane == 0) {  // records fetched once per wave
        atomicAdd(&stats[PT_STAT_PACKETS + 1], (unsigned long long)n_nodes);
        atomicAdd(&stats[PT_STAT_PACKETS + 2], (unsigned long long)n_tris);
        atomicAdd(&stats[PT_STAT_PACKETS], 1ull);
    }
    if (overflow && lane == 0) atomicOr((unsigned int*)&stats[PT_STAT_OVERFLOW], 1u);
}

template <bool COUNT>
__global__ __launch_bounds__(256) void pt_trace_packet(const PtScene sc, const PtFrame f, PtState st, unsigned long long* __restrict__ stats) {
    // (PtState is passed by value: its pointers are written through)
    __shared__ float s_planes[4][64];
    __shared__ unsigned long long s_stack[4][kPkStack];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    float* planes = s_planes[wv];
    unsigned long long* stack = s_stack[wv];
    const uint32_t pid = (blockIdx.x * 4u + wv) * 64u + lane;

    PacketRays pr;
    const bool alive = packet_camera_ray(f, st, pid, pr);
    const v3 o = pr.o, d = pr.d, inv = pr.inv, noi = pr.noi;
    const uint32_t oct_inv = pr.oct_inv;
    Hit best{__builtin_inff(), -1, 0xffffffffu};

    // lane k < 48 decodes plane k of a node: byte 32 + k = qlo.x[8] qlo.y[8] qlo.z[8] qhi.x[8] qhi.y[8] qhi.z[8]
    const uint32_t pl = lane < 48u ? lane : 47u;
    const uint32_t p_axis = (pl >> 3) % 3u, p_child = pl & 7u;
    const bool p_hi = pl >= 24u;
    uint32_t n_nodes = 0, n_tris = 0, overflow = 0;  // wave-uniform

    unsigned long long remaining = __ballot(alive);
    while (remaining) {
        const uint32_t oct = (uint32_t)__builtin_amdgcn_readlane((int)oct_inv, (int)__builtin_ctzll(remaining));
        const bool act = alive && oct_inv == oct;
        const unsigned long long act_mask = __ballot(act);  // wave-uniform
        remaining &= ~act_mask;
        // LDS slot of this lane's plane: child * 8 + {near x, near y, near z, far x, far y, far z}
        const bool dir_pos = ((oct >> (2u - p_axis)) & 1u) != 0u;  // oct bit 4 = x, 2 = y, 1 = z: direction >= 0
        const uint32_t lds_idx = p_child * 8u + (p_hi == dir_pos ? 3u : 0u) + p_axis;

        int sp = 0;
        uint32_t gx = 0u, gy = 0x80000000u;  // the root group
        for (;;) {
            if (gy <= 0x00ffffffu) {
                if (sp == 0) break;
                const unsigned long long e = stack[--sp];
                gx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)e);
                gy = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(e >> 32));
            }
            const uint32_t bit = 31u - (uint32_t)__builtin_clz(gy);
            const uint32_t hits = gy;
            gy &= ~(1u << bit);
            if (gy > 0x00ffffffu) {  // remaining siblings
                if (sp < kPkStack) {
                    if (lane == 0) stack[sp] = ((unsigned long long)gy << 32) | gx;
                    sp++;
                } else {
                    overflow = 1;
                }
            }
            const uint32_t slot = (bit - 24u) ^ oct;
            const uint32_t node = gx + (uint32_t)__builtin_popcount(hits & ~(0xffffffffu << slot));
            const uint32_t* __restrict__ nd = reinterpret_cast<const uint32_t*>(sc.nodes) + (size_t)uniform(node) * 20u;
            if (COUNT) n_nodes++;
            // header: the address is wave-uniform, so the 32 bytes come through the SCALAR cache into scalar registers.  Written as an
            // s_load: left to itself the compiler issues vector loads of the one address (it cannot rule out that the kernel's own
            // stores alias the node array) and moves the seven words to scalar registers with seven v_readfirstlane
            u32x8 hdr;
            asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hdr) : "s"(nd) : "memory");
            const float px_ = __uint_as_float(hdr[0]), py_ = __uint_as_float(hdr[1]), pz_ = __uint_as_float(hdr[2]);
            const uint32_t w3 = hdr[3], child_base = hdr[4], tri_base = hdr[5], leafmask = hdr[6] & 0xffu;
            const float sx = __uint_as_float((w3 & 0xffu) << 23), sy = __uint_as_float(((w3 >> 8) & 0xffu) << 23), sz = __uint_as_float(((w3 >> 16) & 0xffu) << 23);
            const uint32_t imask = w3 >> 24;
            // cooperative decode: one 48-byte vector load for the wave, world-space plane = p + q * scale
            const uint32_t q = reinterpret_cast<const uint8_t*>(nd)[32u + pl];
            const float ps = p_axis == 0u ? sx : p_axis == 1u ? sy : sz, pp = p_axis == 0u ? px_ : p_axis == 1u ? py_ : pz_;
            const float plane = __builtin_fmaf((float)q, ps, pp);
            __builtin_amdgcn_wave_barrier();  // the previous node's plane reads are done (one wave: DS ops run in order)
            if (lane < 48u) planes[lds_idx] = plane;
            __builtin_amdgcn_wave_barrier();
            uint32_t any = 0;  // bit c: some ray of the pass hits child slot c (empty slots hold inverted boxes and never hit)
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const float4 a = *reinterpret_cast<const float4*>(&planes[c * 8]);      // near x, y, z, far x
                const float2 b = *reinterpret_cast<const float2*>(&planes[c * 8 + 4]);  // far y, z
                const float tn = fmax_(fmax_(__builtin_fmaf(a.x, inv.x, noi.x), __builtin_fmaf(a.y, inv.y, noi.y)), fmax_(__builtin_fmaf(a.z, inv.z, noi.z), 0.0f));
                const float tf = fmin_(fmin_(__builtin_fmaf(a.w, inv.x, noi.x), __builtin_fmaf(b.x, inv.y, noi.y)), fmin_(__builtin_fmaf(b.y, inv.z, noi.z), best.t));
                // (scalar arithmetic on the ballot, no bool: a uniform i1 is kept as a lane mask and the select comes back through
                // v_cndmask + v_readfirstlane, two vector instructions per child)
                const uint32_t hit_lanes = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(tn <= tf) & act_mask);
                any |= (hit_lanes < 1u ? hit_lanes : 1u) << c;
            }
            // wave-uniform bookkeeping, branch-free on the scalar unit: inner children to enter, keyed by
            // slot ^ octant (front to back), and the triangles of the leaf children that were hit
            uint32_t ih = any & imask;
            ih = (oct & 1u) ? (((ih & 0x55u) << 1) | ((ih >> 1) & 0x55u)) : ih;
            ih = (oct & 2u) ? (((ih & 0x33u) << 2) | ((ih >> 2) & 0x33u)) : ih;
            ih = (oct & 4u) ? (((ih & 0x0fu) << 4) | ((ih >> 4) & 0x0fu)) : ih;
            const uint32_t inner_hits = ih << 24;
            for (uint32_t lh = any & leafmask; lh; lh &= lh - 1u) {  // the single triangles of the leaf slots some ray hit
                const uint32_t c = (uint32_t)__builtin_ctz(lh);
                const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ~(0xffffffffu << c));
                const float* __restrict__ tp = reinterpret_cast<const float*>(sc.tris) + (size_t)li * 12u;  // wave-uniform: scalar loads
                if (COUNT) n_tris++;
                float t;
                if (act && tri_test(o, d, mk(tp[0], tp[1], tp[2]), mk(tp[3], tp[4], tp[5]), mk(tp[6], tp[7], tp[8]), t) && t > 0.0f) {
                    const uint32_t id = __float_as_uint(tp[9]);
                    if (t < best.t || (t == best.t && id < best.id)) {
                        best.t = t;
                        best.li = (int)li;
                        best.id = id;
                    }
                }
            }
            gx = child_base;
            gy = inner_hits | imask;
        }
    }
    packet_finish<COUNT>(st, stats, pid, lane, alive, best, n_nodes, n_tris, overflow);
}

// ---- packet trace, interval form ---------------------------------------------------------------------
// The same walk with the node test in two steps.  (1) ONE interval test per child for the whole pass, on 8 lanes per child:
// the rays of a pass share their origin and the signs of their direction, so with [imin, imax] the range of 1 / d over the
// pass's lanes (per axis) every lane's slab distance (plane - o) * inv lies between the products with the two ends; lane
// 8c + k holds plane k of child c (k = 0..2 near x y z, 4..6 far x y z, 3 / 7 the constants 0 and -(largest best.t)),
// turns it into a LOWER bound of t_near resp. of -t_far (widened by the rounding of the lanes' own fma form), and two
// quad-wide DPP maxima + one half-row mirror add give  max(lower bounds of t_near, 0) - min(upper bounds of t_far, best)  in
// lane 8c; one ds_bpermute hands the eight verdicts to lanes 0..15 in the two orders the bookkeeping wants (front to back for
// the inner children, slot order for the leaves), so ONE ballot is the next node group and the leaf list: about ten vector
// instructions for all eight children.  (2) Only children that pass - 1.2 of 8 on the metric's scene are hit by any ray -
// get the per-ray slab test of the kernel above (planes parked in LDS as there); PURE skips (2) and enters every child that
// passes (1).  Both walk a superset of the boxes each ray would visit alone and test every triangle with the ray's own
// arithmetic, so frames are unchanged.  The traversal stack lives in two VGPRs (entry i in lane i).
typedef __attribute__((address_space(3))) float lds_f32;
// v = max(v, v of the lane the DPP control names); written out because the builtin form (v_mov_dpp, then fmaxf) pays a
// canonicalising v_max per operand.  s_nop 1: a DPP read of a VGPR needs two wait states behind the VALU write, which the
// compiler does not insert for text it does not parse.
#define RT_DPP_F32(op, v, ctrl) asm("s_nop 1\n\tv_" op "_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf" : "+v"(v))
#define RT_DPP_MAX(v, ctrl) RT_DPP_F32("max", v, ctrl)
#define RT_DPP_ROWS(op, v)                    \
    do {                                      \
        RT_DPP_F32(op, v, "quad_perm:[1,0,3,2]"); \
        RT_DPP_F32(op, v, "quad_perm:[2,3,0,1]"); \
        RT_DPP_F32(op, v, "row_half_mirror");     \
        RT_DPP_F32(op, v, "row_mirror");          \
    } while (0)
// largest (IS_MAX) or smallest of a wave-uniform set of NON-NEGATIVE floats, one per lane (integer order = float order): rows by DPP,
// then the scalar unit
template <bool IS_MAX>
__device__ __forceinline__ float wave_reduce_nonneg(float v) {
    if (IS_MAX) RT_DPP_ROWS("max", v);
    else RT_DPP_ROWS("min", v);
    const uint32_t b = __float_as_uint(v);
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)b, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)b, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)b, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)b, 48);
    const uint32_t m01 = (IS_MAX ? r0 > r1 : r0 < r1) ? r0 : r1, m23 = (IS_MAX ? r2 > r3 : r2 < r3) ? r2 : r3;
    return __uint_as_float((IS_MAX ? m01 > m23 : m01 < m23) ? m01 : m23);
}
template <bool COUNT, bool PURE, bool FARCAP>
__global__ __launch_bounds__(256) void pt_trace_packet_ia(const PtScene sc, const PtFrame f, PtState st, unsigned long long* __restrict__ stats) {
    __shared__ f4v s_planes[4][16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    lds_f32* planes = (lds_f32*)s_planes[wv];
    lds_f4* planes4 = (lds_f4*)s_planes[wv];
    const uint32_t pid = (blockIdx.x * 4u + wv) * 64u + lane;

    PacketRays pr;
    const bool alive = packet_camera_ray(f, st, pid, pr);
    const v3 o = pr.o, d = pr.d, inv = pr.inv, noi = pr.noi;
    const uint32_t oct_inv = pr.oct_inv;
    Hit best{__builtin_inff(), -1, 0xffffffffu};

    // lane 8c + k: plane k of child c
    const uint32_t p_child = lane >> 3, pk = lane & 7u, p_axis = pk & 3u;
    const bool p_plane = p_axis != 3u, p_far = pk >= 4u;
    const float o_ax = p_axis == 0u ? o.x : p_axis == 1u ? o.y : o.z;
    uint32_t n_nodes = 0, n_tris = 0, overflow = 0;  // wave-uniform

    unsigned long long remaining = __ballot(alive);
    while (remaining) {
        const uint32_t oct = (uint32_t)__builtin_amdgcn_readlane((int)oct_inv, (int)__builtin_ctzll(remaining));
        const bool act = alive && oct_inv == oct;
        const unsigned long long act_mask = __ballot(act);  // wave-uniform
        remaining &= ~act_mask;
        // the pass's range of 1 / d per axis (one sign per axis: the octant is shared), and this lane's share of it
        const float inf = __builtin_inff();
        // (by magnitude - rows by DPP, the four rows on the scalar unit in integer order - and the pass's sign put back; which end is
        // "min" does not matter: the bounds below take the smaller of the two products)
        const float ax = __builtin_fabsf(inv.x), ay = __builtin_fabsf(inv.y), az = __builtin_fabsf(inv.z);
        const float ix0 = wave_reduce_nonneg<false>(act ? ax : inf), ix1 = wave_reduce_nonneg<true>(act ? ax : 0.0f);
        const float iy0 = wave_reduce_nonneg<false>(act ? ay : inf), iy1 = wave_reduce_nonneg<true>(act ? ay : 0.0f);
        const float iz0 = wave_reduce_nonneg<false>(act ? az : inf), iz1 = wave_reduce_nonneg<true>(act ? az : 0.0f);
        const float i_sign = ((oct >> (2u - (p_axis < 2u ? p_axis : 2u))) & 1u) != 0u ? 1.0f : -1.0f;  // oct bit set: direction >= 0
        const float imin = i_sign * (p_axis == 0u ? ix0 : p_axis == 1u ? iy0 : iz0), imax = i_sign * (p_axis == 0u ? ix1 : p_axis == 1u ? iy1 : iz1);
        // near lanes bound t from below: min(u * imin, u * imax); far lanes bound -t from below: min(u * -imin, u * -imax)
        const float ia_a = p_plane ? (p_far ? -imin : imin) : 0.0f, ia_b = p_plane ? (p_far ? -imax : imax) : 0.0f;
        // widening: a lane computes fma(plane, inv, -(o * inv)), off the exact (plane - o) * inv by at most 2^-24 (|o * inv| + |t|)
        float ia_m = p_plane ? (__builtin_fabsf(o_ax) * fmax_(__builtin_fabsf(imin), __builtin_fabsf(imax))) * 0x1p-22f : (pk == 3u ? 0.0f : inf);
        const bool dir_pos = p_plane && ((oct >> (2u - p_axis)) & 1u) != 0u;  // oct bit 4 = x, 2 = y, 1 = z: direction >= 0
        const uint32_t q_off = p_plane ? 32u + (p_far == dir_pos ? 24u : 0u) + p_axis * 8u + p_child : 32u + p_child;
        // Lanes 0..15 collect the children's verdicts (one ds_bpermute of lane 8c's value): lane p < 8 reads child slot p ^ oct - the
        // ballot's bits 0..7 are the hit INNER children in front-to-back order, what the group word wants - and lane 8 + c reads
        // slot c for the leaves.  v_sh moves the lane's bit of  imask | leafmask << 8  to the sign.
        const uint32_t v_slot = lane < 8u ? lane ^ oct : lane & 7u;
        const uint32_t v_addr = lane < 16u ? v_slot * 32u : 0u;
        const uint32_t v_sh = lane < 8u ? 31u - v_slot : lane < 16u ? 31u - lane : 0u;  // lanes >= 16: bit 31 of the word, always 0
        const uint32_t p_sh = lane < 8u ? 31u - (lane ^ oct) : 0u;  // (hybrid) bit p ^ oct of a slot-ordered mask to the sign; other lanes: see the & 0xff
        const uint32_t s_sh = 23u - 8u * (p_axis < 2u ? p_axis : 2u);  // this lane's scale exponent of header word 3 to the exponent field
        const float w_x = p_axis == 0u ? 1.0f : 0.0f, w_y = p_axis == 1u ? 1.0f : 0.0f, w_z = p_axis >= 2u ? 1.0f : 0.0f;

        // traversal stack in two VGPRs, entry i in lane i (v_writelane / v_readlane with a scalar index: no LDS, no exec games);
        // render_pt_common sends trees that may need more than kPacketStackEntries (< 64) entries to the per-lane kernel
        int stx = 0, sty = 0;                // entry 0 = (0, 0): the end marker
        uint32_t sp = 1, sp_max = 0;
        uint32_t gx = 0u, gy = 0x80000000u;  // the root group
        for (;;) {
        do {  // (gx, gy) holds at least one child; the inner loop descends while some child is entered
            const uint32_t lz = (uint32_t)__builtin_clz(gy);  // 0..7: the front-most pending child is bit 31 - lz
            const uint32_t hits = gy;
            gy &= ~(0x80000000u >> lz);
            if (gy > 0x00ffffffu) {  // remaining siblings
                // (no builtin for v_writelane in this compiler; below gfx10 the lane select has to come through m0 when the value is a
                // scalar register - one constant-bus operand.  m0 is a reserved register that cannot be named as a clobber, so the
                // statement puts back what it found there)
                uint32_t m0_saved;
                asm("s_mov_b32 %2, m0\n\ts_mov_b32 m0, %5\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %4, m0\n\ts_mov_b32 m0, %2"
                    : "+v"(stx), "+v"(sty), "=&s"(m0_saved)
                    : "s"(gx), "s"(gy), "s"(sp));
                sp++;
                sp_max = sp_max > sp ? sp_max : sp;
            }
            const uint32_t slot = (7u - lz) ^ oct;
            const uint32_t node = gx + (uint32_t)__builtin_popcount(hits & ((1u << slot) - 1u));
            const uint32_t* __restrict__ nd = reinterpret_cast<const uint32_t*>(sc.nodes) + (size_t)uniform(node) * 20u;
            if (COUNT) n_nodes++;
            const uint32_t q = reinterpret_cast<const uint8_t*>(nd)[q_off];  // issued ahead of the header's wait
            u32x8 hdr;
            asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hdr) : "s"(nd) : "memory");
            const float px_ = __uint_as_float(hdr[0]), py_ = __uint_as_float(hdr[1]), pz_ = __uint_as_float(hdr[2]);
            const uint32_t w3 = hdr[3], child_base = hdr[4], tri_base = hdr[5], leafmask = hdr[6] & 0xffu;
            const uint32_t imask = w3 >> 24;
            // this lane's plane: p[axis] + q * 2^e[axis]; the axis is picked with 0 / 1 weights (three fast multiply-adds, one scalar
            // operand each) instead of selects (the constant bus takes one scalar register per instruction)
            const float ps = __uint_as_float((w3 << s_sh) & 0x7f800000u);
            const float pp = __builtin_fmaf(w_z, pz_, __builtin_fmaf(w_y, py_, w_x * px_));
            const float plane = __builtin_fmaf((float)q, ps, pp);
            if (!PURE) {
                __builtin_amdgcn_wave_barrier();  // the previous node's plane reads are done (one wave: DS ops run in order)
                planes[lane] = plane;             // child c: [near x y z, -, far x y z, -]
                __builtin_amdgcn_wave_barrier();
            }
            // (1) interval test: lane 8c + k bounds its plane, quad maxima, near + (-far) <= 0 in lanes 8c..8c+3
            const float u = plane - o_ax;
            const float lo = fmin_(u * ia_a, u * ia_b);
            float qm = __builtin_fmaf(__builtin_fabsf(lo), -0x1p-21f, lo - ia_m);
            RT_DPP_MAX(qm, "quad_perm:[1,0,3,2]");
            RT_DPP_MAX(qm, "quad_perm:[2,3,0,1]");  // every lane holds its quad's maximum
            float gap;  // max(lower bounds of t_near, 0) - min(upper bounds of t_far, cap): all finite
            asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(gap) : "v"(qm));
            const float gap_c = __int_as_float(__builtin_amdgcn_ds_bpermute((int)v_addr, __float_as_int(gap)));
            const uint32_t masks = imask | ((PURE ? leafmask : imask | leafmask) << 8);  // bits 8..15: what step (2) / the triangle loop may be handed
            // (two ballots and a scalar AND: the AND of two i1 would go through v_cndmask and a third compare)
            const uint32_t verdict = (uint32_t)__builtin_amdgcn_ballot_w64(gap_c <= 0.0f) & (uint32_t)__builtin_amdgcn_ballot_w64((int)(masks << v_sh) < 0);
            uint32_t any;  // bit c: leaf / inner child slot c is entered (slot order)
            uint32_t inner_hits;
            if (PURE) {
                any = verdict >> 8;
                inner_hits = verdict << 24;
            } else {  // (2) the rays' own slab tests of the children that passed
                any = 0;
                for (uint32_t m = (verdict >> 8) & 0xffu; m; m &= m - 1u) {
                    const uint32_t c = (uint32_t)__builtin_ctz(m);
                    const f4v a = planes4[2u * c], b = planes4[2u * c + 1u];
                    const float tn = fmax_(fmax_(__builtin_fmaf(a.x, inv.x, noi.x), __builtin_fmaf(a.y, inv.y, noi.y)), fmax_(__builtin_fmaf(a.z, inv.z, noi.z), 0.0f));
                    const float tf = fmin_(fmin_(__builtin_fmaf(b.x, inv.x, noi.x), __builtin_fmaf(b.y, inv.y, noi.y)), fmin_(__builtin_fmaf(b.z, inv.z, noi.z), best.t));
                    // (scalar text: a uniform i1 is kept as a lane mask and comes back through v_cndmask + v_readfirstlane)
                    const unsigned long long hit_mask = __builtin_amdgcn_ballot_w64(tn <= tf) & act_mask;
                    uint32_t some;
                    asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(some) : "s"(hit_mask) : "scc");
                    any |= some << c;
                }
                // front-to-back order of the inner hits: lane p < 8 looks at bit p ^ oct, the ballot is the permuted byte
                inner_hits = (uint32_t)__builtin_amdgcn_ballot_w64((int)((any & imask) << p_sh) < 0 && lane < 8u) << 24;
            }
            unsigned long long improved = 0ull;  // wave-uniform: lanes whose best hit moved at this node
            for (uint32_t lh = any & leafmask; lh; lh &= lh - 1u) {  // the single triangles of the leaf slots that are entered
                const uint32_t c = (uint32_t)__builtin_ctz(lh);
                const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ((1u << c) - 1u));
                const float* __restrict__ tp = reinterpret_cast<const float*>(sc.tris) + (size_t)li * 12u;  // wave-uniform address
                if (COUNT) n_tris++;
                float det;
                v3 qvec;
                const unsigned long long inside = tri_inside_mask(o, d, mk(tp[0], tp[1], tp[2]), mk(tp[3], tp[4], tp[5]), mk(tp[6], tp[7], tp[8]), act_mask, det, qvec);
                if (inside == 0ull) continue;
                const float t = dot(mk(tp[6], tp[7], tp[8]), qvec) / det;
                const uint32_t id = __float_as_uint(tp[9]);
                const unsigned long long closer = __builtin_amdgcn_ballot_w64(t < best.t) | (__builtin_amdgcn_ballot_w64(t == best.t) & __builtin_amdgcn_ballot_w64(id < best.id));
                const unsigned long long take = inside & __builtin_amdgcn_ballot_w64(t > 0.0f) & closer;
                if (FARCAP) improved |= take;
                const bool mine = __builtin_amdgcn_inverse_ballot_w64(take);
                best.t = mine ? t : best.t;
                best.li = mine ? (int)li : best.li;
                best.id = mine ? id : best.id;
            }
            if (FARCAP && improved != 0ull) {
                const float maxbest = wave_reduce_nonneg<true>(act ? best.t : 0.0f);
                if (pk == 7u) ia_m = maxbest;
            }
            gx = child_base;
            gy = inner_hits | imask;
        } while (gy > 0x00ffffffu);
            // no child entered: on with the newest pending group
            sp--;
            gx = (uint32_t)__builtin_amdgcn_readlane(stx, (int)sp);
            gy = (uint32_t)__builtin_amdgcn_readlane(sty, (int)sp);
            if (gy == 0u) break;
        }
        if (sp_max > 63u) overflow = 1;
    }
    packet_finish<COUNT>(st, stats, pid, lane, alive, best, n_nodes, n_tris, overflow);
}

// ---- packet trace, interval form, R rays per lane ------------------------------------------------------
// pt_trace_packet_ia<COUNT, PURE = true, FARCAP = true> with R consecutive 64-path groups in one wave: wave w walks the tree once for
// paths [w * 64R, (w + 1) * 64R), lane l holds paths base + l + 64r (r < R) - with the Morton slots at 4 spp an 8x4 (R = 2) or 8x8
// (R = 4) pixel block, for other sample counts whatever the numbering gives; nothing below depends on it.  Neighbouring 4x4 blocks
// walk almost the same nodes (a block is far narrower than a bottom-level box), so the node step - header, plane decode, interval
// test, ds_bpermute, ballot, VGPR stack: all as above - is paid once for R x 64 rays: the interval test works on the pass's range
// of 1 / d whatever the number of rays, reduced over a lane's R rays first and then across the wave.  Only the triangle test grows
// with R: the record is loaded once, tri_inside_mask and the division run once per ray index, each with its own lane mask, its own
// best hit and its own wave-uniform way out.  A pass takes the rays of ONE direction octant among all R x 64; the others wait for a
// later pass.  Per ray the kernel keeps the direction and the best hit (6 VGPRs); 1 / d is needed for the range only and is
// recomputed at the head of each pass.  Every ray tests a superset of the triangles its own walk would reach, with its own
// arithmetic, so its (t, id)-minimal hit - and the frame - is unchanged.
template <bool COUNT, int R>
__global__ __launch_bounds__(256) void pt_trace_packet_wide(const PtScene sc, const PtFrame f, PtState st, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t pid0 = (blockIdx.x * 4u + wv) * (64u * (uint32_t)R) + lane;  // path of ray index r: pid0 + 64 r

    v3 o = mk(0.0f, 0.0f, 0.0f), d[R];
    Hit best[R];
    uint32_t ray_bits = 0;  // nibble r: 7 - octant of ray r, bit 3 = the path exists
    unsigned long long remaining[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        PacketRays pr;
        const bool alive = packet_camera_ray(f, st, pid0 + 64u * (uint32_t)r, pr);
        o = pr.o;
        d[r] = pr.d;
        best[r] = Hit{__builtin_inff(), -1, 0xffffffffu};
        ray_bits |= (pr.oct_inv | (alive ? 8u : 0u)) << (4 * r);
        remaining[r] = __ballot(alive);
    }

    // lane 8c + k: plane k of child c
    const uint32_t p_child = lane >> 3, pk = lane & 7u, p_axis = pk & 3u;
    const bool p_plane = p_axis != 3u, p_far = pk >= 4u;
    const float o_ax = p_axis == 0u ? o.x : p_axis == 1u ? o.y : o.z;
    uint32_t n_nodes = 0, n_tris = 0, overflow = 0;  // wave-uniform

    for (;;) {
        // the pass's octant: that of the first ray still waiting
        uint32_t oct = 8u;
#pragma unroll
        for (int r = R - 1; r >= 0; r--)
            if (remaining[r]) oct = ((uint32_t)__builtin_amdgcn_readlane((int)ray_bits, (int)__builtin_ctzll(remaining[r])) >> (4 * r)) & 7u;
        if (oct == 8u) break;
        unsigned long long act_mask[R];  // wave-uniform, one per ray index
        const float inf = __builtin_inff();
        // the pass's range of |1 / d| per axis: over the lane's own rays first, then across the wave
        float ax0 = inf, ay0 = inf, az0 = inf, ax1 = 0.0f, ay1 = 0.0f, az1 = 0.0f;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const bool act = ((ray_bits >> (4 * r)) & 15u) == (oct | 8u);
            act_mask[r] = __ballot(act);
            remaining[r] &= ~act_mask[r];
            const v3 inv = safe_inv(d[r]);
            const float ax = __builtin_fabsf(inv.x), ay = __builtin_fabsf(inv.y), az = __builtin_fabsf(inv.z);
            ax0 = fmin_(ax0, act ? ax : inf), ax1 = fmax_(ax1, act ? ax : 0.0f);
            ay0 = fmin_(ay0, act ? ay : inf), ay1 = fmax_(ay1, act ? ay : 0.0f);
            az0 = fmin_(az0, act ? az : inf), az1 = fmax_(az1, act ? az : 0.0f);
        }
        const float ix0 = wave_reduce_nonneg<false>(ax0), ix1 = wave_reduce_nonneg<true>(ax1);
        const float iy0 = wave_reduce_nonneg<false>(ay0), iy1 = wave_reduce_nonneg<true>(ay1);
        const float iz0 = wave_reduce_nonneg<false>(az0), iz1 = wave_reduce_nonneg<true>(az1);
        // from here to the triangle loop: pt_trace_packet_ia's pass, PURE and FARCAP (the comments are there)
        const float i_sign = ((oct >> (2u - (p_axis < 2u ? p_axis : 2u))) & 1u) != 0u ? 1.0f : -1.0f;
        const float imin = i_sign * (p_axis == 0u ? ix0 : p_axis == 1u ? iy0 : iz0), imax = i_sign * (p_axis == 0u ? ix1 : p_axis == 1u ? iy1 : iz1);
        const float ia_a = p_plane ? (p_far ? -imin : imin) : 0.0f, ia_b = p_plane ? (p_far ? -imax : imax) : 0.0f;
        float ia_m = p_plane ? (__builtin_fabsf(o_ax) * fmax_(__builtin_fabsf(imin), __builtin_fabsf(imax))) * 0x1p-22f : (pk == 3u ? 0.0f : inf);
        const bool dir_pos = p_plane && ((oct >> (2u - p_axis)) & 1u) != 0u;
        const uint32_t q_off = p_plane ? 32u + (p_far == dir_pos ? 24u : 0u) + p_axis * 8u + p_child : 32u + p_child;
        const uint32_t v_slot = lane < 8u ? lane ^ oct : lane & 7u;
        const uint32_t v_addr = lane < 16u ? v_slot * 32u : 0u;
        const uint32_t v_sh = lane < 8u ? 31u - v_slot : lane < 16u ? 31u - lane : 0u;
        const uint32_t s_sh = 23u - 8u * (p_axis < 2u ? p_axis : 2u);
        const float w_x = p_axis == 0u ? 1.0f : 0.0f, w_y = p_axis == 1u ? 1.0f : 0.0f, w_z = p_axis >= 2u ? 1.0f : 0.0f;

        int stx = 0, sty = 0;  // entry 0 = (0, 0): the end marker
        uint32_t sp = 1, sp_max = 0;
        uint32_t gx = 0u, gy = 0x80000000u;  // the root group
        for (;;) {
        do {
            const uint32_t lz = (uint32_t)__builtin_clz(gy);
            const uint32_t hits = gy;
            gy &= ~(0x80000000u >> lz);
            if (gy > 0x00ffffffu) {  // remaining siblings
                uint32_t m0_saved;
                asm("s_mov_b32 %2, m0\n\ts_mov_b32 m0, %5\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %4, m0\n\ts_mov_b32 m0, %2"
                    : "+v"(stx), "+v"(sty), "=&s"(m0_saved)
                    : "s"(gx), "s"(gy), "s"(sp));
                sp++;
                sp_max = sp_max > sp ? sp_max : sp;
            }
            const uint32_t slot = (7u - lz) ^ oct;
            const uint32_t node = gx + (uint32_t)__builtin_popcount(hits & ((1u << slot) - 1u));
            const uint32_t* __restrict__ nd = reinterpret_cast<const uint32_t*>(sc.nodes) + (size_t)uniform(node) * 20u;
            if (COUNT) n_nodes++;
            const uint32_t q = reinterpret_cast<const uint8_t*>(nd)[q_off];  // issued ahead of the header's wait
            u32x8 hdr;
            asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hdr) : "s"(nd) : "memory");
            const float px_ = __uint_as_float(hdr[0]), py_ = __uint_as_float(hdr[1]), pz_ = __uint_as_float(hdr[2]);
            const uint32_t w3 = hdr[3], child_base = hdr[4], tri_base = hdr[5], leafmask = hdr[6] & 0xffu;
            const uint32_t imask = w3 >> 24;
            const float ps = __uint_as_float((w3 << s_sh) & 0x7f800000u);
            const float pp = __builtin_fmaf(w_z, pz_, __builtin_fmaf(w_y, py_, w_x * px_));
            const float plane = __builtin_fmaf((float)q, ps, pp);
            const float u = plane - o_ax;
            const float lo = fmin_(u * ia_a, u * ia_b);
            float qm = __builtin_fmaf(__builtin_fabsf(lo), -0x1p-21f, lo - ia_m);
            RT_DPP_MAX(qm, "quad_perm:[1,0,3,2]");
            RT_DPP_MAX(qm, "quad_perm:[2,3,0,1]");
            float gap;
            asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(gap) : "v"(qm));
            const float gap_c = __int_as_float(__builtin_amdgcn_ds_bpermute((int)v_addr, __float_as_int(gap)));
            const uint32_t masks = imask | (leafmask << 8);
            const uint32_t verdict = (uint32_t)__builtin_amdgcn_ballot_w64(gap_c <= 0.0f) & (uint32_t)__builtin_amdgcn_ballot_w64((int)(masks << v_sh) < 0);
            const uint32_t any = verdict >> 8, inner_hits = verdict << 24;
            unsigned long long improved = 0ull;  // wave-uniform: lanes one of whose best hits moved at this node
            for (uint32_t lh = any & leafmask; lh; lh &= lh - 1u) {  // the single triangles of the leaf slots that are entered
                const uint32_t c = (uint32_t)__builtin_ctz(lh);
                const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ((1u << c) - 1u));
                const float* __restrict__ tp = reinterpret_cast<const float*>(sc.tris) + (size_t)li * 12u;  // wave-uniform address
                if (COUNT) n_tris++;
                const v3 v0 = mk(tp[0], tp[1], tp[2]), e1 = mk(tp[3], tp[4], tp[5]), e2 = mk(tp[6], tp[7], tp[8]);
                const uint32_t id = __float_as_uint(tp[9]);
#pragma unroll
                for (int r = 0; r < R; r++) {  // one record, every ray index with its own mask and its own way out
                    float det;
                    v3 qvec;
                    const unsigned long long inside = tri_inside_mask(o, d[r], v0, e1, e2, act_mask[r], det, qvec);
                    if (inside == 0ull) continue;
                    const float t = dot(e2, qvec) / det;
                    const unsigned long long closer = __builtin_amdgcn_ballot_w64(t < best[r].t) | (__builtin_amdgcn_ballot_w64(t == best[r].t) & __builtin_amdgcn_ballot_w64(id < best[r].id));
                    const unsigned long long take = inside & __builtin_amdgcn_ballot_w64(t > 0.0f) & closer;
                    improved |= take;
                    const bool mine = __builtin_amdgcn_inverse_ballot_w64(take);
                    best[r].t = mine ? t : best[r].t;
                    best[r].li = mine ? (int)li : best[r].li;
                    best[r].id = mine ? id : best[r].id;
                }
            }
            if (improved != 0ull) {  // the cap: the farthest best hit of the pass's rays
                float far = 0.0f;
#pragma unroll
                for (int r = 0; r < R; r++) far = fmax_(far, __builtin_amdgcn_inverse_ballot_w64(act_mask[r]) ? best[r].t : 0.0f);
                const float maxbest = wave_reduce_nonneg<true>(far);
                if (pk == 7u) ia_m = maxbest;
            }
            gx = child_base;
            gy = inner_hits | imask;
        } while (gy > 0x00ffffffu);
            // no child entered: on with the newest pending group
            sp--;
            gx = (uint32_t)__builtin_amdgcn_readlane(stx, (int)sp);
            gy = (uint32_t)__builtin_amdgcn_readlane(sty, (int)sp);
            if (gy == 0u) break;
        }
        if (sp_max > 63u) overflow = 1;
    }
#pragma unroll
    for (int r = 1; r < R; r++)
        if ((ray_bits >> (4 * r)) & 8u) st.hit[pid0 + 64u * (uint32_t)r] = make_float2(best[r].t, __int_as_float(best[r].li));
    packet_finish<COUNT>(st, stats, pid0, lane, (ray_bits & 8u) != 0u, best[0], n_nodes, n_tris, overflow);  // one walk: counted once
}

// ---- launchers ------------------------------------------------------------------------------------
// (PURE, FARCAP) of pt_trace_packet_ia for a tune_no_packet mode other than PACKET_EXACT, as compile-time constants
template <class F>
static void with_interval_cfg(uint32_t mode, F&& f) {
    if (mode == PACKET_INTERVAL_ONLY) f(std::true_type{}, std::true_type{});
    else if (mode == PACKET_INTERVAL_NOCAP) f(std::false_type{}, std::false_type{});
    else f(std::false_type{}, std::true_type{});
}

int launch_pt_trace_packet(Ctx* c, const PtScene& sc, const PtFrame& f, const PtState& st, unsigned long long* stats, bool count, uint32_t mode) {
    const uint32_t rays_per_lane = mode == PACKET_WIDE_2 ? 2u : mode == PACKET_WIDE_4 ? 4u : 1u;
    const uint32_t per_block = 256u * rays_per_lane;
    const dim3 g((f.n_paths + per_block - 1u) / per_block), b(256);
    with_bool(count, [&](auto cnt) {
        if (mode == PACKET_WIDE_2) {
            hipLaunchKernelGGL((pt_trace_packet_wide<decltype(cnt)::value, 2>), g, b, 0, c->stream, sc, f, st, stats);
        } else if (mode == PACKET_WIDE_4) {
            hipLaunchKernelGGL((pt_trace_packet_wide<decltype(cnt)::value, 4>), g, b, 0, c->stream, sc, f, st, stats);
        } else if (mode == PACKET_EXACT) {
            hipLaunchKernelGGL(pt_trace_packet<decltype(cnt)::value>, g, b, 0, c->stream, sc, f, st, stats);
        } else {
            with_interval_cfg(mode, [&](auto pure, auto farcap) {
                hipLaunchKernelGGL((pt_trace_packet_ia<decltype(cnt)::value, decltype(pure)::value, decltype(farcap)::value>), g, b, 0, c->stream, sc, f, st, stats);
            });
        }
    });
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

}  // namespace rt
