// pt_clearance_query.hip — path B: clearance queries on device arrays (pt_query_clearance): how far each
// caller-supplied triangle is from the mesh, which mesh triangle is nearest, and the two nearest points.  The refilling loop of
// pt_query_points (pt_point_query.hip) over pt_queue.h's streams around the same nearest-first walk of the BVH8 with a box-to-box
// bound: of pt_traverse.h only the stack and ubyte_f32 are used, the arithmetic that decides an answer is tri_dist.h's, shared with
// the tests' CPU reference.  Nothing of rays, frames, path state, shading or packets is used here.
#include "pt_launch.h"
#include "pt_queue.h"
#include "tri_dist.h"

namespace rt {
using namespace rtk;

// ---- clearance queries on device arrays (rt_query_clearance_device) --------------------------------------
// pt_query_points' loop - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and no
// live lane" - with a source of its own: the caller's triangle, nine coordinates, validity decided when the lane loads them, and its
// padded box Qp.  The walk is the points': (node index, lb2 bits) entries, one pending sibling each, a popped entry whose bound the
// best d2 has passed is dropped unfetched, at most point_stack_need entries.  The bound is box_lb2's: the gap between Qp and the
// child's decoded box; section 6.22 shows lb2 <= d2 in fp32 for every candidate pair of every triangle below, so a walk returns the
// tree-free answer whatever its order.
constexpr uint32_t kNoClearanceNode = 0xffffffffu;

struct NearestPair {
    float d2;
    uint32_t id;  // original triangle index (tie-break)
    int li;       // leaf-order triangle index, -1 = none
};

// Visit node `cur`: point_node_step's five fetches and decode, eight box-to-box bounds, eight verdicts against best.d2.  Leaf slots
// that pass are tested at once (the 48-byte record, then tri_dist), so that they can shrink best.d2 before the inner children are
// judged; of the inner children that still pass, the nearest becomes `cur` and the others are pushed.
template <bool COUNT>
__device__ __forceinline__ void clearance_node_step(const PtScene& sc, const QueryTri& A, const Box& Qp, uint32_t& cur, NearestPair& best, TravStack& stk,
                                                    TravCounters& tc) {
    const float4* nd = sc.nodes + (size_t)cur * 5;
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3], n4 = nd[4];
    if (COUNT) tc.nodes++;
    const uint32_t w3 = __float_as_uint(n0.w);
    const float sx = __uint_as_float((w3 & 0xffu) << 23), sy = __uint_as_float(((w3 >> 8) & 0xffu) << 23), sz = __uint_as_float(((w3 >> 16) & 0xffu) << 23);
    const uint32_t imask = w3 >> 24, leafmask = __float_as_uint(n1.z) & 0xffu;
    const uint32_t child_base = __float_as_uint(n1.x), tri_base = __float_as_uint(n1.y);
    const uint32_t lx[2] = {__float_as_uint(n2.x), __float_as_uint(n2.y)}, ly[2] = {__float_as_uint(n2.z), __float_as_uint(n2.w)};
    const uint32_t lz[2] = {__float_as_uint(n3.x), __float_as_uint(n3.y)}, hx[2] = {__float_as_uint(n3.z), __float_as_uint(n3.w)};
    const uint32_t hy[2] = {__float_as_uint(n4.x), __float_as_uint(n4.y)}, hz[2] = {__float_as_uint(n4.z), __float_as_uint(n4.w)};
    float lb[8];
    uint32_t pass = 0;  // bit s: the box in slot s is not farther than the best triangle (empty slots: masked below)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int w = i >> 2, b = i & 3;
        const float gx = axis_box_gap(Qp.lo[0], Qp.hi[0], n0.x, sx, ubyte_f32(lx[w], b), ubyte_f32(hx[w], b));
        const float gy = axis_box_gap(Qp.lo[1], Qp.hi[1], n0.y, sy, ubyte_f32(ly[w], b), ubyte_f32(hy[w], b));
        const float gz = axis_box_gap(Qp.lo[2], Qp.hi[2], n0.z, sz, ubyte_f32(lz[w], b), ubyte_f32(hz[w], b));
        lb[i] = gap_lb2(gx, gy, gz);
        if (!(lb[i] > best.d2)) pass |= 1u << i;
    }
    uint32_t leaves = pass & leafmask;
    if (leaves) {
        const Box Q = query_box(A);  // re-derived: twelve min / max against six registers held through the walk
#pragma unroll 1
        while (leaves) {
            const uint32_t s = (uint32_t)__builtin_ctz(leaves);
            leaves &= leaves - 1u;
            const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ~(0xffffffffu << s));
            if (COUNT) tc.tris++;
            const float4* tp = sc.tris + (size_t)li * 3;
            const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
            const uint32_t id = __float_as_uint(tcw.y);
            const TriDist td = tri_dist(A, Q, P3{ta.x, ta.y, ta.z}, P3{ta.w, tb.x, tb.y}, P3{tb.z, tb.w, tcw.x});
            if (nearer(td.d2, id, best.d2, best.id)) best = NearestPair{td.d2, id, (int)li};
        }
    }
    uint32_t go = 0, smin = 0;  // inner children still to be entered, the nearest of them
    float lmin = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((imask >> i) & 1u) && !(lb[i] > best.d2)) {
            if (go == 0u || lb[i] < lmin) {
                lmin = lb[i];
                smin = (uint32_t)i;
            }
            go |= 1u << i;
        }
    }
    if (go == 0u) {
        cur = kNoClearanceNode;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((go >> i) & 1u) && (uint32_t)i != smin)
            stk.push(Group{child_base + (uint32_t)__builtin_popcount(imask & ((1u << i) - 1u)), __float_as_uint(lb[i])}, tc.overflow);
    }
    cur = child_base + (uint32_t)__builtin_popcount(imask & ~(0xffffffffu << smin));
}

__device__ __forceinline__ void write_p3(float* out, uint32_t i, P3 p) {
    if (!out) return;
    float* po = out + (size_t)i * 3u;
    po[0] = p.x;
    po[1] = p.y;
    po[2] = p.z;
}

template <bool COUNT>
__global__ __launch_bounds__(256, kClearanceWaves) void pt_query_clearance(const PtScene sc, const ClearanceQuery q, uint32_t* __restrict__ head,
                                                                           unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    QueryTri A{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}};
    Box Qp = query_box(A);
    NearestPair best{0.0f, 0xffffffffu, -1};
    uint32_t cur = kNoClearanceNode;  // the node this lane visits next; kNoClearanceNode: pop one
    uint32_t item = 0;                // index of this lane's query triangle
    float limit2 = 0.0f;              // its bound on d2
    uint32_t invalid = 0;             // invalid triangles this lane has met
    bool has_item = false, alive = false;
    QueueCursor qc{q.n, head, home_stream(), 0u};
    bool exhausted = qc.n == 0u;  // every stream has been found dry
    const float nan = __builtin_nanf("");
    const P3 nan3{nan, nan, nan};

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_item) {  // the sink
                const bool hit = best.li >= 0 && best.d2 < limit2;
                q.dist_out[item] = hit ? sqrt_cr(best.d2) : __builtin_inff();
                q.tri_out[item] = hit ? (int)best.id : RT_POINT_MISS;
                if (q.point_query_out || q.point_mesh_out) {
                    P3 pq = nan3, pm = nan3;
                    if (hit) {  // the pair once more from the record: the same function on the same words, the same bits
                        const float4* tp = sc.tris + (size_t)best.li * 3;
                        const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
                        const P3 v0{ta.x, ta.y, ta.z}, e1{ta.w, tb.x, tb.y}, e2{tb.z, tb.w, tcw.x};
                        const Box Q = query_box(A);
                        const TriDist td = tri_dist(A, Q, v0, e1, e2);
                        tri_dist_points(A, v0, e1, e2, td, pq, pm);
                    }
                    write_p3(q.point_query_out, item, pq);
                    write_p3(q.point_mesh_out, item, pm);
                }
                has_item = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = qc.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(qc.stream, base + (uint32_t)__popcll(idle & lt_mask)) : qc.n;  // >= n: nothing for this lane
                if (!alive && i < qc.n) {  // the source
                    const float* tp = q.tris + (size_t)i * 9u;
                    const QueryTri nt{P3{tp[0], tp[1], tp[2]}, P3{tp[3], tp[4], tp[5]}, P3{tp[6], tp[7], tp[8]}};
                    const float rmax = q.rmax ? q.rmax[i] : __builtin_inff();
                    const float l2 = point_limit2(rmax);
                    bool miss = false;
                    if (!(tri_in_reach(nt, q.reach) && rmax == rmax)) {  // not answered (comparisons that are false for a NaN)
                        q.dist_out[i] = nan;
                        q.tri_out[i] = RT_RAY_INVALID;
                        invalid++;
                        miss = true;
                    } else if (!(rmax > 0.0f) || !(l2 > 0.0f)) {  // nothing has d2 < limit2: a miss without a walk
                        q.dist_out[i] = __builtin_inff();
                        q.tri_out[i] = RT_POINT_MISS;
                        miss = true;
                    } else {
                        A = nt;
                        Qp = padded_query_box(nt);
                        limit2 = l2;
                        best = NearestPair{l2, 0xffffffffu, -1};  // boxes beyond the limit are culled from the start
                        cur = 0u;
                        stk.sp = 0;
                        item = i;
                        has_item = true;
                        alive = true;
                    }
                    if (miss) {
                        write_p3(q.point_query_out, i, nan3);
                        write_p3(q.point_mesh_out, i, nan3);
                    }
                }
                exhausted = qc.advance_if_dry(base + want);
            }
            if (__ballot(alive) == 0ull && exhausted) break;  // every answer of this wave is written (idle lanes retired above)
        }
        if (alive) {
            if (cur == kNoClearanceNode) {  // the nearest pending sibling that the best d2 has not passed
#pragma unroll 1
                while (stk.sp) {
                    const Group e = stk.pop();
                    if (!(__uint_as_float(e.y) > best.d2)) {
                        cur = e.x;
                        break;
                    }
                }
            }
            if (cur != kNoClearanceNode) clearance_node_step<COUNT>(sc, A, Qp, cur, best, stk, tc);
            else alive = false;
        }
    }
    add_wave_total(&stats[CQ_STAT_INVALID], invalid, lane);
    if (COUNT) {
        add_wave_total(&stats[CQ_STAT_NODES], tc.nodes, lane);
        add_wave_total(&stats[CQ_STAT_TRIS], tc.tris, lane);
    }
    if (tc.overflow) atomicOr((unsigned int*)&stats[CQ_STAT_OVERFLOW], 1u);
}

// ---- launcher -------------------------------------------------------------------------------------
int launch_pt_query_clearance(Ctx* c, const PtScene& sc, const ClearanceQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<ClearanceQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_clearance<decltype(cnt)::value>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
