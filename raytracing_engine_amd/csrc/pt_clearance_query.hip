// pt_clearance_query.hip — path B: clearance queries on device arrays (pt_query_clearance): how far each
// caller-supplied triangle is from the mesh, which mesh triangle is nearest, and the two nearest points.  The refilling loop and the
// nearest-first walk of pt_query_loop.h with a box-to-box bound: the arithmetic that decides an answer is tri_dist.h's, shared with
// the tests' CPU reference.  Nothing of rays, frames, path state, shading or packets is used here.
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "tri_dist.h"

namespace rt {
using namespace rtk;

// ---- clearance queries on device arrays (rt_query_clearance_device) --------------------------------------
// The source is the caller's triangle, nine coordinates, validity decided when the lane loads them, and its padded box Qp.  The
// bound is box_lb2's: the gap between Qp and the child's decoded box; section 6.22 shows lb2 <= d2 in fp32 for every candidate pair
// of every triangle below, so a walk returns the tree-free answer whatever its order.
__device__ __forceinline__ void write_p3(float* out, uint32_t i, P3 p) {
    if (!out) return;
    float* po = out + (size_t)i * 3u;
    po[0] = p.x;
    po[1] = p.y;
    po[2] = p.z;
}

template <bool COUNT>
struct ClearanceLane {
    const PtScene& sc;
    const ClearanceQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    QueryTri A{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}};
    Box Qp = query_box(A);
    Nearest best{0.0f, 0xffffffffu, -1};
    uint32_t cur = kNoNode;  // the node this lane visits next; kNoNode: pop one
    uint32_t item = 0;       // index of this lane's query triangle
    float limit2 = 0.0f;     // its bound on d2
    uint32_t invalid = 0;    // invalid triangles this lane has met

    __device__ __forceinline__ void retire() {
        const float nan = __builtin_nanf("");
        const bool hit = best.li >= 0 && best.d2 < limit2;
        q.dist_out[item] = hit ? sqrt_cr(best.d2) : __builtin_inff();
        q.tri_out[item] = hit ? (int)best.id : RT_POINT_MISS;
        if (q.point_query_out || q.point_mesh_out) {
            P3 pq{nan, nan, nan}, pm{nan, nan, nan};
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
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float nan = __builtin_nanf("");
        const float* tp = q.tris + (size_t)i * 9u;
        const QueryTri nt{P3{tp[0], tp[1], tp[2]}, P3{tp[3], tp[4], tp[5]}, P3{tp[6], tp[7], tp[8]}};
        const float rmax = q.rmax ? q.rmax[i] : __builtin_inff();
        const float l2 = point_limit2(rmax);
        if (!(tri_in_reach(nt, q.reach) && rmax == rmax)) {  // not answered (comparisons that are false for a NaN)
            q.dist_out[i] = nan;
            q.tri_out[i] = RT_RAY_INVALID;
            invalid++;
        } else if (!(rmax > 0.0f) || !(l2 > 0.0f)) {  // nothing has d2 < limit2: a miss without a walk
            q.dist_out[i] = __builtin_inff();
            q.tri_out[i] = RT_POINT_MISS;
        } else {
            A = nt;
            Qp = padded_query_box(nt);
            limit2 = l2;
            best = Nearest{l2, 0xffffffffu, -1};  // boxes beyond the limit are culled from the start
            cur = 0u;
            stk.sp = 0;
            item = i;
            return true;
        }
        write_p3(q.point_query_out, i, P3{nan, nan, nan});
        write_p3(q.point_mesh_out, i, P3{nan, nan, nan});
        return false;
    }

    // Visit node `cur`: eight box-to-box bounds, eight verdicts against best.d2.  Leaf slots that pass are tested at once (the 48-byte
    // record, then tri_dist), so that they can shrink best.d2 before the inner children are judged (descend_nearest).
    __device__ __forceinline__ void visit() {
        const NodeRec nd = fetch_node<COUNT>(sc.nodes, cur, tc);
        float lb[8], lmin;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float gx = axis_box_gap(Qp.lo[0], Qp.hi[0], nd.ox, nd.sx, plane_q(nd.lx, i), plane_q(nd.hx, i));
            const float gy = axis_box_gap(Qp.lo[1], Qp.hi[1], nd.oy, nd.sy, plane_q(nd.ly, i), plane_q(nd.hy, i));
            const float gz = axis_box_gap(Qp.lo[2], Qp.hi[2], nd.oz, nd.sz, plane_q(nd.lz, i), plane_q(nd.hz, i));
            lb[i] = gap_lb2(gx, gy, gz);
        }
        uint32_t leaves = within_bound(lb, best.d2) & nd.leafmask;
        if (leaves) {
            const Box Q = query_box(A);  // re-derived: twelve min / max against six registers held through the walk
#pragma unroll 1
            while (leaves) {
                const uint32_t li = nd.leaf_tri((uint32_t)__builtin_ctz(leaves));
                leaves &= leaves - 1u;
                if (COUNT) tc.tris++;
                const float4* tp = sc.tris + (size_t)li * 3;
                const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
                const uint32_t id = __float_as_uint(tcw.y);
                const TriDist td = tri_dist(A, Q, P3{ta.x, ta.y, ta.z}, P3{ta.w, tb.x, tb.y}, P3{tb.z, tb.w, tcw.x});
                if (nearer(td.d2, id, best.d2, best.id)) best = Nearest{td.d2, id, (int)li};
            }
        }
        cur = descend_nearest(nd, lb, best.d2, lmin, stk, tc.overflow);
    }
    __device__ __forceinline__ bool step(bool alive) {
        if (alive) {
            if (cur == kNoNode) cur = pop_within(stk, best.d2);
            if (cur != kNoNode) visit();
            else alive = false;
        }
        return alive;
    }
};

template <bool COUNT>
__global__ __launch_bounds__(256, kClearanceWaves) void pt_query_clearance(const PtScene sc, const ClearanceQuery q, uint32_t* __restrict__ head,
                                                                           unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    ClearanceLane<COUNT> lane{sc, q, make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_wave_total(&stats[CQ_STAT_INVALID], lane.invalid, lane_id);
    if (COUNT) {
        add_wave_total(&stats[CQ_STAT_NODES], lane.tc.nodes, lane_id);
        add_wave_total(&stats[CQ_STAT_TRIS], lane.tc.tris, lane_id);
    }
    if (lane.tc.overflow) atomicOr((unsigned int*)&stats[CQ_STAT_OVERFLOW], 1u);
}

// ---- launcher -------------------------------------------------------------------------------------
int launch_pt_query_clearance(Ctx* c, const PtScene& sc, const ClearanceQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<ClearanceQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_clearance<decltype(cnt)::value>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
