// pt_sweep_query.hip — path B: sphere-cast queries on device arrays (pt_query_sweeps): how far a sphere of
// radius r that starts at o gets along d before it touches the mesh, which triangle it touches first, and where.  The refilling loop
// and the nearest-first walk of pt_query_loop.h with a time as the bound: the arithmetic that decides an answer is sweep_tri.h's,
// shared with the tests' CPU reference.  Nothing of rays, frames, path state, shading or packets is used here.
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "sweep_tri.h"

namespace rt {
using namespace rtk;

// ---- sphere-cast queries on device arrays (rt_query_sweeps_device) ----------------------------------------
// The source is the caller's (o, d, r, tmax), validity decided when the lane loads them.  The bound of a child is the time at which
// the path enters the child's decoded box inflated by R (axis_slab, slab_bound of sweep_tri.h); section 6.24 shows bound <= toi in
// fp32 for every triangle under the box, so a walk returns the tree-free answer whatever its order.  Nearest::d2 holds the best t; it
// starts at min(tmax, FLT_MAX), so a box the path misses (bound +inf) is never within it.
template <bool COUNT>
struct SweepLane {
    const PtScene& sc;
    const SweepQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    Sweep s{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, 0.0f};
    SweepSlabs sl{P3{0.0f, 0.0f, 0.0f}, 0.0f};
    Nearest best{0.0f, 0xffffffffu, -1};
    uint32_t cur = kNoNode;          // the node this lane visits next; kNoNode: pop one
    uint32_t item = 0;               // index of this lane's item
    uint32_t invalid = 0, hits = 0;  // what this lane has met

    __device__ __forceinline__ void write_point(uint32_t i, P3 p) {
        if (!q.point_out) return;
        float* po = q.point_out + (size_t)i * 3u;
        po[0] = p.x;
        po[1] = p.y;
        po[2] = p.z;
    }

    __device__ __forceinline__ void retire() {
        const float nan = __builtin_nanf("");
        const float tmax = q.tmax ? q.tmax[item] : __builtin_inff();  // read again: a register less through the walk
        const bool hit = best.li >= 0 && best.d2 < tmax;
        q.t_out[item] = hit ? best.d2 : __builtin_inff();
        q.tri_out[item] = hit ? (int)best.id : RT_RAY_MISS;
        hits += hit ? 1u : 0u;
        if (q.point_out) {
            P3 c{nan, nan, nan};
            if (hit) {  // the contact point from the record: the centre at the answered time against the answered triangle
                const float4* tp = sc.tris + (size_t)best.li * 3;
                const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
                const P3 v0{ta.x, ta.y, ta.z}, e1{ta.w, tb.x, tb.y}, e2{tb.z, tb.w, tcw.x};
                const ClosestTri ct = closest_on_tri(sweep_centre(s.o, s.d, best.d2), v0, e1, e2);
                c = tri_point(v0, e1, e2, ct.u, ct.v);
            }
            write_point(item, c);
        }
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float nan = __builtin_nanf("");
        const float *po = q.origins + (size_t)i * 3u, *pd = q.dirs + (size_t)i * 3u;
        const Sweep ns{P3{po[0], po[1], po[2]}, P3{pd[0], pd[1], pd[2]}, q.radius[i]};
        const float tmax = q.tmax ? q.tmax[i] : __builtin_inff();
        if (!sweep_valid(ns, tmax, q.reach)) {  // not answered (comparisons that are false for a NaN)
            q.t_out[i] = nan;
            q.tri_out[i] = RT_RAY_INVALID;
            invalid++;
        } else if (!(tmax > 0.0f)) {  // nothing has toi < tmax: a miss without a walk
            q.t_out[i] = __builtin_inff();
            q.tri_out[i] = RT_RAY_MISS;
        } else {
            s = ns;
            sl = sweep_slabs(ns, q.reach);
            best = Nearest{sweep_start_bound(tmax), 0xffffffffu, -1};  // boxes beyond the limit are culled from the start
            cur = 0u;
            stk.sp = 0;
            item = i;
            return true;
        }
        write_point(i, P3{nan, nan, nan});
        return false;
    }

    // Visit node `cur`: eight entry times, eight verdicts against best t.  Leaf slots that pass are tested at once (the 48-byte record,
    // then sweep_toi with the best t as its cut), so that they can shrink best t before the inner children are judged (descend_nearest).
    __device__ __forceinline__ void visit() {
        const NodeRec nd = fetch_node<COUNT>(sc.nodes, cur, tc);
        float lb[8], lmin;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            float tn = -__builtin_inff(), tf = __builtin_inff();
            axis_slab(s.o.x, sl.inv.x, sl.R, nd.ox, nd.sx, plane_q(nd.lx, i), plane_q(nd.hx, i), tn, tf);
            axis_slab(s.o.y, sl.inv.y, sl.R, nd.oy, nd.sy, plane_q(nd.ly, i), plane_q(nd.hy, i), tn, tf);
            axis_slab(s.o.z, sl.inv.z, sl.R, nd.oz, nd.sz, plane_q(nd.lz, i), plane_q(nd.hz, i), tn, tf);
            lb[i] = slab_bound(tn, tf);
        }
        uint32_t leaves = within_bound(lb, best.d2) & nd.leafmask;
#pragma unroll 1
        while (leaves) {
            const uint32_t li = nd.leaf_tri((uint32_t)__builtin_ctz(leaves));
            leaves &= leaves - 1u;
            if (COUNT) tc.tris++;
            const float4* tp = sc.tris + (size_t)li * 3;
            const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
            const uint32_t id = __float_as_uint(tcw.y);
            const SweepToi toi = sweep_toi(s, P3{ta.x, ta.y, ta.z}, P3{ta.w, tb.x, tb.y}, P3{tb.z, tb.w, tcw.x}, best.d2);
            if (toi.hit && nearer(toi.t, id, best.d2, best.id)) best = Nearest{toi.t, id, (int)li};
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
__global__ __launch_bounds__(256, kSweepWaves) void pt_query_sweeps(const PtScene sc, const SweepQuery q, uint32_t* __restrict__ head,
                                                                    unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    SweepLane<COUNT> lane{sc, q, make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_wave_total(&stats[WQ_STAT_INVALID], lane.invalid, lane_id);
    add_wave_total(&stats[WQ_STAT_HITS], lane.hits, lane_id);
    if (COUNT) {
        add_wave_total(&stats[WQ_STAT_NODES], lane.tc.nodes, lane_id);
        add_wave_total(&stats[WQ_STAT_TRIS], lane.tc.tris, lane_id);
    }
    if (lane.tc.overflow) atomicOr((unsigned int*)&stats[WQ_STAT_OVERFLOW], 1u);
}

// ---- launcher -------------------------------------------------------------------------------------
int launch_pt_query_sweeps(Ctx* c, const PtScene& sc, const SweepQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                           uint32_t refill_min) {
    QueryKernel<SweepQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_sweeps<decltype(cnt)::value>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
