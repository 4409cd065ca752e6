// pt_neighbor_query.hip — path B: neighbour queries on device arrays (pt_query_neighbors): every triangle
// within a radius of each caller-supplied point, counted and listed.  The refilling loop and the group walk of pt_query_loop.h with a
// fixed-radius test, the slice record of pt_slice.h: the
// arithmetic that decides an answer is point_tri.h's, shared with the tests' CPU reference.  Nothing of rays, frames, path state,
// shading, packets or the octant table is used here.
#include "point_tri.h"
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "pt_slice.h"

namespace rt {
using namespace rtk;

// ---- neighbour queries on device arrays (rt_count_neighbors_device / rt_fill_neighbors_device) ----------
// The source is the closest-point queries': the caller's point and radius, validity decided when the lane loads them.  The bound is
// a distance bound like theirs (point_child_lb2), but it is FIXED: limit2 = rmax * rmax from
// the first box to the last, and everything below it is kept.  A child box or a leaf slot is skipped exactly when lb2 >= limit2;
// since lb2 <= d2 holds in fp32 for every triangle under the box (section 6.14), a skipped subtree holds only triangles with
// d2 >= limit2, which the strict test d2 < limit2 refuses: the list is the tree-free one.  With a fixed bound the order of the walk
// changes nothing - every box below the bound is entered, every triangle in one is tested exactly once - so there is no nearest-
// first ordering and no (node, lb2) entry: the passing inner children of a node are ONE group (child base + mask), as in the ray
// walks, and node_step's protocol holds: a node visit takes one child out of the current group and pushes what is left of it, so
// the stack holds at most one group per level below the root, depth - 1 <= mesh.stack_need entries (section 6.17 has the proof).
constexpr int kNeighborWaves = 8;

template <bool COUNT, bool FILL>
struct NeighborLane {
    const PtScene& sc;
    const NeighborQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    ListSlice sl{};
    P3 p{0.0f, 0.0f, 0.0f};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t point = 0;   // index of this lane's point
    float limit2 = 0.0f;  // its bound on d2, fixed for the whole walk

    __device__ __forceinline__ void retire() {
        const uint32_t kept = sl.close<FILL>();
        if (FILL) {
            float* ds = q.key_out + sl.lo;
#pragma unroll 1
            for (uint32_t j = 0; j < kept; j++) ds[j] = sqrt_cr(ds[j]);  // d2 -> dist in place: the lane's own stores, program order
        } else {
            write_count(q.count_out, q.count64, point, (int)sl.found, sl.found);
        }
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float* pp = q.points + (size_t)i * 3u;
        const P3 np{pp[0], pp[1], pp[2]};
        const float rmax = q.rmax ? q.rmax[i] : q.rmax_all;
        const float l2 = point_limit2(rmax);
        if (!(point_in_reach(np, q.reach) && rmax == rmax)) {  // not walked (comparisons that are false for a NaN)
            if (!FILL) write_count(q.count_out, q.count64, i, RT_POINT_INVALID, 0ull);
            sl.invalid++;
            return false;
        }
        if (!(rmax > 0.0f) || !(l2 > 0.0f)) {  // nothing has d2 < limit2: no neighbour, without a walk
            if (!FILL) write_count(q.count_out, q.count64, i, 0, 0ull);
            return false;
        }
        p = np;
        limit2 = l2;
        G = root_group();
        T = Group{0u, 0u};
        stk.sp = 0;
        sl.found = 0u;
        if (FILL) sl.open(q.offsets, i, q.capacity);
        point = i;
        return true;
    }

    // Node step: eight lower bounds, eight verdicts against limit2.  !(lb >= limit2): a NaN bound is entered, not skipped.
    __device__ __forceinline__ void node_step() {
        const NodeRec nd = fetch_node<COUNT>(sc.nodes, take_child(G, stk, tc.overflow), tc);
        float lb[8];
        point_child_lb2(nd, p, lb);
        uint32_t pass = 0;  // bit s: the box in slot s reaches below the limit
#pragma unroll
        for (int i = 0; i < 8; i++) pass |= !(lb[i] >= limit2) ? 1u << i : 0u;
        enter_node(nd, pass, G, T);
    }
    // Triangle step: closest_on_tri on the record's own words, the triangle kept when d2 < limit2
    __device__ __forceinline__ void tri_step() {
        const float4* tp = sc.tris + (size_t)take_tri(T) * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        if (COUNT) tc.tris++;
        const float d2 = closest_on_tri(p, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x}).d2;
        if (d2 < limit2) {
            if (FILL) insert_hit(q.key_out + sl.lo, q.tri_out + sl.lo, sl.room, sl.found, d2, (int)__float_as_uint(c.y));  // keyed by d2 until the sink
            sl.found++;
        }
    }
    __device__ __forceinline__ bool step(bool alive) {
        return group_round(G, T, stk, alive, [&] { node_step(); }, [&] { tri_step(); }, [] { return false; });
    }
};

template <bool COUNT, bool FILL>
__global__ __launch_bounds__(256, kNeighborWaves) void pt_query_neighbors(const PtScene sc, const NeighborQuery q, uint32_t* __restrict__ head,
                                                                          unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    NeighborLane<COUNT, FILL> lane{sc, q, make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_listing_totals<COUNT, FILL>(stats, lane_id, lane.sl, lane.tc);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_neighbors(Ctx* c, const PtScene& sc, const NeighborQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<NeighborQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(fill, [&](auto fl) { kernel = pt_query_neighbors<decltype(cnt)::value, decltype(fl)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
