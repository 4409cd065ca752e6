// pt_side_query.hip — path B: inside/outside queries on device arrays (pt_query_sides).  The refilling loop
// and the group walk of pt_query_loop.h around crossing-counting ray walks: node_step of pt_traverse.h in its unordered form with
// tmax = +inf throughout, and ray_parity.h's triangle test, directions and majority rule, shared with the tests' CPU reference.
// Nothing of frames, path state, shading, packets or the octant table is used here.
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "ray_parity.h"

namespace rt {
using namespace rtk;

// ---- inside/outside queries on device arrays (rt_query_sides_device) ---------------------------------
// Up to three walks per point.  A crossing walk is a closest-hit walk that never learns anything: no hit shrinks tmax, so every box
// the ray passes through is entered and every triangle in it is tested, in any order (UNORDERED: children in slot order, no octant
// table, no LDS beside the stacks).  What a lane keeps between rounds is its point, the direction index k, the count of the walk
// under way and the parities of the walks that are over; when a walk ends the lane starts the next direction in the same round,
// without waiting for a refill, and goes idle when ray_parity.h's rule is decided.
constexpr int kSideWaves = 8;

template <bool COUNT, bool CROSSINGS>
struct SideLane {
    const PtScene& sc;
    const SideQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    TRay r{};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t point = 0;      // index of this lane's point
    uint32_t k = 0;          // the direction under way
    uint32_t crossings = 0;  // of the walk under way
    uint32_t pars = 0;       // bit j: parity of the finished walk j
    uint32_t invalid = 0, skipped = 0, walks = 0, third = 0;  // what this lane has met

    // Put direction k of point p into the lane: at the root with an empty stack, no crossing yet
    __device__ __forceinline__ void start_walk(P3 p) {
        const ParityDir pd = parity_dir(k);
        r.o = mk(p.x, p.y, p.z);
        r.d = mk(pd.d.x, pd.d.y, pd.d.z);
        r.inv = mk(pd.inv.x, pd.inv.y, pd.inv.z);
        r.noi = mk(-(p.x * pd.inv.x), -(p.y * pd.inv.y), -(p.z * pd.inv.z));
        r.tmax = __builtin_inff();
        r.oct_inv = pd.oct_inv;
        G = root_group();
        T = Group{0u, 0u};
        stk.sp = 0;
        crossings = 0u;
    }

    __device__ __forceinline__ void retire() {
        const uint32_t in = side_of_parities(pars, pars >> 1, pars >> 2);
        if (q.inside_out) q.inside_out[point] = (int)in;
        if (q.dist_inout && in) q.dist_inout[point] = -q.dist_inout[point];  // inside ? -dist : dist
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float dist = q.dist_inout ? q.dist_inout[i] : 0.0f;
        const float* pp = q.points + (size_t)i * 3u;
        const P3 np{pp[0], pp[1], pp[2]};
        if (dist == __builtin_inff()) {  // beyond the caller's band: not walked, the entry stays +inf
            if (q.inside_out) q.inside_out[i] = RT_POINT_MISS;
            skipped++;
            return false;
        }
        if (!(dist == dist && point_in_reach(np, q.reach))) {  // not answered (comparisons that are false for a NaN)
            if (q.inside_out) q.inside_out[i] = RT_POINT_INVALID;
            invalid++;
            return false;
        }
        k = 0u;
        pars = 0u;
        start_walk(np);
        walks++;
        point = i;
        return true;
    }

    // Walk k is over: its parity, and whether the lane starts the next direction
    __device__ __forceinline__ bool walk_over() {
        if (CROSSINGS) q.crossings_out[(size_t)point * 3u + k] = (int)crossings;
        pars |= (crossings & 1u) << k;
        bool more = k == 0u;
        if (k == 1u) {
            const bool disagree = needs_third_parity(pars, pars >> 1);
            third += disagree ? 1u : 0u;
            more = CROSSINGS || disagree;
        }
        if (more) {
            k++;
            start_walk(P3{r.o.x, r.o.y, r.o.z});
            walks++;
        }
        return more;
    }

    // The triangle phase: the record of the next pending leaf slot, a crossing in front of the origin counted
    __device__ __forceinline__ void cross_step() {
        const float4* tp = sc.tris + (size_t)take_tri(T) * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        if (COUNT) tc.tris++;
        if (ray_crosses(P3{r.o.x, r.o.y, r.o.z}, P3{r.d.x, r.d.y, r.d.z}, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x})) crossings++;
    }

    __device__ __forceinline__ bool step(bool alive) {
        return group_round(
            G, T, stk, alive, [&] { node_step<COUNT, /*UNORDERED*/ true>(sc.nodes, nullptr, r, G, T, stk, tc); }, [&] { cross_step(); }, [&] { return walk_over(); });
    }
};

template <bool COUNT, bool CROSSINGS>
__global__ __launch_bounds__(256, kSideWaves) void pt_query_sides(const PtScene sc, const SideQuery q, uint32_t* __restrict__ head,
                                                                  unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    SideLane<COUNT, CROSSINGS> lane{sc, q, make_trav_stack(lds_stack, sk)};
    lane.start_walk(P3{0.0f, 0.0f, 0.0f});  // (defined values; no lane walks before it is given a point)
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_wave_total(&stats[SQ_STAT_INVALID], lane.invalid, lane_id);
    add_wave_total(&stats[SQ_STAT_SKIPPED], lane.skipped, lane_id);
    add_wave_total(&stats[SQ_STAT_WALKS], lane.walks, lane_id);
    add_wave_total(&stats[SQ_STAT_THIRD], lane.third, lane_id);
    if (COUNT) {
        add_wave_total(&stats[SQ_STAT_NODES], lane.tc.nodes, lane_id);
        add_wave_total(&stats[SQ_STAT_TRIS], lane.tc.tris, lane_id);
    }
    if (lane.tc.overflow) atomicOr((unsigned int*)&stats[SQ_STAT_OVERFLOW], 1u);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_sides(Ctx* c, const PtScene& sc, const SideQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                          const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<SideQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(q.crossings_out != nullptr, [&](auto all) { kernel = pt_query_sides<decltype(cnt)::value, decltype(all)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
