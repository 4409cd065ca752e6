// pt_overlap_query.hip — path B: overlap queries on device arrays (pt_query_overlaps): every triangle of the
// mesh that each caller-supplied triangle intersects, counted and listed with the mask of the edges that pierce.  The refilling loop
// and the group walk of pt_query_loop.h with a box-overlap test, the slice record of pt_slice.h: the arithmetic that decides an answer is tri_overlap.h's, shared with the tests' CPU
// reference.  Nothing of rays, frames, path state, shading, packets or the octant table is used here.
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "pt_slice.h"
#include "tri_overlap.h"

namespace rt {
using namespace rtk;

// ---- overlap queries on device arrays (rt_count_overlaps_device / rt_fill_overlaps_device) ----------------
// The source is the caller's
// triangle, nine coordinates, validity decided when the lane loads them, and its box Q.  The walk's test is closed box overlap:
// a child box or a leaf slot is skipped exactly when its decoded box is disjoint from Q on some axis; since the decoded box contains
// the unpadded box B of every triangle below it (section 6.14's lo <= c <= hi, vertices included), a skipped subtree holds only
// triangles with cand false, which the definition refuses: the list is the tree-free one.  Q is fixed for the whole walk, so the
// order of the walk changes nothing - every box that overlaps is entered, every triangle in one is tested exactly once - and the
// passing inner children of a node are ONE group (child base + mask), node_step's protocol: the stack holds at most one group per
// level below the root, depth - 1 <= mesh.stack_need entries, as for the neighbours (section 6.17 has the proof).

template <bool COUNT, bool FILL>
struct OverlapLane {
    const PtScene& sc;
    const OverlapQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    ListSlice sl{};
    QueryTri A{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}};
    Box Q = query_box(A);
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t item = 0;  // index of this lane's query triangle

    __device__ __forceinline__ void retire() {  // the slice is already in its final order
        sl.close<FILL>();
        if (!FILL) write_count(q.count_out, q.count64, item, (int)sl.found, sl.found);
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float* tp = q.tris + (size_t)i * 9u;
        const QueryTri nt{P3{tp[0], tp[1], tp[2]}, P3{tp[3], tp[4], tp[5]}, P3{tp[6], tp[7], tp[8]}};
        if (!tri_in_reach(nt, q.reach)) {  // not walked (comparisons that are false for a NaN)
            if (!FILL) write_count(q.count_out, q.count64, i, RT_RAY_INVALID, 0ull);
            sl.invalid++;
            return false;
        }
        A = nt;
        Q = query_box(nt);
        G = root_group();
        T = Group{0u, 0u};
        stk.sp = 0;
        sl.found = 0u;
        if (FILL) sl.open(q.offsets, i, q.capacity);
        item = i;
        return true;
    }

    // Node step: both planes of all eight children decoded, eight overlap verdicts against Q (empty slots hold an inverted box that
    // a wide Q overlaps: enter_node masks them)
    __device__ __forceinline__ void node_step() {
        const NodeRec nd = fetch_node<COUNT>(sc.nodes, take_child(G, stk, tc.overflow), tc);
        uint32_t pass = 0;  // bit s: the box in slot s overlaps Q
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float lox = __builtin_fmaf(plane_q(nd.lx, i), nd.sx, nd.ox), hix = __builtin_fmaf(plane_q(nd.hx, i), nd.sx, nd.ox);
            const float loy = __builtin_fmaf(plane_q(nd.ly, i), nd.sy, nd.oy), hiy = __builtin_fmaf(plane_q(nd.hy, i), nd.sy, nd.oy);
            const float loz = __builtin_fmaf(plane_q(nd.lz, i), nd.sz, nd.oz), hiz = __builtin_fmaf(plane_q(nd.hz, i), nd.sz, nd.oz);
            if (box_overlaps(Q, lox, loy, loz, hix, hiy, hiz)) pass |= 1u << i;
        }
        enter_node(nd, pass, G, T);
    }
    // Triangle step: cand on the record's own words, all six segment tests, the triangle kept when mask != 0
    __device__ __forceinline__ void tri_step() {
        const float4* tp = sc.tris + (size_t)take_tri(T) * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        if (COUNT) tc.tris++;
        const P3 v0{a.x, a.y, a.z}, e1{a.w, b.x, b.y}, e2{b.z, b.w, c.x};
        if (!overlap_cand(Q, v0, e1, e2)) return;
        const uint32_t mask = overlap_mask(A, v0, e1, e2);
        if (mask != 0u) {
            if (FILL) insert_pair(q.tri_out + sl.lo, q.key_out + sl.lo, sl.room, sl.found, (int)__float_as_uint(c.y), (int)mask);
            sl.found++;
        }
    }
    __device__ __forceinline__ bool step(bool alive) {
        return group_round(G, T, stk, alive, [&] { node_step(); }, [&] { tri_step(); }, [] { return false; });
    }
};

template <bool COUNT, bool FILL>
__global__ __launch_bounds__(256, kOverlapWaves) void pt_query_overlaps(const PtScene sc, const OverlapQuery q, uint32_t* __restrict__ head,
                                                                        unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    OverlapLane<COUNT, FILL> lane{sc, q, make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_listing_totals<COUNT, FILL>(stats, lane_id, lane.sl, lane.tc);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_overlaps(Ctx* c, const PtScene& sc, const OverlapQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                             const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<OverlapQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(fill, [&](auto fl) { kernel = pt_query_overlaps<decltype(cnt)::value, decltype(fl)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
