// pt_knn_query.hip — path B: k-nearest queries on device arrays (pt_query_knn): the k triangles nearest to
// each caller-supplied point, sorted, in a rectangular n x k output.  The refilling loop and the nearest-first walk of
// pt_query_loop.h, with the sorted slice of the listing queries (insert_hit, pt_slice.h) as the lane's candidate list: the arithmetic
// that decides an answer is point_tri.h's, shared with the tests' CPU reference.  Nothing of rays, frames, path state, shading or
// packets is used here.
#include "point_tri.h"
#include "pt_launch.h"
#include "pt_query_loop.h"
#include "pt_slice.h"

namespace rt {
using namespace rtk;

// ---- k-nearest queries on device arrays (rt_query_knn_device) ---------------------------------------------
// The closest-point queries' source and walk ; what differs is what a lane holds.  Its list is its own output row: k
// entries of dist_out / tri_out from i * k on, kept sorted by (d2, original index) with insert_hit (room = k) and keyed by d2 until
// the sink turns the keys into distances, pads the row and writes the count.  A lane reads back only what it stored itself, so
// program order is all the ordering the row needs; no LDS and no register array hold candidates.  Its bound is ONE register:
// limit2 while fewer than k entries are held, then the d2 of the row's last entry, re-read after every accepted insertion and at no
// other time.  A triangle is accepted iff d2 < limit2 and, with k held, (d2, id) lies lexicographically below the last entry; a box
// or a leaf slot is skipped only when lb2 > bound (strictly, and written so that a NaN bound is entered: a tie must reach the index
// comparison).  Since lb2 <= d2 holds in fp32 for every triangle under a box (section 6.14), a skipped subtree holds only triangles
// with d2 > bound: beyond the limit, or strictly behind k held entries, none of which ever leaves the row for a worse one.  The row
// is the first k of the tree-free sorted list on any tree and in any order (section 6.23 has the argument in full).
constexpr int kKnnWaves = 8;

// Entries from..k - 1 of row i: (dist, tri) of a point that is not walked, or the padding behind a short row
__device__ __forceinline__ void knn_fill_row(const KnnQuery& q, uint32_t i, uint32_t from, float dist, int tri) {
    float* ds = q.dist_out + (size_t)i * q.k;
    int* ids = q.tri_out + (size_t)i * q.k;
    // one pair a pass: vectorised, the loop holds its four constants in eight registers from the kernel's entry on, which then spill
#pragma clang loop vectorize(disable) unroll(disable)
    for (uint32_t j = from; j < q.k; j++) {
        ds[j] = dist;
        ids[j] = tri;
    }
}

// What a lane holds of its row beside the row itself is `held` and `bound`.  Where the row lies is formed from the point's index
// where it is needed (one 64-bit multiply-add per pointer): two pointers held through the walk are four registers this kernel does
// not have.
template <bool COUNT>
struct KnnLane {
    const PtScene& sc;
    const KnnQuery& q;
    TravStack stk;
    TravCounters tc{0, 0, 0};
    P3 p{0.0f, 0.0f, 0.0f};
    uint32_t held = 0;       // entries held, <= k
    float bound = 0.0f;      // limit2 while held < k, then the row's last d2
    uint32_t cur = kNoNode;  // the node this lane visits next; kNoNode: pop one
    uint32_t point = 0;      // index of this lane's point
    uint32_t invalid = 0, neighbors = 0;  // what this lane has met

    __device__ __forceinline__ void retire() {
        float* ds = q.dist_out + (size_t)point * q.k;
#pragma unroll 1
        for (uint32_t j = 0; j < held; j++) ds[j] = sqrt_cr(ds[j]);  // d2 -> dist in place: the lane's own stores, program order
        knn_fill_row(q, point, held, __builtin_inff(), RT_POINT_MISS);
        if (q.count_out) q.count_out[point] = (int)held;
        neighbors += held;
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float* pp = q.points + (size_t)i * 3u;
        const P3 np{pp[0], pp[1], pp[2]};
        const float rmax = q.rmax ? q.rmax[i] : __builtin_inff();
        const float l2 = point_limit2(rmax);
        const bool bad = !(point_in_reach(np, q.reach) && rmax == rmax);  // not answered (comparisons that are false for a NaN)
        if (bad || !(rmax > 0.0f) || !(l2 > 0.0f)) {  // or nothing has d2 < limit2: an empty row without a walk
            knn_fill_row(q, i, 0u, bad ? __builtin_nanf("") : __builtin_inff(), bad ? RT_POINT_INVALID : RT_POINT_MISS);
            if (q.count_out) q.count_out[i] = bad ? RT_POINT_INVALID : 0;
            invalid += bad ? 1u : 0u;
            return false;
        }
        p = np;
        held = 0u;
        bound = l2;  // boxes beyond the limit are culled from the start
        cur = 0u;
        stk.sp = 0;
        point = i;
        return true;
    }

    // Visit node `cur`: eight lower bounds, eight verdicts against the bound.  Of the inner children that pass, the nearest is kept
    // aside and the others are pushed; then the leaf slots that pass are tested, which can tighten the bound; then the nearest child is
    // judged once more and becomes `cur` (kNoNode: none, or the bound has passed it).
    __device__ __forceinline__ void visit() {
        const NodeRec nd = fetch_node<COUNT>(sc.nodes, cur, tc);
        float lb[8], lmin = 0.0f;
        point_child_lb2(nd, p, lb);
        // (the choice below is this lane's own text, keyed by the bits of `pass`: descend_nearest compares the eight bounds once more, and
        // with sixteen more lane masks alive this kernel kept 26 SGPRs in lanes of a VGPR for 6)
        const uint32_t pass = within_bound(lb, bound);
        uint32_t go = 0, smin = 0;  // inner children still to be entered, the nearest of them
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if ((((pass & nd.imask) >> i) & 1u) && (go == 0u || lb[i] < lmin)) {
                lmin = lb[i];
                smin = (uint32_t)i;
            }
            go |= pass & nd.imask & (1u << i);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (((go >> i) & 1u) && (uint32_t)i != smin) stk.push(Group{nd.child((uint32_t)i), __float_as_uint(lb[i])}, tc.overflow);
        }
        const uint32_t next = go ? nd.child(smin) : kNoNode;
        uint32_t leaves = pass & nd.leafmask;
#pragma unroll 1
        while (leaves) {
            const uint32_t li = nd.leaf_tri((uint32_t)__builtin_ctz(leaves));
            leaves &= leaves - 1u;
            if (COUNT) tc.tris++;
            const float4* tp = sc.tris + (size_t)li * 3;
            const float4 a = tp[0], b = tp[1], c = tp[2];
            const float d2 = closest_on_tri(p, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x}).d2;
            // Fewer than k held: bound = limit2, and d2 < limit2 refuses a NaN and +inf.  k held: bound < limit2 (every entry was accepted
            // below the limit), !(d2 > bound) lets a tie with the last entry through to insert_hit's index comparison, which refuses a NaN.
            if (held < q.k ? d2 < bound : !(d2 > bound)) {
                float* ds = q.dist_out + (size_t)point * q.k;
                insert_hit(ds, q.tri_out + (size_t)point * q.k, q.k, held, d2, (int)__float_as_uint(c.y));
                if (held < q.k) held++;
                if (held == q.k) bound = ds[q.k - 1u];  // the lane's own stores, program order
            }
        }
        cur = (next != kNoNode && !(lmin > bound)) ? next : kNoNode;
    }
    __device__ __forceinline__ bool step(bool alive) {
        if (alive) {
            if (cur == kNoNode) cur = pop_within(stk, bound);
            if (cur != kNoNode) visit();
            else alive = false;
        }
        return alive;
    }
};

template <bool COUNT>
__global__ __launch_bounds__(256, kKnnWaves) void pt_query_knn(const PtScene sc, const KnnQuery q, uint32_t* __restrict__ head, unsigned long long* __restrict__ stats,
                                                               const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    KnnLane<COUNT> lane{sc, q, make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id);
    add_wave_total(&stats[KQ_STAT_INVALID], lane.invalid, lane_id);
    add_wave_total(&stats[KQ_STAT_NEIGHBORS], lane.neighbors, lane_id);
    if (COUNT) {
        add_wave_total(&stats[KQ_STAT_NODES], lane.tc.nodes, lane_id);
        add_wave_total(&stats[KQ_STAT_TRIS], lane.tc.tris, lane_id);
    }
    if (lane.tc.overflow) atomicOr((unsigned int*)&stats[KQ_STAT_OVERFLOW], 1u);
}

// ---- launcher -------------------------------------------------------------------------------------
int launch_pt_query_knn(Ctx* c, const PtScene& sc, const KnnQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                        uint32_t refill_min) {
    QueryKernel<KnnQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_knn<decltype(cnt)::value>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
