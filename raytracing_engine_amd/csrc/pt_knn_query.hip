// pt_knn_query.hip — path B: k-nearest queries on device arrays (pt_query_knn): the k triangles nearest to
// each caller-supplied point, sorted, in a rectangular n x k output.  The refilling loop of pt_query_points (pt_point_query.hip)
// over pt_queue.h's streams around its nearest-first walk of the BVH8, with the sorted slice of the listing queries (insert_hit,
// pt_slice.h) as the lane's candidate list: of pt_traverse.h only the stack and ubyte_f32 are used, the arithmetic that decides an
// answer is point_tri.h's, shared with the tests' CPU reference.  Nothing of rays, frames, path state, shading or packets is used here.
#include "point_tri.h"
#include "pt_launch.h"
#include "pt_queue.h"
#include "pt_slice.h"

namespace rt {
using namespace rtk;

// ---- k-nearest queries on device arrays (rt_query_knn_device) ---------------------------------------------
// pt_query_points' loop - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and no
// live lane" - and its walk: (node index, lb2 bits) entries, one pending sibling each, a popped entry that the bound has passed is
// dropped unfetched, at most point_stack_need entries.  What differs is what a lane holds.  Its list is its own output row: k
// entries of dist_out / tri_out from i * k on, kept sorted by (d2, original index) with insert_hit (room = k) and keyed by d2 until
// the sink turns the keys into distances, pads the row and writes the count.  A lane reads back only what it stored itself, so
// program order is all the ordering the row needs; no LDS and no register array hold candidates.  Its bound is ONE register:
// limit2 while fewer than k entries are held, then the d2 of the row's last entry, re-read after every accepted insertion and at no
// other time.  A triangle is accepted iff d2 < limit2 and, with k held, (d2, id) lies lexicographically below the last entry; a box
// or a leaf slot is skipped only when lb2 > bound (strictly, and written so that a NaN bound is entered: a tie must reach the index
// comparison).  Since lb2 <= d2 holds in fp32 for every triangle under a box (section 6.14), a skipped subtree holds only triangles
// with d2 > bound: beyond the limit, or strictly behind k held entries, none of which ever leaves the row for a worse one.  The row
// is the first k of the tree-free sorted list on any tree and in any order (section 6.23 has the argument in full).
// The node step is point_node_step's decode with this bound and this triangle phase, and it handles the inner children BEFORE the
// triangles (below); a step of its own, not a shared template: pt_point_query.hip and the kernels compiled from it stay as they are.
constexpr uint32_t kNoKnnNode = 0xffffffffu;
constexpr int kKnnWaves = 8;

// What a lane holds of its row beside the row itself.  Where the row lies is formed from the point's index where it is needed (one
// 64-bit multiply-add per pointer): two pointers held through the walk are four registers this kernel does not have.
struct KnnRow {
    uint32_t held;  // entries held, <= k
    float bound;    // limit2 while held < k, then the row's last d2
};

// Visit node `cur`: point_node_step's five fetches and decode, eight lower bounds, eight verdicts against row.bound.  Of the inner
// children that pass, the nearest is kept aside and the others are pushed; then the leaf slots that pass are tested, which can tighten
// the bound; then the nearest child is judged once more and becomes `cur` (kNoKnnNode: none, or the bound has passed it).
template <bool COUNT>
__device__ __forceinline__ void knn_node_step(const PtScene& sc, const KnnQuery& q, P3 p, uint32_t point, uint32_t& cur, KnnRow& row, TravStack& stk, TravCounters& tc) {
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
    uint32_t pass = 0;  // bit s: the box in slot s is not beyond the bound (empty slots: masked below)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int w = i >> 2, b = i & 3;
        const float gx = axis_gap(p.x, n0.x, sx, ubyte_f32(lx[w], b), ubyte_f32(hx[w], b));
        const float gy = axis_gap(p.y, n0.y, sy, ubyte_f32(ly[w], b), ubyte_f32(hy[w], b));
        const float gz = axis_gap(p.z, n0.z, sz, ubyte_f32(lz[w], b), ubyte_f32(hz[w], b));
        lb[i] = gap_lb2(gx, gy, gz);
        if (!(lb[i] > row.bound)) pass |= 1u << i;
    }
    // The inner children first, on the bound as it stands: the nearest waits in two registers, the others are pushed.  The eight bounds,
    // the child base and the inner mask are dead before the first triangle is fetched: held through the triangle phase, beside the sorted
    // insertion, they put 4 - 6 registers into scratch at this kernel's 64.  What the triangles tighten still counts: the nearest child
    // is judged again below, a pushed one when it is popped - no node is fetched that point_node_step's order would not fetch, though
    // entries are pushed that it would not push (at most seven per level all the same: point_stack_need holds).
    uint32_t go = 0, smin = 0;  // inner children still to be entered, the nearest of them
    float lmin = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if ((((pass & imask) >> i) & 1u) && (go == 0u || lb[i] < lmin)) {
            lmin = lb[i];
            smin = (uint32_t)i;
        }
        go |= pass & imask & (1u << i);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((go >> i) & 1u) && (uint32_t)i != smin)
            stk.push(Group{child_base + (uint32_t)__builtin_popcount(imask & ((1u << i) - 1u)), __float_as_uint(lb[i])}, tc.overflow);
    }
    const uint32_t next = go ? child_base + (uint32_t)__builtin_popcount(imask & ~(0xffffffffu << smin)) : kNoKnnNode;
    uint32_t leaves = pass & leafmask;
#pragma unroll 1
    while (leaves) {
        const uint32_t s = (uint32_t)__builtin_ctz(leaves);
        leaves &= leaves - 1u;
        const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ~(0xffffffffu << s));
        if (COUNT) tc.tris++;
        const float4* tp = sc.tris + (size_t)li * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        const float d2 = closest_on_tri(p, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x}).d2;
        // Fewer than k held: bound = limit2, and d2 < limit2 refuses a NaN and +inf.  k held: bound < limit2 (every entry was accepted
        // below the limit), !(d2 > bound) lets a tie with the last entry through to insert_hit's index comparison, which refuses a NaN.
        if (row.held < q.k ? d2 < row.bound : !(d2 > row.bound)) {
            float* ds = q.dist_out + (size_t)point * q.k;
            insert_hit(ds, q.tri_out + (size_t)point * q.k, q.k, row.held, d2, (int)__float_as_uint(c.y));
            if (row.held < q.k) row.held++;
            if (row.held == q.k) row.bound = ds[q.k - 1u];  // the lane's own stores, program order
        }
    }
    cur = (next != kNoKnnNode && !(lmin > row.bound)) ? next : kNoKnnNode;
}

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

template <bool COUNT>
__global__ __launch_bounds__(256, kKnnWaves) void pt_query_knn(const PtScene sc, const KnnQuery q, uint32_t* __restrict__ head, unsigned long long* __restrict__ stats,
                                                               const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    P3 p{0.0f, 0.0f, 0.0f};
    KnnRow row{0u, 0.0f};
    uint32_t cur = kNoKnnNode;  // the node this lane visits next; kNoKnnNode: pop one
    uint32_t point = 0;         // index of this lane's point
    uint32_t invalid = 0, neighbors = 0;  // what this lane has met
    bool has_point = false, alive = false;
    QueueCursor qc{q.n, head, home_stream(), 0u};
    bool exhausted = qc.n == 0u;  // every stream has been found dry
    const float nan = __builtin_nanf("");

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_point) {  // the sink
                float* ds = q.dist_out + (size_t)point * q.k;
#pragma unroll 1
                for (uint32_t j = 0; j < row.held; j++) ds[j] = sqrt_cr(ds[j]);  // d2 -> dist in place: the lane's own stores, program order
                knn_fill_row(q, point, row.held, __builtin_inff(), RT_POINT_MISS);
                if (q.count_out) q.count_out[point] = (int)row.held;
                neighbors += row.held;
                has_point = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = qc.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(qc.stream, base + (uint32_t)__popcll(idle & lt_mask)) : qc.n;  // >= n: nothing for this lane
                if (!alive && i < qc.n) {  // the source
                    const float* pp = q.points + (size_t)i * 3u;
                    const P3 np{pp[0], pp[1], pp[2]};
                    const float rmax = q.rmax ? q.rmax[i] : __builtin_inff();
                    const float l2 = point_limit2(rmax);
                    const bool bad = !(point_in_reach(np, q.reach) && rmax == rmax);  // not answered (comparisons that are false for a NaN)
                    if (bad || !(rmax > 0.0f) || !(l2 > 0.0f)) {  // or nothing has d2 < limit2: an empty row without a walk
                        knn_fill_row(q, i, 0u, bad ? nan : __builtin_inff(), bad ? RT_POINT_INVALID : RT_POINT_MISS);
                        if (q.count_out) q.count_out[i] = bad ? RT_POINT_INVALID : 0;
                        invalid += bad ? 1u : 0u;
                    } else {
                        p = np;
                        row = KnnRow{0u, l2};  // boxes beyond the limit are culled from the start
                        cur = 0u;
                        stk.sp = 0;
                        point = i;
                        has_point = true;
                        alive = true;
                    }
                }
                exhausted = qc.advance_if_dry(base + want);
            }
            if (__ballot(alive) == 0ull && exhausted) break;  // every answer of this wave is written (idle lanes retired above)
        }
        if (alive) {
            if (cur == kNoKnnNode) {  // the nearest pending sibling that the bound has not passed
#pragma unroll 1
                while (stk.sp) {
                    const Group e = stk.pop();
                    if (!(__uint_as_float(e.y) > row.bound)) {
                        cur = e.x;
                        break;
                    }
                }
            }
            if (cur != kNoKnnNode) knn_node_step<COUNT>(sc, q, p, point, cur, row, stk, tc);
            else alive = false;
        }
    }
    add_wave_total(&stats[KQ_STAT_INVALID], invalid, lane);
    add_wave_total(&stats[KQ_STAT_NEIGHBORS], neighbors, lane);
    if (COUNT) {
        add_wave_total(&stats[KQ_STAT_NODES], tc.nodes, lane);
        add_wave_total(&stats[KQ_STAT_TRIS], tc.tris, lane);
    }
    if (tc.overflow) atomicOr((unsigned int*)&stats[KQ_STAT_OVERFLOW], 1u);
}

// ---- launcher -------------------------------------------------------------------------------------
int launch_pt_query_knn(Ctx* c, const PtScene& sc, const KnnQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                        uint32_t refill_min) {
    QueryKernel<KnnQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_knn<decltype(cnt)::value>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
