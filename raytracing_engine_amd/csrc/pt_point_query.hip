// pt_point_query.hip — path B: closest-point queries on device arrays (pt_query_points).  The refilling
// loop of pt_query_rays (pt_trace.hip) over pt_queue.h's streams around a nearest-first walk of the BVH8: of pt_traverse.h only the
// stack and ubyte_f32 are used, the arithmetic that decides an answer is point_tri.h's.  Nothing of rays, frames, path state,
// shading or packets is used here.
#include "hit_attr.h"
#include "point_tri.h"
#include "pt_launch.h"
#include "pt_queue.h"

namespace rt {
using namespace rtk;

// ---- closest-point queries on device arrays (rt_query_points_device) -----------------------
// The loop of pt_query_rays - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and
// no live lane" - around another walk.  A nearest-neighbour walk is not a ray walk: the box test is a distance bound (child_lb2 of
// point_tri.h), the order of the children follows that bound and not a direction octant, and the pruning radius - the lane's best
// d2 - shrinks as the walk goes.  Stack entries are (node index, lb2 bits) in TravStack's 8-byte slots: one pending sibling each, so
// a popped entry whose bound the best d2 has passed meanwhile is dropped without fetching its node (the ray kernels' group-per-level
// entries carry no distance).  Worst case 7 entries per level below the root (point_stack_need, rt_internal.h).
// All arithmetic that decides an answer is point_tri.h's, shared with the tests' CPU reference.
constexpr uint32_t kNoNode = 0xffffffffu;
constexpr int kPointWaves = 8;

struct NearestTri {
    float d2;
    uint32_t id;  // original triangle index (tie-break)
    int li;       // leaf-order triangle index, -1 = none
};

// the triangle at leaf position li against p: (d2, u, v) and the triangle's original index
__device__ __forceinline__ ClosestTri point_tri_test(const float4* __restrict__ tris, uint32_t li, P3 p, uint32_t& id) {
    const float4* tp = tris + (size_t)li * 3;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    id = __float_as_uint(c.y);
    return closest_on_tri(p, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x});
}

// Visit node `cur`: five 16-byte fetches, BOTH planes of every child on every axis decoded (v_cvt_f32_ubyteN + fma), eight lower
// bounds, eight verdicts against best.d2.  Leaf slots that pass are tested at once, so that they can shrink best.d2 before the inner
// children are judged; of the inner children that still pass, the nearest becomes `cur` (kNoNode: none) and the others are pushed.
// The eight bounds stay in registers: every loop that indexes them is unrolled.
template <bool COUNT>
__device__ __forceinline__ void point_node_step(const PtScene& sc, P3 p, uint32_t& cur, NearestTri& best, TravStack& stk, TravCounters& tc) {
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
        const float gx = axis_gap(p.x, n0.x, sx, ubyte_f32(lx[w], b), ubyte_f32(hx[w], b));
        const float gy = axis_gap(p.y, n0.y, sy, ubyte_f32(ly[w], b), ubyte_f32(hy[w], b));
        const float gz = axis_gap(p.z, n0.z, sz, ubyte_f32(lz[w], b), ubyte_f32(hz[w], b));
        lb[i] = gap_lb2(gx, gy, gz);
        if (!(lb[i] > best.d2)) pass |= 1u << i;
    }
    uint32_t leaves = pass & leafmask;
#pragma unroll 1
    while (leaves) {
        const uint32_t s = (uint32_t)__builtin_ctz(leaves);
        leaves &= leaves - 1u;
        const uint32_t li = tri_base + (uint32_t)__builtin_popcount(leafmask & ~(0xffffffffu << s));
        if (COUNT) tc.tris++;
        uint32_t id;
        const ClosestTri ct = point_tri_test(sc.tris, li, p, id);
        if (nearer(ct.d2, id, best.d2, best.id)) best = NearestTri{ct.d2, id, (int)li};
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
        cur = kNoNode;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((go >> i) & 1u) && (uint32_t)i != smin)
            stk.push(Group{child_base + (uint32_t)__builtin_popcount(imask & ((1u << i) - 1u)), __float_as_uint(lb[i])}, tc.overflow);
    }
    cur = child_base + (uint32_t)__builtin_popcount(imask & ~(0xffffffffu << smin));
}

// Hit attributes (ATTR, rt_query_points_attr_device): the sink writes the (u, v) it forms for point_out anyway and
// hit_attr.h's normal of the record it fetched for them.  The sink stands before the source: p, best and point are the retiring
// point's.  The attribute arrays come in an argument block of their own (PointAttrQuery), so the plain instantiations keep theirs and
// are the code of a kernel without ATTR (profiles/hit_attributes.txt).
template <bool ATTR>
using PointQueryOf = std::conditional_t<ATTR, PointAttrQuery, PointQuery>;

template <bool COUNT, bool ATTR>
__global__ __launch_bounds__(256, kPointWaves) void pt_query_points(const PtScene sc, const PointQueryOf<ATTR> q, uint32_t* __restrict__ head,
                                                                    unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    P3 p{0.0f, 0.0f, 0.0f};
    NearestTri best{0.0f, 0xffffffffu, -1};
    uint32_t cur = kNoNode;  // the node this lane visits next; kNoNode: pop one
    uint32_t point = 0;      // index of this lane's point
    float limit2 = 0.0f;     // its bound on d2
    uint32_t invalid = 0;    // invalid points this lane has met
    bool has_point = false, alive = false;
    QueueCursor qc{q.n, head, home_stream(), 0u};
    bool exhausted = qc.n == 0u;  // every stream has been found dry
    const float nan = __builtin_nanf("");

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_point) {  // the sink
                const bool hit = best.li >= 0 && best.d2 < limit2;
                q.dist_out[point] = hit ? sqrt_cr(best.d2) : __builtin_inff();
                q.tri_out[point] = hit ? (int)best.id : RT_POINT_MISS;
                bool want_record = q.point_out != nullptr;
                if constexpr (ATTR) want_record = q.point_out || q.uv_out || q.normal_out;
                if (want_record) {
                    P3 c{nan, nan, nan};
                    if (hit) {  // (u, v) once more from the record: the same function on the same words, the same bits
                        const float4* tp = sc.tris + (size_t)best.li * 3;
                        const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
                        const P3 v0{ta.x, ta.y, ta.z}, e1{ta.w, tb.x, tb.y}, e2{tb.z, tb.w, tcw.x};
                        const ClosestTri ct = closest_on_tri(p, v0, e1, e2);
                        c = tri_point(v0, e1, e2, ct.u, ct.v);
                        if constexpr (ATTR) write_attr(q.uv_out, q.normal_out, point, ct.u, ct.v, unit_normal(e1, e2));
                    } else if constexpr (ATTR) {
                        write_no_attr(q.uv_out, q.normal_out, point);
                    }
                    if (!ATTR || q.point_out) {  // (without ATTR the record was fetched for nothing else)
                        float* po = q.point_out + (size_t)point * 3u;
                        po[0] = c.x;
                        po[1] = c.y;
                        po[2] = c.z;
                    }
                }
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
                    bool miss = false;
                    if (!(point_in_reach(np, q.reach) && rmax == rmax)) {  // not answered (comparisons that are false for a NaN)
                        q.dist_out[i] = nan;
                        q.tri_out[i] = RT_POINT_INVALID;
                        invalid++;
                        miss = true;
                    } else if (!(rmax > 0.0f) || !(l2 > 0.0f)) {  // nothing has d2 < limit2: a miss without a walk
                        q.dist_out[i] = __builtin_inff();
                        q.tri_out[i] = RT_POINT_MISS;
                        miss = true;
                    } else {
                        p = np;
                        limit2 = l2;
                        best = NearestTri{l2, 0xffffffffu, -1};  // boxes beyond the limit are culled from the start
                        cur = 0u;
                        stk.sp = 0;
                        point = i;
                        has_point = true;
                        alive = true;
                    }
                    if (miss && q.point_out) {
                        float* po = q.point_out + (size_t)i * 3u;
                        po[0] = nan;
                        po[1] = nan;
                        po[2] = nan;
                    }
                    if constexpr (ATTR) {
                        if (miss) write_no_attr(q.uv_out, q.normal_out, i);
                    }
                }
                exhausted = qc.advance_if_dry(base + want);
            }
            if (__ballot(alive) == 0ull && exhausted) break;  // every answer of this wave is written (idle lanes retired above)
        }
        if (alive) {
            if (cur == kNoNode) {  // the nearest pending sibling that the best d2 has not passed
#pragma unroll 1
                while (stk.sp) {
                    const Group e = stk.pop();
                    if (!(__uint_as_float(e.y) > best.d2)) {
                        cur = e.x;
                        break;
                    }
                }
            }
            if (cur != kNoNode) point_node_step<COUNT>(sc, p, cur, best, stk, tc);
            else alive = false;
        }
    }
    add_wave_total(&stats[PQ_STAT_INVALID], invalid, lane);
    if (COUNT) {
        add_wave_total(&stats[PQ_STAT_NODES], tc.nodes, lane);
        add_wave_total(&stats[PQ_STAT_TRIS], tc.tris, lane);
    }
    if (tc.overflow) atomicOr((unsigned int*)&stats[PQ_STAT_OVERFLOW], 1u);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_points(Ctx* c, const PtScene& sc, const PointQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                           const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<PointQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_points<decltype(cnt)::value, false>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

int launch_pt_query_points_attr(Ctx* c, const PtScene& sc, const PointAttrQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                                const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<PointAttrQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { kernel = pt_query_points<decltype(cnt)::value, true>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
