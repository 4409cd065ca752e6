// pt_neighbor_query.hip — path B: neighbour queries on device arrays (pt_query_neighbors): every triangle
// within a radius of each caller-supplied point, counted and listed.  The refilling loop of pt_query_hits (pt_hit_query.hip) over
// pt_queue.h's streams around a fixed-radius walk of the BVH8: of pt_traverse.h the stack and the work items (Group) are used, the
// arithmetic that decides an answer is point_tri.h's, shared with the tests' CPU reference.  Nothing of rays, frames, path state,
// shading, packets or the octant table is used here.
#include "point_tri.h"
#include "pt_launch.h"
#include "pt_queue.h"
#include "pt_slice.h"

namespace rt {
using namespace rtk;

// ---- neighbour queries on device arrays (rt_count_neighbors_device / rt_fill_neighbors_device) ----------
// The loop of pt_query_hits - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and
// no live lane", the slice bookkeeping (lo, room, len, found), the sink and the wave totals - with pt_query_points' source: the
// caller's point and radius, validity decided when the lane loads them.  The walk is neither of theirs.  Its bound is a distance
// bound like pt_query_points' (child_lb2 of point_tri.h, in point_node_step's decode), but it is FIXED: limit2 = rmax * rmax from
// the first box to the last, and everything below it is kept.  A child box or a leaf slot is skipped exactly when lb2 >= limit2;
// since lb2 <= d2 holds in fp32 for every triangle under the box (section 6.14), a skipped subtree holds only triangles with
// d2 >= limit2, which the strict test d2 < limit2 refuses: the list is the tree-free one.  With a fixed bound the order of the walk
// changes nothing - every box below the bound is entered, every triangle in one is tested exactly once - so there is no nearest-
// first ordering and no (node, lb2) entry: the passing inner children of a node are ONE group (child base + mask), as in the ray
// walks, and node_step's protocol holds: a node visit takes one child out of the current group and pushes what is left of it, so
// the stack holds at most one group per level below the root, depth - 1 <= mesh.stack_need entries (section 6.17 has the proof).
constexpr int kNeighborWaves = 8;

// Visit the highest pending inner child of node group G (node_step's bookkeeping): five 16-byte fetches, both planes of all eight
// children decoded (point_node_step's decode: v_cvt_f32_ubyteN + fma), eight lower bounds, eight verdicts against limit2.  The
// verdicts become the new node group and the triangle group.  !(lb >= limit2): a NaN bound is entered, not skipped.
template <bool COUNT>
__device__ __forceinline__ void neighbor_node_step(const float4* __restrict__ nodes, P3 p, float limit2, Group& G, Group& T, TravStack& stk, TravCounters& tc) {
    const uint32_t pend = G.y;
    const uint32_t bit = 31u - (uint32_t)__builtin_clz(pend);
    G.y &= ~(1u << bit);
    if (has_nodes(G)) stk.push(G, tc.overflow);  // remaining siblings
    const uint32_t slot = bit - 24u;
    const uint32_t rel = (uint32_t)__builtin_popcount(pend & ~(0xffffffffu << slot));  // low byte of pend = imask
    const float4* nd = nodes + (size_t)(G.x + rel) * 5;
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3], n4 = nd[4];
    if (COUNT) tc.nodes++;
    const uint32_t w3 = __float_as_uint(n0.w);
    const float sx = __uint_as_float((w3 & 0xffu) << 23), sy = __uint_as_float(((w3 >> 8) & 0xffu) << 23), sz = __uint_as_float(((w3 >> 16) & 0xffu) << 23);
    const uint32_t imask = w3 >> 24, leafmask = __float_as_uint(n1.z) & 0xffu;
    const uint32_t lx[2] = {__float_as_uint(n2.x), __float_as_uint(n2.y)}, ly[2] = {__float_as_uint(n2.z), __float_as_uint(n2.w)};
    const uint32_t lz[2] = {__float_as_uint(n3.x), __float_as_uint(n3.y)}, hx[2] = {__float_as_uint(n3.z), __float_as_uint(n3.w)};
    const uint32_t hy[2] = {__float_as_uint(n4.x), __float_as_uint(n4.y)}, hz[2] = {__float_as_uint(n4.z), __float_as_uint(n4.w)};
    uint32_t pass = 0;  // bit s: the box in slot s reaches below the limit (empty slots: masked below)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int w = i >> 2, b = i & 3;
        const float gx = axis_gap(p.x, n0.x, sx, ubyte_f32(lx[w], b), ubyte_f32(hx[w], b));
        const float gy = axis_gap(p.y, n0.y, sy, ubyte_f32(ly[w], b), ubyte_f32(hy[w], b));
        const float gz = axis_gap(p.z, n0.z, sz, ubyte_f32(lz[w], b), ubyte_f32(hz[w], b));
        if (!(gap_lb2(gx, gy, gz) >= limit2)) pass |= 1u << i;
    }
    G.x = __float_as_uint(n1.x);
    G.y = ((pass & imask) << 24) | imask;
    T.x = __float_as_uint(n1.y);
    T.y = (pass & leafmask) | (leafmask << 8);
}

// Fetch the record of the lowest pending leaf slot of T, closest_on_tri on its own words, keep the triangle when d2 < limit2
template <bool COUNT, bool FILL>
__device__ __forceinline__ void neighbor_tri_step(const float4* __restrict__ tris, P3 p, float limit2, const NeighborQuery& q, long long lo, uint32_t room, uint32_t& found,
                                                  Group& T, TravCounters& tc) {
    const uint32_t bit = (uint32_t)__builtin_ctz(T.y);  // (caller checked has_tris)
    T.y &= T.y - 1u;
    const uint32_t li = T.x + (uint32_t)__builtin_popcount((T.y >> 8) & ~(0xffffffffu << bit));
    const float4* tp = tris + (size_t)li * 3;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    if (COUNT) tc.tris++;
    const float d2 = closest_on_tri(p, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x}).d2;
    if (d2 < limit2) {
        if (FILL) insert_hit(q.key_out + lo, q.tri_out + lo, room, found, d2, (int)__float_as_uint(c.y));  // keyed by d2 until the sink
        found++;
    }
}

template <bool COUNT, bool FILL>
__global__ __launch_bounds__(256, kNeighborWaves) void pt_query_neighbors(const PtScene sc, const NeighborQuery q, uint32_t* __restrict__ head,
                                                                          unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    P3 p{0.0f, 0.0f, 0.0f};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t point = 0;   // index of this lane's point
    float limit2 = 0.0f;  // its bound on d2, fixed for the whole walk
    uint32_t found = 0;   // its neighbours so far
    long long lo = 0;     // FILL: where its slice starts
    uint32_t room = 0;    // FILL: entries its slice may hold (0: it does not fit, nothing is written)
    uint32_t len = 0;     // FILL: the slice's own length
    uint32_t invalid = 0, neighbors = 0, written = 0, incomplete = 0, beyond = 0;  // what this lane has met
    bool has_point = false, alive = false;
    QueueCursor cur{q.n, head, home_stream(), 0u};
    bool exhausted = cur.n == 0u;  // every stream has been found dry

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_point) {  // the sink
                neighbors += found;
                if (FILL) {
                    const uint32_t kept = found < room ? found : room;
                    float* ds = q.key_out + lo;
#pragma unroll 1
                    for (uint32_t j = 0; j < kept; j++) ds[j] = sqrt_cr(ds[j]);  // d2 -> dist in place: the lane's own stores, program order
                    written += kept;
                    incomplete += (found != 0u && room != len) ? 1u : 0u;
                    beyond += found > len ? found - len : 0u;
                } else {
                    if (q.count_out) q.count_out[point] = (int)found;
                    if (q.count64) q.count64[point] = found;
                }
                has_point = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = cur.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(cur.stream, base + (uint32_t)__popcll(idle & lt_mask)) : cur.n;  // >= n: nothing for this lane
                if (!alive && i < cur.n) {  // the source
                    const float* pp = q.points + (size_t)i * 3u;
                    const P3 np{pp[0], pp[1], pp[2]};
                    const float rmax = q.rmax ? q.rmax[i] : q.rmax_all;
                    const float l2 = point_limit2(rmax);
                    if (!(point_in_reach(np, q.reach) && rmax == rmax)) {  // not walked (comparisons that are false for a NaN)
                        if (!FILL) write_count(q.count_out, q.count64, i, RT_POINT_INVALID, 0ull);
                        invalid++;
                    } else if (!(rmax > 0.0f) || !(l2 > 0.0f)) {  // nothing has d2 < limit2: no neighbour, without a walk
                        if (!FILL) write_count(q.count_out, q.count64, i, 0, 0ull);
                    } else {
                        p = np;
                        limit2 = l2;
                        G = root_group();
                        T = Group{0u, 0u};
                        stk.sp = 0;
                        found = 0u;
                        if (FILL) {
                            const Slice s = open_slice(q.offsets, i, q.capacity);
                            lo = s.lo, len = s.len, room = s.room;
                        }
                        point = i;
                        has_point = true;
                        alive = true;
                    }
                }
                exhausted = cur.advance_if_dry(base + want);
            }
            if (__ballot(alive) == 0ull && exhausted) break;  // every answer of this wave is written (idle lanes retired above)
        }
        // node phase: lanes without pending triangles visit their next node
        if (alive && !has_tris(T)) {
            if (!has_nodes(G)) {
                if (stk.sp) G = stk.pop();
                else alive = false;
            }
            if (alive) neighbor_node_step<COUNT>(sc.nodes, p, limit2, G, T, stk, tc);
        }
        // triangle phase: one test
        if (alive && has_tris(T)) neighbor_tri_step<COUNT, FILL>(sc.tris, p, limit2, q, lo, room, found, T, tc);
    }
    add_listing_totals<COUNT, FILL>(stats, lane, invalid, neighbors, written, incomplete, beyond, tc);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_neighbors(Ctx* c, const PtScene& sc, const NeighborQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<NeighborQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(fill, [&](auto fl) { kernel = pt_query_neighbors<decltype(cnt)::value, decltype(fl)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
