// pt_overlap_query.hip — path B: overlap queries on device arrays (pt_query_overlaps): every triangle of the
// mesh that each caller-supplied triangle intersects, counted and listed with the mask of the edges that pierce.  The refilling loop
// of pt_query_neighbors (pt_neighbor_query.hip) over pt_queue.h's streams around a box-overlap walk of the BVH8: of pt_traverse.h the
// stack and the work items (Group) are used, the arithmetic that decides an answer is tri_overlap.h's, shared with the tests' CPU
// reference.  Nothing of rays, frames, path state, shading, packets or the octant table is used here.
#include "pt_launch.h"
#include "pt_queue.h"
#include "pt_slice.h"
#include "tri_overlap.h"

namespace rt {
using namespace rtk;

// ---- overlap queries on device arrays (rt_count_overlaps_device / rt_fill_overlaps_device) ----------------
// The loop of pt_query_neighbors - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and
// no live lane", the slice bookkeeping (lo, room, len, found), the sink and the wave totals - with a source of its own: the caller's
// triangle, nine coordinates, validity decided when the lane loads them, and its box Q.  The walk's test is closed box overlap:
// a child box or a leaf slot is skipped exactly when its decoded box is disjoint from Q on some axis; since the decoded box contains
// the unpadded box B of every triangle below it (section 6.14's lo <= c <= hi, vertices included), a skipped subtree holds only
// triangles with cand false, which the definition refuses: the list is the tree-free one.  Q is fixed for the whole walk, so the
// order of the walk changes nothing - every box that overlaps is entered, every triangle in one is tested exactly once - and the
// passing inner children of a node are ONE group (child base + mask), node_step's protocol: the stack holds at most one group per
// level below the root, depth - 1 <= mesh.stack_need entries, as for the neighbours (section 6.17 has the proof).

// Visit the highest pending inner child of node group G (node_step's bookkeeping): five 16-byte fetches, both planes of all eight
// children decoded (neighbor_node_step's decode: v_cvt_f32_ubyteN + fma), eight overlap verdicts against Q.  The verdicts become
// the new node group and the triangle group (empty slots hold an inverted box that a wide Q overlaps: masked by imask / leafmask).
template <bool COUNT>
__device__ __forceinline__ void overlap_node_step(const float4* __restrict__ nodes, const Box& Q, Group& G, Group& T, TravStack& stk, TravCounters& tc) {
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
    uint32_t pass = 0;  // bit s: the box in slot s overlaps Q (empty slots: masked below)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int w = i >> 2, b = i & 3;
        const float lox = __builtin_fmaf(ubyte_f32(lx[w], b), sx, n0.x), hix = __builtin_fmaf(ubyte_f32(hx[w], b), sx, n0.x);
        const float loy = __builtin_fmaf(ubyte_f32(ly[w], b), sy, n0.y), hiy = __builtin_fmaf(ubyte_f32(hy[w], b), sy, n0.y);
        const float loz = __builtin_fmaf(ubyte_f32(lz[w], b), sz, n0.z), hiz = __builtin_fmaf(ubyte_f32(hz[w], b), sz, n0.z);
        if (box_overlaps(Q, lox, loy, loz, hix, hiy, hiz)) pass |= 1u << i;
    }
    G.x = __float_as_uint(n1.x);
    G.y = ((pass & imask) << 24) | imask;
    T.x = __float_as_uint(n1.y);
    T.y = (pass & leafmask) | (leafmask << 8);
}

// Fetch the record of the lowest pending leaf slot of T, cand on its own words, all six segment tests, keep the triangle when mask != 0
template <bool COUNT, bool FILL>
__device__ __forceinline__ void overlap_tri_step(const float4* __restrict__ tris, const QueryTri& A, const Box& Q, const OverlapQuery& q, long long lo, uint32_t room,
                                                 uint32_t& found, Group& T, TravCounters& tc) {
    const uint32_t bit = (uint32_t)__builtin_ctz(T.y);  // (caller checked has_tris)
    T.y &= T.y - 1u;
    const uint32_t li = T.x + (uint32_t)__builtin_popcount((T.y >> 8) & ~(0xffffffffu << bit));
    const float4* tp = tris + (size_t)li * 3;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    if (COUNT) tc.tris++;
    const P3 v0{a.x, a.y, a.z}, e1{a.w, b.x, b.y}, e2{b.z, b.w, c.x};
    if (!overlap_cand(Q, v0, e1, e2)) return;
    const uint32_t mask = overlap_mask(A, v0, e1, e2);
    if (mask != 0u) {
        if (FILL) insert_pair(q.tri_out + lo, q.key_out + lo, room, found, (int)__float_as_uint(c.y), (int)mask);
        found++;
    }
}

template <bool COUNT, bool FILL>
__global__ __launch_bounds__(256, kOverlapWaves) void pt_query_overlaps(const PtScene sc, const OverlapQuery q, uint32_t* __restrict__ head,
                                                                        unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    QueryTri A{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}};
    Box Q = query_box(A);
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t item = 0;   // index of this lane's query triangle
    uint32_t found = 0;  // its overlaps so far
    long long lo = 0;    // FILL: where its slice starts
    uint32_t room = 0;   // FILL: entries its slice may hold (0: it does not fit, nothing is written)
    uint32_t len = 0;    // FILL: the slice's own length
    uint32_t invalid = 0, overlaps = 0, written = 0, incomplete = 0, beyond = 0;  // what this lane has met
    bool has_item = false, alive = false;
    QueueCursor cur{q.n, head, home_stream(), 0u};
    bool exhausted = cur.n == 0u;  // every stream has been found dry

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_item) {  // the sink: the slice is already in its final order
                overlaps += found;
                if (FILL) {
                    written += found < room ? found : room;
                    incomplete += (found != 0u && room != len) ? 1u : 0u;
                    beyond += found > len ? found - len : 0u;
                } else {
                    if (q.count_out) q.count_out[item] = (int)found;
                    if (q.count64) q.count64[item] = found;
                }
                has_item = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = cur.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(cur.stream, base + (uint32_t)__popcll(idle & lt_mask)) : cur.n;  // >= n: nothing for this lane
                if (!alive && i < cur.n) {  // the source
                    const float* tp = q.tris + (size_t)i * 9u;
                    const QueryTri nt{P3{tp[0], tp[1], tp[2]}, P3{tp[3], tp[4], tp[5]}, P3{tp[6], tp[7], tp[8]}};
                    if (!tri_in_reach(nt, q.reach)) {  // not walked (comparisons that are false for a NaN)
                        if (!FILL) write_count(q.count_out, q.count64, i, RT_RAY_INVALID, 0ull);
                        invalid++;
                    } else {
                        A = nt;
                        Q = query_box(nt);
                        G = root_group();
                        T = Group{0u, 0u};
                        stk.sp = 0;
                        found = 0u;
                        if (FILL) {
                            const Slice s = open_slice(q.offsets, i, q.capacity);
                            lo = s.lo, len = s.len, room = s.room;
                        }
                        item = i;
                        has_item = true;
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
            if (alive) overlap_node_step<COUNT>(sc.nodes, Q, G, T, stk, tc);
        }
        // triangle phase: one triangle, six tests
        if (alive && has_tris(T)) overlap_tri_step<COUNT, FILL>(sc.tris, A, Q, q, lo, room, found, T, tc);
    }
    add_listing_totals<COUNT, FILL>(stats, lane, invalid, overlaps, written, incomplete, beyond, tc);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_overlaps(Ctx* c, const PtScene& sc, const OverlapQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                             const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<OverlapQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(fill, [&](auto fl) { kernel = pt_query_overlaps<decltype(cnt)::value, decltype(fl)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
