// pt_hit_query.hip — path B: all-hits ray queries on device arrays (pt_query_hits).  The refilling loop of
// pt_query_sides (pt_side_query.hip) over pt_queue.h's streams around ONE crossing walk per caller-supplied ray: node_step of
// pt_traverse.h in its unordered form with tmax = +inf throughout, and ray_parity.h's triangle test with the caller's limit, shared
// with the tests' CPU reference.  Nothing of frames, path state, shading, packets or the octant table is used here.
#include "pt_launch.h"
#include "pt_queue.h"
#include "pt_slice.h"
#include "ray_parity.h"

namespace rt {
using namespace rtk;

// ---- all-hits queries on device arrays (rt_count_ray_hits_device / rt_fill_ray_hits_device) ------------
// The loop of pt_query_sides - implicit queue, 16 stream heads, ballot + prefix-popcount refill, the exit rule "last stream dry and
// no live lane" - with pt_query_rays' source: the caller's ray, its validity decided when the lane loads it.  The walk never learns
// anything and is pt_query_sides' walk exactly: r.tmax is +inf from the first box to the last, so every box the ray passes through
// is entered and every triangle in it is tested exactly once, in any order (UNORDERED: children in slot order, no octant table, no
// LDS beside the stacks).  The caller's limit is applied to the triangle's t alone and culls no box: the t that ray_tri_t computes
// may lie beyond the computed entry of the box that holds the triangle (a far origin, a grazing ray: section 6.16 has the ray), so a
// box culled against the limit would take an accepted hit with it.  What a lane keeps between rounds is its ray, its limit, the
// number of hits found so far and, in the fill step, where its slice starts and how many entries it may hold.
constexpr int kHitWaves = 8;

// cross_step's counterpart: fetch the record of the lowest pending leaf slot of T, test it, take a hit inside (0, limit)
template <bool COUNT, bool FILL>
__device__ __forceinline__ void hit_step(const float4* __restrict__ tris, const TRay& r, float limit, const HitQuery& q, long long lo, uint32_t room, uint32_t& found,
                                         Group& T, TravCounters& tc) {
    const uint32_t bit = (uint32_t)__builtin_ctz(T.y);  // (caller checked has_tris)
    T.y &= T.y - 1u;
    const uint32_t li = T.x + (uint32_t)__builtin_popcount((T.y >> 8) & ~(0xffffffffu << bit));
    const float4* tp = tris + (size_t)li * 3;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    if (COUNT) tc.tris++;
    float t;
    if (ray_tri_t(P3{r.o.x, r.o.y, r.o.z}, P3{r.d.x, r.d.y, r.d.z}, P3{a.x, a.y, a.z}, P3{a.w, b.x, b.y}, P3{b.z, b.w, c.x}, t) && t > 0.0f && t < limit) {
        if (FILL) insert_hit(q.key_out + lo, q.tri_out + lo, room, found, t, (int)__float_as_uint(c.y));
        found++;
    }
}

template <bool COUNT, bool FILL>
__global__ __launch_bounds__(256, kHitWaves) void pt_query_hits(const PtScene sc, const HitQuery q, uint32_t* __restrict__ head,
                                                                unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    TravStack stk = make_trav_stack(lds_stack, sk);

    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    TravCounters tc{0, 0, 0};
    TRay r = make_tray(mk(0.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f), __builtin_inff());  // (defined values; no lane walks before it is given a ray)
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t ray = 0;    // index of this lane's ray
    float limit = 0.0f;  // its distance limit
    uint32_t found = 0;  // its hits so far
    long long lo = 0;    // FILL: where its slice starts
    uint32_t room = 0;   // FILL: entries its slice may hold (0: it does not fit, nothing is written)
    uint32_t len = 0;    // FILL: the slice's own length
    uint32_t invalid = 0, hits = 0, written = 0, incomplete = 0, beyond = 0;  // what this lane has met
    bool has_ray = false, alive = false;
    QueueCursor cur{q.n, head, home_stream(), 0u};
    bool exhausted = cur.n == 0u;  // every stream has been found dry

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_ray) {  // the sink
                hits += found;
                if (FILL) {
                    written += found < room ? found : room;
                    incomplete += (found != 0u && room != len) ? 1u : 0u;
                    beyond += found > len ? found - len : 0u;
                } else {
                    if (q.count_out) q.count_out[ray] = (int)found;
                    if (q.count64) q.count64[ray] = found;
                }
                has_ray = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = cur.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(cur.stream, base + (uint32_t)__popcll(idle & lt_mask)) : cur.n;  // >= n: nothing for this lane
                if (!alive && i < cur.n) {  // the source
                    const float* po = q.origins + (size_t)i * 3u;
                    const float* pd = q.dirs + (size_t)i * 3u;
                    const v3 o = mk(po[0], po[1], po[2]), d = mk(pd[0], pd[1], pd[2]);
                    limit = q.tmax ? q.tmax[i] : __builtin_inff();
                    // (comparisons that are false for a NaN; +-inf origins fail the range test)
                    const bool in_reach = __builtin_fabsf(o.x) <= q.reach && __builtin_fabsf(o.y) <= q.reach && __builtin_fabsf(o.z) <= q.reach;
                    const bool d_finite = __builtin_fabsf(d.x) < __builtin_inff() && __builtin_fabsf(d.y) < __builtin_inff() && __builtin_fabsf(d.z) < __builtin_inff();
                    if (!(in_reach && d_finite && limit == limit)) {  // not walked
                        if (!FILL) write_count(q.count_out, q.count64, i, RT_RAY_INVALID, 0ull);
                        invalid++;
                    } else if (!(limit > 0.0f)) {  // an empty interval: no hit, without a walk
                        if (!FILL) write_count(q.count_out, q.count64, i, 0, 0ull);
                    } else {
                        r = make_tray(o, d, __builtin_inff());
                        G = root_group();
                        T = Group{0u, 0u};
                        stk.sp = 0;
                        found = 0u;
                        if (FILL) {
                            const Slice s = open_slice(q.offsets, i, q.capacity);
                            lo = s.lo, len = s.len, room = s.room;
                        }
                        ray = i;
                        has_ray = true;
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
            if (alive) node_step<COUNT, /*UNORDERED*/ true>(sc.nodes, nullptr, r, G, T, stk, tc);
        }
        // triangle phase: one test
        if (alive && has_tris(T)) hit_step<COUNT, FILL>(sc.tris, r, limit, q, lo, room, found, T, tc);
    }
    add_listing_totals<COUNT, FILL>(stats, lane, invalid, hits, written, incomplete, beyond, tc);
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_query_hits(Ctx* c, const PtScene& sc, const HitQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                         const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<HitQuery> kernel = nullptr;
    with_bool(count, [&](auto cnt) { with_bool(fill, [&](auto fl) { kernel = pt_query_hits<decltype(cnt)::value, decltype(fl)::value>; }); });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
