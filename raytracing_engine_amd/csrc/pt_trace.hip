// pt_trace.hip — path B: every kernel in which a lane walks the BVH8 with a ray of its own (stage map: path_b.hip).  The render
// kernels pt_trace<closest|any> and pt_trace_fused with the four schedules of their triangle tests (inline, pooled, postponed,
// inline with the software-pipelined refill), the wave's pool and prefetch rings, retiring a ray into the path state and loading
// one from it; then the kernels that run the same rounds on caller-supplied rays: the rt_trace_rays test hook (pt_trace_rays) and
// the ray queries on device arrays (pt_query_rays).  The walk itself is pt_traverse.h's, the queue pt_queue.h's.
// Why the hook and the ray queries are here and not beside the point queries: they share instantiations of inline_round with the
// render kernels, and what the compiler makes of a shared function depends on the callers it sees in the unit (constant arguments
// are propagated into it before it is inlined).  In a unit of their own two of them compile to other code (profiles/split_path_b.txt).
#include "hit_attr.h"
#include "pt_launch.h"
#include "pt_query_loop.h"

namespace rt {
using namespace rtk;

// ---- wave-pooled triangle tests --------------------------------------------------------------------
// In the per-lane loop a triangle phase runs with the 5-7 lanes that happen to hold a leaf hit (0.12 triangles per node
// visit on the 1 M soup), at the price of ~65 vector instructions for the whole wave, every round.  Pooled mode takes
// the phase out of the round: a lane whose node step hit leaf slots appends ONE 8-byte group (tri_base, hit bits,
// leafmask, owner lane) to a per-wave ring in LDS and keeps traversing; when the ring holds enough groups the whole
// wave tests one triangle per lane - ray origin / direction of the owner through ds_bpermute, the result merged into
// the owner's slot with a 64-bit LDS minimum on (t bits, triangle id), which is exactly tri_step's tie-break rule
// (t > 0, so the float's bits order like the float) - and groups with further hit slots go back to the ring.
// The owner learns its new tmax / its occlusion after the flush; until then it may enter nodes a tighter tmax would
// have culled, which never changes a result (boxes are conservative, the hit is a minimum over
// every triangle tested).  The ring is drained before any lane retires, so a ray's result is complete when it is stored.
// Ring bound: a round starts with at most kPoolRing - 64 groups pending and adds at most 64.  A flush tests 64 groups but puts
// back every one with further hit slots (all 64 of them, possibly), so one pass per round would let the ring grow by up to 64
// a round; the flush is therefore repeated until the bound holds again (each pass takes one hit slot from every group it tests,
// and flush_at <= 64 makes it fire whenever more than 64 groups are pending).
constexpr uint32_t kPoolRing = 128;  // groups
// The pool is read and written by different lanes of ONE wave: DS operations of a wave execute in program order, so no
// barrier instruction is needed; pool_sync() only keeps the COMPILER from moving LDS accesses across the phase boundaries
// (the pointers are not volatile: volatile accesses would stay on generic pointers and become flat_* instructions).
struct TriPool {
    lds_u64* ring;  // kPoolRing groups: x = tri_base, y = hit slots 7..0 | leafmask 15..8 | owner lane 21..16
    lds_u64* best;  // 64 owners: closest = (t bits << 32) | triangle id; any-hit: != 0 = occluded
    lds_u32* li;    // 64 owners: leaf-order index of the best triangle
    uint32_t head, count;  // wave-uniform
};
__device__ __forceinline__ void pool_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
constexpr unsigned long long kPoolNoHit = (0x7f800000ull << 32) | 0xffffffffull;  // (inf, no id)

__device__ __forceinline__ float lane_read(float v, uint32_t src_lane) {  // ds_bpermute_b32: every lane reads lane src_lane's v
    return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __float_as_int(v)));
}

// One pass over (at most) the 64 oldest groups of the ring: lane i tests the first pending triangle of group i.
// Must be called by the whole wave in convergent code.
template <bool ANY, bool COUNT>
__device__ __forceinline__ void pool_test(const float4* __restrict__ tris, const TRay& r, TriPool& P, uint32_t lane, TravCounters& tc) {
    const uint32_t n = P.count < 64u ? P.count : 64u;
    const bool has = lane < n;
    if (COUNT) tc.flushes++;
    const unsigned long long e = has ? P.ring[(P.head + lane) & (kPoolRing - 1u)] : 0x100ull << 32;
    const uint32_t ex = (uint32_t)e, ey = (uint32_t)(e >> 32);
    P.head = uniform(P.head + n);
    P.count = uniform(P.count - n);
    const uint32_t bit = (uint32_t)__builtin_ctz(ey);  // lowest pending leaf slot (the idle lanes' dummy has bit 8 set)
    const uint32_t rest = ey & (ey - 1u);
    const uint32_t li = ex + (uint32_t)__builtin_popcount((ey >> 8) & 0xffu & ~(0xffffffffu << bit));
    const uint32_t owner = (ey >> 16) & 63u;
    const v3 o = mk(lane_read(r.o.x, owner), lane_read(r.o.y, owner), lane_read(r.o.z, owner));
    const v3 d = mk(lane_read(r.d.x, owner), lane_read(r.d.y, owner), lane_read(r.d.z, owner));
    bool hit = false;
    float t = 0.0f;
    uint32_t id = 0;
    if (has) {
        const float4* tp = tris + (size_t)li * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        if (COUNT) tc.tris++;
        hit = tri_test(o, d, mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, c.x), t) && t > 0.0f;
        id = __float_as_uint(c.y);
    }
    if (ANY) {
        if (hit && t < kShadowTmax) P.best[owner] = 1ull;
    } else {
        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | id;
        if (hit) __hip_atomic_fetch_min(&P.best[owner], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        pool_sync();
        if (hit && P.best[owner] == key) P.li[owner] = li;  // ids are unique: at most one lane per owner sees its own key
    }
    // groups with further hit slots go back to the ring
    const bool more = has && (rest & 0xffu) != 0u;
    const unsigned long long mm = __ballot(more);
    if (mm) {
        const uint32_t pos = P.head + P.count + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
        if (more) P.ring[pos & (kPoolRing - 1u)] = ((unsigned long long)rest << 32) | ex;
        P.count = uniform(P.count + (uint32_t)__popcll(mm));
    }
    pool_sync();
}

// ---- trace ----------------------------------------------------------------------------------------
// Persistent waves with per-lane refill.  Traversal lengths are heavy-tailed (a ray may end after 3
// nodes or after 500), so a wave that waits for its slowest ray idles most lanes.  Instead every
// lane carries its own ray: whenever at least `refill_min` lanes have finished, the wave retires
// their results and hands them the next rays of the device-resident queue (one atomic per refill on
// one of PT_HEADS interleaved stream heads, ballot + prefix-popcount to assign entries; a wave whose
// stream runs dry moves on to the next one, so the tail of the queue is shared by all waves).  The wave exits when the queue is drained and all its
// lanes are done, so the grid is sized for the machine, not for the queue length.
// Between two refill checks every lane visits one node and tests up to `kTrisPerRound` triangles.

// How the triangle tests of the per-lane kernels are scheduled (rt_pt_params.tune_tri_mode):
//   TRI_INLINE  every round ends with a triangle phase for the lanes that hold a leaf hit (rounds 1 and 2 of the build)
//   TRI_POOL    wave-pooled tests: leaf hits go to a per-wave LDS ring, the wave tests 64 of them at once (above)
//   TRI_INLINE_PF  the inline phase with the software-pipelined refill (trace_queue_pf below): rays wait in a per-wave LDS ring
//   TRI_DEFER   postponed tests: a lane parks up to two leaf-hit groups in registers and keeps visiting nodes; the triangle
//               phase runs when enough lanes hold a group (or enough of them can do nothing else)
enum { TRI_INLINE = TRI_MODE_INLINE, TRI_POOL = TRI_MODE_POOL, TRI_DEFER = TRI_MODE_DEFER, TRI_INLINE_PF = TRI_MODE_INLINE_PF };

// Retire a finished ray: a closest-hit ray stores (t, triangle) for pt_shade, an unoccluded shadow ray adds its contribution to its path.
__device__ __forceinline__ void retire_ray(const PtState& st, bool is_any, uint32_t slot, bool occluded, const Hit& best) {
    if (is_any) {
        if (!occluded) {
            const uint32_t pid = __float_as_uint(st.sh_o[slot].w);
            const float4 c = st.sh_c[slot];
            float4 L = st.rad[pid];
            L.x += c.x;
            L.y += c.y;
            L.z += c.z;
            st.rad[pid] = L;
        }
    } else {
        st.hit[slot] = make_float2(best.t, __int_as_float(best.li));
    }
}

// Entry i of a queue -> its ray.  Returns the ray's slot: the path id of a closest-hit ray, the shadow-queue index of a shadow ray.
__device__ __forceinline__ uint32_t load_ray(const PtState& st, const uint32_t* __restrict__ queue, bool is_any, uint32_t i, v3& o, v3& d) {
    if (is_any) {
        const float4 so = st.sh_o[i], sd = st.sh_d[i];
        o = mk(so.x, so.y, so.z);
        d = mk(sd.x, sd.y, sd.z);
        return i;
    }
    const uint32_t slot = queue[i];
    const float4 ro = st.ray_o[slot], rd = st.ray_d[slot];
    o = mk(ro.x, ro.y, ro.z);
    d = mk(rd.x, rd.y, rd.z);
    return slot;
}

// What a wave's loop leaves in stats[].  kinds: bit 0 = the loop carried closest-hit rays (counted in `closest`), bit 1 = shadow rays
// (`shadow`, added at shadow_word: PT_STAT_SHADOW or PT_STAT_FUSED_SHADOW); node / triangle counts per lane, the rest wave-uniform.
template <bool COUNT>
__device__ __forceinline__ void flush_trace_counters(unsigned long long* __restrict__ stats, uint32_t lane, uint32_t kinds, const TravCounters& closest,
                                                     const TravCounters& shadow, uint32_t shadow_word, uint32_t rounds, uint32_t alive_rounds, uint32_t flushes,
                                                     uint32_t overflow) {
    if (COUNT) {
        if (kinds & 1u) {
            add_wave_total(&stats[PT_STAT_NODES], closest.nodes, lane);
            add_wave_total(&stats[PT_STAT_NODES + 1], closest.tris, lane);
        }
        if (kinds & 2u) {
            add_wave_total(&stats[shadow_word], shadow.nodes, lane);
            add_wave_total(&stats[shadow_word + 1u], shadow.tris, lane);
        }
        if (lane == 0) {
            if (kinds & 1u) {  // occupancy of the rounds: wave-rounds and alive lane-rounds
                atomicAdd(&stats[PT_STAT_ROUNDS], (unsigned long long)rounds);
                atomicAdd(&stats[PT_STAT_ROUNDS + 1], (unsigned long long)alive_rounds);
            }
            atomicAdd(&stats[PT_STAT_FLUSHES], (unsigned long long)flushes);
            atomicAdd(&stats[PT_STAT_ROUNDS_ALL], (unsigned long long)rounds);
        }
    }
    if (overflow) atomicOr((unsigned int*)&stats[PT_STAT_OVERFLOW], 1u);
}

struct QueueRef {  // a device-resident ray queue: its size and its stream heads (the rays: PtState)
    const uint32_t* count;
    uint32_t* head;
};

// ---- the inline schedule -----------------------------------------------------------------------------
// KIND: the rays a loop carries.  RAYS_BOTH is the fused launch.  A loop for the closest-hit queue followed by one for the shadow
// queue makes every wave DRAIN between the two: once the closest-hit queue is dry a wave gets no refills, its lanes run out one by
// one (a tenth of its rounds, at nine of 64 lanes alive) and only then does it turn to the shadow queue.  The node step is the same
// for both kinds of ray and the triangle step differs only in what a hit means, so with RAYS_BOTH the kind is a per-lane flag: when
// the closest-hit queue is dry the wave's idle lanes are refilled from the shadow queue while its last closest-hit rays are still
// walking.  One tail per wave and launch instead of two.  Every ray is traced by exactly the step functions of the one-kind loops,
// where the flag is a constant that folds away, so frames and counts are unchanged.
enum { RAYS_CLOSEST = 0, RAYS_ANY = 1, RAYS_BOTH = 2 };

template <int KIND, bool COUNT>
__device__ __forceinline__ void trace_queue_inline(const PtScene& sc, const PtState& st, const uint32_t* __restrict__ queue, QueueRef closest_q, QueueRef shadow_q,
                                                   unsigned long long* __restrict__ stats, TravStack& stk, const uint8_t* perm_lut, uint32_t refill_min,
                                                   uint32_t shadow_stat) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t n_closest = KIND == RAYS_ANY ? 0u : uniform(*closest_q.count), n_shadow = KIND == RAYS_CLOSEST ? 0u : uniform(*shadow_q.count);
    const int tris_per_round = tris_per_round_of(refill_min);
    refill_min &= 0xffu;
    TravCounters tc{0, 0, 0};                            // COUNT: the current ray of this lane (one kind: every ray)
    TravCounters cl_done{0, 0, 0}, any_done{0, 0, 0};  // COUNT, RAYS_BOTH: retired rays of this lane, by kind

    TRay r = make_tray(mk(0.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f), 0.0f);
    Hit best{0.0f, -1, 0u};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t slot = 0;  // closest: path id; any-hit: shadow-queue index
    bool has_ray = false, occluded = false;
    bool alive = false;             // this lane still has traversal work for its ray
    bool is_any = KIND == RAYS_ANY;  // the kind of this lane's ray
    // wave-uniform: which queue the wave refills from, and where it stands in it
    uint32_t phase = KIND == RAYS_ANY || (KIND == RAYS_BOTH && n_closest == 0u) ? 1u : 0u;  // 0 = closest-hit queue, 1 = shadow queue
    const uint32_t stream0 = home_stream();
    QueueCursor cur{phase == 0u ? n_closest : n_shadow, phase == 0u ? closest_q.head : shadow_q.head, stream0, 0u};
    bool exhausted = cur.n == 0u;           // every stream of the last queue has been found dry
    uint32_t rounds = 0, alive_rounds = 0;  // COUNT only

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (!alive && has_ray) {
                retire_ray(st, is_any, slot, occluded, best);
                if (COUNT && KIND == RAYS_BOTH) {
                    if (is_any) {
                        any_done.nodes += tc.nodes;
                        any_done.tris += tc.tris;
                    } else {
                        cl_done.nodes += tc.nodes;
                        cl_done.tris += tc.tris;
                    }
                    tc.nodes = tc.tris = 0;
                }
                has_ray = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = cur.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(cur.stream, base + (uint32_t)__popcll(idle & lt_mask)) : cur.n;  // >= n: nothing for this lane
                if (!alive && i < cur.n) {
                    const auto take = [&](bool any) {  // (the kind as a constant: one make_tray per kind, as the loads differ anyway)
                        v3 o, d;
                        slot = load_ray(st, queue, any, i, o, d);
                        start_ray(any, o, d, r, best, G, T, stk);
                        is_any = any;
                    };
                    if (KIND == RAYS_ANY || (KIND == RAYS_BOTH && phase != 0u)) take(true);
                    else take(false);
                    occluded = false;
                    has_ray = true;
                    alive = true;
                }
                if (cur.advance_if_dry(base + want)) {  // this queue is dry: on to the shadow queue, or done
                    if (KIND == RAYS_BOTH && phase == 0u && n_shadow != 0u) {
                        phase = 1u;
                        cur = QueueCursor{n_shadow, shadow_q.head, stream0, 0u};
                    } else {
                        exhausted = true;
                    }
                }
            }
            // every lane retired and nothing handed out: a one-kind loop is done (the streams this wave has not seen are drained by the
            // waves that started on them), the loop for both queues goes on until it has found the last stream of the last queue dry
            if (__ballot(alive) == 0ull && (KIND != RAYS_BOTH || exhausted)) break;
        }
        if (COUNT) {  // occupancy of the round: wave-rounds and alive lane-rounds
            rounds++;
            alive_rounds += (uint32_t)__popcll(__ballot(alive));
        }
        // (UNORDERED for the any-hit rays of an all-shadow launch)
        alive = inline_round<COUNT, KIND == RAYS_ANY>(sc, perm_lut, r, best, G, T, stk, tc, alive, occluded, is_any, tris_per_round);
    }
    flush_trace_counters<COUNT>(stats, lane, KIND == RAYS_BOTH ? 3u : KIND == RAYS_ANY ? 2u : 1u, KIND == RAYS_BOTH ? cl_done : tc, KIND == RAYS_BOTH ? any_done : tc,
                                shadow_stat, rounds, alive_rounds, 0u, tc.overflow);
}

// ---- the pooled and the postponed schedule -------------------------------------------------------------
struct PoolMem {  // LDS of one wave's pool (TRI_POOL kernels only)
    lds_u64* ring;
    lds_u64* best;
    lds_u32* li;
};

template <bool ANY, bool COUNT, int MODE>
__device__ __forceinline__ void trace_queue(const PtScene& sc, const PtState& st, const uint32_t* __restrict__ queue, QueueRef q,
                                            unsigned long long* __restrict__ stats, TravStack& stk, const uint8_t* perm_lut, uint32_t refill_min,
                                            const PoolMem& pm, uint32_t tri_cfg /* TRI_POOL: byte 0 = groups that trigger a flush, byte 1 = rounds a group may wait */,
                                            uint32_t shadow_stat) {
    static_assert(MODE == TRI_POOL || MODE == TRI_DEFER, "the inline schedules have loops of their own");
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    refill_min &= 0xffu;
    TravCounters tc{0, 0, 0};

    TRay r = make_tray(mk(0.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f), 0.0f);
    Hit best{0.0f, -1, 0u};
    Group G{0u, 0u}, T{0u, 0u}, T2{0u, 0u};  // T2: TRI_DEFER's second parking slot
    uint32_t slot = 0;  // closest: path id; any-hit: shadow-queue index
    bool has_ray = false, occluded = false;
    QueueCursor cur{uniform(*q.count), q.head, home_stream(), 0u};
    bool exhausted = cur.n == 0u;            // wave-uniform: every stream of the queue has been found dry
    uint32_t rounds = 0, alive_rounds = 0;  // COUNT only
    bool alive = false;       // this lane still has traversal work for its ray

    // TRI_POOL state (all wave-uniform)
    TriPool P{pm.ring, pm.best, pm.li, 0u, 0u};
    const lds_u32* best32 = reinterpret_cast<const lds_u32*>(pm.best);
    // TRI_POOL: groups in the ring that trigger a flush / rounds a group may wait;  TRI_DEFER: holding lanes / stuck lanes that trigger the phase
    const uint32_t flush_at = (tri_cfg & 0xffu) ? ((tri_cfg & 0xffu) < 64u ? (tri_cfg & 0xffu) : 64u) : (MODE == TRI_DEFER ? 32u : 40u);
    const uint32_t wait_max = ((tri_cfg >> 8) & 0xffu) ? ((tri_cfg >> 8) & 0xffu) : (MODE == TRI_DEFER ? 8u : 6u);
    uint32_t waited = 0;
    bool flushed = false;

    for (;;) {
        const unsigned long long idle = __ballot(!alive);
        if (idle == ~0ull || (!exhausted && (uint32_t)__popcll(idle) >= refill_min)) {
            if (MODE == TRI_POOL) {  // a ray's result is complete only when none of its triangles is pending
                while (P.count) {
                    pool_test<ANY, COUNT>(sc.tris, r, P, lane, tc);
                    flushed = true;
                }
                waited = 0;
            }
            if (!alive && has_ray) {
                if (MODE == TRI_POOL) {
                    if (ANY) occluded = best32[2u * lane] != 0u;
                    else {
                        best.t = __uint_as_float(best32[2u * lane + 1u]);
                        best.li = (int)pm.li[lane];
                    }
                }
                retire_ray(st, ANY, slot, occluded, best);
                has_ray = false;
            }
            if (!exhausted) {  // exactly what the idle lanes need, assigned by ballot + prefix popcount
                const uint32_t want = (uint32_t)__popcll(idle);
                const uint32_t base = cur.reserve(want, lane);
                const uint32_t i = !alive ? stream_entry(cur.stream, base + (uint32_t)__popcll(idle & lt_mask)) : cur.n;  // >= n: nothing for this lane
                if (!alive && i < cur.n) {
                    v3 o, d;
                    slot = load_ray(st, queue, ANY, i, o, d);
                    start_ray(ANY, o, d, r, best, G, T, stk);
                    T2 = Group{0u, 0u};
                    occluded = false;
                    has_ray = true;
                    alive = true;
                    if (MODE == TRI_POOL) {
                        pm.best[lane] = ANY ? 0ull : kPoolNoHit;
                        if (!ANY) pm.li[lane] = 0xffffffffu;
                    }
                }
                exhausted = cur.advance_if_dry(base + want);
            }
            if (__ballot(alive) == 0ull) break;  // nothing left for this wave: the streams it has not seen are drained by their own waves
        }
        if (COUNT) {  // occupancy of the round: wave-rounds and alive lane-rounds
            rounds++;
            alive_rounds += (uint32_t)__popcll(__ballot(alive));
        }
        if (MODE == TRI_POOL) {
            if (flushed) {  // owners pick up what the pool found for them (wave-uniform branch)
                flushed = false;
                if (ANY) {
                    if (alive && best32[2u * lane] != 0u) alive = false;  // occluded: the ray is done
                } else if (alive) {
                    r.tmax = __uint_as_float(best32[2u * lane + 1u]);
                }
            }
            // node phase: every lane with traversal work visits its next node
            T.y = 0u;
            if (alive) {
                if (!has_nodes(G)) {
                    if (stk.sp) G = stk.pop();
                    else alive = false;
                }
                if (alive) node_step<COUNT>(sc.nodes, perm_lut, r, G, T, stk, tc);
            }
            // leaf hits of this round -> the ring (ballot + prefix popcount, no atomic: head / count are wave-uniform)
            const bool add = has_tris(T);
            const unsigned long long am = __ballot(add);
            if (am) {
                const uint32_t pos = P.head + P.count + (uint32_t)__popcll(am & lt_mask);
                if (add) P.ring[pos & (kPoolRing - 1u)] = ((unsigned long long)(T.y | (lane << 16)) << 32) | T.x;
                P.count = uniform(P.count + (uint32_t)__popcll(am));
                pool_sync();
            }
            waited = P.count ? waited + 1u : 0u;
            if (P.count >= flush_at || waited >= wait_max) {
                do pool_test<ANY, COUNT>(sc.tris, r, P, lane, tc);
                while (P.count > kPoolRing - 64u);
                flushed = true;
                waited = 0;
            }
        } else {
            // node phase: a lane visits its next node as long as it has somewhere to park a leaf-hit group
            bool stuck = false;  // holds a group and cannot visit a node: out of nodes, or both parking slots taken
            if (alive) {
                if (!has_nodes(G) && stk.sp) G = stk.pop();
                if (!has_nodes(G)) {
                    if (has_tris(T)) stuck = true;
                    else alive = false;  // no nodes left, nothing parked: the ray is done
                } else if (has_tris(T2)) {
                    stuck = true;
                } else {
                    Group N{0u, 0u};
                    node_step<COUNT>(sc.nodes, perm_lut, r, G, N, stk, tc);
                    if (has_tris(N)) {
                        if (has_tris(T)) T2 = N;
                        else T = N;
                    }
                }
            }
            // triangle phase: one test per holding lane, when enough lanes hold a group or enough of them are stuck
            const unsigned long long hold = __ballot(alive && has_tris(T));
            const unsigned long long stuck_m = __ballot(stuck);
            const uint32_t n_hold = (uint32_t)__popcll(hold), n_stuck = (uint32_t)__popcll(stuck_m);
            if (n_hold >= flush_at || n_stuck >= wait_max || (n_stuck != 0u && n_stuck == (uint32_t)__popcll(__ballot(alive)))) {
                if (alive && has_tris(T)) {
                    if (tri_step<ANY, COUNT>(sc.tris, r, best, T, tc)) {
                        occluded = true;
                        alive = false;
                    }
                    if (!has_tris(T)) {
                        T = T2;
                        T2 = Group{0u, 0u};
                    }
                }
                if (COUNT) tc.flushes++;
            }
        }
    }
    flush_trace_counters<COUNT>(stats, lane, ANY ? 2u : 1u, tc, tc, shadow_stat, rounds, alive_rounds, tc.flushes, tc.overflow);
}

// ---- software-pipelined refill (TRI_INLINE_PF) ------------------------------------------------------
// The blocking refill above is three dependent memory round trips (head atomic -> queue entry -> ray) during which the whole
// wave stands still, plus ~190 vector instructions, and that is why its threshold sits at 24 idle lanes: measured, a refill event
// costs what 2.2 traversal rounds cost, so on average 16 of a wave's 64 lanes wait for the next one (47.8 alive per round).
// Here the fetch is taken out of the lanes' way: the wave keeps a ring of kPfRing ready rays in LDS and a four-stage pipeline
// that advances ONE stage per traversal round - reserve kPfBatch queue entries (returning atomic, result not awaited), read the
// queue entries, read the rays, park them in the ring - so every load was issued a round earlier and its data has arrived behind
// the node fetches in between (vector memory returns in order).  A lane that finishes takes the next ray out of LDS as soon as
// `pop_min` lanes are idle (default 8).  The rays in flight chip-wide grow by at most kPfRing per wave (25 %).
constexpr uint32_t kPfRing = 16, kPfBatch = 8;

template <bool ANY, bool COUNT>
__device__ __forceinline__ void trace_queue_pf(const PtScene& sc, const PtState& st, const uint32_t* __restrict__ queue, QueueRef q,
                                               unsigned long long* __restrict__ stats, TravStack& stk, const uint8_t* perm_lut, uint32_t refill_min,
                                               lds_f4* ring /* 2 x kPfRing: origin as loaded, (direction, slot bits) */, uint32_t shadow_stat) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int tris_per_round = tris_per_round_of(refill_min);
    const uint32_t pop_min = (refill_min & 0xffu) ? ((refill_min & 0xffu) < 64u ? (refill_min & 0xffu) : 64u) : 8u;
    TravCounters tc{0, 0, 0};

    TRay r = make_tray(mk(0.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f), 0.0f);
    Hit best{0.0f, -1, 0u};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t slot = 0;  // closest: path id; any-hit: shadow-queue index
    bool has_ray = false, occluded = false, alive = false;
    uint32_t rounds = 0, alive_rounds = 0;  // COUNT only

    // fetch pipeline (wave-uniform unless noted)
    QueueCursor cur{uniform(*q.count), q.head, home_stream(), 0u};
    const uint32_t n = cur.n;
    uint32_t fetch_done = n == 0u ? 1u : 0u;  // every stream of the queue has been found dry
    uint32_t pf_stage = 0;                // 0 idle, 1 entries reserved, 2 queue entries read (closest-hit only), 3 rays read
    uint32_t pf_base = 0;                 // lane 0: what the head atomic returned
    uint32_t pf_idx = n, pf_slot = 0;     // per lane < kPfBatch: queue index (>= n: none), path id / shadow index
    // per lane: the ray, kept as the two 16-byte tuples the loads deliver and the LDS stores take (scalars would be copied out of the
    // load's registers as soon as it is issued, and the copies wait for the data)
    f4v pf_o = {0.0f, 0.0f, 0.0f, 0.0f}, pf_d = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t ring_head = 0, ring_count = 0;

    for (;;) {
        // (the wave-uniform state, pinned to scalar registers: without this the divergence analysis taints it through the lane-
        // dependent code around it and every branch below becomes a lane-masked region whose merges wait for the loads just issued)
        pf_stage = uniform(pf_stage);
        ring_head = uniform(ring_head);
        ring_count = uniform(ring_count);
        cur.stream = uniform(cur.stream);
        cur.dry_streams = uniform(cur.dry_streams);
        fetch_done = uniform(fetch_done);
        // ---- one pipeline stage per round; every value used here was requested a round ago ----
        if (pf_stage == 3u) {
            const bool valid = pf_idx < n;
            const unsigned long long vm = __ballot(valid);
            if (valid) {
                const uint32_t pos = (ring_head + ring_count + (uint32_t)__popcll(vm & lt_mask)) & (kPfRing - 1u);
                f4v d4 = pf_d;
                d4.w = __uint_as_float(pf_slot);
                ring[2u * pos] = pf_o;
                ring[2u * pos + 1u] = d4;
            }
            ring_count = uniform(ring_count + (uint32_t)__popcll(vm));
            pf_stage = 0u;
            pool_sync();
        } else if (pf_stage == 2u) {
            // (every lane loads, lanes without an entry a clamped address: a load under a lane predicate is merged into the live
            // registers with copies, and the copies would wait for the data right here)
            pf_o = *reinterpret_cast<const f4v*>(&st.ray_o[pf_slot]);
            pf_d = *reinterpret_cast<const f4v*>(&st.ray_d[pf_slot]);
            pf_stage = 3u;
        } else if (pf_stage == 1u) {
            const uint32_t base = uniform(pf_base);
            pf_idx = lane < kPfBatch ? stream_entry(cur.stream, base + lane) : n;
            if (cur.advance_if_dry(base + kPfBatch)) fetch_done = 1u;
            const uint32_t safe = pf_idx < n ? pf_idx : n - 1u;  // n > 0 here
            if (ANY) {
                pf_o = *reinterpret_cast<const f4v*>(&st.sh_o[safe]);
                pf_d = *reinterpret_cast<const f4v*>(&st.sh_d[safe]);
                pf_slot = safe;
                pf_stage = 3u;
            } else {
                pf_slot = queue[safe];
                pf_stage = 2u;
            }
        }
        if (pf_stage == 0u && !fetch_done && ring_count + kPfBatch <= kPfRing) {
            if (lane == 0) pf_base = atomicAdd(cur.head_word(), kPfBatch);  // (QueueCursor::reserve without the wait for the answer)
            pf_stage = 1u;
        }

        // ---- retire finished lanes and hand them rays from the ring ----
        const unsigned long long idle = __ballot(!alive);
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        const bool drained = fetch_done && pf_stage == 0u && ring_count == 0u;
        if ((ring_count != 0u && n_idle >= pop_min) || (n_idle == 64u && (ring_count != 0u || drained))) {
            if (!alive && has_ray) {
                retire_ray(st, ANY, slot, occluded, best);
                has_ray = false;
            }
            const uint32_t m = n_idle < ring_count ? n_idle : ring_count;
            const uint32_t rank = (uint32_t)__popcll(idle & lt_mask);
            if (!alive && rank < m) {
                const uint32_t pos = (ring_head + rank) & (kPfRing - 1u);
                const f4v ro = ring[2u * pos], rd = ring[2u * pos + 1u];
                slot = __float_as_uint(rd.w);
                start_ray(ANY, mk(ro.x, ro.y, ro.z), mk(rd.x, rd.y, rd.z), r, best, G, T, stk);
                occluded = false;
                has_ray = true;
                alive = true;
            }
            ring_head = uniform(ring_head + m);
            ring_count = uniform(ring_count - m);
            pool_sync();
            if (m == 0u && drained) break;  // queue and ring empty, every lane retired
        }
        if (COUNT) {
            rounds++;
            alive_rounds += (uint32_t)__popcll(__ballot(alive));
        }
        alive = inline_round<COUNT, false>(sc, perm_lut, r, best, G, T, stk, tc, alive, occluded, ANY, tris_per_round);
    }
    flush_trace_counters<COUNT>(stats, lane, ANY ? 2u : 1u, tc, tc, shadow_stat, rounds, alive_rounds, 0u, tc.overflow);
}

// LDS of a 256-thread workgroup of the per-lane kernels: the traversal stacks (dynamic), the octant table and, for TRI_POOL
// kernels, four pools of 1.75 KiB.
template <int MODE>
struct PoolLds {
    __device__ __forceinline__ PoolMem get(uint32_t) { return PoolMem{nullptr, nullptr, nullptr}; }
};
template <>
struct PoolLds<TRI_POOL> {
    unsigned long long ring[4][kPoolRing];
    unsigned long long best[4][64];
    uint32_t li[4][64];
    __device__ __forceinline__ PoolMem get(uint32_t wave) {
        return PoolMem{(lds_u64*)ring[wave], (lds_u64*)best[wave], (lds_u32*)li[wave]};
    }
};
template <>
struct PoolLds<TRI_INLINE_PF> {
    f4v rays[4][2 * kPfRing];
    __device__ __forceinline__ lds_f4* ring(uint32_t wave) { return (lds_f4*)rays[wave]; }
};
constexpr uint32_t kPoolLdsBytes = 4u * (kPoolRing * 8u + 64u * 8u + 64u * 4u);
constexpr uint32_t kPfLdsBytes = 4u * 2u * kPfRing * 16u;
constexpr int kPfWaves = 6;    // TRI_INLINE_PF: the prefetch registers (two 16-byte tuples, index, slot) do not fit 72 VGPRs without spills in the loop
constexpr int kPoolWaves = 7;  // waves per SIMD the TRI_POOL / TRI_DEFER kernels are compiled for (72 VGPRs; the default stack split leaves room for seven workgroups per CU anyway)
constexpr int trace_waves(int mode) { return mode == TRI_INLINE ? kInlineWaves : mode == TRI_INLINE_PF ? kPfWaves : kPoolWaves; }

// One queue with the schedule MODE, for a wave whose stack, octant table and pool memory stand
template <bool ANY, bool COUNT, int MODE>
__device__ __forceinline__ void trace_one_queue(const PtScene& sc, const PtState& st, const uint32_t* __restrict__ queue, QueueRef q,
                                                unsigned long long* __restrict__ stats, TravStack& stk, const uint8_t* perm_lut, PoolLds<MODE>& pool,
                                                uint32_t refill_min, uint32_t tri_cfg, uint32_t shadow_stat) {
    const uint32_t wave = threadIdx.x >> 6;
    if constexpr (MODE == TRI_INLINE_PF) trace_queue_pf<ANY, COUNT>(sc, st, queue, q, stats, stk, perm_lut, refill_min, pool.ring(wave), shadow_stat);
    else if constexpr (MODE == TRI_INLINE) trace_queue_inline<ANY ? RAYS_ANY : RAYS_CLOSEST, COUNT>(sc, st, queue, q, q, stats, stk, perm_lut, refill_min, shadow_stat);
    else trace_queue<ANY, COUNT, MODE>(sc, st, queue, q, stats, stk, perm_lut, refill_min, pool.get(wave), tri_cfg, shadow_stat);
}

template <bool ANY, bool COUNT, int MODE>
__global__ __launch_bounds__(256, trace_waves(MODE)) void pt_trace(const PtScene sc, PtState st, const uint32_t* __restrict__ queue,
                                                                   const uint32_t* __restrict__ count_ptr, uint32_t* __restrict__ head,
                                                                   unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min, uint32_t tri_cfg) {
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    __shared__ uint8_t perm_lut[2048];
    __shared__ PoolLds<MODE> pool;
    build_perm_lut(perm_lut);
    TravStack stk = make_trav_stack(lds_stack, sk);
    trace_one_queue<ANY, COUNT, MODE>(sc, st, queue, QueueRef{count_ptr, head}, stats, stk, perm_lut, pool, refill_min, tri_cfg, PT_STAT_SHADOW);
}

// closest-hit rays of depth d + 1 and the shadow rays of depth d in ONE persistent launch: the two are independent (the
// shadow rays only add to the paths' radiance, the closest-hit rays only read rays), so every wave first pulls from the
// closest-hit queue - the frame's critical path: shade(d + 1) waits for it - and moves on to the shadow queue when that one
// is dry, instead of leaving the machine to the few long rays of a launch's tail.  One tail per bounce instead of two.
template <bool COUNT, int MODE>
__global__ __launch_bounds__(256, trace_waves(MODE)) void pt_trace_fused(const PtScene sc, PtState st, const uint32_t* __restrict__ queue,
                                                                         const uint32_t* __restrict__ closest_count, uint32_t* __restrict__ closest_head,
                                                                         const uint32_t* __restrict__ shadow_count, uint32_t* __restrict__ shadow_head,
                                                                         unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min, uint32_t tri_cfg) {
    extern __shared__ unsigned long long lds_stack[];
    __shared__ uint8_t perm_lut[2048];
    __shared__ PoolLds<MODE> pool;
    build_perm_lut(perm_lut);
    TravStack stk = make_trav_stack(lds_stack, sk);
    const QueueRef closest_q{closest_count, closest_head}, shadow_q{shadow_count, shadow_head};
    // the inline schedule carries both kinds of ray in one loop; the other schedules, and as a tuning variant the inline one too
    // (tri_cfg bit 0), run the two loops one after the other (every wave drains between the queues)
    // (the one loop in the else branch, not first behind an early return: there the compiler lays it out with its header block last,
    // two more taken branches per round - 2 % of the fused launch on the terrain scene, profiles/refactor_trace_loops.txt)
    if (MODE != TRI_INLINE || (tri_cfg & 1u)) {
        trace_one_queue<false, COUNT, MODE>(sc, st, queue, closest_q, stats, stk, perm_lut, pool, refill_min, tri_cfg, PT_STAT_SHADOW);
        trace_one_queue<true, COUNT, MODE>(sc, st, nullptr, shadow_q, stats, stk, perm_lut, pool, refill_min, tri_cfg, PT_STAT_FUSED_SHADOW);
    } else {
        trace_queue_inline<RAYS_BOTH, COUNT>(sc, st, queue, closest_q, shadow_q, stats, stk, perm_lut, refill_min, PT_STAT_FUSED_SHADOW);
    }
}

// ---- test hook: trace a batch of caller-supplied rays ---------------------------------------------
template <bool COUNT>
__device__ __forceinline__ void trace_one_ray(const PtScene& sc, const float* __restrict__ origins, const float* __restrict__ dirs, uint32_t i,
                                              int any_hit, float* __restrict__ t_out, int* __restrict__ tri_out, TravStack& stk, const uint8_t* perm_lut,
                                              TravCounters& tc) {
    const v3 o = mk(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]), d = mk(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
    if (any_hit) {
        Hit h{kShadowTmax, -1, 0u};
        const bool occ = traverse<true, COUNT>(sc, perm_lut, o, d, stk, h, tc);
        t_out[i] = occ ? 1.0f : 0.0f;
        tri_out[i] = occ ? 1 : 0;
    } else {
        Hit h{__builtin_inff(), -1, 0xffffffffu};
        traverse<false, COUNT>(sc, perm_lut, o, d, stk, h, tc);
        t_out[i] = h.t;
        tri_out[i] = h.li < 0 ? -1 : (int)h.id;
    }
}

// counts != nullptr: per-ray node fetches and triangle tests (counts[2i], counts[2i+1]) of the very step
// functions the render kernels run, for the host-side cross-check of the traversal statistics
template <bool COUNT>
__global__ __launch_bounds__(256) void pt_trace_rays(const PtScene sc, const float* __restrict__ origins, const float* __restrict__ dirs, uint32_t n,
                                                     int any_hit, float* __restrict__ t_out, int* __restrict__ tri_out, uint32_t* __restrict__ counts,
                                                     const StackCfg sk) {
    extern __shared__ unsigned long long lds_stack[];
    __shared__ uint8_t perm_lut[2048];
    build_perm_lut(perm_lut);
    // grid-stride so the spill columns (one per launched thread) stay within sk.spill_stride
    TravStack stk = make_trav_stack(lds_stack, sk);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        TravCounters tc{0, 0, 0};
        trace_one_ray<COUNT>(sc, origins, dirs, i, any_hit, t_out, tri_out, stk, perm_lut, tc);
        if (COUNT) {
            counts[2 * (size_t)i] = tc.nodes;
            counts[2 * (size_t)i + 1] = tc.tris;
        }
    }
}

// ---- ray queries on device arrays (rt_query_rays_device) -----------------------
// A lane of the query kernels' refilling loop (pt_query_loop.h): the queue is implicit (entry i is ray i of the
// caller's arrays), a retiring lane writes the caller's answer arrays.  Every ray is traced by start_ray / inline_round - node_step
// and tri_step inside - exactly as in the render kernels and in the hook, so the answers are theirs bit for bit.  Differences:
//   - a per-ray distance limit: r.tmax starts at it (boxes beyond it are culled from the start; a triangle inside a conservative
//     box may still be tested and accepted beyond it, which only moves r.tmax to that hit's t - never below min(limit, best.t), so no
//     hit nearer than the limit is lost) and the comparison at retire is the strict one: a closest hit at t >= limit is a miss;
//   - validity is decided when the lane loads the ray: an invalid ray is answered on the spot and the lane stays idle.  A refill may
//     therefore hand out 64 entries and leave no lane alive, and with few workgroups a stream may have no wave that started on it: a
//     wave leaves only when it has found the last stream dry AND holds no live ray (the rule of RAYS_BOTH, not of the one-kind loops).
// Hit attributes (ATTR, rt_query_rays_attr_device): the sink of a lane that retires a ray with a winner fetches
// the 48-byte record at best.li once more and evaluates hit_attr.h on the lane's own r.o, r.d - the values the accepting tri_step used,
// so u, v, det are its u, v, det bit for bit.  tri_step carries nothing new: it and the rounds are the plain kernels'.
// The attribute arrays come in an argument
// block of their own (RayAttrQuery), so the plain instantiations keep theirs and are the code of a kernel without ATTR (profiles/hit_attributes.txt).
template <bool ATTR>
using RayQueryOf = std::conditional_t<ATTR, RayAttrQuery, RayQuery>;

template <bool ANY, bool ATTR>
struct RayLane {
    const PtScene& sc;
    const RayQueryOf<ATTR>& q;
    const uint8_t* perm_lut;
    int tris_per_round;  // byte 1 of tune_refill_min
    TravStack stk;
    TravCounters tc{0, 0, 0};
    TRay r = make_tray(mk(0.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f), 0.0f);
    Hit best{0.0f, -1, 0u};
    Group G{0u, 0u}, T{0u, 0u};
    uint32_t ray = 0;      // index of this lane's ray
    float limit = 0.0f;    // its distance limit
    uint32_t invalid = 0;  // invalid rays this lane has met
    bool occluded = false;

    __device__ __forceinline__ void retire() {
        if (ANY) {
            q.tri_out[ray] = occluded ? 1 : 0;
            return;
        }
        const bool hit = best.li >= 0 && best.t < limit;
        q.t_out[ray] = hit ? best.t : __builtin_inff();
        q.tri_out[ray] = hit ? (int)best.id : RT_RAY_MISS;
        if constexpr (ATTR) {
            if (hit) {
                const float4* tp = sc.tris + (size_t)best.li * 3;
                const float4 ta = tp[0], tb = tp[1], tcw = tp[2];
                const P3 e1{ta.w, tb.x, tb.y}, e2{tb.z, tb.w, tcw.x};
                const Bary b = ray_bary(P3{r.o.x, r.o.y, r.o.z}, P3{r.d.x, r.d.y, r.d.z}, P3{ta.x, ta.y, ta.z}, e1, e2);
                write_attr(q.uv_out, q.normal_out, ray, b.u, b.v, unit_normal(e1, e2));
            } else {
                write_no_attr(q.uv_out, q.normal_out, ray);  // a miss, or a hit that its limit cuts off
            }
        }
    }

    __device__ __forceinline__ bool admit(uint32_t i) {
        const float* po = q.origins + (size_t)i * 3u;
        const float* pd = q.dirs + (size_t)i * 3u;
        const v3 o = mk(po[0], po[1], po[2]), d = mk(pd[0], pd[1], pd[2]);
        limit = q.tmax ? q.tmax[i] : ANY ? kShadowTmax : __builtin_inff();
        // (comparisons that are false for a NaN; +-inf origins fail the range test)
        const bool in_reach = __builtin_fabsf(o.x) <= q.reach && __builtin_fabsf(o.y) <= q.reach && __builtin_fabsf(o.z) <= q.reach;
        const bool d_finite = __builtin_fabsf(d.x) < __builtin_inff() && __builtin_fabsf(d.y) < __builtin_inff() && __builtin_fabsf(d.z) < __builtin_inff();
        if (!(in_reach && d_finite && limit == limit)) {  // not traced
            if (!ANY) q.t_out[i] = __builtin_nanf("");
            q.tri_out[i] = RT_RAY_INVALID;
            invalid++;
        } else if (!(limit > 0.0f)) {  // an empty interval: a miss without a walk
            if (!ANY) q.t_out[i] = __builtin_inff();
            q.tri_out[i] = ANY ? 0 : RT_RAY_MISS;
        } else {
            start_ray(ANY, o, d, r, best, G, T, stk);
            r.tmax = limit;
            ray = i;
            occluded = false;
            return true;
        }
        if constexpr (ATTR) write_no_attr(q.uv_out, q.normal_out, i);
        return false;
    }

    // (UNORDERED for any-hit rays, as in an all-shadow launch)
    __device__ __forceinline__ bool step(bool alive) {
        return inline_round<false, ANY>(sc, perm_lut, r, best, G, T, stk, tc, alive, occluded, ANY, tris_per_round, limit);
    }
};

template <bool ANY, bool ATTR>
__global__ __launch_bounds__(256, kInlineWaves) void pt_query_rays(const PtScene sc, const RayQueryOf<ATTR> q, uint32_t* __restrict__ head,
                                                                   unsigned long long* __restrict__ stats, const StackCfg sk, uint32_t refill_min) {
    static_assert(!(ANY && ATTR), "an occlusion query has no winner");
    extern __shared__ unsigned long long lds_stack[];  // sk.lds_cap x 256 entries
    __shared__ uint8_t perm_lut[2048];
    build_perm_lut(perm_lut);
    RayLane<ANY, ATTR> lane{sc, q, perm_lut, tris_per_round_of(refill_min), make_trav_stack(lds_stack, sk)};
    const uint32_t lane_id = threadIdx.x & 63u;
    RT_QUERY_LOOP(lane, q.n, head, refill_min & 0xffu, lane_id);
    add_wave_total(&stats[RQ_STAT_INVALID], lane.invalid, lane_id);
    if (lane.tc.overflow) atomicOr((unsigned int*)&stats[RQ_STAT_OVERFLOW], 1u);
}

// ---- launchers ------------------------------------------------------------------------------------
template <class F>
static void with_tri_mode(uint32_t tri_mode, F&& f) {
    if (tri_mode == TRI_POOL) f(std::integral_constant<int, TRI_POOL>{});
    else if (tri_mode == TRI_DEFER) f(std::integral_constant<int, TRI_DEFER>{});
    else if (tri_mode == TRI_INLINE_PF) f(std::integral_constant<int, TRI_INLINE_PF>{});
    else f(std::integral_constant<int, TRI_INLINE>{});
}

int launch_pt_trace(Ctx* c, hipStream_t stream, const PtScene& sc, const PtState& st, const uint32_t* queue, const uint32_t* count_ptr, uint32_t* head,
                    unsigned long long* stats, bool any_hit, bool count, uint32_t grid, const StackCfg& stack_cap, uint32_t refill_min, uint32_t tri_mode,
                    uint32_t tri_cfg) {
    if (!valid_stack_cfg(stack_cap, grid)) return c->fail(RT_ERR_INVALID, "bad traversal stack configuration");
    with_bool(any_hit, [&](auto any) {
        with_bool(count, [&](auto cnt) {
            with_tri_mode(tri_mode, [&](auto mode) {
                hipLaunchKernelGGL((pt_trace<decltype(any)::value, decltype(cnt)::value, decltype(mode)::value>), dim3(grid), dim3(256), stack_lds_bytes(stack_cap),
                                   stream, sc, st, queue, count_ptr, head, stats, stack_cap, refill_min, tri_cfg);
            });
        });
    });
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int launch_pt_trace_fused(Ctx* c, const PtScene& sc, const PtState& st, const uint32_t* queue, const uint32_t* closest_count, uint32_t* closest_head,
                          const uint32_t* shadow_count, uint32_t* shadow_head, unsigned long long* stats, bool count, uint32_t grid,
                          const StackCfg& stack_cap, uint32_t refill_min, uint32_t tri_mode, uint32_t tri_cfg) {
    if (!valid_stack_cfg(stack_cap, grid)) return c->fail(RT_ERR_INVALID, "bad traversal stack configuration");
    with_bool(count, [&](auto cnt) {
        with_tri_mode(tri_mode, [&](auto mode) {
            hipLaunchKernelGGL((pt_trace_fused<decltype(cnt)::value, decltype(mode)::value>), dim3(grid), dim3(256), stack_lds_bytes(stack_cap), c->stream, sc, st, queue,
                               closest_count, closest_head, shadow_count, shadow_head, stats, stack_cap, refill_min, tri_cfg);
        });
    });
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

uint32_t pt_pool_lds_bytes(uint32_t tri_mode) { return tri_mode == TRI_POOL ? kPoolLdsBytes : tri_mode == TRI_INLINE_PF ? kPfLdsBytes : 0u; }

int launch_pt_trace_rays(Ctx* c, const PtScene& sc, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out, int* tri_out,
                         uint32_t* counts, const StackCfg& sk, uint32_t grid) {
    if (!valid_stack_cfg(sk, grid)) return c->fail(RT_ERR_INVALID, "bad traversal stack configuration");
    with_bool(counts != nullptr, [&](auto cnt) {
        hipLaunchKernelGGL(pt_trace_rays<decltype(cnt)::value>, dim3(grid), dim3(256), stack_lds_bytes(sk), c->stream, sc, origins, dirs, n, any_hit, t_out, tri_out,
                           counts, sk);
    });
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int launch_pt_query_rays(Ctx* c, const PtScene& sc, const RayQuery& q, bool any_hit, uint32_t* head, unsigned long long* stats, uint32_t grid,
                         const StackCfg& sk, uint32_t refill_min) {
    QueryKernel<RayQuery> kernel = nullptr;
    with_bool(any_hit, [&](auto any) { kernel = pt_query_rays<decltype(any)::value, false>; });
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

int launch_pt_query_rays_attr(Ctx* c, const PtScene& sc, const RayAttrQuery& q, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                              uint32_t refill_min) {
    const QueryKernel<RayAttrQuery> kernel = pt_query_rays<false, true>;
    return launch_query(c, kernel, sc, q, head, stats, grid, sk, refill_min);
}

}  // namespace rt
