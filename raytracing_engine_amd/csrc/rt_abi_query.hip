// rt_abi_query.hip — C-ABI entry points of path B's queries on device arrays: rays, closest points (§6.14),
// sides (§6.15), all hits (§6.16), neighbours (§6.17), the attribute variants of the first two (§6.18), overlaps (§6.20) and their
// segments (§6.21: a flat kernel over a list, with an enqueue of its own), clearance (§6.22), k nearest (§6.23), sphere casts (§6.24).  Host code only.
// A kind is a parameter struct, its arrays, a launcher and its counters; its state in the context is a member of rt::Queries
// (rt_internal.h).  What the kinds share is written once here:
//   the refusals before a parameter struct is looked at (check_query_items) and those of the struct (check_query_params), the
//   prologue of an entry (enter_query, or use_params .. begin_query around a check of the entry's own);
//   the array checks: check_arrays over a list of {pointer, bytes, name, required};
//   a kind's first use (ensure_block), scratch that grows by size class (grow_scratch), the plan and the enqueue (prepare_query,
//   run_query);
//   the read-back: query_stats over a kind's table of (member, counter word).
// A single-answer kind - rays, points, sides, clearance, k nearest, sphere casts - is prepare_* (the array checks, the query struct, the plan:
// everything that can refuse) and run_* (the launch and the host's part of the statistics); its entry is the prologue, prepare, run,
// and rt_query_signed_distance_device is two prepares and then two runs.  The listing kinds - all hits, neighbours, overlaps - are a
// description each (HitKind, NeighborKind, OverlapKind); their protocol of a count step, a fill step or both in one call is
// listing_call, and their read-back is listing_stats.
#include <algorithm>
#include <initializer_list>

#include "rt_internal.h"
#include "rt_roctx.h"

using rt::Ctx;
using rt::QueryState;

namespace {

constexpr uint32_t kMaxQueryItems = 1u << 30;  // stream_entry() of a dry reservation stays below 2^32
constexpr uint32_t kQueryRefillMin = 24;       // idle lanes per wave that trigger a refill in the query kernels (the render kernels' default)

// What every call is checked for first, whatever its parameters
int check_query_items(Ctx* c, uint32_t n) {
    if (!c->pt.mesh().n_tris) return c->fail(RT_ERR_STATE, "rt_set_mesh has not been called");
    if (int rc = rt::check_mesh_domain(c, c->pt.mesh())) return rc;
    if (n > kMaxQueryItems) return c->fail(RT_ERR_INVALID, "n %u is above 2^30", n);
    return RT_OK;
}

// What every parameter struct is checked for, in the order the refusals have: `flag` is the kind's own switch (any_hit, count_traversal)
template <class Params>
int check_query_params(Ctx* c, uint32_t n, const Params& prm, uint32_t flag, const char* flag_name) {
    if (int rc = check_query_items(c, n)) return rc;
    if (flag > 1u) return c->fail(RT_ERR_INVALID, "%s %u (0 or 1)", flag_name, flag);
    if ((prm.tune_refill_min & 0xffu) > 64u || prm.tune_refill_min > 0xffffu) return c->fail(RT_ERR_INVALID, "tune_refill_min %u (low byte 0 .. 64)", prm.tune_refill_min);
    if (prm.tune_blocks_per_cu > 8u) return c->fail(RT_ERR_INVALID, "tune_blocks_per_cu %u (0 .. 8)", prm.tune_blocks_per_cu);
    if (prm.tune_lds_stack > 78u) return c->fail(RT_ERR_INVALID, "tune_lds_stack %u (0 .. 78)", prm.tune_lds_stack);
    return RT_OK;
}

// The prologue of an entry, in two parts for the entries that have something between them (a second parameter struct, k).
// use_params: the defaults for a NULL struct, then check_query_params.  begin_query: n == 0 is *done (the caller returns RT_OK), else
// the context's device is bound.
template <class Params>
int use_params(Ctx* c, uint32_t n, const Params*& prm, const Params& defaults, uint32_t Params::*flag = &Params::count_traversal, const char* flag_name = "count_traversal") {
    if (!prm) prm = &defaults;
    return check_query_params(c, n, *prm, prm->*flag, flag_name);
}

int begin_query(Ctx* c, uint32_t n, int* done) {
    *done = n == 0;
    return *done ? RT_OK : rt::bind(c);
}

template <class Params>
int enter_query(Ctx* c, uint32_t n, const Params*& prm, const Params& defaults, int* done, uint32_t Params::*flag = &Params::count_traversal,
                const char* flag_name = "count_traversal") {
    if (int rc = use_params(c, n, prm, defaults, flag, flag_name)) return rc;
    return begin_query(c, n, done);
}

template <class Params>
int default_params(Params* p) {
    if (!p) return RT_ERR_INVALID;
    *p = Params{};
    return RT_OK;
}

// One array of a call: `bytes` of device memory of the context's device behind p; an array that is not required may be NULL
struct ArrayArg {
    const void* p;
    size_t bytes;
    const char* name;
    bool required = true;
};

// The arrays in list order; the first refusal is the call's
int check_arrays(Ctx* c, std::initializer_list<ArrayArg> arrays) {
    for (const ArrayArg& a : arrays)
        if (a.p || a.required)
            if (int rc = rt::check_device_array(c, a.p, a.bytes, a.name)) return rc;
    return RT_OK;
}

// A kind's first use: its device block and the two events, all of them or none (a first use that fails leaves the next query of the
// kind to try again from nothing).  `part`: what the kind has in the block, for the message
int ensure_block(Ctx* c, QueryState& qs, const char* part) {
    if (qs.block) return RT_OK;
    rt::DevPtr<char> block;
    rt::Event ev[2];
    if (!dalloc(block, rt::query_block_bytes(qs.n_counters))) return c->fail(RT_ERR_OOM, "%s %s", qs.name, part);
    for (rt::Event& e : ev) RT_HIP_AS(c, rt::kTextEventCreate, rt::make_event(e));
    qs.block = std::move(block);
    qs.ev[0] = std::move(ev[0]);
    qs.ev[1] = std::move(ev[1]);
    return RT_OK;
}

// Scratch of at least `need` words, by size class (powers of two)
template <class T>
int grow_scratch(Ctx* c, rt::Scratch<T>& s, size_t need, const char* what) {
    if (need <= s.words) return RT_OK;
    size_t words = 4096;
    while (words < need) words *= 2;
    RT_HIP(c, hipStreamSynchronize(c->stream));  // an earlier call may still be working in the old one
    s.words = 0;
    if (!rt::dalloc(s.d, words)) return c->fail(RT_ERR_OOM, "%s (%zu words)", what, words);
    s.words = words;
    return RT_OK;
}

// A query that nothing can refuse any more: its stack, its persistent grid, its refill threshold
struct QueryPlan {
    rt::StackCfg sk;
    uint32_t grid, refill_min;
};

// After the kind's array checks, what can still refuse: the device block and the events (first query of the kind), the stack of
// stack_need entries per lane.  max_grid: what the kernel's register budget keeps resident, where that is less than the stack's
// figure (0: no such bound).  Enqueues nothing and writes nothing the caller can see.
template <class Params>
int prepare_query(Ctx* c, QueryState& qs, uint32_t n, const Params& prm, uint32_t stack_need, QueryPlan* plan, uint32_t max_grid = 0) {
    if (int rc = ensure_block(c, qs, "stream heads")) return rc;
    plan->sk = rt::StackCfg{};
    plan->grid = 0;
    if (int rc = rt::pt_stack_config(c, stack_need, qs.fixed_lds_bytes, qs.spill_halves, prm.tune_lds_stack, prm.tune_blocks_per_cu, (uint64_t)n, &plan->sk, &plan->grid)) return rc;
    plan->grid = std::min<uint32_t>(plan->grid, (n + 255u) / 256u);
    if (prm.tune_max_blocks) plan->grid = std::min<uint32_t>(plan->grid, prm.tune_max_blocks);
    if (max_grid) plan->grid = std::min<uint32_t>(plan->grid, max_grid);
    plan->refill_min = prm.tune_refill_min & 0xffu ? prm.tune_refill_min & 0xffu : kQueryRefillMin;
    return RT_OK;
}

// The enqueue: clear the block, launch(head, stats, grid, stack, refill_min's low byte) between the two events, remember that there
// is something to read.  The spill columns are taken now: a plan made before another kind's plan grew them still launches on what is there.
// A call of two walks (a listing kind's list) is first = true, last = false and then first = false, last = true: the second walk clears
// the stream heads only - its counters are words the first did not touch - and the events enclose both.
template <class Launch>
int run_query(Ctx* c, QueryState& qs, QueryPlan plan, const char* range, Launch&& launch, bool first = true, bool last = true) {
    plan.sk.spill = c->pt.d_spill.get();
    uint32_t* head = reinterpret_cast<uint32_t*>(qs.block.get());
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(qs.block.get() + rt::kQueryHeadBytes);
    rt::RoctxRange rr(range);
    RT_HIP(c, hipMemsetAsync(qs.block.get(), 0, first ? rt::query_block_bytes(qs.n_counters) : rt::kQueryHeadBytes, c->stream));
    if (first) RT_HIP(c, hipEventRecord(qs.ev[0].get(), c->stream));
    if (int rc = launch(head, stats, plan.grid, plan.sk, plan.refill_min)) return rc;
    if (last) RT_HIP(c, hipEventRecord(qs.ev[1].get(), c->stream));
    qs.pending = true;
    return RT_OK;
}

// ---- the read-back ----
// The pending query's qs.n_counters counters and its time (waits for it)
constexpr uint32_t kMaxStatWords = rt::LQ_STAT_WORDS;
static_assert(rt::RQ_STAT_WORDS <= kMaxStatWords && rt::PQ_STAT_WORDS <= kMaxStatWords && rt::SQ_STAT_WORDS <= kMaxStatWords && rt::SG_STAT_WORDS <= kMaxStatWords &&
                  rt::CQ_STAT_WORDS <= kMaxStatWords && rt::KQ_STAT_WORDS <= kMaxStatWords && rt::WQ_STAT_WORDS <= kMaxStatWords,
              "read_query's callers hold kMaxStatWords words");

int read_query(Ctx* c, QueryState& qs, unsigned long long* counters, float* ms) {
    if (int rc = rt::bind(c)) return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    RT_HIP(c, hipMemcpy(counters, qs.block.get() + rt::kQueryHeadBytes, qs.n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    RT_HIP(c, hipEventElapsedTime(ms, qs.ev[0].get(), qs.ev[1].get()));
    qs.pending = false;
    return RT_OK;
}

// Where a counter word of a kind's block goes in its public struct: a 64-bit member, or the 32-bit stack_overflow
template <class Stats>
struct StatWord {
    constexpr StatWord(uint64_t Stats::*m, uint32_t w) : m64(m), m32(nullptr), word(w) {}
    constexpr StatWord(uint32_t Stats::*m, uint32_t w) : m64(nullptr), m32(m), word(w) {}
    uint64_t Stats::*m64;
    uint32_t Stats::*m32;
    uint32_t word;
};

// rt_get_*_query_stats of a single-answer kind: the counters of the pending query, if there is one, into the context's copy by the
// kind's table (derive: what the kind computes from them), then the copy - it stays, so a second call returns the same
template <class Stats, size_t N>
int query_stats(rt_ctx* ctx, rt::QueryKind<Stats> rt::Queries::*kind, const StatWord<Stats> (&table)[N], Stats* stats, void (*derive)(Stats&) = nullptr) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !stats) return RT_ERR_INVALID;
    rt::QueryKind<Stats>& k = c->pt.queries.*kind;
    Stats& s = k.stats;
    if (k.qs.pending) {
        unsigned long long w[kMaxStatWords] = {};
        if (int rc = read_query(c, k.qs, w, &s.ms)) return rc;
        for (const StatWord<Stats>& t : table) {
            if (t.m64)
                s.*t.m64 = w[t.word];
            else
                s.*t.m32 = (uint32_t)w[t.word];
        }
        if (derive) derive(s);
    }
    *stats = s;
    return RT_OK;
}

// (the members the host sets at the enqueue - the item count, launches - are not the counters')
using RayStats = rt_ray_query_stats;
using PointStats = rt_point_query_stats;
using SideStats = rt_side_query_stats;
using ClearanceStats = rt_clearance_query_stats;
using KnnStats = rt_knn_query_stats;
using SegmentStats = rt_overlap_segment_stats;
using SweepStats = rt_sweep_query_stats;
constexpr StatWord<RayStats> kRayStats[] = {{&RayStats::invalid_rays, rt::RQ_STAT_INVALID}, {&RayStats::stack_overflow, rt::RQ_STAT_OVERFLOW}};
constexpr StatWord<PointStats> kPointStats[] = {{&PointStats::invalid_points, rt::PQ_STAT_INVALID}, {&PointStats::stack_overflow, rt::PQ_STAT_OVERFLOW},
                                                {&PointStats::nodes_visited, rt::PQ_STAT_NODES}, {&PointStats::tris_tested, rt::PQ_STAT_TRIS}};
constexpr StatWord<SideStats> kSideStats[] = {{&SideStats::invalid_points, rt::SQ_STAT_INVALID}, {&SideStats::skipped_points, rt::SQ_STAT_SKIPPED},
                                              {&SideStats::walks, rt::SQ_STAT_WALKS}, {&SideStats::third_walks, rt::SQ_STAT_THIRD},
                                              {&SideStats::stack_overflow, rt::SQ_STAT_OVERFLOW}, {&SideStats::nodes_visited, rt::SQ_STAT_NODES},
                                              {&SideStats::tris_tested, rt::SQ_STAT_TRIS}};
constexpr StatWord<ClearanceStats> kClearanceStats[] = {{&ClearanceStats::invalid_triangles, rt::CQ_STAT_INVALID}, {&ClearanceStats::stack_overflow, rt::CQ_STAT_OVERFLOW},
                                                        {&ClearanceStats::nodes_visited, rt::CQ_STAT_NODES}, {&ClearanceStats::tris_tested, rt::CQ_STAT_TRIS}};
constexpr StatWord<KnnStats> kKnnStats[] = {{&KnnStats::invalid_points, rt::KQ_STAT_INVALID}, {&KnnStats::neighbors, rt::KQ_STAT_NEIGHBORS},
                                            {&KnnStats::stack_overflow, rt::KQ_STAT_OVERFLOW}, {&KnnStats::nodes_visited, rt::KQ_STAT_NODES},
                                            {&KnnStats::tris_tested, rt::KQ_STAT_TRIS}};
constexpr StatWord<SweepStats> kSweepStats[] = {{&SweepStats::invalid_sweeps, rt::WQ_STAT_INVALID}, {&SweepStats::hits, rt::WQ_STAT_HITS},
                                                {&SweepStats::stack_overflow, rt::WQ_STAT_OVERFLOW}, {&SweepStats::nodes_visited, rt::WQ_STAT_NODES},
                                                {&SweepStats::tris_tested, rt::WQ_STAT_TRIS}};
constexpr StatWord<SegmentStats> kSegmentStats[] = {{&SegmentStats::entries, rt::SG_STAT_ENTRIES}, {&SegmentStats::touches, rt::SG_STAT_TOUCHES},
                                                    {&SegmentStats::skipped_incomplete, rt::SG_STAT_SKIPPED}, {&SegmentStats::bad_entries, rt::SG_STAT_BAD}};

void derive_segments(rt_overlap_segment_stats& s) {
    s.segments = s.entries - s.touches - s.skipped_incomplete - s.bad_entries;  // every entry is one of the four
}

// ---- rays: rt_query_rays_device and, with attr, rt_query_rays_attr_device ----
// prepare_*: the array checks and the plan - everything that can refuse a call comes before the first enqueue; run_*: the enqueue
int prepare_rays(Ctx* c, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_ray_query_params& prm, void* t_out, void* tri_out, bool attr,
                 void* uv_out, void* normal_out, rt::RayAttrQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    const bool any_hit = prm.any_hit != 0u;
    if (attr && any_hit) return c->fail(RT_ERR_INVALID, "any_hit 1 with an attribute query: an occlusion has no winner");
    if (int rc = check_arrays(c, {{origins, (size_t)n * 12, "origins_dev"}, {dirs, (size_t)n * 12, "dirs_dev"}, {tmax, (size_t)n * 4, "tmax_dev", false},
                                  {t_out, (size_t)n * 4, "t_out_dev", !any_hit}, {tri_out, (size_t)n * 4, "tri_out_dev"}, {uv_out, (size_t)n * 8, "uv_out_dev", false},
                                  {normal_out, (size_t)n * 12, "normal_out_dev", false}}))
        return rc;
    *q = rt::RayAttrQuery{};
    q->origins = static_cast<const float*>(origins);
    q->dirs = static_cast<const float*>(dirs);
    q->tmax = static_cast<const float*>(tmax);
    q->t_out = any_hit ? nullptr : static_cast<float*>(t_out);
    q->tri_out = static_cast<int*>(tri_out);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    q->uv_out = static_cast<float*>(uv_out);
    q->normal_out = static_cast<float*>(normal_out);
    return prepare_query(c, c->pt.queries.rays.qs, n, prm, mesh.stack_need, plan);  // one group per level
}

int run_rays(Ctx* c, const rt::RayAttrQuery& q, const rt_ray_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_ray_query_stats>& k = c->pt.queries.rays;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        const uint32_t refill = refill_min | (prm.tune_refill_min & 0xff00u);  // byte 1: triangle tests per round
        if (q.uv_out || q.normal_out) return rt::launch_pt_query_rays_attr(c, rt::scene_view(c->pt.mesh()), q, head, stats, grid, sk, refill);
        return rt::launch_pt_query_rays(c, rt::scene_view(c->pt.mesh()), q, prm.any_hit != 0u, head, stats, grid, sk, refill);  // without attribute arrays: the plain query
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_rays", launch)) return rc;
    k.stats = rt_ray_query_stats{};
    k.stats.rays = q.n;
    k.stats.launches = 1;
    return RT_OK;
}

int query_rays(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_ray_query_params* prm, void* t_out, void* tri_out, bool attr,
               void* uv_out, void* normal_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_ray_query_params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done, &rt_ray_query_params::any_hit, "any_hit")) return rc;
    if (done) return RT_OK;
    rt::RayAttrQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_rays(c, origins, dirs, tmax, n, *prm, t_out, tri_out, attr, uv_out, normal_out, &q, &plan)) return rc;
    return run_rays(c, q, *prm, plan);
}

// ---- closest points (uv_out, normal_out: rt_query_points_attr_device's, NULL from every other entry) ----
int prepare_points(Ctx* c, const void* points, const void* rmax, uint32_t n, const rt_point_query_params& prm, void* dist_out, void* tri_out, void* point_out,
                   void* uv_out, void* normal_out, rt::PointAttrQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{points, (size_t)n * 12, "points_dev"}, {rmax, (size_t)n * 4, "rmax_dev", false}, {dist_out, (size_t)n * 4, "dist_out_dev"},
                                  {tri_out, (size_t)n * 4, "tri_out_dev"}, {point_out, (size_t)n * 12, "point_out_dev", false},
                                  {uv_out, (size_t)n * 8, "uv_out_dev", false}, {normal_out, (size_t)n * 12, "normal_out_dev", false}}))
        return rc;
    *q = rt::PointAttrQuery{};
    q->points = static_cast<const float*>(points);
    q->rmax = static_cast<const float*>(rmax);
    q->dist_out = static_cast<float*>(dist_out);
    q->tri_out = static_cast<int*>(tri_out);
    q->point_out = static_cast<float*>(point_out);
    q->uv_out = static_cast<float*>(uv_out);
    q->normal_out = static_cast<float*>(normal_out);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // point_stack_need entries per lane: one pending sibling each, not stack_need's one group per level; the spill columns grow to it once per mesh
    return prepare_query(c, c->pt.queries.points.qs, n, prm, rt::point_stack_need(mesh.depth), plan);
}

int run_points(Ctx* c, const rt::PointAttrQuery& q, const rt_point_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_point_query_stats>& k = c->pt.queries.points;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        if (q.uv_out || q.normal_out) return rt::launch_pt_query_points_attr(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);
        return rt::launch_pt_query_points(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_points", launch)) return rc;
    k.stats = rt_point_query_stats{};
    k.stats.points = q.n;
    k.stats.launches = 1;
    return RT_OK;
}

// ---- sides (need_inside: the entry of its own; the signed distance may go without inside_out) ----
int prepare_sides(Ctx* c, const void* points, uint32_t n, const rt_side_query_params& prm, void* inside_out, bool need_inside, void* crossings_out, void* dist_inout,
                  rt::SideQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{points, (size_t)n * 12, "points_dev"}, {inside_out, (size_t)n * 4, "inside_out_dev", need_inside},
                                  {crossings_out, (size_t)n * 12, "crossings_out_dev", false}, {dist_inout, (size_t)n * 4, "dist_inout_dev", false}}))
        return rc;
    *q = rt::SideQuery{};
    q->points = static_cast<const float*>(points);
    q->inside_out = static_cast<int*>(inside_out);
    q->crossings_out = static_cast<int*>(crossings_out);
    q->dist_inout = static_cast<float*>(dist_inout);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    return prepare_query(c, c->pt.queries.sides.qs, n, prm, mesh.stack_need, plan);  // a ray walk: one group per level
}

int run_sides(Ctx* c, const rt::SideQuery& q, const rt_side_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_side_query_stats>& k = c->pt.queries.sides;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return rt::launch_pt_query_sides(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_sides", launch)) return rc;
    k.stats = rt_side_query_stats{};
    k.stats.points = q.n;
    k.stats.launches = 1;
    return RT_OK;
}

// ---- clearance ----
int prepare_clearance(Ctx* c, const void* tris, const void* rmax, uint32_t n, const rt_clearance_query_params& prm, void* tri_out, void* dist_out, void* point_query_out,
                      void* point_mesh_out, rt::ClearanceQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{tris, (size_t)n * 36, "tris_dev"}, {rmax, (size_t)n * 4, "rmax_dev", false}, {tri_out, (size_t)n * 4, "tri_out_dev"},
                                  {dist_out, (size_t)n * 4, "dist_out_dev"}, {point_query_out, (size_t)n * 12, "point_query_out_dev", false},
                                  {point_mesh_out, (size_t)n * 12, "point_mesh_out_dev", false}}))
        return rc;
    *q = rt::ClearanceQuery{};
    q->tris = static_cast<const float*>(tris);
    q->rmax = static_cast<const float*>(rmax);
    q->tri_out = static_cast<int*>(tri_out);
    q->dist_out = static_cast<float*>(dist_out);
    q->point_query_out = static_cast<float*>(point_query_out);
    q->point_mesh_out = static_cast<float*>(point_mesh_out);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // the points' walk: point_stack_need entries per lane; the grid is what the kernel's register budget keeps resident
    return prepare_query(c, c->pt.queries.clearance.qs, n, prm, rt::point_stack_need(mesh.depth), plan, (uint32_t)c->n_cus * (uint32_t)rt::kClearanceWaves);
}

int run_clearance(Ctx* c, const rt::ClearanceQuery& q, const rt_clearance_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_clearance_query_stats>& k = c->pt.queries.clearance;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return rt::launch_pt_query_clearance(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_clearance", launch)) return rc;
    k.stats = rt_clearance_query_stats{};
    k.stats.queries = q.n;
    return RT_OK;
}

// ---- k nearest: the points' inputs, rows of k ----
int prepare_knn(Ctx* c, const void* points, const void* rmax, uint32_t n, uint32_t k, const rt_knn_query_params& prm, void* dist_out, void* tri_out, void* count_out,
                rt::KnnQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{points, (size_t)n * 12, "points_dev"}, {rmax, (size_t)n * 4, "rmax_dev", false}, {dist_out, (size_t)n * k * 4, "dist_out_dev"},
                                  {tri_out, (size_t)n * k * 4, "tri_out_dev"}, {count_out, (size_t)n * 4, "count_out_dev", false}}))
        return rc;
    *q = rt::KnnQuery{};
    q->points = static_cast<const float*>(points);
    q->rmax = static_cast<const float*>(rmax);
    q->dist_out = static_cast<float*>(dist_out);
    q->tri_out = static_cast<int*>(tri_out);
    q->count_out = static_cast<int*>(count_out);
    q->n = n;
    q->k = k;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // the points' walk: point_stack_need entries per lane, so the spill columns grow no further than the point query grows them
    return prepare_query(c, c->pt.queries.knn.qs, n, prm, rt::point_stack_need(mesh.depth), plan);
}

int run_knn(Ctx* c, const rt::KnnQuery& q, const rt_knn_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_knn_query_stats>& k = c->pt.queries.knn;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return rt::launch_pt_query_knn(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_knn", launch)) return rc;
    k.stats = rt_knn_query_stats{};
    k.stats.points = q.n;
    k.stats.launches = 1;
    return RT_OK;
}

// ---- sphere casts: the rays' inputs and a radius each ----
int prepare_sweeps(Ctx* c, const void* origins, const void* dirs, const void* radius, const void* tmax, uint32_t n, const rt_sweep_query_params& prm, void* t_out,
                   void* tri_out, void* point_out, rt::SweepQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{origins, (size_t)n * 12, "origins_dev"}, {dirs, (size_t)n * 12, "dirs_dev"}, {radius, (size_t)n * 4, "radius_dev"},
                                  {tmax, (size_t)n * 4, "tmax_dev", false}, {t_out, (size_t)n * 4, "t_out_dev"}, {tri_out, (size_t)n * 4, "tri_out_dev"},
                                  {point_out, (size_t)n * 12, "point_out_dev", false}}))
        return rc;
    *q = rt::SweepQuery{};
    q->origins = static_cast<const float*>(origins);
    q->dirs = static_cast<const float*>(dirs);
    q->radius = static_cast<const float*>(radius);
    q->tmax = static_cast<const float*>(tmax);
    q->t_out = static_cast<float*>(t_out);
    q->tri_out = static_cast<int*>(tri_out);
    q->point_out = static_cast<float*>(point_out);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // the points' walk: point_stack_need entries per lane; the grid is what the kernel's register budget keeps resident
    return prepare_query(c, c->pt.queries.sweeps.qs, n, prm, rt::point_stack_need(mesh.depth), plan, (uint32_t)c->n_cus * (uint32_t)rt::kSweepWaves);
}

int run_sweeps(Ctx* c, const rt::SweepQuery& q, const rt_sweep_query_params& prm, const QueryPlan& plan) {
    rt::QueryKind<rt_sweep_query_stats>& k = c->pt.queries.sweeps;
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return rt::launch_pt_query_sweeps(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    if (int rc = run_query(c, k.qs, plan, "rt.path_b.query_sweeps", launch)) return rc;
    k.stats = rt_sweep_query_stats{};
    k.stats.sweeps = q.n;
    k.stats.launches = 1;
    return RT_OK;
}

// ---- the listing kinds: all hits, neighbours and overlaps.  The kinds' own array checks, then what they are to the shared protocol ----
struct RaySource {
    const void *origins, *dirs, *tmax;
};
struct PointSource {
    const void *points, *rmax;
    float rmax_all;
};
struct TriSource {
    const void* tris;
};

int prepare_hits(Ctx* c, const RaySource& src, uint32_t n, const rt_hit_query_params& prm, rt::HitQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{src.origins, (size_t)n * 12, "origins_dev"}, {src.dirs, (size_t)n * 12, "dirs_dev"}, {src.tmax, (size_t)n * 4, "tmax_dev", false}})) return rc;
    *q = rt::HitQuery{};
    q->origins = static_cast<const float*>(src.origins);
    q->dirs = static_cast<const float*>(src.dirs);
    q->tmax = static_cast<const float*>(src.tmax);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    return prepare_query(c, c->pt.queries.hits.qs, n, prm, mesh.stack_need, plan);  // a ray walk: one group per level
}

// pt_query_points' inputs
int prepare_neighbors(Ctx* c, const PointSource& src, uint32_t n, const rt_neighbor_query_params& prm, rt::NeighborQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{src.points, (size_t)n * 12, "points_dev"}, {src.rmax, (size_t)n * 4, "rmax_dev", false}})) return rc;
    *q = rt::NeighborQuery{};
    q->points = static_cast<const float*>(src.points);
    q->rmax = static_cast<const float*>(src.rmax);
    q->rmax_all = src.rmax_all;
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // a group walk like the rays': one pending sibling group per level, so the spill columns are the ray kinds' 
    return prepare_query(c, c->pt.queries.neighbors.qs, n, prm, mesh.stack_need, plan);
}

// the caller's triangles: nine floats each
int prepare_overlaps(Ctx* c, const TriSource& src, uint32_t n, const rt_overlap_query_params& prm, rt::OverlapQuery* q, QueryPlan* plan) {
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_arrays(c, {{src.tris, (size_t)n * 36, "tris_dev"}})) return rc;
    *q = rt::OverlapQuery{};
    q->tris = static_cast<const float*>(src.tris);
    q->n = n;
    q->reach = rt::kCameraReach * mesh.maxabs;
    // a group walk like the neighbours': one pending sibling group per level; the grid is what the kernel's register budget keeps resident
    return prepare_query(c, c->pt.queries.overlaps.qs, n, prm, mesh.stack_need, plan, (uint32_t)c->n_cus * (uint32_t)rt::kOverlapWaves);
}

struct HitKind {
    using Source = RaySource;
    using Query = rt::HitQuery;
    using Params = rt_hit_query_params;
    using Stats = rt_hit_query_stats;
    static constexpr auto prepare = prepare_hits;
    static constexpr auto launch = rt::launch_pt_query_hits;
    static constexpr auto state = &rt::Queries::hits;
    static constexpr const char *count_range = "rt.path_b.count_ray_hits", *fill_range = "rt.path_b.fill_ray_hits", *key_name = "t_out_dev";
    static constexpr auto items = &Stats::rays, invalid = &Stats::invalid_rays, found = &Stats::hits, written = &Stats::hits_written, incomplete = &Stats::incomplete_rays;
};
struct NeighborKind {
    using Source = PointSource;
    using Query = rt::NeighborQuery;
    using Params = rt_neighbor_query_params;
    using Stats = rt_neighbor_query_stats;
    static constexpr auto prepare = prepare_neighbors;
    static constexpr auto launch = rt::launch_pt_query_neighbors;
    static constexpr auto state = &rt::Queries::neighbors;
    static constexpr const char *count_range = "rt.path_b.count_neighbors", *fill_range = "rt.path_b.fill_neighbors", *key_name = "dist_out_dev";
    static constexpr auto items = &Stats::points, invalid = &Stats::invalid_points, found = &Stats::neighbors, written = &Stats::neighbors_written,
                          incomplete = &Stats::incomplete_points;
};

struct OverlapKind {  // the second entry array holds the edge masks (i32), keyed "edges_out_dev"
    using Source = TriSource;
    using Query = rt::OverlapQuery;
    using Params = rt_overlap_query_params;
    using Stats = rt_overlap_query_stats;
    static constexpr auto prepare = prepare_overlaps;
    static constexpr auto launch = rt::launch_pt_query_overlaps;
    static constexpr auto state = &rt::Queries::overlaps;
    static constexpr const char *count_range = "rt.path_b.count_overlaps", *fill_range = "rt.path_b.fill_overlaps", *key_name = "edges_out_dev";
    static constexpr auto items = &Stats::triangles, invalid = &Stats::invalid_triangles, found = &Stats::overlaps, written = &Stats::overlaps_written,
                          incomplete = &Stats::incomplete_triangles;
};

// ---- the listing protocol: the count step (walk, then the scan into offsets_out) and the fill step ----
struct ListScan {  // where the scan's scratch lies in Queries::list_scan
    unsigned long long *counts, *sums, *total;
};

// The count step's outputs and, with offsets_out, the scan's scratch: n + 1 counts, the tile sums, the total
int prepare_count(Ctx* c, uint32_t n, void* count_out, void* offsets_out, ListScan* ls) {
    if (!count_out && !offsets_out) return c->fail(RT_ERR_INVALID, "count_out_dev and offsets_out_dev are both NULL");
    if (int rc = check_arrays(c, {{count_out, (size_t)n * 4, "count_out_dev", false}, {offsets_out, ((size_t)n + 1) * 8, "offsets_out_dev", false}})) return rc;
    *ls = ListScan{};
    if (!offsets_out) return RT_OK;
    rt::Scratch<unsigned long long>& scan = c->pt.queries.list_scan;
    if (int rc = grow_scratch(c, scan, (size_t)n + 1 + rt::scan_u64_sums_words((size_t)n + 1) + 1, "hit-query scan scratch")) return rc;
    ls->counts = scan.d.get();
    ls->sums = ls->counts + (size_t)n + 1;
    ls->total = ls->sums + rt::scan_u64_sums_words((size_t)n + 1);
    return RT_OK;
}

int prepare_fill(Ctx* c, uint32_t n, const void* offsets, uint64_t capacity, void* key_out, void* tri_out, bool offsets_checked, const char* key_name) {
    if (capacity > (uint64_t)1 << 40) return c->fail(RT_ERR_INVALID, "capacity %llu is above 2^40", (unsigned long long)capacity);
    if (!offsets_checked)
        if (int rc = check_arrays(c, {{offsets, ((size_t)n + 1) * 8, "offsets_in_dev"}})) return rc;
    return check_arrays(c, {{key_out, (size_t)capacity * 4, key_name, capacity != 0}, {tri_out, (size_t)capacity * 4, "tri_out_dev", capacity != 0}});
}

template <class K>
int run_count(Ctx* c, typename K::Query q, const typename K::Params& prm, const QueryPlan& plan, void* count_out, void* offsets_out, const ListScan& ls, bool last) {
    rt::ListingKind<typename K::Stats>& st = c->pt.queries.*K::state;
    q.count_out = static_cast<int*>(count_out);
    q.count64 = ls.counts;
    if (ls.counts) RT_HIP(c, hipMemsetAsync(ls.counts + q.n, 0, sizeof(unsigned long long), c->stream));  // entry n: offsets[n] = the total
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return K::launch(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, false, head, stats, grid, sk, refill_min);  // (byte 1 has no meaning here)
    };
    // the scan lies between the events too: it is part of the step
    if (int rc = run_query(c, st.qs, plan, K::count_range, launch, true, false)) return rc;
    st.steps |= 1u;
    st.stats.launches += 1;
    if (ls.counts) {
        if (int rc = rt::scan_u64_device(c, ls.counts, static_cast<unsigned long long*>(offsets_out), (size_t)q.n + 1, ls.sums, ls.total)) return rc;
        st.stats.launches += 3;
    }
    if (last) RT_HIP(c, hipEventRecord(st.qs.ev[1].get(), c->stream));
    return RT_OK;
}

template <class K>
int run_fill(Ctx* c, typename K::Query q, const typename K::Params& prm, const QueryPlan& plan, const void* offsets, uint64_t capacity, void* key_out, void* tri_out,
             bool first) {
    rt::ListingKind<typename K::Stats>& st = c->pt.queries.*K::state;
    q.offsets = static_cast<const long long*>(offsets);
    q.capacity = (long long)capacity;
    q.key_out = static_cast<decltype(q.key_out)>(key_out);  // f32 keys, or the overlaps' i32 masks: four bytes an entry either way
    q.tri_out = static_cast<int*>(tri_out);
    const auto launch = [&](uint32_t* head, unsigned long long* stats, uint32_t grid, const rt::StackCfg& sk, uint32_t refill_min) {
        return K::launch(c, rt::scene_view(c->pt.mesh()), q, prm.count_traversal != 0u, true, head, stats + rt::LQ_STEP_WORDS, grid, sk, refill_min);
    };
    if (int rc = run_query(c, st.qs, plan, K::fill_range, launch, first, true)) return rc;
    st.steps |= 2u;
    st.stats.launches += 1;
    return RT_OK;
}

// A call of a listing kind.  steps = 1: the count step (count_out, offsets_out), 2: the fill step on the caller's offsets, 3: the
// list call - the count step, then the fill step on its offsets_out, one plan for the two walks (the same kind on the same items)
// and one pair of events around both.  Both steps' refusals and first-use allocations come before the first enqueue.
template <class K>
int listing_call(rt_ctx* ctx, const typename K::Source& src, uint32_t n, const typename K::Params* prm, uint32_t steps, void* count_out, void* offsets_out,
                 const void* offsets_in, uint64_t capacity, void* key_out, void* tri_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const typename K::Params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done)) return rc;
    if (done) return RT_OK;
    const bool count = steps & 1u, fill = steps & 2u;
    typename K::Query q{};
    QueryPlan plan{};
    ListScan ls{};
    if (count && fill) {
        if (!offsets_out) return c->fail(RT_ERR_INVALID, "offsets_out_dev is NULL");
        offsets_in = offsets_out;
    }
    if (count)
        if (int rc = prepare_count(c, n, count_out, offsets_out, &ls)) return rc;
    if (fill)
        if (int rc = prepare_fill(c, n, offsets_in, capacity, key_out, tri_out, count, K::key_name)) return rc;
    if (int rc = K::prepare(c, src, n, *prm, &q, &plan)) return rc;
    rt::ListingKind<typename K::Stats>& st = c->pt.queries.*K::state;
    st.stats = typename K::Stats{};
    st.stats.*K::items = n;
    st.steps = 0;
    if (count)
        if (int rc = run_count<K>(c, q, *prm, plan, count_out, offsets_out, ls, !fill)) return rc;
    if (fill) return run_fill<K>(c, q, *prm, plan, offsets_in, capacity, key_out, tri_out, !count);
    return RT_OK;
}

// rt_get_*_query_stats of a listing kind: the two steps' counter words folded into the public struct
template <class K>
int listing_stats(rt_ctx* ctx, typename K::Stats* stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !stats) return RT_ERR_INVALID;
    rt::ListingKind<typename K::Stats>& st = c->pt.queries.*K::state;
    typename K::Stats& s = st.stats;
    if (st.qs.pending) {
        unsigned long long w[kMaxStatWords] = {};
        if (int rc = read_query(c, st.qs, w, &s.ms)) return rc;
        const unsigned long long *cs = w, *fs = w + rt::LQ_STEP_WORDS;  // the count step's words, the fill step's
        const unsigned long long* any = (st.steps & 1u) ? cs : fs;      // both steps meet the same items and find the same
        s.*K::invalid = any[rt::LQ_STAT_INVALID];
        s.*K::found = any[rt::LQ_STAT_FOUND];
        s.*K::written = fs[rt::LQ_STAT_WRITTEN];
        s.*K::incomplete = fs[rt::LQ_STAT_INCOMPLETE];
        s.slice_overflow = fs[rt::LQ_STAT_SLICE_OVERFLOW];
        s.nodes_visited = cs[rt::LQ_STAT_NODES] + fs[rt::LQ_STAT_NODES];
        s.tris_tested = cs[rt::LQ_STAT_TRIS] + fs[rt::LQ_STAT_TRIS];
        s.stack_overflow = (uint32_t)(cs[rt::LQ_STAT_OVERFLOW] | fs[rt::LQ_STAT_OVERFLOW]);
    }
    *stats = s;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_default_ray_query_params(rt_ray_query_params* p) { return default_params(p); }

int rt_query_rays_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_ray_query_params* prm, void* t_out, void* tri_out) {
    return query_rays(ctx, origins, dirs, tmax, n, prm, t_out, tri_out, false, nullptr, nullptr);
}

int rt_query_rays_attr_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_ray_query_params* prm, void* t_out, void* tri_out,
                              void* uv_out, void* normal_out) {
    return query_rays(ctx, origins, dirs, tmax, n, prm, t_out, tri_out, true, uv_out, normal_out);
}

int rt_get_ray_query_stats(rt_ctx* ctx, rt_ray_query_stats* stats) { return query_stats(ctx, &rt::Queries::rays, kRayStats, stats); }

int rt_default_point_query_params(rt_point_query_params* p) { return default_params(p); }

int rt_query_points_device(rt_ctx* ctx, const void* points, const void* rmax, uint32_t n, const rt_point_query_params* prm, void* dist_out, void* tri_out, void* point_out) {
    return rt_query_points_attr_device(ctx, points, rmax, n, prm, dist_out, tri_out, point_out, nullptr, nullptr);
}

int rt_query_points_attr_device(rt_ctx* ctx, const void* points, const void* rmax, uint32_t n, const rt_point_query_params* prm, void* dist_out, void* tri_out,
                                void* point_out, void* uv_out, void* normal_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_point_query_params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done)) return rc;
    if (done) return RT_OK;
    rt::PointAttrQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_points(c, points, rmax, n, *prm, dist_out, tri_out, point_out, uv_out, normal_out, &q, &plan)) return rc;
    return run_points(c, q, *prm, plan);
}

int rt_get_point_query_stats(rt_ctx* ctx, rt_point_query_stats* stats) { return query_stats(ctx, &rt::Queries::points, kPointStats, stats); }

int rt_default_side_query_params(rt_side_query_params* p) { return default_params(p); }

int rt_query_sides_device(rt_ctx* ctx, const void* points, uint32_t n, const rt_side_query_params* prm, void* inside_out, void* crossings_out, void* dist_inout) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_side_query_params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done)) return rc;
    if (done) return RT_OK;
    rt::SideQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_sides(c, points, n, *prm, inside_out, true, crossings_out, dist_inout, &q, &plan)) return rc;
    return run_sides(c, q, *prm, plan);
}

// rt_query_points_device, then rt_query_sides_device on its distances; both steps' refusals and first-use allocations before the first enqueue
int rt_query_signed_distance_device(rt_ctx* ctx, const void* points, const void* rmax, uint32_t n, const rt_point_query_params* pprm, const rt_side_query_params* sprm,
                                    void* sdist_out, void* tri_out, void* point_out, void* inside_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_point_query_params pdefaults{};
    const rt_side_query_params sdefaults{};
    int done;
    if (int rc = use_params(c, n, pprm, pdefaults)) return rc;
    if (int rc = use_params(c, n, sprm, sdefaults)) return rc;
    if (int rc = begin_query(c, n, &done)) return rc;
    if (done) return RT_OK;
    rt::PointAttrQuery pq{};
    rt::SideQuery sq{};
    QueryPlan pplan{}, splan{};
    if (int rc = prepare_points(c, points, rmax, n, *pprm, sdist_out, tri_out, point_out, nullptr, nullptr, &pq, &pplan)) return rc;
    if (int rc = prepare_sides(c, points, n, *sprm, inside_out, false, nullptr, sdist_out, &sq, &splan)) return rc;
    if (int rc = run_points(c, pq, *pprm, pplan)) return rc;
    return run_sides(c, sq, *sprm, splan);
}

int rt_get_side_query_stats(rt_ctx* ctx, rt_side_query_stats* stats) { return query_stats(ctx, &rt::Queries::sides, kSideStats, stats); }

int rt_default_hit_query_params(rt_hit_query_params* p) { return default_params(p); }

int rt_count_ray_hits_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_hit_query_params* prm, void* count_out,
                             void* offsets_out) {
    return listing_call<HitKind>(ctx, {origins, dirs, tmax}, n, prm, 1u, count_out, offsets_out, nullptr, 0, nullptr, nullptr);
}

int rt_fill_ray_hits_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_hit_query_params* prm, const void* offsets_in,
                            uint64_t capacity, void* t_out, void* tri_out) {
    return listing_call<HitKind>(ctx, {origins, dirs, tmax}, n, prm, 2u, nullptr, nullptr, offsets_in, capacity, t_out, tri_out);
}

int rt_list_ray_hits_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* tmax, uint32_t n, const rt_hit_query_params* prm, void* count_out,
                            void* offsets_out, uint64_t capacity, void* t_out, void* tri_out) {
    return listing_call<HitKind>(ctx, {origins, dirs, tmax}, n, prm, 3u, count_out, offsets_out, nullptr, capacity, t_out, tri_out);
}

int rt_get_hit_query_stats(rt_ctx* ctx, rt_hit_query_stats* stats) { return listing_stats<HitKind>(ctx, stats); }

int rt_default_neighbor_query_params(rt_neighbor_query_params* p) { return default_params(p); }

int rt_count_neighbors_device(rt_ctx* ctx, const void* points, const void* rmax, float rmax_all, uint32_t n, const rt_neighbor_query_params* prm, void* count_out,
                              void* offsets_out) {
    return listing_call<NeighborKind>(ctx, {points, rmax, rmax_all}, n, prm, 1u, count_out, offsets_out, nullptr, 0, nullptr, nullptr);
}

int rt_fill_neighbors_device(rt_ctx* ctx, const void* points, const void* rmax, float rmax_all, uint32_t n, const rt_neighbor_query_params* prm, const void* offsets_in,
                             uint64_t capacity, void* dist_out, void* tri_out) {
    return listing_call<NeighborKind>(ctx, {points, rmax, rmax_all}, n, prm, 2u, nullptr, nullptr, offsets_in, capacity, dist_out, tri_out);
}

int rt_list_neighbors_device(rt_ctx* ctx, const void* points, const void* rmax, float rmax_all, uint32_t n, const rt_neighbor_query_params* prm, void* count_out,
                             void* offsets_out, uint64_t capacity, void* dist_out, void* tri_out) {
    return listing_call<NeighborKind>(ctx, {points, rmax, rmax_all}, n, prm, 3u, count_out, offsets_out, nullptr, capacity, dist_out, tri_out);
}

int rt_get_neighbor_query_stats(rt_ctx* ctx, rt_neighbor_query_stats* stats) { return listing_stats<NeighborKind>(ctx, stats); }

int rt_default_overlap_query_params(rt_overlap_query_params* p) { return default_params(p); }

int rt_count_overlaps_device(rt_ctx* ctx, const void* tris, uint32_t n, const rt_overlap_query_params* prm, void* count_out, void* offsets_out) {
    return listing_call<OverlapKind>(ctx, {tris}, n, prm, 1u, count_out, offsets_out, nullptr, 0, nullptr, nullptr);
}

int rt_fill_overlaps_device(rt_ctx* ctx, const void* tris, uint32_t n, const rt_overlap_query_params* prm, const void* offsets_in, uint64_t capacity, void* tri_out,
                            void* edges_out) {
    return listing_call<OverlapKind>(ctx, {tris}, n, prm, 2u, nullptr, nullptr, offsets_in, capacity, edges_out, tri_out);
}

int rt_list_overlaps_device(rt_ctx* ctx, const void* tris, uint32_t n, const rt_overlap_query_params* prm, void* count_out, void* offsets_out, uint64_t capacity,
                            void* tri_out, void* edges_out) {
    return listing_call<OverlapKind>(ctx, {tris}, n, prm, 3u, count_out, offsets_out, nullptr, capacity, edges_out, tri_out);
}

int rt_get_overlap_query_stats(rt_ctx* ctx, rt_overlap_query_stats* stats) { return listing_stats<OverlapKind>(ctx, stats); }

// ---- overlap segments: every refusal and the first-use allocations, then the map, then one lane per entry ----
int rt_overlap_segments_device(rt_ctx* ctx, const void* tris, uint32_t n, const void* offsets, uint64_t capacity, const void* tri, void* seg_out, void* ends_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    rt::Queries& qr = c->pt.queries;
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (int rc = check_query_items(c, n)) return rc;
    if (capacity > (uint64_t)1 << 40) return c->fail(RT_ERR_INVALID, "capacity %llu is above 2^40", (unsigned long long)capacity);
    if (n == 0 || capacity == 0) return RT_OK;
    if (int rc = rt::bind(c)) return rc;
    if (int rc = check_arrays(c, {{tris, (size_t)n * 36, "tris_dev"}, {offsets, ((size_t)n + 1) * 8, "offsets_dev"}, {tri, (size_t)capacity * 4, "tri_dev"},
                                  {seg_out, (size_t)capacity * 24, "seg_out_dev"}, {ends_out, (size_t)capacity * 4, "ends_out_dev", false}}))
        return rc;
    QueryState& qs = qr.segments.qs;
    if (int rc = ensure_block(c, qs, "counters")) return rc;
    if (int rc = grow_scratch(c, qr.tri_inverse, mesh.n_tris, "overlap-segments index map")) return rc;
    rt::SegmentQuery q{};
    q.tris = static_cast<const float*>(tris);
    q.offsets = static_cast<const long long*>(offsets);
    q.tri = static_cast<const int*>(tri);
    q.capacity = (long long)capacity;
    q.seg_out = static_cast<float*>(seg_out);
    q.ends_out = static_cast<int*>(ends_out);
    q.n = n;
    q.reach = rt::kCameraReach * mesh.maxabs;
    // nothing can refuse any more
    rt::RoctxRange rr("rt.path_b.overlap_segments");
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(qs.block.get() + rt::kQueryHeadBytes);
    RT_HIP(c, hipMemsetAsync(stats, 0, qs.n_counters * sizeof(unsigned long long), c->stream));
    RT_HIP(c, hipEventRecord(qs.ev[0].get(), c->stream));
    if (int rc = rt::launch_pt_tri_inverse(c, rt::scene_view(mesh), qr.tri_inverse.d.get())) return rc;
    if (int rc = rt::launch_pt_overlap_segments(c, rt::scene_view(mesh), q, qr.tri_inverse.d.get(), stats)) return rc;
    RT_HIP(c, hipEventRecord(qs.ev[1].get(), c->stream));
    qs.pending = true;
    qr.segments.stats = rt_overlap_segment_stats{};
    qr.segments.stats.launches = 2;
    return RT_OK;
}

int rt_get_overlap_segment_stats(rt_ctx* ctx, rt_overlap_segment_stats* stats) {
    return query_stats(ctx, &rt::Queries::segments, kSegmentStats, stats, derive_segments);
}

// ---- clearance ----
int rt_default_clearance_query_params(rt_clearance_query_params* p) { return default_params(p); }

int rt_query_clearance_device(rt_ctx* ctx, const void* tris, const void* rmax, uint32_t n, const rt_clearance_query_params* prm, void* tri_out, void* dist_out,
                              void* point_query_out, void* point_mesh_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_clearance_query_params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done)) return rc;
    if (done) return RT_OK;
    rt::ClearanceQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_clearance(c, tris, rmax, n, *prm, tri_out, dist_out, point_query_out, point_mesh_out, &q, &plan)) return rc;
    return run_clearance(c, q, *prm, plan);
}

int rt_get_clearance_query_stats(rt_ctx* ctx, rt_clearance_query_stats* stats) { return query_stats(ctx, &rt::Queries::clearance, kClearanceStats, stats); }

// ---- k nearest: k is checked between the parameters and the device ----
int rt_default_knn_query_params(rt_knn_query_params* p) { return default_params(p); }

int rt_query_knn_device(rt_ctx* ctx, const void* points, const void* rmax, uint32_t n, uint32_t k, const rt_knn_query_params* prm, void* dist_out, void* tri_out,
                        void* count_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_knn_query_params defaults{};
    int done;
    if (int rc = use_params(c, n, prm, defaults)) return rc;
    if (k == 0u || k > RT_KNN_MAX_K) return c->fail(RT_ERR_INVALID, "k %u (1 .. %u)", k, RT_KNN_MAX_K);
    if (int rc = begin_query(c, n, &done)) return rc;
    if (done) return RT_OK;
    rt::KnnQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_knn(c, points, rmax, n, k, *prm, dist_out, tri_out, count_out, &q, &plan)) return rc;
    return run_knn(c, q, *prm, plan);
}

int rt_get_knn_query_stats(rt_ctx* ctx, rt_knn_query_stats* stats) { return query_stats(ctx, &rt::Queries::knn, kKnnStats, stats); }

// ---- sphere casts ----
int rt_default_sweep_query_params(rt_sweep_query_params* p) { return default_params(p); }

int rt_query_sweeps_device(rt_ctx* ctx, const void* origins, const void* dirs, const void* radius, const void* tmax, uint32_t n, const rt_sweep_query_params* prm,
                           void* t_out, void* tri_out, void* point_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    const rt_sweep_query_params defaults{};
    int done;
    if (int rc = enter_query(c, n, prm, defaults, &done)) return rc;
    if (done) return RT_OK;
    rt::SweepQuery q{};
    QueryPlan plan{};
    if (int rc = prepare_sweeps(c, origins, dirs, radius, tmax, n, *prm, t_out, tri_out, point_out, &q, &plan)) return rc;
    return run_sweeps(c, q, *prm, plan);
}

int rt_get_sweep_query_stats(rt_ctx* ctx, rt_sweep_query_stats* stats) { return query_stats(ctx, &rt::Queries::sweeps, kSweepStats, stats); }

}  // extern "C"
