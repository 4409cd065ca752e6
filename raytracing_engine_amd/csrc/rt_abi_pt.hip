// rt_abi_pt.hip — C-ABI entry points of path B's frames (wavefront path tracer over a triangle mesh + BVH), the host-side
// stage schedule and the rt_trace_rays test hook.  No reference counterpart (include/rt_abi.h, "Path B").  The mesh's lifetime is
// in rt_abi_mesh.hip, the queries on device arrays in rt_abi_query.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_roctx.h"

using rt::Ctx;
using rt::kCameraReach;
using rt::PtData;
using rt::scene_view;

namespace {

constexpr uint64_t kMaxPathsInFlight = 1ull << 25;  // 33.5 M paths = 4.3 GB of wavefront state
constexpr uint32_t kMaxBounces = 15;
// chosen on the headline scene among the interval-only walk with 1, 2 and 4 rays per lane (profiles/packet_wide.txt): 2 and 4 both beat 1
// by the gain gate; 4 over 2 is inside the run-to-run spread with three frame lanes and costs the context scenes 6 % (2: under 1 %)
constexpr uint32_t kDefaultPacketMode = rt::PACKET_WIDE_2;
constexpr uint32_t kDefaultTriMode = rt::TRI_MODE_INLINE;  // rt_pt_params.tune_tri_mode = 0
void free_wavefront(PtData& pt) {
    for (auto& mem : pt.wavefront) mem.reset();
    pt.st = rt::PtState{};
    pt.d_queue[0] = pt.d_queue[1] = nullptr;
    pt.d_acc = nullptr;
    pt.cap_paths = 0;
    pt.cap_slots = 0;
}

int ensure_wavefront(Ctx* c, uint64_t n_paths, uint64_t n_slots) {
    PtData& pt = c->pt;
    if (!pt.d_ctr) {
        if (!dalloc(pt.d_ctr, (size_t)rt::PT_CTR_STRIDE * (kMaxBounces + 3)) || !dalloc(pt.d_stats, rt::PT_STAT_WORDS)) return c->fail(RT_ERR_OOM, "path-tracer counters");
    }
    if (n_paths > pt.cap_paths || n_slots > pt.cap_slots) {
        RT_HIP(c, hipStreamSynchronize(c->stream));
        free_wavefront(pt);
        size_t used = 0;
        auto take = [&](auto*& p, size_t count) {  // one allocation of pt.wavefront per array
            rt::DevPtr<char>& mem = pt.wavefront[used++];
            if (!dalloc(mem, count * sizeof(*p))) return false;
            p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(mem.get());
            return true;
        };
        const size_t n = (size_t)n_paths;
        const bool ok = take(pt.st.ray_o, n) && take(pt.st.ray_d, n) && take(pt.st.thr, n) && take(pt.st.rad, n) && take(pt.st.hit, n) && take(pt.st.sh_o, n) &&
                        take(pt.st.sh_d, n) && take(pt.st.sh_c, n) && take(pt.d_queue[0], n) && take(pt.d_queue[1], n) && take(pt.d_acc, (size_t)n_slots * 3);
        if (!ok) {
            free_wavefront(pt);
            return c->fail(RT_ERR_OOM, "wavefront buffers for %llu paths", (unsigned long long)n_paths);
        }
        pt.cap_paths = n_paths;
        pt.cap_slots = n_slots;
    }
    return RT_OK;
}

// The stages of a frame that per-stage timing tells apart, and where each one's time goes
enum Stage { STAGE_GENERATE, STAGE_TRACE_CLOSEST, STAGE_SHADE, STAGE_TRACE_SHADOW, STAGE_RESOLVE, STAGE_TRACE_PACKET, STAGE_TRACE_FUSED, STAGE_COUNT };
constexpr float rt_pt_stats::* kStageMs[STAGE_COUNT] = {&rt_pt_stats::ms_generate,     &rt_pt_stats::ms_trace_closest, &rt_pt_stats::ms_shade,
                                                         &rt_pt_stats::ms_trace_shadow, &rt_pt_stats::ms_resolve,       &rt_pt_stats::ms_trace_packet,
                                                         &rt_pt_stats::ms_trace_fused};

struct StageTimer {  // HIP-event pairs around launches, summed per stage after the frame
    Ctx* c;
    bool on;
    std::vector<rt::Event>& pool;  // the context's own events: created after hipSetDevice(c->device), they go with the context
    std::vector<std::pair<Stage, size_t>> marks;  // stage, index of begin event
    size_t used = 0;
    hipError_t err = hipSuccess;  // first failure of an event call (reported by the frame)
    hipEvent_t next() {
        if (used == pool.size()) {
            rt::Event e;  // owned from the moment it exists, whatever the pool's growth does
            const hipError_t rc = rt::make_event(e);
            if (rc != hipSuccess) {
                if (err == hipSuccess) err = rc;
                return nullptr;
            }
            pool.push_back(std::move(e));
        }
        return pool[used++].get();
    }
    void record() {
        hipEvent_t e = next();
        if (!e) return;
        const hipError_t rc = hipEventRecord(e, c->stream);
        if (rc != hipSuccess && err == hipSuccess) err = rc;
    }
    void begin(Stage stage) {
        if (!on) return;
        marks.push_back({stage, used});
        record();
    }
    void end() {
        if (on) record();
    }
};

struct FramePlan {  // what a frame's launches have in common: rt_pt_params decoded, buffers sized
    uint64_t n_slots = 0;    // owned tiles * 4096; 0: this rank owns nothing of the frame
    uint32_t spp_batch = 0;  // samples of a pixel in flight at once
    bool count = false;      // rt_pt_params.count_traversal
    bool packet = false;     // camera rays through the packet kernel
    uint32_t packet_mode = 0;
    uint32_t tri_mode = 0, tri_cfg = 0, refill_min = 0, sort_rays = 0;
    rt::StackCfg stack{};
    size_t spill_half = 0;  // two-stream mode: where the shadow kernel's spill columns begin
    uint32_t grid_persistent = 0, grid_stride = 0;
    bool fused = false, overlap = false;  // how shadow(d) and closest(d + 1) share the machine (plan_frame)
};

struct FrameCounts {  // summed over the sample batches of a frame
    uint64_t cam = 0, bnc = 0, shd = 0;
    uint64_t shd_fused = 0;  // shadow rays traced inside fused launches
    uint32_t launches_closest = 0, launches_shadow = 0, launches_fused = 0;
};

// Checks, decoding of the tuning words, buffers.  p->n_slots = 0 on return: nothing to render
int plan_frame(Ctx* c, const float rot[4], const float pos[3], const rt_pt_params* prm, bool timed, FramePlan* p) {
    if (!rot || !pos || !prm) return c->fail(RT_ERR_INVALID, "rot/pos/params must not be NULL");
    const rt::DeviceMesh& mesh = c->pt.mesh();
    if (!mesh.n_tris) return c->fail(RT_ERR_STATE, "rt_set_mesh has not been called");
    if (!c->width) return c->fail(RT_ERR_STATE, "rt_resize has not been called");
    if (prm->spp == 0 || prm->bounces > kMaxBounces) return c->fail(RT_ERR_INVALID, "spp %u / bounces %u out of range", prm->spp, prm->bounces);
    if (int rc = rt::check_mesh_domain(c, mesh)) return rc;
    {
        // The slab test's rounding error is about 2^-22 * (|origin| + |plane|) in position space and the boxes are
        // padded by 2e-5 * M (M = largest |vertex coordinate|, at least 1): the invariant "results do not depend on
        // which boxes are visited"  holds for ray origins within about 40 M.  Bounce and shadow
        // rays start on the mesh; the camera is checked here.
        const float reach = kCameraReach * mesh.maxabs;  // stored at build time (pad / 2e-5f does not round-trip in fp32)
        for (int a = 0; a < 3; a++)
            if (!(std::fabs(pos[a]) <= reach))
                return c->fail(RT_ERR_INVALID, "camera position %g is outside +-%g (= %g x the mesh's largest |coordinate|): beyond the range the BVH box padding covers",
                               (double)pos[a], (double)reach, (double)kCameraReach);
    }
    if (int rc = rt::bind(c)) return rc;

    p->n_slots = (uint64_t)rt::owned_tiles(c->part) * RT_TILE * RT_TILE;
    if (p->n_slots == 0) return RT_OK;
    if (p->n_slots > kMaxPathsInFlight) return c->fail(RT_ERR_INVALID, "view too large for one rank");
    const uint64_t max_paths = prm->max_paths ? std::min<uint64_t>(prm->max_paths, kMaxPathsInFlight) : kMaxPathsInFlight;
    p->spp_batch = (uint32_t)std::min<uint64_t>(prm->spp, std::max<uint64_t>(1, max_paths / p->n_slots));
    if (int rc = ensure_wavefront(c, p->n_slots * p->spp_batch, p->n_slots)) return rc;

    p->count = prm->count_traversal != 0;
    p->sort_rays = prm->tune_sort_rays;
    // triangle-test schedule of the per-lane kernels: byte 0 = mode (0 = default), bytes 1-2 = the pool's flush parameters
    p->tri_mode = (prm->tune_tri_mode & 0xffu) ? (prm->tune_tri_mode & 0xffu) : kDefaultTriMode;
    if (p->tri_mode < rt::TRI_MODE_INLINE || p->tri_mode > rt::TRI_MODE_INLINE_PF) return c->fail(RT_ERR_INVALID, "tune_tri_mode %u (0 .. 4)", p->tri_mode);
    p->tri_cfg = prm->tune_tri_mode >> 8;
    // low byte: idle lanes that trigger a refill (24; 8 with the software-pipelined refill, whose refill is a read from LDS); next byte (tuning): inner steps per round
    p->refill_min = (prm->tune_refill_min & 0xffu ? std::min<uint32_t>(prm->tune_refill_min & 0xffu, 64u) : p->tri_mode == rt::TRI_MODE_INLINE_PF ? 8u : 24u) |
                    (prm->tune_refill_min & 0xff00u);
    // (two halves of spill columns: the second for the shadow kernel when it overlaps the next closest-hit kernel)
    if (int rc = rt::pt_stack_config(c, mesh.stack_need, 2048u + rt::pt_pool_lds_bytes(p->tri_mode), 2u, prm->tune_lds_stack, prm->tune_blocks_per_cu,
                                     p->n_slots * p->spp_batch, &p->stack, &p->grid_persistent))
        return rc;
    p->spill_half = rt::spill_half_words(p->stack);
    p->grid_stride = (uint32_t)c->n_cus * 2u;  // 1024-thread workgroups, grid-stride
    // camera rays through the packet kernel, which makes its own rays: no generate stage, no queue 0.  Its wave-uniform stack is a
    // fixed LDS array: a tree that may need more (a deep two-level tree) takes the per-lane kernel, whose stack is sized from stack_need
    p->packet = prm->tune_no_packet != rt::PACKET_OFF && mesh.stack_need <= rt::kPacketStackEntries;
    p->packet_mode = prm->tune_no_packet == rt::PACKET_DEFAULT ? kDefaultPacketMode : prm->tune_no_packet;

    // How shadow(d) and closest(d + 1) share the machine (they are independent: the shadow rays only add to the paths'
    // radiance, the closest-hit rays only read rays):  0 (default) one persistent launch pulls from both queues
    // (pt_trace_fused);  2 two launches on two streams (the auxiliary stream exists from the first frame that wants it:
    // streams are dealt onto a few hardware queues in creation order, and a context that only renders path A should
    // not occupy two; falls back to 1 under per-stage timing);  1 one launch after the other on one stream.
    const uint32_t overlap_mode = mesh.n_lights == 0 ? 1u : (timed && prm->tune_no_overlap == 2u) ? 1u : prm->tune_no_overlap;  // per-stage timing needs one stream
    p->fused = overlap_mode == 0u;
    if (overlap_mode == 2u && !c->aux_stream) RT_HIP_AS(c, rt::kTextAuxStream, rt::make_stream(c->aux_stream, hipStreamNonBlocking));
    p->overlap = overlap_mode == 2u && c->aux_stream;
    if (p->overlap && !c->pt.ev_shaded) {  // both events or neither: a frame that fails here leaves the next one to try again from nothing
        rt::Event shaded, shadowed;
        RT_HIP_AS(c, rt::kTextEvShaded, rt::make_event(shaded, hipEventDisableTiming));
        RT_HIP_AS(c, rt::kTextEvShadowed, rt::make_event(shadowed, hipEventDisableTiming));
        c->pt.ev_shaded = std::move(shaded);
        c->pt.ev_shadowed = std::move(shadowed);
    }
    return RT_OK;
}

// One sample batch (f.sample0, f.spp_batch) of the schedule: camera rays, then per depth closest hit, shade and shadow rays, then resolve
int enqueue_batch(Ctx* c, const FramePlan& p, const rt::PtScene& sc, const rt::PtFrame& f, StageTimer& tm, FrameCounts& n, float* dst_dev, int tile_major) {
    PtData& pt = c->pt;
    const rt::DeviceMesh& mesh = pt.mesh();
    unsigned long long* stats = pt.d_stats.get();
    RT_HIP(c, hipMemsetAsync(pt.d_ctr.get(), 0, (size_t)rt::PT_CTR_STRIDE * (f.bounces + 2) * sizeof(uint32_t), c->stream));
    if (!p.packet) {
        rt::RoctxRange rr("rt.path_b.generate");
        tm.begin(STAGE_GENERATE);
        if (int rc = rt::launch_pt_generate(c, f, pt.st, pt.d_queue[0], pt.d_ctr.get())) return rc;
        tm.end();
    }
    bool shadow_deferred = false;  // fused mode: shadow(d - 1) waits for the launch of closest(d)
    bool shadow_pending = false;   // two-stream mode: shadow(d - 1) is running on the auxiliary stream
    for (uint32_t d = 0; d <= f.bounces; d++) {
        uint32_t* ctr_d = pt.d_ctr.get() + (size_t)rt::PT_CTR_STRIDE * d;
        uint32_t* ctr_n = pt.d_ctr.get() + (size_t)rt::PT_CTR_STRIDE * (d + 1);
        const uint32_t* q = pt.d_queue[d & 1];
        uint32_t* qn = pt.d_queue[(d + 1) & 1];
        const bool camera_packet = d == 0 && p.packet;
        {
            rt::RoctxRange rr(camera_packet ? "rt.path_b.trace_packet depth" : shadow_deferred ? "rt.path_b.trace_fused depth" : "rt.path_b.trace_closest depth", d);
            tm.begin(camera_packet ? STAGE_TRACE_PACKET : shadow_deferred ? STAGE_TRACE_FUSED : STAGE_TRACE_CLOSEST);
            if (camera_packet) {  // camera rays: one shared origin, coherent 4x4-pixel blocks per wave
                if (int rc = rt::launch_pt_trace_packet(c, sc, f, pt.st, stats, p.count, p.packet_mode)) return rc;
            } else if (shadow_deferred) {  // closest(d) + shadow(d - 1): ctr_d holds both the closest count of depth d and the shadow count of depth d - 1
                if (int rc = rt::launch_pt_trace_fused(c, sc, pt.st, q, ctr_d + rt::PT_CTR_COUNT, ctr_d + rt::PT_CTR_HEAD_CLOSEST, ctr_d + rt::PT_CTR_SHADOW_COUNT,
                                                       ctr_d + rt::PT_CTR_HEAD_SHADOW, stats, p.count, p.grid_persistent, p.stack, p.refill_min, p.tri_mode, p.tri_cfg))
                    return rc;
                shadow_deferred = false;
                n.launches_shadow++;
                n.launches_fused++;
            } else if (int rc = rt::launch_pt_trace(c, c->stream, sc, pt.st, q, ctr_d + rt::PT_CTR_COUNT, ctr_d + rt::PT_CTR_HEAD_CLOSEST, stats, false, p.count,
                                                    p.grid_persistent, p.stack, p.refill_min, p.tri_mode, p.tri_cfg)) {
                return rc;
            }
            tm.end();
        }
        n.launches_closest++;
        if (shadow_pending) {  // shade(d) adds sky/emission after shadow(d-1)'s contribution
            RT_HIP(c, hipStreamWaitEvent(c->stream, pt.ev_shadowed.get(), 0));
            shadow_pending = false;
        }
        {
            rt::RoctxRange rr("rt.path_b.shade depth", d);
            tm.begin(STAGE_SHADE);
            if (int rc = rt::launch_pt_shade(c, sc, f, pt.st, camera_packet ? nullptr : q, ctr_d + rt::PT_CTR_COUNT, d, qn, ctr_n, p.grid_stride, p.sort_rays,
                                             mesh.has_surfaces))
                return rc;
            tm.end();
        }
        if (!mesh.n_lights) continue;
        if (p.fused && d < f.bounces) {  // goes into the same launch as closest(d + 1)
            shadow_deferred = true;
            continue;
        }
        // two-stream mode: the shadow kernel runs on the auxiliary stream beside the next closest-hit kernel;
        // shade(d+1) and resolve read the radiance and therefore wait for it (keeps the per-path sum order)
        rt::StackCfg sk2 = p.stack;
        hipStream_t shadow_stream = c->stream;
        if (p.overlap) {
            sk2.spill = p.stack.spill + p.spill_half;
            shadow_stream = c->aux_stream.get();
            RT_HIP(c, hipEventRecord(pt.ev_shaded.get(), c->stream));
            RT_HIP(c, hipStreamWaitEvent(shadow_stream, pt.ev_shaded.get(), 0));
        }
        {
            rt::RoctxRange rr("rt.path_b.trace_shadow depth", d);
            tm.begin(STAGE_TRACE_SHADOW);
            if (int rc = rt::launch_pt_trace(c, shadow_stream, sc, pt.st, nullptr, ctr_n + rt::PT_CTR_SHADOW_COUNT, ctr_n + rt::PT_CTR_HEAD_SHADOW, stats, true, p.count,
                                             p.grid_persistent, sk2, p.refill_min, p.tri_mode, p.tri_cfg))
                return rc;
            tm.end();
        }
        if (p.overlap) {
            RT_HIP(c, hipEventRecord(pt.ev_shadowed.get(), shadow_stream));
            shadow_pending = true;
        }
        n.launches_shadow++;
    }
    if (shadow_pending) RT_HIP(c, hipStreamWaitEvent(c->stream, pt.ev_shadowed.get(), 0));
    rt::RoctxRange rr("rt.path_b.resolve");
    tm.begin(STAGE_RESOLVE);
    if (int rc = rt::launch_pt_resolve(c, f, pt.st, pt.d_acc, dst_dev, tile_major)) return rc;
    tm.end();
    return RT_OK;
}

// Ray counters of the batch just enqueued, added to n (synchronises: the copy is ordered after the kernels on the stream)
int count_batch_rays(Ctx* c, const FramePlan& p, const rt::PtFrame& f, std::vector<uint32_t>& h_ctr, FrameCounts& n) {
    RT_HIP(c, hipMemcpyAsync(h_ctr.data(), c->pt.d_ctr.get(), h_ctr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (p.packet) {  // no queue 0: camera rays = samples of the owned pixels inside the frame
        uint64_t px_owned = 0;
        for (uint32_t t = c->part.rank; t < c->part.tiles_x * c->part.tiles_y; t += c->part.n_ranks) {
            const uint32_t ty = t / c->part.tiles_x, tx = t % c->part.tiles_x;
            px_owned += (uint64_t)std::min<uint32_t>(RT_TILE, c->width - tx * RT_TILE) * std::min<uint32_t>(RT_TILE, c->height - ty * RT_TILE);
        }
        n.cam += px_owned * f.spp_batch;
    } else {
        n.cam += h_ctr[rt::PT_CTR_COUNT];
    }
    for (uint32_t d = 1; d <= f.bounces + 1; d++) {
        if (d <= f.bounces) n.bnc += h_ctr[(size_t)rt::PT_CTR_STRIDE * d + rt::PT_CTR_COUNT];
        n.shd += h_ctr[(size_t)rt::PT_CTR_STRIDE * d + rt::PT_CTR_SHADOW_COUNT];
        if (p.fused && d <= f.bounces) n.shd_fused += h_ctr[(size_t)rt::PT_CTR_STRIDE * d + rt::PT_CTR_SHADOW_COUNT];  // shadow(d - 1) rides with closest(d)
    }
    return RT_OK;
}

// The frame is enqueued: wait for it and fill the per-frame part of rt_pt_stats
int read_frame_stats(Ctx* c, const StageTimer& tm, const FrameCounts& n) {
    PtData& pt = c->pt;
    rt_pt_stats& s = pt.stats;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long st[rt::PT_STAT_WORDS] = {};
    RT_HIP(c, hipMemcpy(st, pt.d_stats.get(), sizeof st, hipMemcpyDeviceToHost));
    s.camera_rays = n.cam;
    s.bounce_rays = n.bnc;
    s.shadow_rays = n.shd;
    s.nodes_visited = st[rt::PT_STAT_NODES];
    s.tris_tested = st[rt::PT_STAT_NODES + 1];
    s.shadow_nodes_visited = st[rt::PT_STAT_SHADOW] + st[rt::PT_STAT_FUSED_SHADOW];
    s.shadow_tris_tested = st[rt::PT_STAT_SHADOW + 1] + st[rt::PT_STAT_FUSED_SHADOW + 1];
    s.fused_shadow_nodes = st[rt::PT_STAT_FUSED_SHADOW];
    s.fused_shadow_tris = st[rt::PT_STAT_FUSED_SHADOW + 1];
    s.packet_nodes_fetched = st[rt::PT_STAT_PACKETS + 1];
    s.packet_tris_fetched = st[rt::PT_STAT_PACKETS + 2];
    s.fused_shadow_rays = n.shd_fused;
    s.launches_trace_fused = n.launches_fused;
    s.wave_rounds = st[rt::PT_STAT_ROUNDS];
    s.alive_lane_rounds = st[rt::PT_STAT_ROUNDS + 1];
    s.packets = st[rt::PT_STAT_PACKETS];
    s.pool_flushes = st[rt::PT_STAT_FLUSHES];
    s.wave_rounds_all = st[rt::PT_STAT_ROUNDS_ALL];
    s.stack_overflow = (uint32_t)st[rt::PT_STAT_OVERFLOW];
    RT_HIP(c, hipEventElapsedTime(&s.ms_total, c->ev_begin.get(), c->ev_end.get()));
    for (auto field : kStageMs) s.*field = 0.0f;
    for (auto& m : tm.marks) {
        float ms = 0.0f;
        if (m.second + 1 < tm.used && hipEventElapsedTime(&ms, pt.ev_pool[m.second].get(), pt.ev_pool[m.second + 1].get()) == hipSuccess) s.*kStageMs[m.first] += ms;
    }
    return RT_OK;
}

// clear_bytes: dst_dev is zeroed first (rt_render_pt's frame: the tiles of other ranks stay black) - after every refusal of plan_frame,
// so that a refused call has enqueued nothing and the frame that was there still reads back
int render_pt_common(Ctx* c, const float rot[4], const float pos[3], const rt_pt_params* prm, float* dst_dev, int tile_major, bool sync, size_t clear_bytes = 0) {
    if (!c) return RT_ERR_INVALID;
    PtData& pt = c->pt;
    StageTimer tm{c, c->cfg.profile_stages != 0, pt.ev_pool, {}, 0};
    FramePlan plan;
    if (int rc = plan_frame(c, rot, pos, prm, tm.on, &plan)) return rc;
    if (clear_bytes) RT_HIP(c, hipMemsetAsync(dst_dev, 0, clear_bytes, c->stream));
    if (plan.n_slots == 0) return RT_OK;

    rt::PtFrame f{};  // per batch only spp_batch, n_paths and sample0 change
    std::memcpy(f.cam.rot, rot, 16);
    std::memcpy(f.cam.pos, pos, 12);
    f.cam.ratio[0] = c->ratio[0];
    f.cam.ratio[1] = c->ratio[1];
    f.width = c->width;
    f.height = c->height;
    f.part = c->part;
    f.n_slots = (uint32_t)plan.n_slots;
    f.spp_total = prm->spp;
    f.bounces = prm->bounces;
    f.seed = prm->seed;
    std::memcpy(f.sky, prm->sky, 12);
    f.ray_eps = prm->ray_eps;
    const rt::PtScene sc = scene_view(pt.mesh());

    rt::RoctxRange frame_range("rt.path_b.frame");
    RT_HIP(c, hipMemsetAsync(pt.d_stats.get(), 0, rt::PT_STAT_WORDS * sizeof(unsigned long long), c->stream));
    RT_HIP(c, hipEventRecord(c->ev_begin.get(), c->stream));
    FrameCounts n;
    std::vector<uint32_t> h_ctr((size_t)rt::PT_CTR_STRIDE * (prm->bounces + 2));
    for (uint32_t s0 = 0; s0 < prm->spp; s0 += plan.spp_batch) {
        f.spp_batch = std::min(plan.spp_batch, prm->spp - s0);
        f.n_paths = (uint32_t)(plan.n_slots * f.spp_batch);
        f.sample0 = s0;
        if (int rc = enqueue_batch(c, plan, sc, f, tm, n, dst_dev, tile_major)) return rc;
        if (sync)
            if (int rc = count_batch_rays(c, plan, f, h_ctr, n)) return rc;
    }
    RT_HIP(c, hipEventRecord(c->ev_end.get(), c->stream));
    if (tm.err != hipSuccess) return c->fail(RT_ERR_HIP, "stage-timing event: %s", hipGetErrorString(tm.err));
    c->frame_valid = true;
    pt.stats.launches_trace_closest = n.launches_closest;
    pt.stats.launches_trace_shadow = n.launches_shadow;
    return sync ? read_frame_stats(c, tm, n) : RT_OK;
}

}  // namespace

namespace rt {
// The first lds_cap entries of every lane's stack live in LDS (8-byte entries: 2 x lds_cap KiB per 256-thread workgroup, next to
// fixed_lds_bytes: the ray kernels' 2 KiB octant table and triangle pools), which bounds residency at floor(160 KiB / that) workgroups
// per CU, 8 at most (32 waves per CU); the rest of `need` spills to global memory.
int pt_stack_config(Ctx* c, uint32_t need, uint32_t fixed_lds_bytes, uint32_t spill_halves, uint32_t tune_lds, uint32_t tune_blocks, uint64_t n_items,
                    StackCfg* sk, uint32_t* grid) {
    PtData& pt = c->pt;
    need = std::max<uint32_t>(need, 1u);
    // default: up to ten entries in LDS - the whole stack of the 1 M-triangle tree (depth 9) - at seven workgroups per CU
    // (measured 1 % ahead of eight entries at eight workgroups)
    const uint32_t lds_cap = std::min<uint32_t>(need, tune_lds ? std::min<uint32_t>(tune_lds, 78u) : 10u);
    const uint32_t fit = std::max<uint32_t>(1u, std::min<uint32_t>(8u, (160u * 1024u) / (2048u * lds_cap + fixed_lds_bytes)));  // 2 KiB per entry per workgroup
    // Few items (a rank's small share of a frame): fewer resident waves.  Every lane of the grid takes a ray
    // at once, so with ~2 rays per lane the rays in flight span half the frame instead of a compact window
    // and the short launches are all ramp and tail; about four rays per lane and more measured best
    // (1/8 of the headline frame: 2.87 -> 2.62 ms with 4 instead of 8 workgroups per CU).
    const uint32_t by_load = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(3, (n_items + (uint64_t)c->n_cus * 1024 - 1) / ((uint64_t)c->n_cus * 1024)));
    const uint32_t blocks_per_cu = tune_blocks ? std::min<uint32_t>(tune_blocks, fit) : std::min(fit, by_load);
    *grid = (uint32_t)c->n_cus * blocks_per_cu;
    sk->lds_cap = (int)lds_cap;
    sk->spill_cap = (int)(need - lds_cap);
    sk->spill_stride = (size_t)c->n_cus * 8u * 256u;  // covers every grid this function can return
    const size_t words = spill_halves * spill_half_words(*sk);
    if (words > pt.spill_words) {  // the columns grow to the largest need a mesh has met
        RT_HIP(c, hipStreamSynchronize(c->stream));
        pt.spill_words = 0;
        if (!dalloc(pt.d_spill, words)) return c->fail(RT_ERR_OOM, "traversal spill stack (%zu words)", words);
        pt.spill_words = words;
    }
    sk->spill = pt.d_spill.get();
    return RT_OK;
}
}  // namespace rt

extern "C" {

int rt_default_pt_params(rt_pt_params* p) {
    if (!p) return RT_ERR_INVALID;
    p->spp = 4;
    p->bounces = 1;
    p->seed = 1;
    p->sky[0] = p->sky[1] = p->sky[2] = 0.0f;
    p->ray_eps = 1e-3f;
    p->count_traversal = 0;
    p->max_paths = 0;
    p->tune_refill_min = 0;
    p->tune_blocks_per_cu = 0;
    p->tune_lds_stack = 0;
    p->tune_no_overlap = 0;
    p->tune_no_packet = 0;
    p->tune_sort_rays = 0;
    p->tune_tri_mode = 0;
    return RT_OK;
}

int rt_render_pt(rt_ctx* ctx, const float rot[4], const float pos[3], const rt_pt_params* params, float* rgb_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    if (!c->width) return c->fail(RT_ERR_STATE, "rt_resize has not been called");
    if (int rc = rt::bind(c)) return rc;
    const size_t bytes = (size_t)c->width * c->height * 3 * sizeof(float);
    if (int rc = render_pt_common(c, rot, pos, params, c->d_rgb.get(), 0, true, bytes)) return rc;
    if (rgb_out) RT_HIP(c, hipMemcpy(rgb_out, c->d_rgb.get(), bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_render_pt_device(rt_ctx* ctx, const float rot[4], const float pos[3], const rt_pt_params* params, void* rgb_dev, int tile_major) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    if (!rgb_dev) return c->fail(RT_ERR_INVALID, "rgb_dev is NULL");
    return render_pt_common(c, rot, pos, params, static_cast<float*>(rgb_dev), tile_major, false);
}

int rt_get_pt_stats(rt_ctx* ctx, rt_pt_stats* stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !stats) return RT_ERR_INVALID;
    *stats = c->pt.stats;
    return RT_OK;
}

int rt_trace_rays_counted(rt_ctx* ctx, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out, int32_t* tri_out,
                          uint32_t* counts_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    if (!origins || !dirs || !t_out || !tri_out) return c->fail(RT_ERR_INVALID, "NULL ray buffer");
    if (!c->pt.mesh().n_tris) return c->fail(RT_ERR_STATE, "rt_set_mesh has not been called");
    if (n == 0) return RT_OK;
    if (int rc = rt::bind(c)) return rc;
    rt::DevPtr<float> d_o, d_d, d_t;
    rt::DevPtr<int> d_i;
    rt::DevPtr<uint32_t> d_c;
    const size_t nb = (size_t)n;
    if (!dalloc(d_o, nb * 3) || !dalloc(d_d, nb * 3) || !dalloc(d_t, nb) || !dalloc(d_i, nb) || (counts_out && !dalloc(d_c, nb * 2))) return c->fail(RT_ERR_OOM, "ray buffers");
    RT_HIP(c, hipMemcpy(d_o.get(), origins, nb * 12, hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(d_d.get(), dirs, nb * 12, hipMemcpyHostToDevice));
    rt::StackCfg sk{};
    uint32_t grid = 0;
    if (int rc = rt::pt_stack_config(c, c->pt.mesh().stack_need, 2048u, 2u, 0, 0, (uint64_t)n, &sk, &grid)) return rc;
    if (int rc = rt::launch_pt_trace_rays(c, scene_view(c->pt.mesh()), d_o.get(), d_d.get(), n, any_hit, d_t.get(), d_i.get(), d_c.get(), sk, std::min<uint32_t>(grid, (n + 255u) / 256u)))
        return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));  // the buffers are freed on return: nothing may still use them
    RT_HIP(c, hipMemcpy(t_out, d_t.get(), nb * 4, hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(tri_out, d_i.get(), nb * 4, hipMemcpyDeviceToHost));
    if (counts_out) RT_HIP(c, hipMemcpy(counts_out, d_c.get(), nb * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_trace_rays(rt_ctx* ctx, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out, int32_t* tri_out) {
    return rt_trace_rays_counted(ctx, origins, dirs, n, any_hit, t_out, tri_out, nullptr);
}

}  // extern "C"
