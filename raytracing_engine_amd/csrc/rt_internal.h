// rt_internal.h — context object and launch-parameter blocks shared by the .hip files.
// Nothing is freed by hand: every device allocation is a DevPtr, every other handle an Owned (rt_owned.h) member of what holds it, made
// by the helpers next to dalloc, and goes when its holder does.  What has an order is written down at rt_destroy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "bvh_build.h"
#include "rt_owned.h"

struct ncclComm;  // RCCL's communicator (rt_abi_comm.hip)

static_assert(sizeof(rt_material) == 32, "std140 Material stride");
static_assert(sizeof(rt_object) == 16, "std140 Object stride");
static_assert(sizeof(rt_light) == 32, "std140 Light stride");
static_assert(sizeof(rt_mutable_data) == 656, "std140 MutableData size");
static_assert(offsetof(rt_mutable_data, mats) == 16 && offsetof(rt_mutable_data, objs) == 272 &&
                  offsetof(rt_mutable_data, lights) == 400,
              "std140 MutableData offsets");

namespace rt {

// Spheres of the scene, passed by value in the kernarg segment: the compiler keeps them in
// SGPRs (s_load from kernarg), so the 8 objects cost no VGPRs and no vector memory traffic.
struct SphereSet {
    float4 s[RT_MAX_OBJECTS];  // xyz = centre, w = radius
};

struct ShadeSet {  // everything fragment.glsl reads from MutableData
    float4 sphere[RT_MAX_OBJECTS];
    float4 mat_color_ambient[RT_MAX_MATERIALS];  // rgb, ambient
    float mat_shine[RT_MAX_MATERIALS];
    float mat_specular[RT_MAX_MATERIALS];  // read only by the mirror-reflection variant (the reference never reads mat.specular)
    float mat_diffuse[RT_MAX_MATERIALS];   // read only by the transmission variant (the reference never reads mat.diffuse)
    float4 light_pos[RT_MAX_LIGHTS];
    float4 light_color[RT_MAX_LIGHTS];
    uint32_t light_count;
};

// Framebuffer partition (multi-GPU): RT_TILE^2 tiles, tile t belongs to rank t % n_ranks.
struct Partition {
    uint32_t rank, n_ranks, tiles_x, tiles_y;
};

struct Camera {
    float rot[4];
    float pos[3];
    float ratio[2];
    float jitter[2];
};

// compute.glsl push constants + ConstantBuffer for one pyramid level
struct ConeLevelParams {
    Camera cam;
    float image_size[2];  // 2^(count-1-level) / view   (src/main.rs:303-305)
    uint32_t level;       // pc.iter
    uint32_t w, h;        // level image dims (multiples of 8)
    uint32_t parent_w;
    uint32_t shift;       // count-1-level: level pixel -> full-res pixel
    uint32_t width, height;  // full-res view
    float render_dist;
    uint32_t max_steps;
    Partition part;
    uint32_t partitioned;  // 1: skip level tiles this rank does not own / that are off-screen
    // sample batch: blockIdx.y = b traces sample sample0 + b of an n_strata x n_strata stratified pixel
    // into image b of the level (images level_stride floats apart; parents parent_stride apart)
    uint32_t sample0, n_strata;
    uint32_t level_stride, parent_stride;
    uint32_t alg;     // march loop body: 3 = compute.glsl:46-65, 1 / 2 = tracing_algorithms.txt:2-13 / :16-37
    float repeat[3];  // > 0: domain repetition period on that axis (utilities.glsl:31-34)
};

struct ShadeParams {
    Camera cam;
    float view[2];
    uint32_t width, height;
    uint32_t depth_w;  // row pitch of the last pyramid level
    float render_dist, cam_fall_off, light_fall_off, ray_radius;
    uint32_t max_steps;
    Partition part;
    uint32_t tile_major;  // 0: dst is a full frame, 1: dst holds owned tiles packed tile-major
    uint32_t mode;        // bit0: accumulate onto dst, bit1: divide by spp after adding
    float spp;
    // sample batch: the kernel shades samples sample0 .. sample0 + n_batch - 1 of the pixel in index
    // order (depth image b is depth_stride floats after image 0) and adds them in that order
    uint32_t sample0, n_batch, n_strata;
    uint32_t depth_stride;
    float repeat[3];  // > 0: domain repetition period on that axis (utilities.glsl:31-34)
    uint32_t reflections;  // mirror bounces (0 = the reference as shipped)
    float reflectivity;
    uint32_t transmissions;  // spheres a transmitted ray may cross (0 = the reference as shipped)
    float transparency, refraction_index;
};

// Sub-pixel offset of sample s of an n x n stratified pixel in NDC: the stratum centre (i + 0.5)/n inside
// the pixel is ((2i + 1)/n - 1)/view; n = 1 gives exactly 0 = the reference's pixel-centre sample.  The
// same IEEE expression on host and device (correctly rounded divisions on both).
__host__ __device__ inline void sample_jitter(uint32_t s, uint32_t n, uint32_t width, uint32_t height, float* jx, float* jy) {
    const uint32_t si = s % n, sj = s / n;
    *jx = ((float)(2u * si + 1u) / (float)n - 1.0f) / (float)width;
    *jy = ((float)(2u * sj + 1u) / (float)n - 1.0f) / (float)height;
}

// One-launch pyramid: every level for a 32x32 pixel block per workgroup (path_a.hip)
struct PyramidParams {
    Camera cam;
    uint32_t width, height;
    float render_dist;
    uint32_t max_steps;
    Partition part;
    uint32_t count;                        // pyramid levels
    float image_size[RT_MAX_LEVELS][2];    // per level: 2^(count-1-level) / view
    uint32_t level_w[RT_MAX_LEVELS];       // row pitch of each level image
    float* level[RT_MAX_LEVELS];           // level images in HBM
};

// ---- path B (triangles + BVH + path tracing) -------------------------------------
// Per-depth counter block.  The ray queues are consumed through PT_HEADS interleaved streams: stream k
// owns the 64-entry blocks k, k + PT_HEADS, k + 2 PT_HEADS ... of the queue and has its own head word
// on its own 128-byte line (one hot word answers only ~90 atomics/us chip-wide; sixteen words let the
// traversal waves refill a few lanes at a time while all streams together still advance as one
// compact window over the queue).
enum {
    PT_HEADS = 16,
    PT_HEAD_STRIDE = 32,  // words between head words
    PT_CTR_COUNT = 0,
    PT_CTR_SHADOW_COUNT = 1,
    PT_CTR_HEAD_CLOSEST = PT_HEAD_STRIDE,
    PT_CTR_HEAD_SHADOW = PT_HEAD_STRIDE * (1 + PT_HEADS),
    PT_CTR_STRIDE = PT_HEAD_STRIDE * (1 + 2 * PT_HEADS)
};

// Words of the device-side statistics block (PtData::d_stats): the kernels add to them, the frame's read-back names them
enum {
    PT_STAT_NODES = 0,          // closest-hit rays of the per-lane kernels: node visits, + 1: triangle tests
    PT_STAT_OVERFLOW = 2,       // != 0: some traversal stack overflowed
    PT_STAT_SHADOW = 4,         // shadow rays of a launch of their own: node visits, + 1: triangle tests
    PT_STAT_ROUNDS = 6,         // wave-rounds of the loops that carry closest-hit rays, + 1: alive lane-rounds
    PT_STAT_PACKETS = 8,        // packet kernels: waves, + 1: node records fetched, + 2: triangle records fetched
    PT_STAT_FUSED_SHADOW = 11,  // shadow rays inside the fused launch: node visits, + 1: triangle tests
    PT_STAT_FLUSHES = 13,       // TRI_POOL: pool_test passes, TRI_DEFER: triangle phases
    PT_STAT_ROUNDS_ALL = 14,    // wave-rounds of every per-lane loop
    PT_STAT_WORDS = 16
};

struct PtScene {
    const float4* nodes;     // 5 x float4 (80 B) per compressed 8-wide BVH node (bvh_node.h layout)
    const float4* tris;      // 3 x float4 per triangle, leaf order: v0.xyz e1.x | e1.yz e2.xy | e2.z id emissive-flag -
    const float4* albedo;    // leaf order
    const float4* emission;  // leaf order
    const uint32_t* lights;  // leaf-order indices of emissive triangles, ascending original id
    uint32_t n_lights;
    uint32_t n_tris;
};

constexpr uint32_t kPacketStackEntries = 40;  // pt_trace_packet's LDS stack of node groups (pt_packet.hip)
// rt_pt_params.tune_no_packet: 0 = default, 1 = no packet kernel (camera rays through the per-lane kernel), then the packet kernel's node test:
// per-ray slab tests of all eight children; interval test for the pass, per-ray tests of the children that pass; interval test only; the second without the best-hit cap
// 6 / 7: the interval test only, with 2 / 4 rays per lane: one tree walk per 128 / 256 camera rays (pt_trace_packet_wide)
enum { PACKET_DEFAULT = 0, PACKET_OFF = 1, PACKET_EXACT = 2, PACKET_INTERVAL = 3, PACKET_INTERVAL_ONLY = 4, PACKET_INTERVAL_NOCAP = 5, PACKET_WIDE_2 = 6, PACKET_WIDE_4 = 7 };
enum { TRI_MODE_INLINE = 1, TRI_MODE_POOL = 2, TRI_MODE_DEFER = 3, TRI_MODE_INLINE_PF = 4 };  // rt_pt_params.tune_tri_mode, byte 0 (pt_trace.hip: TRI_INLINE, TRI_POOL)

struct StackCfg {  // per-lane traversal stack of 8-byte entries: lds_cap in LDS, then spill_cap in global memory
    unsigned long long* spill;  // spill_cap x spill_stride entries, entry-major
    size_t spill_stride;  // = threads of the persistent grid
    int lds_cap, spill_cap;
};

struct PtState {  // SoA over path ids; one float4 per lane per array = 16-byte coalesced accesses
    float4* ray_o;
    float4* ray_d;
    float4* thr;   // path throughput
    float4* rad;   // accumulated radiance of the path
    float2* hit;   // t, leaf-order triangle index (int bits, -1 = miss)
    float4* sh_o;  // shadow queue: origin.xyz, path id bits
    float4* sh_d;  // shadow queue: unnormalised direction to the light sample
    float4* sh_c;  // shadow queue: contribution if unoccluded
};

struct PtFrame {
    Camera cam;
    uint32_t width, height;
    Partition part;
    uint32_t n_slots;    // owned tiles * 4096
    uint32_t n_paths;    // n_slots * spp_batch
    uint32_t spp_batch;  // samples in flight per pixel in this pass
    uint32_t sample0;    // first sample index of this pass
    uint32_t spp_total;
    uint32_t bounces;
    uint32_t seed;
    float sky[3];
    float ray_eps;
};

// rt_query_rays_device: the rays of one query and where their answers go.  Ray i is queue entry i.
struct RayQuery {
    const float* origins;  // n x 3
    const float* dirs;     // n x 3
    const float* tmax;     // n, or nullptr: +inf (closest hit) / 0.999 (any hit)
    float* t_out;          // n, closest hit only
    int* tri_out;          // n
    uint32_t n;
    float reach;  // |origin component| limit: kCameraReach x the mesh's maxabs
};
// rt_query_rays_attr_device: the same rays and answers, and where the winner's attributes go.  A struct of its own:
// the plain kernels keep their argument block.
struct RayAttrQuery : RayQuery {
    float* uv_out;      // n x 2, or nullptr
    float* normal_out;  // n x 3, or nullptr
};
// Counters of a ray query (QueryState's device block)
enum { RQ_STAT_INVALID = 0, RQ_STAT_OVERFLOW = 1, RQ_STAT_WORDS = 2 };

// rt_query_points_device: the points of one query and where their answers go.  Point i is queue entry i.
struct PointQuery {
    const float* points;  // n x 3
    const float* rmax;    // n, or nullptr: +inf
    float* dist_out;      // n
    int* tri_out;         // n
    float* point_out;     // n x 3, or nullptr
    uint32_t n;
    float reach;  // |component| limit: kCameraReach x the mesh's maxabs
};
// rt_query_points_attr_device
struct PointAttrQuery : PointQuery {
    float* uv_out;      // n x 2, or nullptr
    float* normal_out;  // n x 3, or nullptr
};
// Counters of a closest-point query
enum { PQ_STAT_INVALID = 0, PQ_STAT_OVERFLOW = 1, PQ_STAT_NODES = 2, PQ_STAT_TRIS = 3, PQ_STAT_WORDS = 4 };
// Stack entries the nearest-first walk of pt_query_points can hold at once in a tree of `depth` levels of 8-wide nodes (root = 1): an
// entry is one pending sibling, a node visit descends into one inner child and pushes at most seven, and the entries of one level
// on the stack are always children of one node (they lie above every entry of the levels before them and are popped first), so at
// most seven for each of the levels 2 .. depth.
constexpr uint32_t point_stack_need(uint32_t depth) { return depth > 1u ? 7u * (depth - 1u) : 1u; }

// rt_query_sides_device: the points of one query and where their answers go.  Point i is queue entry i.
struct SideQuery {
    const float* points;  // n x 3
    int* inside_out;      // n, or nullptr (rt_query_signed_distance_device without inside_out_dev)
    int* crossings_out;   // n x 3, or nullptr: the third walk only where the first two parities disagree
    float* dist_inout;    // n, or nullptr: +inf = not walked, NaN = invalid, else the sign is written into it
    uint32_t n;
    float reach;  // |component| limit: kCameraReach x the mesh's maxabs
};
// Counters of an inside/outside query
enum { SQ_STAT_INVALID = 0, SQ_STAT_OVERFLOW = 1, SQ_STAT_NODES = 2, SQ_STAT_TRIS = 3, SQ_STAT_SKIPPED = 4, SQ_STAT_WALKS = 5, SQ_STAT_THIRD = 6, SQ_STAT_WORDS = 7 };

// rt_count_ray_hits_device / rt_fill_ray_hits_device: the rays of one step and where its answers go.  Ray i is queue entry i.
struct HitQuery {
    const float* origins;  // n x 3
    const float* dirs;     // n x 3
    const float* tmax;     // n, or nullptr: +inf
    // the count step
    int* count_out;               // n, or nullptr
    unsigned long long* count64;  // n (the scan's input column: max(count, 0)), or nullptr
    // the fill step
    const long long* offsets;  // n + 1
    long long capacity;        // elements of key_out / tri_out
    float* key_out;            // t
    int* tri_out;
    uint32_t n;
    float reach;  // |origin component| limit: kCameraReach x the mesh's maxabs
};

// rt_count_neighbors_device / rt_fill_neighbors_device: the points of one step and where its answers go.  Point i is queue entry i.
struct NeighborQuery {
    const float* points;  // n x 3
    const float* rmax;    // n, or nullptr: rmax_all for every point
    float rmax_all;
    // the count step
    int* count_out;               // n, or nullptr
    unsigned long long* count64;  // n (the scan's input column: max(count, 0)), or nullptr
    // the fill step
    const long long* offsets;  // n + 1
    long long capacity;        // elements of key_out / tri_out
    float* key_out;            // dist (d2 until the lane retires)
    int* tri_out;
    uint32_t n;
    float reach;  // |component| limit: kCameraReach x the mesh's maxabs
};
// rt_count_overlaps_device / rt_fill_overlaps_device: the query triangles of one step and where its answers go.  Triangle i is queue entry i.
struct OverlapQuery {
    const float* tris;  // n x 9: the three vertices, rt_set_mesh's layout
    // the count step
    int* count_out;               // n, or nullptr
    unsigned long long* count64;  // n (the scan's input column: max(count, 0)), or nullptr
    // the fill step
    const long long* offsets;  // n + 1
    long long capacity;        // elements of key_out / tri_out
    int* key_out;              // the edge mask of each listed triangle
    int* tri_out;
    uint32_t n;
    float reach;  // |coordinate| limit: kCameraReach x the mesh's maxabs
};
// Waves per SIMD pt_query_overlaps is bounded to, = its workgroups per CU: at the neighbours' 8 (64 VGPRs) the six segment tests spill
// 9 - 23 registers to scratch, at 6 (75 - 79 VGPRs) nothing does (profiles/overlap_queries.txt); the host caps the persistent grid to it.
constexpr int kOverlapWaves = 6;
// rt_overlap_segments_device: an overlap list and where the segment of each of its entries goes.  Entry k is lane k.
struct SegmentQuery {
    const float* tris;         // n x 9: the query triangles the list was made for
    const long long* offsets;  // n + 1: the list's slices; offsets[n] is read on the device
    const int* tri;            // capacity: the listed mesh triangles, original indices
    long long capacity;        // elements of tri, ends_out; rows of seg_out
    float* seg_out;            // capacity x 6
    int* ends_out;             // capacity, or nullptr
    uint32_t n;
    float reach;  // |coordinate| limit: kCameraReach x the mesh's maxabs
};
// Counters of a segment call (TOUCHES, SKIPPED, BAD in this order: one thread each adds them); segments = entries - the other three
enum { SG_STAT_ENTRIES = 0, SG_STAT_TOUCHES = 1, SG_STAT_SKIPPED = 2, SG_STAT_BAD = 3, SG_STAT_WORDS = 4 };
// rt_query_clearance_device: the query triangles of one query and where their answers go.  Triangle i is queue entry i.
struct ClearanceQuery {
    const float* tris;       // n x 9: the three vertices, rt_set_mesh's layout
    const float* rmax;       // n, or nullptr: +inf
    int* tri_out;            // n
    float* dist_out;         // n
    float* point_query_out;  // n x 3, or nullptr: the nearest point on the query triangle
    float* point_mesh_out;   // n x 3, or nullptr: the nearest point on the mesh triangle
    uint32_t n;
    float reach;  // |coordinate| limit: kCameraReach x the mesh's maxabs
};
// Counters of a clearance query
enum { CQ_STAT_INVALID = 0, CQ_STAT_OVERFLOW = 1, CQ_STAT_NODES = 2, CQ_STAT_TRIS = 3, CQ_STAT_WORDS = 4 };
// Waves per SIMD pt_query_clearance is bounded to, = its workgroups per CU (the compiler's figures: DESIGN.md §6.22); the host caps the
// persistent grid to it.
constexpr int kClearanceWaves = 4;
// rt_query_knn_device: the points of one query and where their rows go.  Point i is queue entry i; its row is
// elements i * k .. i * k + k - 1 of dist_out and tri_out (64-bit addressing: n x k reaches 2^40).
struct KnnQuery {
    const float* points;  // n x 3
    const float* rmax;    // n, or nullptr: +inf
    float* dist_out;      // n x k (d2 until the lane retires)
    int* tri_out;         // n x k
    int* count_out;       // n, or nullptr
    uint32_t n, k;
    float reach;  // |component| limit: kCameraReach x the mesh's maxabs
};
// Counters of a k-nearest query
enum { KQ_STAT_INVALID = 0, KQ_STAT_OVERFLOW = 1, KQ_STAT_NODES = 2, KQ_STAT_TRIS = 3, KQ_STAT_NEIGHBORS = 4, KQ_STAT_WORDS = 5 };
// rt_query_sweeps_device: the sphere casts of one query and where their answers go.  Item i is queue entry i.
struct SweepQuery {
    const float* origins;  // n x 3
    const float* dirs;     // n x 3
    const float* radius;   // n
    const float* tmax;     // n, or nullptr: +inf
    float* t_out;          // n
    int* tri_out;          // n
    float* point_out;      // n x 3, or nullptr: the contact point
    uint32_t n;
    float reach;  // |origin component| and radius limit: kCameraReach x the mesh's maxabs
};
// Counters of a sphere-cast query (SQ_ is the sides')
enum { WQ_STAT_INVALID = 0, WQ_STAT_OVERFLOW = 1, WQ_STAT_NODES = 2, WQ_STAT_TRIS = 3, WQ_STAT_HITS = 4, WQ_STAT_WORDS = 5 };
// Waves per SIMD pt_query_sweeps is bounded to, = its workgroups per CU (the compiler's figures: DESIGN.md §6.24); the host caps the
// persistent grid to it.
constexpr int kSweepWaves = 4;
// Counters of a listing query (all hits, neighbours, overlaps): one set per step (the fill step's LQ_STEP_WORDS words behind the count step's),
// so that the two launches of a list call report side by side.  FOUND: hits / neighbours met.
enum { LQ_STAT_INVALID = 0, LQ_STAT_OVERFLOW = 1, LQ_STAT_NODES = 2, LQ_STAT_TRIS = 3, LQ_STAT_FOUND = 4, LQ_STAT_WRITTEN = 5, LQ_STAT_INCOMPLETE = 6,
       LQ_STAT_SLICE_OVERFLOW = 7, LQ_STEP_WORDS = 8, LQ_STAT_WORDS = 2 * LQ_STEP_WORDS };

struct MeshHost {  // host side of a two-level mesh: what rt_update_mesh_chunk needs to rebuild one chunk
    TwoLevelBvh tl;
    std::vector<float> v0, e1, e2;          // original triangle order
    std::vector<float> albedo, emission;    // original triangle order, 3 floats each
    std::vector<uint32_t> light_ids;        // emissive triangles, ascending
    std::vector<float> surf;                // albedo.w per triangle, original order (rt_set_mesh_surfaces); empty = all Lambert
};

// Move-only owner of one hipMalloc allocation
struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <class T>
using DevPtr = std::unique_ptr<T, HipFree>;

template <class T>
bool dalloc(DevPtr<T>& p, size_t count) {  // frees what p held first; false: out of device memory, p is empty
    p.reset();
    T* raw = nullptr;
    if (hipMalloc((void**)&raw, count * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    p.reset(raw);
    return true;
}

// The other handles of a context, each with its owner (rt_owned.h).  The make_* helpers free what the owner held first and leave it
// empty on failure.
inline void destroy_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void destroy_stream(hipStream_t s) { (void)hipStreamDestroy(s); }
inline void free_pinned(void* p) { (void)hipHostFree(p); }
struct Frames;                      // the frames-in-flight slots (rt_abi_frames.hip)
void frames_release(Frames* f);     // rt_abi_frames.hip: waits for the frames in flight, then every slot goes
void comm_destroy(ncclComm* comm);  // rt_abi_comm.hip: ncclCommDestroy, found at run time
using Event = Owned<hipEvent_t, destroy_event>;
using Stream = Owned<hipStream_t, destroy_stream>;
using Pinned = Owned<void*, free_pinned>;
using Lane = Owned<rt_ctx*, rt_destroy>;  // a child context
using FramesPtr = Owned<Frames*, frames_release>;
using CommPtr = Owned<ncclComm*, comm_destroy>;

inline hipError_t make_event(Event& ev, unsigned flags = hipEventDefault) {  // (hipEventDefault: what hipEventCreate makes)
    ev.reset();
    hipEvent_t raw = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&raw, flags);
    if (e == hipSuccess) ev.reset(raw);
    return e;
}
inline hipError_t make_stream(Stream& s, unsigned flags, const int* priority = nullptr) {
    s.reset();
    hipStream_t raw = nullptr;
    const hipError_t e = priority ? hipStreamCreateWithPriority(&raw, flags, *priority) : hipStreamCreateWithFlags(&raw, flags);
    if (e == hipSuccess) s.reset(raw);
    return e;
}
inline hipError_t make_pinned(Pinned& p, size_t bytes) {
    p.reset();
    void* raw = nullptr;
    const hipError_t e = hipHostMalloc(&raw, bytes, hipHostMallocDefault);
    if (e == hipSuccess) p.reset(raw);
    return e;
}
// The HIP call that a helper makes at each first-use site, as that site's failure message names it (RT_HIP_AS): the text is part of
// the message, like the code, and names the call by what it creates
constexpr char kTextEventCreate[] = "hipEventCreate(&e)";  // a query kind's and the refit's events
constexpr char kTextAuxStream[] = "hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking)";
constexpr char kTextEvShaded[] = "hipEventCreateWithFlags(&c->pt.ev_shaded, hipEventDisableTiming)";
constexpr char kTextEvShadowed[] = "hipEventCreateWithFlags(&c->pt.ev_shadowed, hipEventDisableTiming)";

// What a context keeps per query kind.  The device block is PT_HEADS stream heads (PT_HEAD_STRIDE words apart), then the kind's
// 64-bit counters; it is cleared before every launch.  One block per kind: a query's counters stay until rt_get_*_query_stats reads
// them, whatever the other kinds do meanwhile.  The block and the two events are made together by the kind's first query (ensure_block,
// rt_abi_query.hip: all of them or none) and go with the context.
constexpr size_t kQueryHeadBytes = (size_t)PT_HEADS * PT_HEAD_STRIDE * sizeof(uint32_t);
constexpr size_t query_block_bytes(uint32_t n_counters) { return kQueryHeadBytes + (size_t)n_counters * sizeof(unsigned long long); }
struct QueryState {
    QueryState(uint32_t k, const char* what, uint32_t lds, uint32_t halves) : n_counters(k), name(what), fixed_lds_bytes(lds), spill_halves(halves) {}
    uint32_t n_counters;  // RQ_STAT_WORDS / PQ_STAT_WORDS / SQ_STAT_WORDS / LQ_STAT_WORDS / SG_STAT_WORDS / CQ_STAT_WORDS / KQ_STAT_WORDS / WQ_STAT_WORDS
    const char* name;     // for messages
    uint32_t fixed_lds_bytes, spill_halves;  // pt_stack_config's: the kernel's LDS beside the stacks, the sets of spill columns it is given
    DevPtr<char> block;
    Event ev[2];  // around the launch
    bool pending = false;  // a query has been enqueued whose counters and time rt_get_*_query_stats has not read yet
};
// One query kind in a context: what is in flight and the public statistics of the kind's last query (what the host knows at the
// enqueue; rt_get_*_query_stats adds the counters and the time)
template <class Stats>
struct QueryKind {
    QueryKind(uint32_t k, const char* what, uint32_t lds, uint32_t halves) : qs(k, what, lds, halves) {}
    QueryState qs;
    Stats stats{};
};
// A listing kind (no LDS beside the stacks, one set of spill columns: one group per level) and its pending call's steps
template <class Stats>
struct ListingKind : QueryKind<Stats> {
    explicit ListingKind(const char* what) : QueryKind<Stats>(LQ_STAT_WORDS, what, 0u, 1u) {}
    uint32_t steps = 0;  // bit 0: the count step ran, bit 1: the fill step
};
// Device scratch that grows by size class (powers of two), first use only
template <class T>
struct Scratch {
    DevPtr<T> d;
    size_t words = 0;
};
// Every query kind of a context, and the scratch two of them keep; nothing outside rt_abi_query.hip looks inside.  A new kind is a
// member here and its entries there.
struct Queries {
    // (rays: the 2 KiB octant table, two spill halves as the frames hold; the others: no table, one set of columns)
    QueryKind<rt_ray_query_stats> rays{RQ_STAT_WORDS, "ray-query", 2048u, 2u};
    QueryKind<rt_point_query_stats> points{PQ_STAT_WORDS, "point-query", 0u, 1u};
    QueryKind<rt_side_query_stats> sides{SQ_STAT_WORDS, "side-query", 0u, 1u};
    ListingKind<rt_hit_query_stats> hits{"hit-query"};                 // rt_count / fill / list_ray_hits_device
    ListingKind<rt_neighbor_query_stats> neighbors{"neighbor-query"};  // rt_count / fill / list_neighbors_device
    ListingKind<rt_overlap_query_stats> overlaps{"overlap-query"};     // rt_count / fill / list_overlaps_device
    // rt_overlap_segments_device: a flat kernel, no stack (the block's stream heads stay unused)
    QueryKind<rt_overlap_segment_stats> segments{SG_STAT_WORDS, "overlap-segments", 0u, 0u};
    QueryKind<rt_clearance_query_stats> clearance{CQ_STAT_WORDS, "clearance-query", 0u, 1u};  // rt_query_clearance_device: the points' walk, one set of columns
    QueryKind<rt_knn_query_stats> knn{KQ_STAT_WORDS, "knn-query", 0u, 1u};                    // rt_query_knn_device: the points' walk, one set of columns
    QueryKind<rt_sweep_query_stats> sweeps{WQ_STAT_WORDS, "sweep-query", 0u, 1u};             // rt_query_sweeps_device: the points' walk, one set of columns
    // rt_overlap_segments_device: original triangle index -> leaf position of the current mesh, rewritten by every call; the context's own
    // (a DeviceMesh is shared read-only, §6.12)
    Scratch<uint32_t> tri_inverse;
    // the listing kinds' scan: the 64-bit count column (n + 1), the scan's tile sums and its total
    Scratch<unsigned long long> list_scan;
};

// A mesh resident on the device: the arrays the kernels read and what the host knows about them.  Made by the host build
// (rt_abi_mesh.hip) or by build_bvh_device.  Contexts hold it through a shared pointer (PtData::own): contexts that were given the same host
// mesh hold the same record and treat it as read-only; whoever writes into it makes sure first that it is the only holder (detach_mesh,
// DESIGN.md §6.12).  A context's frame-slot lanes read it through a plain pointer.
struct DeviceMesh {
    DevPtr<float4> nodes;     // cap_nodes x 80 B of which n_nodes are used, bvh_node.h layout
    DevPtr<float4> tris;      // leaf order, 48 B per triangle (PtScene::tris)
    DevPtr<float4> albedo;    // leaf order
    DevPtr<float4> emission;  // leaf order
    DevPtr<uint32_t> lights;  // max(n_lights, 1) entries
    uint32_t n_tris = 0, n_nodes = 0, n_lights = 0, depth = 0;
    uint32_t stack_need = 0;  // worst-case traversal stack occupancy reported by the builder
    float pad = 0.0f, maxabs = 1.0f, build_ms = 0.0f;  // maxabs = max(1, largest |vertex coordinate|): what the padding covers
    size_t cap_nodes = 0;       // nodes the node array has room for
    bool has_surfaces = false;  // some triangle is a mirror or glass (albedo.w != 0): frames take pt_shade<true>, DESIGN.md §6.11
    // single-level meshes: level d of the breadth-first tree = nodes [level_start[d], level_start[d + 1]) (empty: no refit)
    std::vector<uint32_t> level_start;
    std::unique_ptr<MeshHost> host;  // two-level meshes only
};

struct PtData {  // device residency of one mesh + the wavefront buffers
    std::shared_ptr<DeviceMesh> own;       // the mesh this context holds, alone or with other contexts (empty: none)
    const DeviceMesh* borrowed = nullptr;  // frame-slot lanes: the parent's mesh, which the parent takes back (frames_drop_mesh) before it frees or replaces it
    const DeviceMesh& mesh() const {       // what frames render (n_tris = 0: nothing)
        static const DeviceMesh none;
        return borrowed ? *borrowed : own ? *own : none;
    }
    MeshHost* host() const { return own ? own->host.get() : nullptr; }  // lanes do not see it
    // rt_refit_mesh_device: scratch (refit_scratch_size) and timing events, made together by the first refit (all of them or none), go with the mesh
    DevPtr<char> d_refit;
    Event ev_refit[2];
    DevPtr<unsigned long long> d_spill;
    size_t spill_words = 0;
    Event ev_shaded, ev_shadowed;  // ordering between the main and the auxiliary stream; made together by the first frame on two streams
    std::vector<Event> ev_pool;    // profile_stages: timing events, created on this context's device
    // wavefront buffers, sized for cap_paths; st, d_queue and d_acc point into the allocations `wavefront` owns
    uint64_t cap_paths = 0;
    DevPtr<char> wavefront[11];
    PtState st{};
    uint32_t* d_queue[2] = {nullptr, nullptr};
    float* d_acc = nullptr;  // per-slot running sums across sample batches
    uint64_t cap_slots = 0;
    DevPtr<uint32_t> d_ctr;
    DevPtr<unsigned long long> d_stats;  // PT_STAT_WORDS words
    rt_pt_stats stats{};
    // the query kinds (rays, closest points, sides, all hits, neighbours, overlaps, overlap segments, clearance, k-nearest): what is in
    // flight, the statistics of the last query of each kind and their scratch
    Queries queries;
};

struct Ctx {
    int device = -1;
    // The two streams are declared before everything that has ever been used on them: members go in reverse order, so the streams go last
    // (rt_destroy's step 6)
    Stream own_stream;
    Stream aux_stream;             // path B: shadow kernel beside the next closest-hit kernel; made by the first frame that wants it
    hipStream_t stream = nullptr;  // own_stream, or the caller's (rt_set_stream): borrowed, never destroyed
    std::string err;

    rt_config cfg{};
    bool have_scene = false;
    rt_mutable_data scene{};

    uint32_t width = 0, height = 0;
    float ratio[2] = {1.0f, 1.0f};
    uint32_t level_count = 0;
    uint32_t dims[RT_MAX_LEVELS][2] = {};
    DevPtr<float> d_level[RT_MAX_LEVELS];  // level i: level_batch images of dims[i], one per sample of a batch
    uint32_t level_batch = 0;              // images allocated per level
    uint32_t last_image = 0;               // image of the batch that holds the last sample rendered
    uint32_t last_sample0 = 0;             // sample index of image 0 of that batch (rt_read_level_image)
    DevPtr<float> d_rgb;                   // full frame, f32 x 3
    float* d_chain = nullptr;  // borrowed, set only inside rt_render_chains (which owns the records): the shade launch records the secondary marches here
    DevPtr<uint8_t> d_rgba8;   // rt_read_rgba8 staging, width*height*4, allocated on first use, goes with the frame
    DevPtr<uint64_t> d_counters;  // 4 x 1024 slots: hit pixels, secondary hits shaded, mirror rays, transmitted rays; summed on the host; + 1 word: d_chain for the recording kernel
    Partition part{0, 1, 0, 0};

    Event ev_begin, ev_end;
    Event ev_stage[RT_MAX_LEVELS + 2];  // profile_stages
    rt_stats stats{};
    bool frame_valid = false;
    PtData pt;
    int n_cus = 256;
    FramesPtr frames;  // frames-in-flight slots (rt_abi_frames.hip); their lanes borrow pt's mesh and go before it (rt_destroy's step 3)
    uint64_t state_version = 1;  // bumped by rt_set_config / rt_set_scene / rt_set_mesh: frame-slot lanes re-sync on submit
    CommPtr comm;  // once rt_comm_init ran (rt_abi_comm.hip)
    uint32_t comm_rank = 0, comm_ranks = 1;

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

// RT_HIP_AS: the message names `text` instead of the expression: for a call through a make_* helper, whose message names the HIP call
#define RT_HIP_AS(ctx, text, call)                                                                 \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return (ctx)->fail(RT_ERR_HIP, "%s: %s", text, hipGetErrorString(e_)); \
    } while (0)
#define RT_HIP(ctx, call) RT_HIP_AS(ctx, #call, call)

inline int bind(Ctx* c) {
    RT_HIP(c, hipSetDevice(c->device));
    return RT_OK;
}

inline uint32_t owned_tiles(const Partition& p) {
    const uint32_t total = p.tiles_x * p.tiles_y;
    return total > p.rank ? (total - p.rank + p.n_ranks - 1u) / p.n_ranks : 0u;
}

void frames_drop_mesh(Ctx* c);     // rt_abi_frames.hip: the parent's mesh is about to be freed: idle the lanes, forget the borrowed mesh
void pt_borrow_mesh(Ctx* lane, const Ctx* owner);  // rt_abi_mesh.hip: lane renders with owner's device mesh
void pt_free_mesh(PtData& pt);     // rt_abi_mesh.hip: this context's hold on its mesh (held or borrowed) and everything sized for it

// path_a.hip
int launch_cone_level(Ctx* c, const SphereSet& spheres, uint32_t n_obj, const ConeLevelParams& p, const float* parent,
                      float* out, uint32_t batch);
// chain (rt_render_chains only): the recording kernel; the address of the records ((reflections + transmissions) x 7 floats per
// pixel of the full frame) stands in counters[4096], the word behind the four groups of counter slots
int launch_shade(Ctx* c, const ShadeSet& set, uint32_t n_obj, const ShadeParams& p, const float* depth, float* dst,
                 uint64_t* counters, bool chain = false);
int launch_pyramid_fused(Ctx* c, const SphereSet& spheres, uint32_t n_obj, const PyramidParams& fp);
int launch_selftest_sqrt(Ctx* c, unsigned long long* mismatches_dev);
int launch_detile(Ctx* c, const float* tiles, uint32_t n_ranks, uint32_t tiles_per_rank, float* rgb);
int launch_to_rgba8(Ctx* c, const float* rgb, uint8_t* rgba, uint64_t n_pixels);

// path_b.hip (generate, shade, scatter_surfaces, resolve), pt_trace.hip (trace, trace_fused, pool_lds_bytes, trace_rays, query_rays), pt_packet.hip (trace_packet),
// pt_point_query.hip (query_points), pt_side_query.hip (query_sides), pt_hit_query.hip (query_hits), pt_neighbor_query.hip (query_neighbors), pt_overlap_query.hip (query_overlaps), pt_knn_query.hip (query_knn), pt_sweep_query.hip (query_sweeps): every unit ends with the launchers of its own kernels
int launch_pt_generate(Ctx* c, const PtFrame& f, const PtState& st, uint32_t* queue, uint32_t* ctr);
int launch_pt_trace(Ctx* c, hipStream_t stream, const PtScene& sc, const PtState& st, const uint32_t* queue, const uint32_t* count_ptr, uint32_t* head,
                    unsigned long long* stats, bool any_hit, bool count, uint32_t grid, const StackCfg& stack_cap, uint32_t refill_min, uint32_t tri_mode,
                    uint32_t tri_cfg);  // on `stream` (c->stream or c->aux_stream)
int launch_pt_trace_fused(Ctx* c, const PtScene& sc, const PtState& st, const uint32_t* queue, const uint32_t* closest_count, uint32_t* closest_head,
                          const uint32_t* shadow_count, uint32_t* shadow_head, unsigned long long* stats, bool count, uint32_t grid,
                          const StackCfg& stack_cap, uint32_t refill_min, uint32_t tri_mode, uint32_t tri_cfg);
uint32_t pt_pool_lds_bytes(uint32_t tri_mode);  // static LDS a 256-thread workgroup of the per-lane kernels needs beyond the stacks and the octant table
int launch_pt_trace_packet(Ctx* c, const PtScene& sc, const PtFrame& f, const PtState& st, unsigned long long* stats, bool count, uint32_t mode);
int launch_pt_shade(Ctx* c, const PtScene& sc, const PtFrame& f, const PtState& st, const uint32_t* queue, const uint32_t* count_ptr,
                    uint32_t depth, uint32_t* next_queue, uint32_t* next_ctr, uint32_t grid, uint32_t sort_rays, bool surfaces);
// albedo.w of the n leaf-order triangles from surf[original index] (nullptr: all 0 = Lambert), on c->stream
int launch_pt_scatter_surfaces(Ctx* c, const float4* tris, const float* surf, float4* albedo, uint32_t n);
int launch_pt_resolve(Ctx* c, const PtFrame& f, const PtState& st, float* acc, float* dst, int tile_major);
int launch_pt_trace_rays(Ctx* c, const PtScene& sc, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out,
                         int* tri_out, uint32_t* counts, const StackCfg& sk, uint32_t grid);
// persistent refilling query kernels on c->stream; head / stats: the two parts of the kind's QueryState block, cleared by the caller
int launch_pt_query_rays(Ctx* c, const PtScene& sc, const RayQuery& q, bool any_hit, uint32_t* head, unsigned long long* stats, uint32_t grid,
                         const StackCfg& sk, uint32_t refill_min);
int launch_pt_query_points(Ctx* c, const PtScene& sc, const PointQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                           const StackCfg& sk, uint32_t refill_min);
// the ATTR instantiations (closest hit only; q.uv_out / q.normal_out, either may be nullptr)
int launch_pt_query_rays_attr(Ctx* c, const PtScene& sc, const RayAttrQuery& q, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                              uint32_t refill_min);
int launch_pt_query_points_attr(Ctx* c, const PtScene& sc, const PointAttrQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                                const StackCfg& sk, uint32_t refill_min);
int launch_pt_query_sides(Ctx* c, const PtScene& sc, const SideQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                          const StackCfg& sk, uint32_t refill_min);  // q.crossings_out != nullptr: all three walks for every point
// fill = false: the count step (q.count_out / q.count64), true: the fill step (q.offsets, q.capacity, q.key_out, q.tri_out); stats: the step's own LQ_STEP_WORDS
int launch_pt_query_hits(Ctx* c, const PtScene& sc, const HitQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                         const StackCfg& sk, uint32_t refill_min);
// the same two steps of a neighbour query
int launch_pt_query_neighbors(Ctx* c, const PtScene& sc, const NeighborQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min);
// the same two steps of an overlap query (pt_overlap_query.hip)
int launch_pt_query_overlaps(Ctx* c, const PtScene& sc, const OverlapQuery& q, bool count, bool fill, uint32_t* head, unsigned long long* stats, uint32_t grid,
                             const StackCfg& sk, uint32_t refill_min);
// pt_overlap_segments.hip: inv[original index] = leaf position over the mesh's records; one lane per entry of an overlap list (stats: SG_STAT_WORDS words)
int launch_pt_tri_inverse(Ctx* c, const PtScene& sc, uint32_t* inv);
int launch_pt_overlap_segments(Ctx* c, const PtScene& sc, const SegmentQuery& q, const uint32_t* inv, unsigned long long* stats);
// pt_clearance_query.hip: the persistent refilling clearance kernel (stats: CQ_STAT_WORDS words)
int launch_pt_query_clearance(Ctx* c, const PtScene& sc, const ClearanceQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid,
                              const StackCfg& sk, uint32_t refill_min);
// pt_knn_query.hip: the persistent refilling k-nearest kernel (stats: KQ_STAT_WORDS words)
int launch_pt_query_knn(Ctx* c, const PtScene& sc, const KnnQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                        uint32_t refill_min);
// pt_sweep_query.hip: the persistent refilling sphere-cast kernel (stats: WQ_STAT_WORDS words)
int launch_pt_query_sweeps(Ctx* c, const PtScene& sc, const SweepQuery& q, bool count, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                           uint32_t refill_min);

// |coordinate| limit of a camera position, a query ray's origin and a query point in units of DeviceMesh::maxabs (plan_frame, rt_abi_pt.hip)
constexpr float kCameraReach = 32.0f;
// Largest DeviceMesh::maxabs that path B renders and queries: 2^RT_PT_MAX_COORD_LOG2.  Up to it no intermediate of a path B operation
// overflows (DESIGN.md sections 6.3 and 6.19); rt_set_mesh*, the refit, a chunk update and rt_read_bvh take every finite mesh.
constexpr float kMaxCoord = (float)(1u << RT_PT_MAX_COORD_LOG2);
// The refusal of a render or a query on a mesh beyond it: one host comparison, before anything is enqueued or written
inline int check_mesh_domain(Ctx* c, const DeviceMesh& mesh) {
    if (!(mesh.maxabs <= kMaxCoord))
        return c->fail(RT_ERR_INVALID, "the mesh's largest |coordinate| %g is above the limit %g (2^%u) of path B's renders and queries: beyond it fp32 intermediates overflow",
                       (double)mesh.maxabs, (double)kMaxCoord, (unsigned)RT_PT_MAX_COORD_LOG2);
    return RT_OK;
}
inline PtScene scene_view(const DeviceMesh& m) {
    PtScene s{};
    s.nodes = m.nodes.get();
    s.tris = m.tris.get();
    s.albedo = m.albedo.get();
    s.emission = m.emission.get();
    s.lights = m.lights.get();
    s.n_lights = m.n_lights;
    s.n_tris = m.n_tris;
    return s;
}
inline size_t spill_half_words(const StackCfg& sk) { return (sk.spill_cap > 1 ? (size_t)sk.spill_cap : 1) * sk.spill_stride; }
// rt_abi_pt.hip: traversal stack + persistent grid of one launch over n_items rays or points.  need: worst-case entries per lane; fixed_lds_bytes:
// a workgroup's LDS beside its stacks; spill_halves: sets of spill columns (spill_half_words each) that PtData::d_spill must hold at once.
int pt_stack_config(Ctx* c, uint32_t need, uint32_t fixed_lds_bytes, uint32_t spill_halves, uint32_t tune_lds, uint32_t tune_blocks, uint64_t n_items,
                    StackCfg* sk, uint32_t* grid);
// rt_abi_mesh.hip: RT_OK when p is a device allocation of c's device that holds at least `bytes` bytes from p on, else RT_ERR_INVALID
int check_device_array(Ctx* c, const void* p, size_t bytes, const char* what);

// bvh_build_gpu.hip: path B mesh built on the GPU from device-resident triangles (rt_set_mesh_device), on c->stream.
// On failure *out is empty and nothing else has changed.
int build_bvh_device(Ctx* c, const float* verts, const float* albedo, const float* emission, uint32_t n, DeviceMesh* out);

// bvh_build_gpu.hip: refit of a single-level mesh to new vertices (rt_refit_mesh_device), on c->stream, in two steps.
// refit_measure validates verts and returns the largest |coordinate| (build_bvh's maxabs, before the max with 1); it writes only
// the scratch, so a refusal (RT_ERR_INVALID: a non-finite coordinate) leaves the mesh as it was.  refit_write rewrites words 0-8 of
// every triangle record and every node's box words bottom-up, one launch per level (the top levels in one workgroup), and is
// synchronous on return; *ms = HIP-event time from `begin` (recorded by refit_measure) to its last kernel.
size_t refit_scratch_size(uint32_t n_nodes);  // exact node boxes (24 B per node) + the validation partials
int refit_measure(Ctx* c, const float* verts, uint32_t n, void* scratch, hipEvent_t begin, float* maxabs);
int refit_write(Ctx* c, const float* verts, uint32_t n, float pad, uint32_t n_nodes, float4* nodes, float4* tris, const std::vector<uint32_t>& level_start,
                void* scratch, hipEvent_t begin, hipEvent_t end, float* ms);

// bvh_build_gpu.hip: the build's exclusive scan (three launches on c->stream, 4096-element tiles) of `count` 64-bit words: out[i] = in[0] + ..
// + in[i - 1], *total = the sum of all.  sums: scan_u64_sums_words(count) words of scratch.  in and out are different arrays.
size_t scan_u64_sums_words(size_t count);
int scan_u64_device(Ctx* c, const unsigned long long* in, unsigned long long* out, size_t count, unsigned long long* sums, unsigned long long* total);

}  // namespace rt
