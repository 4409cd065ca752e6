/*
 * rt_abi.h — C ABI of librt_amd.so: the MI355X (gfx950) replacement for the GPU hot path of
 * IvoteSligte/raytracing_engine (per-pixel ray/scene intersection + shading).
 *
 * The reference has no FFI/plugin API for this path: its host (src/main.rs) reaches the GLSL
 * kernels through vulkano descriptor sets and push constants.  The drop-in boundary is therefore
 * that binding contract, restated as plain C:
 *
 *   reference interface (file:line in the reference repo)          replaced by
 *   -------------------------------------------------------------  ---------------------------
 *   Vulkan instance/device/queue selection  src/main.rs:418-460    rt_create / rt_destroy
 *   spec-const RENDER_DIST  src/main.rs:521,636; compute.glsl:32;
 *     GLSL consts fragment.glsl:35-37                              rt_set_config
 *   set0/binding1 MutableData UBO upload  src/main.rs:593-605      rt_set_scene
 *   ConstantBuffer{view,ratio} + image pyramid allocation
 *     src/main.rs:203-266, 608-615, 639-648, resize :813-861       rt_resize / rt_level_info
 *   get_command_buffer: per-level push constants + dispatch,
 *     then the full-screen draw  src/main.rs:268-341;
 *     submit + fence  src/main.rs:909-927                          rt_render / rt_render_spp /
 *                                                                  rt_render_device
 *   swapchain *_UNORM colour attachment  src/main.rs:471-486       rt_read_rgba8
 *   (none: the reference cannot read a pyramid level back)         rt_read_level / rt_read_level_image / rt_render_chains  [test hooks]
 *   FPS println  src/main.rs:719,730                               rt_get_stats
 *   swapchain images + one fence per image: wait the image's fence,
 *     record, submit after the previous frame, present
 *     src/main.rs:664-667, 882-927                                 rt_frames_configure /
 *                                                                  rt_frame_submit(_pt) /
 *                                                                  rt_frame_wait / rt_frame_poll
 *
 * Conventions: every function returns RT_OK (0) or a negative rt_status and never throws or
 * aborts across the boundary; the caller owns every host/device pointer it passes; the context
 * owns all device memory it allocates; one context is bound to one GPU and is single-threaded
 * (like the reference's single queue, src/main.rs:460); distinct contexts are independent (one
 * per GPU / per process).  There is NO CPU fallback: rt_create fails with RT_ERR_NO_DEVICE when
 * no gfx950 device is usable.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,   /* bad argument (NULL, size mismatch, out-of-range count) */
    RT_ERR_NO_DEVICE = -2, /* no usable HIP device / ordinal out of range */
    RT_ERR_HIP = -3,       /* a HIP runtime call failed; see rt_last_error */
    RT_ERR_STATE = -4,     /* call order violated (e.g. render before set_scene/resize) */
    RT_ERR_OOM = -5        /* host or device allocation failed */
} rt_status;

#define RT_MAX_MATERIALS 8u /* shaders/utilities.glsl:2 */
#define RT_MAX_OBJECTS 8u   /* shaders/utilities.glsl:3 */
#define RT_MAX_LIGHTS 8u    /* shaders/utilities.glsl:4 */
#define RT_MAX_LEVELS 9u    /* shaders/compute.glsl:14-15; src/main.rs:359 */
#define RT_TILE 64u         /* multi-GPU framebuffer tile edge in full-resolution pixels */

/* std140 images of the reference's shader structs, byte-identical to what
 * vulkano_shaders::shader! generates (src/main.rs:47-66; fields at :524-591), so the
 * reference's own `shaders::ty::MutableData` can be passed by pointer. */
typedef struct rt_material { float color[3]; float diffuse; float specular; float shine; float ambient; uint32_t _pad; } rt_material; /* 32 B, utilities.glsl:8-14 */
typedef struct rt_object { float pos[3]; float size; } rt_object;                                                            /* 16 B, utilities.glsl:16-19 */
typedef struct rt_light { float pos[3]; uint32_t _pad0; float color[3]; uint32_t _pad1; } rt_light;                          /* 32 B, utilities.glsl:21-24 */
typedef struct rt_mutable_data { /* compute.glsl:17-24 == fragment.glsl:17-24; 656 B */
    uint32_t matCount, objCount, lightCount, _pad;
    rt_material mats[RT_MAX_MATERIALS];
    rt_object objs[RT_MAX_OBJECTS];
    rt_light lights[RT_MAX_LIGHTS];
} rt_mutable_data;

/* constants the reference bakes in at pipeline-creation / shader-compile time */
typedef struct rt_config {
    float render_dist;    /* RENDER_DIST = 1000   src/main.rs:362 */
    float cam_fall_off;   /* CAM_FALL_OFF = 0.01  fragment.glsl:35 */
    float light_fall_off; /* LIGHT_FALL_OFF = 0.01 fragment.glsl:36 */
    float ray_radius;     /* RAY_RADIUS = 0.01    fragment.glsl:37 */
    uint32_t max_steps;   /* cap on either march loop so every wave terminates (default 1<<20; 0 = none) */
    uint32_t profile_stages; /* 1: bracket every kernel with HIP events (rt_get_stats.stage_ms) */
    uint32_t fuse_levels;    /* 0 (default): one launch per level, the reference's schedule (src/main.rs:300-316);
                                1: the whole depth pyramid in one launch (parent levels kept in LDS; measured slower).
                                Same results; in fused mode level texels without a descendant inside the frame are left 0 */
    /* SDF feature growth the author sketched; 0 / {0,0,0} = the reference as shipped.  Both need fuse_levels = 0. */
    uint32_t march_algorithm; /* cone-march loop body: 0 or 3 = compute.glsl:46-65 ("algorithm 3");
                                 1, 2 = shaders/tracing_algorithms.txt:2-13 / :16-37 in the same loop */
    float repeat[3];          /* > 0: domain repetition period on that axis, repeat() of utilities.glsl:31-34,
                                 applied to the position of every SDF evaluation and of the surface normal */
    uint32_t reflections;     /* mirror bounces, 0..8 (shaders/fragment.glsl:125 "TODO: reflection"; build-defined): after
                                 shading a hit P seen along `step`, r = reflect(step, normal) starts one unit off the surface
                                 (the shadowRay idiom, fragment.glsl:176) and is marched by compute.glsl's loop (:44-66) with
                                 cone threshold RAY_RADIUS: len = 1 + traceCone(P + r, r, RAY_RADIUS); a hit at
                                 P + r * max(len, 0) is shaded by fragment.glsl:144-186 with P as the eye and added with
                                 weight prod(reflectivity * mat.specular) over the surfaces passed */
    float reflectivity;       /* 0..1, default 0.5 (mat.specular, which the reference never reads, scales it per material) */
    uint32_t transmissions;   /* spheres a transmitted ray may cross, 0..8 (shaders/fragment.glsl:124 "TODO: transparency", :126 "TODO:
                                 refraction"; build-defined): after shading a hit P on sphere S seen along I (outward normal n) the ray
                                 enters S - straight on for refraction_index == 1, else T = normalize(refract(I, n, 1 / index)) -
                                 crosses it to the far side in closed form (oc = domain(P) - S.pos, b = oc.T,
                                 disc = b*b - (oc.oc - S.size^2), t = max(disc > 0 ? sqrt(disc) - b : 0, 0), Q = P + T t), leaves along
                                 D = T or normalize(refract(T, -n2, index)) with n2 = normalize(oc + T t) (total internal reflection
                                 ends the chain), and is marched like a mirror ray: len = 1 + traceCone(Q + D, D, RAY_RADIUS); a hit at
                                 Q + D * max(len, 0) is shaded by fragment.glsl:144-186 with Q as the eye and added with weight
                                 prod(transparency * mat.diffuse) over the surfaces passed.  Starts at the camera ray's hit,
                                 independent of the mirror chain.  Needs fuse_levels = 0 only as far as march_algorithm / repeat do. */
    float transparency;       /* 0..1, default 0.5 (mat.diffuse, which the reference never reads, scales it per material: 1 in its scene) */
    float refraction_index;   /* 1..4, default 1 = straight through (transparency); > 1 bends the ray at both surfaces (refraction) */
} rt_config;

typedef struct rt_stats {
    uint32_t width, height, level_count, spp;
    uint64_t frames;           /* rt_render* calls since rt_resize */
    uint64_t primary_rays;     /* last call: width*height*spp (owned tiles only) */
    uint64_t shadow_rays;      /* last call: lightCount per shaded surface point (hit pixel samples + reflection / transmission hits) */
    uint64_t hit_pixels;       /* last call */
    uint64_t cone_threads;     /* last call: compute-stage invocations over all levels */
    float    ms_total;         /* last call: HIP-event time around the whole stage loop */
    float    ms_cone;          /* last call: sum over level kernels (profile_stages=1 only) */
    float    ms_shade;         /* last call: shade kernel(s) (profile_stages=1 only) */
    float    ms_level[RT_MAX_LEVELS]; /* last call, last sample (profile_stages=1, fuse_levels=0 only) */
    float    ms_fused;         /* last call, last sample: the one-launch pyramid kernel (profile_stages=1, fuse_levels=1) */
    uint64_t reflection_rays;  /* last call: mirror rays marched (rt_config.reflections > 0) */
    uint64_t transmission_rays; /* last call: rays marched behind a crossed sphere (rt_config.transmissions > 0) */
} rt_stats;

typedef struct rt_ctx rt_ctx;

int rt_abi_version(void);
int rt_device_count(int* count);

/* device_ordinal >= 0: HIP device index.  No CPU backend exists. */
int rt_create(rt_ctx** out, int device_ordinal);
void rt_destroy(rt_ctx* ctx);
/* message of the last failure on ctx (ctx == NULL: last rt_create failure of this thread) */
const char* rt_last_error(const rt_ctx* ctx);

int rt_default_config(rt_config* cfg);
int rt_set_config(rt_ctx* ctx, const rt_config* cfg);
/* default scene of src/main.rs:524-591 */
int rt_default_scene(rt_mutable_data* scene);
/* bytes must equal sizeof(rt_mutable_data) == 656 */
int rt_set_scene(rt_ctx* ctx, const void* mutable_data, size_t bytes);

/* (re)allocate the depth pyramid for a width x height view; ratio == NULL selects
 * {FOV, FOV*height/width} with FOV = 1 (src/main.rs:364,610) */
int rt_resize(rt_ctx* ctx, uint32_t width, uint32_t height, const float ratio[2]);
/* level count (src/main.rs:639, floor form, capped at 9) and dims[level] = {w,h} (src/main.rs:209-213) */
int rt_level_info(const rt_ctx* ctx, uint32_t* count, uint32_t dims[RT_MAX_LEVELS][2]);

/* Framebuffer partition for multi-GPU rendering: RT_TILE x RT_TILE tiles, tile t (row-major)
 * belongs to rank t % n_ranks.  Default rank 0 of 1 = whole frame. */
int rt_set_partition(rt_ctx* ctx, uint32_t rank, uint32_t n_ranks);
/* tiles_x, tiles_y of the current view and the number of tiles owned by this rank */
int rt_tile_info(const rt_ctx* ctx, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* owned);

/* Use an external HIP stream (hipStream_t as void*) for all launches; NULL = context's own. */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);

/* One frame at the reference's single pixel-centre sample.  rot = quaternion [x,y,z,w]
 * (push_constants.rot, src/main.rs:772), pos = camera position (:773).
 * rgb_out: host, width*height*3 f32, row-major, row 0 = gl_FragCoord.y 0.5, may be NULL;
 * depth_out: host, the last pyramid level (level dims, see rt_level_info), may be NULL.
 * Synchronous: results are complete on return. */
int rt_render(rt_ctx* ctx, const float rot[4], const float pos[3], float* rgb_out, float* depth_out);
/* spp = n*n stratified sub-pixel centres (n = 1,2,3,..), each sample one full frame, averaged
 * in sample order, ((s0 + s1) + s2) + ... then / spp; spp = 1 is rt_render.  Sample s has the stratum i = s % n in x and
 * j = s / n in y and adds the fp32 offset ((2i + 1) / n - 1) / width resp. ((2j + 1) / n - 1) / height to the normalised
 * coordinates of every level texel and of the pixel, before the ratio is applied (n = 1: exactly 0). */
int rt_render_spp(rt_ctx* ctx, const float rot[4], const float pos[3], uint32_t spp, float* rgb_out);
/* Asynchronous device-side variant: rgb_dev is a device pointer receiving either the full frame
 * (tile_major = 0: width*height*3 f32) or only this rank's tiles packed tile-major
 * (tile_major = 1: owned * RT_TILE*RT_TILE*3 f32, tile k = global tile rank + k*n_ranks).
 * Work is enqueued on the context's stream; no host synchronisation. */
int rt_render_device(rt_ctx* ctx, const float rot[4], const float pos[3], uint32_t spp, void* rgb_dev, int tile_major);
/* Scatter gathered tile-major buffers (n_ranks * tiles_per_rank tiles, rank-major) into a full
 * frame on the device: the de-tile step after an RCCL gather. */
int rt_detile_device(rt_ctx* ctx, const void* tiles_dev, uint32_t n_ranks, uint32_t tiles_per_rank, void* rgb_dev);
int rt_synchronize(rt_ctx* ctx);

/* The exchange step for hosts without a communication library of their own (no reference
 * counterpart: the reference drives one GPU, src/main.rs:448-460).  One process per GPU:
 * rank 0 calls rt_comm_unique_id and hands the 128 bytes to every rank (file, socket, MPI...);
 * every rank calls rt_comm_init (collective; it also sets the framebuffer partition to rank/n_ranks);
 * after rendering tile-major, every rank calls rt_gather_tiles: the tiles go to rank 0 over RCCL
 * (grouped ncclSend/ncclRecv, one direct xGMI link per peer) on the context's stream, into
 * gathered_dev[rank][tiles_per_rank][64][64][3] on rank 0 (ignored elsewhere); rt_detile_device then
 * scatters them into the frame.  tiles_dev holds the `owned` tiles of this rank (rt_tile_info), exactly
 * what rt_render*_device(tile_major = 1) wrote; every rank sends its own count and the root receives each
 * peer's own count, so uneven splits (510 tiles on 8 ranks: 64,64,64,64,64,64,63,63) read and write
 * nothing beyond the owned tiles; tiles_per_rank (the same on every rank) must be >= ceil(tiles / n_ranks).
 * RCCL is loaded on first use. */
#define RT_COMM_ID_BYTES 128
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_init(rt_ctx* ctx, const uint8_t id[RT_COMM_ID_BYTES], uint32_t rank, uint32_t n_ranks);
int rt_gather_tiles(rt_ctx* ctx, const void* tiles_dev, void* gathered_dev, uint32_t tiles_per_rank);
int rt_comm_destroy(rt_ctx* ctx);

/* Test hook: copy pyramid level `level` of the last frame to host. */
int rt_read_level(rt_ctx* ctx, uint32_t level, float* out, uint32_t* w, uint32_t* h);
/* Test hook: the same for any image of the last enqueued sample batch.  A multi-sample frame is rendered in batches of up to 16
 * samples (one sample per batch with fuse_levels = 1), each level holding one image per sample of the batch; image = 0 .. the
 * batch's last image (RT_ERR_INVALID beyond it), *sample = the sample index that image belongs to (the batch's first sample +
 * image).  rt_read_level is this call with the last image, which holds the frame's last sample. */
int rt_read_level_image(rt_ctx* ctx, uint32_t level, uint32_t image, float* out, uint32_t* w, uint32_t* h, uint32_t* sample);
/* Test hook: rt_render (1 spp, jitter 0, the whole frame; rgb_out and depth_out bit-equal to its) that also returns what every
 * secondary march did.  chain_out: host, width*height*(reflections + transmissions)*7 f32, rows by pixel (row-major), the mirror
 * bounces first, in order, then the transmission passes; a row is eye[3], dir[3], len: eye = the point the formulas at
 * rt_config.reflections / transmissions call P (mirror ray) or Q (transmitted ray) - the march starts at eye + dir -, dir = r or D,
 * len = 1 + traceCone(...) exactly as computed (a value >= render_dist ends the chain and is still recorded).  A march that did
 * not run - a miss pixel, a chain that ended earlier, k < 0 or k2 < 0 in a refraction - leaves seven NaNs.
 * RT_ERR_INVALID for a NULL output, RT_ERR_STATE when reflections and transmissions are both 0 or the partition has more than
 * one rank; nothing is written then. */
int rt_render_chains(rt_ctx* ctx, const float rot[4], const float pos[3], float* rgb_out, float* depth_out, float* chain_out);
/* Last frame as a *_UNORM swapchain would hold it (src/main.rs:471-486): linear, clamped,
 * round-to-nearest, alpha = 255 (never written by fragment.glsl:138,159). width*height*4 bytes. */
int rt_read_rgba8(rt_ctx* ctx, uint8_t* rgba_out);

int rt_get_stats(const rt_ctx* ctx, rt_stats* stats);
/* Test hook: the kernels take square roots with a shortened correctly rounded sequence; this runs it against the
 * compiler's IEEE sqrt on the device for every one of the 2^32 fp32 inputs and returns how many differ (0). */
int rt_selftest_math(rt_ctx* ctx, uint64_t* mismatches);

/* Frames in flight - the reference's swapchain loop (src/main.rs:664-667, 882-927: one fence per
 * swapchain image; a frame waits for its image's fence, is recorded, submitted behind the previous
 * frame and presented) with "present" = the pixels arriving in host memory.  A slot is one swapchain
 * image: a device frame, a pinned host frame and two events.  rt_frame_submit waits until the slot's
 * previous frame has reached the host (the image fence, :882-884), enqueues the render on the
 * slot's own render lane (a child context: own stream and buffers, configuration / scene / mesh of
 * this context as of the submit) and the read-back on a copy stream behind it, and returns without
 * waiting: frames in different slots overlap on the GPU, and every read-back overlaps later renders.
 * Frames of one slot complete in submit order; different slots are independent.  rt_frame_wait blocks until the slot's
 * pixels are in host memory and returns a pointer that stays valid until the slot is submitted
 * again.  format RT_FRAME_F32 = width*height*3 f32 (linear RGB), RT_FRAME_RGBA8 = width*height*4
 * bytes as rt_read_rgba8 defines them.  rt_resize releases the slots: configure again afterwards.
 * Single-rank contexts only (a partitioned context gathers tiles instead). */
#define RT_FRAME_F32 0u
#define RT_FRAME_RGBA8 1u
#define RT_MAX_FRAME_SLOTS 8u
int rt_frames_configure(rt_ctx* ctx, uint32_t n_slots, uint32_t format);
int rt_frame_submit(rt_ctx* ctx, uint32_t slot, const float rot[4], const float pos[3], uint32_t spp);
int rt_frame_wait(rt_ctx* ctx, uint32_t slot, const void** pixels, size_t* bytes);
int rt_frame_poll(rt_ctx* ctx, uint32_t slot, int* ready);

/* ------------------------------------------------------------------------------------------------
 * Path B — build-defined extension (BASELINE.json configs[2..4]): triangle meshes, a BVH and a
 * wavefront path tracer.  NO REFERENCE COUNTERPART: the reference has only sphere SDFs, one
 * deterministic sample and direct lighting (shaders/utilities.glsl:16-19, fragment.glsl:123-126
 * list reflection etc. as TODO).  The camera model (rot/pos/ratio, rt_resize) and the framebuffer
 * partition are shared with path A.  Specification: DESIGN.md §6.
 *
 * THE COORDINATE AND DIRECTION DOMAIN of every path B render and query entry (rt_render_pt, rt_render_pt_device,
 * rt_frame_submit_pt, every rt_query_*, rt_count_*, rt_fill_* and rt_list_* below); derivation: DESIGN.md §6.3,
 * measurements: §6.19.
 *   mesh        max(1, M) <= 2^RT_PT_MAX_COORD_LOG2, M = the largest |vertex coordinate|.  One limit for all entries.  Beyond it
 *               these entries return RT_ERR_INVALID before anything is enqueued or written; the message names M and the limit.
 *               rt_set_mesh*, rt_refit_mesh_device, rt_update_mesh_chunk and rt_read_bvh take every finite mesh.
 *   positions   camera position, ray origins, query points and the vertices of query triangles (rt_*_overlaps_device) within the reach
 *               32 x max(1, M) on every axis (the camera is refused beyond it, a ray, a point or a triangle is answered as invalid).
 *   directions  query directions are only checked for being finite.  The answers hold - no intermediate overflows, and t means what
 *               the entry says - for direction components of magnitude <= 1 (a unit vector; an occlusion segment as long as the
 *               reach allows is rescaled by the caller).  Components below 1e-20 in magnitude count as 1e-20 in the ray/box test
 *               only, which is conservative.  Longer directions work while |component| x M^2 stays below 2^110.
 *   scale       within this domain all answers are covariant: a problem with every length (vertices, origins, points, tmax, rmax,
 *               ray_eps, camera position) multiplied by 2^k gives bit for bit the same indices, counts, sides, barycentrics, unit
 *               normals and frames, and t, dist, signed distances and closest points multiplied by 2^k - as long as the smallest
 *               feature (a triangle's edges and altitudes, the distance from a shaded point to a light sample, ray_eps, a query
 *               point's distance from the surface where it is not zero) stays above 2^RT_PT_MIN_FEATURE_LOG2.  Smaller features
 *               are legitimate and never refused: there products of three and four lengths go subnormal, answers keep their
 *               contracts' meaning but lose covariance and precision, a normal may be the zero vector (§6.18), and a light
 *               sample closer than about 2^-37 contributes nothing.  A frame of a finite mesh with the camera in reach and a
 *               finite ray_eps has no non-finite pixel at any scale down to zero.
 * ------------------------------------------------------------------------------------------------ */
#define RT_PT_MAX_COORD_LOG2 20     /* max(1, M) <= 2^20 = 1 048 576 */
#define RT_PT_MIN_FEATURE_LOG2 (-24) /* documentation only: nothing is refused on the small side */
typedef struct rt_pt_params {
    uint32_t spp;      /* samples per pixel (any value >= 1) */
    uint32_t bounces;  /* indirect bounces after the camera ray (0..15) */
    uint32_t seed;
    float sky[3];      /* radiance of rays that leave the scene */
    float ray_eps;     /* origin offset along the shading normal (default 1e-3) */
    uint32_t count_traversal; /* 1: count BVH nodes fetched / triangles tested (rt_pt_stats) */
    uint32_t max_paths;       /* cap on paths in flight per pass (0 = default 2^25); spp is split into passes */
    uint32_t tune_refill_min;    /* tuning: idle lanes per wave that trigger a refill (0 = default 24; byte 1: triangle tests per round, 0 = 1) */
    uint32_t tune_blocks_per_cu; /* tuning: persistent workgroups per CU (0 = as many as the LDS stacks allow, fewer for few paths) */
    uint32_t tune_lds_stack;     /* tuning: traversal-stack entries kept in LDS per lane (0 = default 8), rest spills */
    uint32_t tune_no_overlap;    /* tuning: how the shadow rays of depth d and the closest-hit rays of depth d + 1 (independent work) share the
                                    GPU: 0 (default) one persistent launch pulls from both queues; 1 one launch after the other;
                                    2 two launches on two streams */
    uint32_t tune_no_packet;     /* tuning: how the camera rays are traced.  0 = default (6); 1 = through the per-lane traversal kernel
                                    like every other ray; 2..5 = wave-uniform packet traversal (one tree walk per 64 camera rays)
                                    with the node test as: 2 = every ray's slab test of all eight children; 3 = one interval test
                                    per child for the whole wave, then the rays' slab tests of the children that pass; 4 = the
                                    interval test alone; 5 = 3 without the cap at the wave's farthest best hit;
                                    6 / 7 = 4 with two / four rays per lane (one tree walk per 128 / 256 camera rays).
                                    Frames do not depend on it. */
    uint32_t tune_sort_rays;     /* tuning: 1 = bounce and shadow rays are sorted inside each 1024-ray workgroup of the shade stage
                                    (LDS counting sort on direction octant + origin cell) before they enter the queues;
                                    2 = the same sort on keys that predict work (shadow rays: segment length in quarter-octaves;
                                    bounce rays: dominant axis and steepness of the direction) */
    uint32_t tune_tri_mode;      /* tuning: how the per-lane traversal kernels schedule their ray/triangle tests.  Byte 0: 0 = default,
                                    1 = inline (every round ends with a triangle phase for the lanes that hold a leaf hit),
                                    2 = wave-pooled (leaf hits go to a per-wave ring in LDS; the whole wave tests 64 of them at once,
                                    results merged with a 64-bit LDS minimum on (t, triangle id)).  Pooled mode: byte 1 = groups in the
                                    ring that trigger a flush (0 = default), byte 2 = rounds a group may wait (0 = default).
                                    3 = postponed tests (bytes 1-2: holding / stuck lanes that trigger the phase), 4 = inline with a
                                    software-pipelined refill (a ring of ready rays per wave in LDS).  Inline mode, byte 1 bit 0: the
                                    fused launch as two loops one after the other instead of one loop with a per-lane ray kind.
                                    Frames do not depend on any of it. */
} rt_pt_params;

typedef struct rt_pt_stats {
    uint32_t n_tris, n_nodes, bvh_depth, n_lights; /* n_nodes / bvh_depth of the compressed 8-wide BVH */
    uint32_t stack_need;       /* worst-case traversal stack entries for this BVH */
    float bvh_build_ms;        /* last build or refit of the mesh (rt_refit_mesh_device: HIP-event time of its kernels) */
    uint32_t stack_overflow;   /* must be 0: traversal stack never exceeded */
    uint64_t camera_rays, bounce_rays, shadow_rays; /* last render: rays handed to BVH traversal */
    uint64_t nodes_visited, tris_tested;            /* per-lane closest-hit traversal (pt_trace<closest>, alone or inside a fused launch): BVH node
                                                       records fetched / triangle records fetched and tested; last render, count_traversal = 1 only */
    uint64_t shadow_nodes_visited, shadow_tris_tested; /* any-hit (shadow) launches, same condition */
    uint64_t wave_rounds, alive_lane_rounds;           /* closest-hit launches: traversal rounds per wave summed, lanes holding a live ray summed */
    float ms_total;            /* last render: HIP-event time around the stage loop */
    float ms_generate, ms_trace_closest, ms_shade, ms_trace_shadow, ms_resolve; /* profile_stages = 1 only */
    uint32_t launches_trace_closest, launches_trace_shadow;
    uint64_t packets;          /* camera-ray waves walked by the packet kernel; last render, count_traversal = 1 only */
    uint64_t packet_nodes_fetched, packet_tris_fetched; /* packet kernel: records fetched, once per wave of 64 camera rays (count_traversal = 1) */
    uint64_t fused_shadow_nodes, fused_shadow_tris, fused_shadow_rays; /* the part of the shadow_* counts / of shadow_rays that ran inside fused launches */
    float ms_trace_packet, ms_trace_fused; /* profile_stages = 1: the packet kernel; the fused shadow(d) + closest(d + 1) launches */
    uint32_t launches_trace_fused;
    uint32_t bvh_levels, blas_chunks, tlas_nodes; /* 1 / 0 / 0 for a single-level mesh */
    float ms_build_blas, ms_build_tlas, ms_build_flatten; /* two-level meshes: phases of the last build or chunk rebuild (bvh_build_ms = all of it) */
    uint64_t pool_flushes;     /* count_traversal = 1, wave-pooled triangle tests: passes in which a wave tested up to 64 pooled triangles */
    uint64_t wave_rounds_all;  /* count_traversal = 1: traversal rounds per wave summed over closest-hit AND any-hit launches */
} rt_pt_stats;

/* How rt_set_mesh_ex builds the acceleration structure.  bvh_levels = 1: one BVH8 over all triangles (rt_set_mesh).
 * bvh_levels = 2 (BASELINE.json configs[2] "2-level BVH"): the triangles are cut into blas_chunks chunks (0 = 64), the
 * leaves of a top-down binned-SAH split that always divides the fullest leaf, every chunk gets a bottom-level BVH8 of its
 * own, a top-level BVH8 is built over the chunk boxes, and both levels are flattened into the one node array the kernels traverse.  Frames are identical either
 * way (results do not depend on the tree); the two-level mesh can have one chunk's vertices replaced and only that
 * chunk rebuilt (rt_update_mesh_chunk). */
typedef struct rt_mesh_options {
    uint32_t bvh_levels;  /* 1 or 2 */
    uint32_t blas_chunks; /* bvh_levels = 2: number of bottom-level chunks, 0 = 64 (on average at least four triangles per chunk) */
} rt_mesh_options;

int rt_default_pt_params(rt_pt_params* p);
/* verts: n_tris*9 (v0,v1,v2), albedo: n_tris*3, emission: n_tris*3 (any component > 0 = light).
 * Uploads the mesh and builds the BVH on the host (binned SAH -> compressed 8-wide nodes, threaded; the result does
 * not depend on the thread count).  Host pointers, copied. */
int rt_set_mesh(rt_ctx* ctx, const float* verts, const float* albedo, const float* emission, uint32_t n_tris);
/* rt_set_mesh with build options (options == NULL: rt_set_mesh). */
int rt_set_mesh_ex(rt_ctx* ctx, const float* verts, const float* albedo, const float* emission, uint32_t n_tris, const rt_mesh_options* options);
/* Two-level meshes: the triangles of bottom-level chunk `chunk` (count, and their original indices into tri_ids[capacity]
 * when tri_ids != NULL), in the order rt_update_mesh_chunk expects their vertices. */
int rt_mesh_chunk_info(rt_ctx* ctx, uint32_t chunk, uint32_t* count, uint32_t* tri_ids, uint32_t capacity);
/* Two-level meshes: replace the vertices of one chunk's triangles (n_tris * 9 floats, rt_mesh_chunk_info order; materials
 * and chunk membership stay) and rebuild that chunk's BVH, the top level and the flattened node array only.  n_tris must
 * equal the chunk's triangle count (RT_ERR_INVALID otherwise: nothing is read).  The new vertices must stay within the
 * coordinate range of the mesh as first set (RT_ERR_INVALID otherwise: set the mesh again).  Transactional: on any error
 * other than RT_ERR_STATE the mesh is exactly as it was; RT_ERR_STATE means an upload failed and the mesh was dropped. */
int rt_update_mesh_chunk(rt_ctx* ctx, uint32_t chunk, const float* verts, uint32_t n_tris);
/* Path B mesh from device-resident arrays; the BVH is built on the GPU (LBVH -> compressed BVH8, the same node format as
 * rt_set_mesh's, so frames are bit-identical to those of a host-built tree).  verts / albedo / emission have rt_set_mesh's
 * layouts and are device pointers on the context's device (each allocation must hold the whole array).  They are read on
 * the context's stream, after the work already enqueued there; the call is synchronous on return and does not reference
 * them afterwards.  RT_ERR_INVALID, with the previous mesh untouched: a NULL, host or other-device pointer, n_tris outside
 * [1, 2^28), or a non-finite vertex coordinate.  The result is a single-level mesh (rt_update_mesh_chunk: RT_ERR_STATE);
 * rt_pt_stats.bvh_build_ms is the HIP-event time of the build's kernels.  The same input gives byte-identical trees. */
int rt_set_mesh_device(rt_ctx* ctx, const void* verts_dev, const void* albedo_dev, const void* emission_dev, uint32_t n_tris);
/* New vertex positions for the current single-level mesh (rt_set_mesh with bvh_levels = 1, or rt_set_mesh_device): the
 * tree's topology, leaf order, materials and light list stay; every box is recomputed on the GPU from the new vertices with
 * the padding of a build (2e-5 x the new largest |coordinate|, at least 1) and quantised outward as a build does, so frames
 * stay bit-identical to the oracle on the moved mesh and unchanged vertices give the tree byte for byte.  Works on host- and
 * device-built trees; the tree's quality degrades as triangles move apart (rebuild then: DESIGN.md §6.10).  verts_dev has
 * rt_set_mesh's layout (n_tris x 9 floats, original triangle order), is a device pointer on the context's device whose
 * allocation holds n_tris x 36 bytes, and is read on the context's stream after the work already enqueued there; the call is
 * synchronous on return.  The camera range of rt_render_pt* follows the new coordinates.  Errors, all with the mesh exactly as
 * it was: RT_ERR_INVALID for a NULL, host or other-device pointer, a too short allocation, n_tris other than the mesh's, a
 * non-finite coordinate; RT_ERR_STATE when there is no mesh or it is two-level (rt_update_mesh_chunk updates those);
 * RT_ERR_OOM if the scratch (24 B per node, allocated by the first refit of a mesh, freed with it) cannot be allocated.  A HIP
 * failure after the first write drops the mesh and returns RT_ERR_STATE, as rt_update_mesh_chunk does for a failed upload. */
int rt_refit_mesh_device(rt_ctx* ctx, const void* verts_dev, uint32_t n_tris);
/* Surface of every triangle of the current mesh.  Until this is called every triangle is a Lambert reflector
 * (§6.4).  kind[n_tris], original triangle order: RT_SURFACE_LAMBERT; RT_SURFACE_MIRROR (perfect reflection, tinted by the
 * albedo); RT_SURFACE_GLASS (a dielectric interface of index ior[i], 1 <= ior <= 4: Fresnel-weighted choice between reflection
 * and refraction, tinted by the albedo, albedo 1 = clear glass; the ray enters on the side e1 x e2 points to, so closed solids
 * need outward winding).  Emissive triangles stay lights whatever their kind.  Mirror and glass vertices take no next-event
 * estimation (shadow rays are still blocked by them); a light reached through them is counted when the path hits it.  ior is
 * read only where kind is GLASS and may be NULL when no kind is; kind == NULL resets the mesh to all Lambert.  Host arrays,
 * copied.  Works on every mesh (host-built single- and two-level, device-built); kept by rt_refit_mesh_device and
 * rt_update_mesh_chunk; any rt_set_mesh* starts the mesh all Lambert again.  Runs on the context's stream after the work already
 * enqueued there and is synchronous on return.  Errors, with the surfaces exactly as they were: RT_ERR_STATE (no mesh),
 * RT_ERR_INVALID (n_tris other than the mesh's, a kind above 2, a GLASS entry whose ior is not finite or outside [1, 4],
 * ior == NULL while some kind is GLASS), RT_ERR_OOM.  A HIP failure after the first write drops the mesh (RT_ERR_STATE). */
#define RT_SURFACE_LAMBERT 0u
#define RT_SURFACE_MIRROR 1u
#define RT_SURFACE_GLASS 2u
int rt_set_mesh_surfaces(rt_ctx* ctx, const uint32_t* kind, const float* ior, uint32_t n_tris);
/* Contexts of one process that are given the same host mesh on the same device (rt_set_mesh / rt_set_mesh_ex: every byte of the three
 * arrays, the triangle count and the build options equal) render one resident copy of it: the first builds and uploads, the others take
 * the copy that is there, and it is freed with the last of them.  A context that changes its mesh (rt_refit_mesh_device,
 * rt_update_mesh_chunk, rt_set_mesh_surfaces) continues with a copy of its own if others render the mesh too, so no context ever sees
 * another's change; when that copy cannot be allocated the call returns RT_ERR_OOM and nothing has changed.  rt_pt_stats' build times
 * are those of the build that made the copy.  Meshes from rt_set_mesh_device are never shared.  RT_AMD_MESH_SHARING=0 in the
 * environment, read by each rt_set_mesh*, makes that call build and upload for itself.
 * Returns the number of contexts that render this context's device mesh: 0 = no mesh, 1 = only this one; RT_ERR_INVALID for NULL. */
int rt_mesh_sharers(rt_ctx* ctx);
/* Test hook: node words (n_nodes x 20 u32, csrc/bvh_node.h layout) and leaf order (leaf position -> original triangle index,
 * n_tris u32) of the current mesh, host- or device-built.  NULL outputs: only *n_nodes is written (capacity query);
 * a non-NULL output whose capacity is too small: RT_ERR_INVALID.  No mesh: RT_ERR_STATE. */
int rt_read_bvh(rt_ctx* ctx, uint32_t* nodes_out, uint32_t node_capacity, uint32_t* leaf_tris_out, uint32_t tri_capacity, uint32_t* n_nodes);
/* Synchronous path-traced frame of the current view (rt_resize) into host memory.
 * Every |pos| component must be <= 32 x max(1, largest |vertex coordinate| of the mesh): that is the range
 * over which the BVH's conservative box padding covers the fp32 rounding of the ray/box test (beyond it the
 * frame could depend on the tree); RT_ERR_INVALID otherwise.  RT_ERR_INVALID too for a mesh beyond
 * 2^RT_PT_MAX_COORD_LOG2 (the domain above; the same for the two entries below).  A refused call has
 * enqueued and written nothing: the frame the context held before still reads back (rt_read_rgba8). */
int rt_render_pt(rt_ctx* ctx, const float rot[4], const float pos[3], const rt_pt_params* params, float* rgb_out);
/* Asynchronous device-side variant, same output layouts as rt_render_device. */
int rt_render_pt_device(rt_ctx* ctx, const float rot[4], const float pos[3], const rt_pt_params* params, void* rgb_dev, int tile_major);
/* Path B frame into a frames-in-flight slot (see rt_frame_submit). */
int rt_frame_submit_pt(rt_ctx* ctx, uint32_t slot, const float rot[4], const float pos[3], const rt_pt_params* params);
int rt_get_pt_stats(rt_ctx* ctx, rt_pt_stats* stats);
/* Ray queries on device arrays: what does each of n caller-supplied rays hit in the current mesh?  Enqueued on the
 * context's stream behind the work already there; no host synchronisation, and no allocation after the first query of a mesh or
 * size class.  origins_dev / dirs_dev: n x 3 f32, tmax_dev: n f32 or NULL, all device memory of the context's device, only read.
 * A triangle is hit when 0 < t < tmax[i] (strict; without tmax_dev the limit is +inf for closest hit and 0.999 for any hit, the
 * path tracer's shadow segment).  any_hit = 0: t_out_dev[i] = distance along dirs[i] (in units of its length), tri_out_dev[i] =
 * original triangle index (i32) of the closest hit, ties to the lower index; a miss is RT_RAY_MISS and +inf.  any_hit = 1:
 * tri_out_dev[i] = 1 if something is hit, else 0; t_out_dev may be NULL and is not written.  A ray with a non-finite origin or
 * direction component, a NaN tmax, or an origin component beyond 32 x max(1, largest |vertex coordinate| of the mesh) - the range
 * over which the BVH's box padding covers the rounding of the ray/box test, the one rt_render_pt enforces for the camera - is not
 * traced: tri_out = RT_RAY_INVALID, t_out = NaN (closest hit), and it is counted in rt_ray_query_stats.invalid_rays.  tmax = +inf
 * is valid; tmax <= 0 and a zero direction miss everything.  Nothing beyond element n - 1 of an output is written.  The caller
 * keeps all arrays alive until the stream has passed the call; lifetime rules against rt_set_mesh* are rt_render_pt_device's.
 * Works on every mesh (host-built single- and two-level, device-built, refitted, with surfaces); reads the mesh only, so a
 * shared mesh stays shared.  Errors, all before anything is enqueued or written: RT_ERR_INVALID (a NULL, host or other-device
 * pointer, an allocation shorter than n rows, n above 2^30, tune_refill_min above 64, tune_blocks_per_cu above 8, tune_lds_stack
 * above 78, a mesh beyond 2^RT_PT_MAX_COORD_LOG2 - the domain at the head of this section, which also says for which direction
 * magnitudes the answers hold; the same refusal in every query entry below), RT_ERR_STATE (no mesh), RT_ERR_OOM (scratch).
 * n == 0: RT_OK, nothing is done. */
typedef struct rt_ray_query_params {
    uint32_t any_hit;            /* 0 closest hit, 1 occlusion */
    uint32_t tune_refill_min;    /* as rt_pt_params (0 = default) */
    uint32_t tune_blocks_per_cu; /* as rt_pt_params */
    uint32_t tune_lds_stack;     /* as rt_pt_params */
    uint32_t tune_max_blocks;    /* cap on persistent workgroups, 0 = none (small batches through many refills; tests) */
} rt_ray_query_params;
typedef struct rt_ray_query_stats {
    uint64_t rays, invalid_rays; /* the last query with n > 0: rays asked, rays refused as invalid */
    uint32_t stack_overflow;     /* must be 0 */
    uint32_t launches;           /* kernel launches of that query */
    float ms;                    /* HIP-event time of its launch */
} rt_ray_query_stats;
#define RT_RAY_MISS (-1)
#define RT_RAY_INVALID (-2)
int rt_default_ray_query_params(rt_ray_query_params* p);
int rt_query_rays_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* tmax_dev /* may be NULL */,
                         uint32_t n, const rt_ray_query_params* params /* NULL = defaults */, void* t_out_dev, void* tri_out_dev);
int rt_get_ray_query_stats(rt_ctx* ctx, rt_ray_query_stats* stats); /* synchronises the stream; the last query */
/* Closest-point queries on device arrays: which triangle of the current mesh is nearest to each of n caller-supplied
 * points, how far away is it, and where on it?  Enqueued on the context's stream behind the work already there; no host
 * synchronisation, and no allocation after the first query of a mesh or size class.  points_dev: n x 3 f32, rmax_dev: n f32 or NULL,
 * device memory of the context's device, only read.  The answer for point i is the lexicographic minimum of (d2, original triangle
 * index) over all triangles with d2 < rmax[i] * rmax[i] (strict; the product is formed in fp32; without rmax_dev the limit is +inf),
 * d2 = the fp32 squared distance of csrc/point_tri.h; the limited answer is the unlimited one if its d2 is below the limit, else a
 * miss.  dist_out_dev[i] = sqrt(d2), correctly rounded; tri_out_dev[i] = the original triangle index (i32); point_out_dev (n x 3 f32,
 * may be NULL) = the nearest point of that triangle.  A miss (nothing within the limit) is RT_POINT_MISS, +inf and three NaNs.
 * rmax = +inf is valid; !(rmax > 0) misses without a walk, and so does an rmax so small that its square underflows to 0 (rmax below
 * 2^-75, about 2.6e-23: no d2 is below 0).  A point with a non-finite component, a NaN rmax, or a component beyond 32 x max(1, largest
 * |vertex coordinate| of the mesh) - the reach of rt_query_rays_device - is not answered: tri_out = RT_POINT_INVALID, dist_out = NaN,
 * point_out = NaNs, and it is counted in rt_point_query_stats.invalid_points.  Nothing beyond element n - 1 of an output is written.
 * The caller keeps all arrays alive until the stream has passed the call; lifetime rules against rt_set_mesh* are
 * rt_render_pt_device's.  Works on every mesh (host-built single- and two-level, device-built, refitted, with surfaces); reads the
 * mesh only, so a shared mesh stays shared.  Errors, all before anything is enqueued or written: RT_ERR_INVALID (a NULL context; a
 * NULL, host or other-device pointer, an allocation shorter than n rows, n above 2^30, count_traversal above 1, tune_refill_min above
 * 64, tune_blocks_per_cu above 8, tune_lds_stack above 78, a mesh beyond 2^RT_PT_MAX_COORD_LOG2 (the domain at the head of this
 * section)), RT_ERR_STATE (no mesh), RT_ERR_OOM (scratch).  n == 0: RT_OK, nothing is done. */
typedef struct rt_point_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_ray_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_point_query_params;
typedef struct rt_point_query_stats {
    uint64_t points, invalid_points;     /* the last query with n > 0: points asked, points refused as invalid */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangles tested, over all points */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that query */
    float ms;                            /* HIP-event time of its launch */
} rt_point_query_stats;
#define RT_POINT_MISS RT_RAY_MISS
#define RT_POINT_INVALID RT_RAY_INVALID
int rt_default_point_query_params(rt_point_query_params* p);
int rt_query_points_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, uint32_t n,
                           const rt_point_query_params* params /* NULL = defaults */, void* dist_out_dev, void* tri_out_dev,
                           void* point_out_dev /* may be NULL */);
int rt_get_point_query_stats(rt_ctx* ctx, rt_point_query_stats* stats); /* synchronises the stream; the last query */
/* Hit attributes: rt_query_rays_device (closest hit) and rt_query_points_device that also say where in the winning
 * triangle the hit or the nearest point lies and which way that triangle faces.  t_out / tri_out resp. dist_out / tri_out / point_out
 * come from the same walk under the same validity and limit rules and are bit for bit the plain functions' answers; parameters,
 * stream order, lifetime rules, meshes and statistics (rt_get_ray_query_stats / rt_get_point_query_stats) are theirs as well.
 * uv_out_dev (n x 2 f32, may be NULL) = (u, v): the point is v0 + u (v1 - v0) + v (v2 - v0) of the caller's vertices of triangle tri_out,
 * i.e. the weights of v0, v1, v2 are (1 - u - v, u, v).  For a ray u = U / det, v = V / det of the ray / triangle test that accepted the
 * triangle (csrc/hit_attr.h): u >= 0, v >= 0 (-0.0 can occur), u + v <= 1 + 2^-22.  For a point they are the parameters of the nearest
 * point as csrc/point_tri.h finds them (u + v <= 1 + 2^-24), of which point_out is the evaluation.  normal_out_dev (n x 3 f32, may be
 * NULL) = the unit geometric normal (v1 - v0) x (v2 - v0) / |..| in the caller's winding, never turned towards the ray or the point; three
 * zeros for a triangle without area (or one whose squared doubled area underflows or overflows in fp32).  On a miss - a hit cut off by
 * its limit included - and for an invalid ray or point uv is two NaNs and normal three NaNs.  With both arrays NULL the call is the plain
 * query.  Errors, all before anything is enqueued or written: those of the plain functions, the same checks on the two arrays, and
 * RT_ERR_INVALID for params->any_hit = 1 (an occlusion has no winner).  Nothing beyond row n - 1 of an output is written. */
int rt_query_rays_attr_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* tmax_dev /* may be NULL */, uint32_t n,
                              const rt_ray_query_params* params /* NULL = defaults */, void* t_out_dev, void* tri_out_dev,
                              void* uv_out_dev /* n x 2 f32, may be NULL */, void* normal_out_dev /* n x 3 f32, may be NULL */);
int rt_query_points_attr_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, uint32_t n,
                                const rt_point_query_params* params /* NULL = defaults */, void* dist_out_dev, void* tri_out_dev,
                                void* point_out_dev /* may be NULL */, void* uv_out_dev /* may be NULL */, void* normal_out_dev /* may be NULL */);
/* Inside/outside queries on device arrays: on which side of the current mesh's surface does each of n caller-supplied
 * points lie?  Enqueued on the context's stream behind the work already there; no host synchronisation, and no allocation after the
 * first query of a mesh or size class.  points_dev: n x 3 f32, device memory of the context's device, only read.  For point i and each
 * of three fixed directions D[k] (csrc/ray_parity.h) crossings(i, k) = the number of triangles that the ray / triangle test of
 * rt_query_rays_device accepts with t > 0 for the ray from the point along D[k], without an upper limit; inside_out_dev[i] (i32) = the
 * majority of the three parities crossings(i, k) & 1: 1 inside, 0 outside.  The answer is defined on every mesh as this parity of
 * crossings and does not depend on the tree; it means "inside" on closed meshes (every edge shared by two triangles).  Three rays and
 * not one because the triangle test is not watertight: a single ray through a shared edge or a vertex may count it twice or not at all.
 * The third ray is walked only where the first two parities disagree (the majority is the same).  crossings_out_dev (n x 3 i32, may be
 * NULL): all three rays are walked for every point and crossings_out_dev[3 i + k] = crossings(i, k); inside_out_dev is the same either
 * way.  dist_inout_dev (n f32, may be NULL; read and written): entry i is read first - +inf: the point is not walked, inside_out =
 * RT_POINT_MISS, the entry stays +inf, counted in skipped_points; NaN: not walked, inside_out = RT_POINT_INVALID, counted in
 * invalid_points; anything else: the entry is negated when the point is inside (an unsigned distance becomes a signed one) and is left
 * as it is when outside.  A point with a non-finite component or a component beyond 32 x max(1, largest |vertex coordinate| of the
 * mesh) - the reach of rt_query_rays_device - is not walked: inside_out = RT_POINT_INVALID, its crossings_out and dist_inout entries
 * are not written, and it is counted in invalid_points.  Nothing beyond element n - 1 of an output is written.  The caller keeps all
 * arrays alive until the stream has passed the call; lifetime rules against rt_set_mesh* are rt_render_pt_device's.  Works on every
 * mesh (host-built single- and two-level, device-built, refitted, with surfaces); reads the mesh only, so a shared mesh stays shared.
 * Errors, all before anything is enqueued or written: RT_ERR_INVALID (a NULL context; a NULL (where not allowed), host or other-device
 * pointer, an allocation shorter than n rows, n above 2^30, count_traversal above 1, tune_refill_min above 64, tune_blocks_per_cu above
 * 8, tune_lds_stack above 78, a mesh beyond 2^RT_PT_MAX_COORD_LOG2 (the domain at the head of this section)), RT_ERR_STATE (no
 * mesh), RT_ERR_OOM (scratch).  n == 0: RT_OK, nothing is done.
 * rt_query_signed_distance_device is exactly rt_query_points_device(points_dev, rmax_dev, n, point_params, sdist_out_dev, tri_out_dev,
 * point_out_dev) followed by rt_query_sides_device(points_dev, n, side_params, inside_out_dev, NULL, sdist_out_dev): sdist_out_dev[i] =
 * the distance to the nearest triangle, negative inside; with rmax_dev a narrow-band signed distance, the points beyond the band (+inf)
 * cost no ray walk.  inside_out_dev may be NULL here.  Everything that can refuse either step - and the first-use allocations of
 * both - comes before the first step is enqueued, so a refused call has written nothing.  rt_get_point_query_stats and
 * rt_get_side_query_stats then report the two steps of this call. */
typedef struct rt_side_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_ray_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_side_query_params;
typedef struct rt_side_query_stats {
    uint64_t points, invalid_points;     /* the last query with n > 0: points asked, points answered RT_POINT_INVALID */
    uint64_t skipped_points;             /* not walked because their dist_inout entry was +inf (answered RT_POINT_MISS) */
    uint64_t walks;                      /* ray walks: 2 per walked point + third_walks, or 3 per walked point with crossings_out_dev */
    uint64_t third_walks;                /* points whose first two parities disagreed: rare on closed meshes, a diagnostic for leaky or open ones */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangles tested, over all walks */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that query */
    float ms;                            /* HIP-event time of its launch */
} rt_side_query_stats;
int rt_default_side_query_params(rt_side_query_params* p);
int rt_query_sides_device(rt_ctx* ctx, const void* points_dev, uint32_t n, const rt_side_query_params* params /* NULL = defaults */,
                          void* inside_out_dev, void* crossings_out_dev /* may be NULL */, void* dist_inout_dev /* may be NULL */);
int rt_query_signed_distance_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, uint32_t n,
                                    const rt_point_query_params* point_params /* NULL = defaults */,
                                    const rt_side_query_params* side_params /* NULL = defaults */, void* sdist_out_dev, void* tri_out_dev,
                                    void* point_out_dev /* may be NULL */, void* inside_out_dev /* may be NULL */);
int rt_get_side_query_stats(rt_ctx* ctx, rt_side_query_stats* stats); /* synchronises the stream; the last query */
/* All-hits ray queries on device arrays: EVERY triangle of the current mesh that each of n caller-supplied rays passes
 * through, counted and listed, not only the nearest.  Enqueued on the context's stream behind the work already there; no host
 * synchronisation, and no allocation after the first query of a size class.  Ray i is origins_dev[i], dirs_dev[i] (n x 3 f32) and
 * tmax_dev[i] (n f32, or NULL: +inf), exactly as rt_query_rays_device takes them, device memory of the context's device, only read.
 * hits(i) = the triangles that the ray / triangle test of rt_query_rays_device (csrc/ray_parity.h: ray_tri_t) accepts with
 * 0 < t < tmax[i], strict at both ends.  The answer is defined without the tree and does not depend on it; for that a limit shortens
 * the list and not the walk (a segment costs what its whole ray costs).
 *   rt_count_ray_hits_device: count_out_dev[i] (n i32, may be NULL) = |hits(i)|; offsets_out_dev (n + 1 i64, may be NULL): [i] = the
 * exclusive prefix sum of the counts, [n] = their total; at least one of the two is required.
 *   rt_fill_ray_hits_device: the hits of ray i, sorted ascending by (t, original triangle index), into elements [offsets_in_dev[i],
 * offsets_in_dev[i + 1]) of t_out_dev (f32) and tri_out_dev (i32), arrays of `capacity` elements; offsets_in_dev (n + 1 i64) is read
 * on the stream.  A ray whose slice ends beyond the arrays (offsets[i + 1] > capacity) writes NOTHING; every other ray's slice is
 * complete and sorted: what a too small capacity leaves out never depends on the tree.  The caller sees offsets[n] > capacity, grows
 * the arrays and calls this step again.  The step is memory-safe against offsets that it did not make: ray i writes its hit number j
 * only while 0 <= offsets[i] and offsets[i] + j < offsets[i + 1] <= capacity; a slice shorter than its ray's hits keeps the first of
 * them in (t, index) order and the others are counted in slice_overflow, which is 0 whenever the offsets are the count step's for
 * the same rays and mesh.  capacity == 0: t_out_dev / tri_out_dev may be NULL, nothing is written.
 *   rt_list_ray_hits_device is exactly rt_count_ray_hits_device(..., count_out_dev, offsets_out_dev) followed by
 * rt_fill_ray_hits_device(..., offsets_out_dev, capacity, t_out_dev, tri_out_dev); everything that can refuse either step - and the
 * first-use allocations of both - comes before the first step is enqueued, so a refused call has written nothing.
 * A ray with a non-finite origin or direction component, a NaN tmax, or an origin component beyond 32 x max(1, largest |vertex
 * coordinate| of the mesh) - rt_query_rays_device's rule - is not walked: count_out = RT_RAY_INVALID, it adds 0 to the offsets, writes
 * no hit, and is counted in invalid_rays.  tmax = +inf is valid; tmax <= 0 and a zero direction give count 0.  Nothing beyond element
 * n - 1 of count_out_dev, n of offsets_out_dev and capacity - 1 of the hit arrays is written.  The caller keeps all arrays alive until
 * the stream has passed the call; lifetime rules against rt_set_mesh* are rt_render_pt_device's.  Works on every mesh (host-built
 * single- and two-level, device-built, refitted, with surfaces); reads the mesh only, so a shared mesh stays shared.  Errors, all
 * before anything is enqueued or written: RT_ERR_INVALID (a NULL context; a NULL (where not allowed), host or other-device pointer,
 * an allocation shorter than n / n + 1 / capacity rows, n above 2^30, capacity above 2^40, count_traversal above 1, tune_refill_min above 64,
 * tune_blocks_per_cu above 8, tune_lds_stack above 78, a mesh beyond 2^RT_PT_MAX_COORD_LOG2 (the domain at the head of this
 * section)), RT_ERR_STATE (no mesh), RT_ERR_OOM (scratch: 8 bytes per ray for the scan, grown by size class).  n == 0: RT_OK,
 * nothing is done. */
typedef struct rt_hit_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_ray_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_hit_query_params;
typedef struct rt_hit_query_stats {
    uint64_t rays, invalid_rays;         /* the last call with n > 0: rays asked, rays answered RT_RAY_INVALID */
    uint64_t hits;                       /* sum of |hits(i)| over the valid rays */
    uint64_t hits_written;               /* fill step: entries written into the hit arrays */
    uint64_t incomplete_rays;            /* fill step: rays with hits whose slice did not fit (offsets[i + 1] > capacity): nothing written */
    uint64_t slice_overflow;             /* fill step: hits beyond the length of their ray's slice; 0 with the count step's offsets */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangles tested, over all walks of the call */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that call: 1 per walk, 3 for the scan */
    float ms;                            /* HIP-event time from the first to the last launch of the call */
} rt_hit_query_stats;
int rt_default_hit_query_params(rt_hit_query_params* p);
int rt_count_ray_hits_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* tmax_dev /* may be NULL */, uint32_t n,
                             const rt_hit_query_params* params /* NULL = defaults */, void* count_out_dev /* may be NULL */,
                             void* offsets_out_dev /* may be NULL */);
int rt_fill_ray_hits_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* tmax_dev /* may be NULL */, uint32_t n,
                            const rt_hit_query_params* params /* NULL = defaults */, const void* offsets_in_dev, uint64_t capacity,
                            void* t_out_dev, void* tri_out_dev);
int rt_list_ray_hits_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* tmax_dev /* may be NULL */, uint32_t n,
                            const rt_hit_query_params* params /* NULL = defaults */, void* count_out_dev /* may be NULL */,
                            void* offsets_out_dev, uint64_t capacity, void* t_out_dev, void* tri_out_dev);
int rt_get_hit_query_stats(rt_ctx* ctx, rt_hit_query_stats* stats); /* synchronises the stream; the last call */
/* Neighbour queries on device arrays: EVERY triangle of the current mesh within a radius of each of n caller-supplied
 * points, counted and listed, not only the nearest.  Enqueued on the context's stream behind the work already there; no host
 * synchronisation, and no allocation after the first query of a size class.  Point i is points_dev[i] (n x 3 f32) with the radius
 * rmax_dev[i] (n f32), or rmax_all for every point when rmax_dev is NULL (with rmax_dev given, rmax_all is ignored); device memory of
 * the context's device, only read.  near(i) = the triangles with d2 < rmax[i] * rmax[i], strict and without a tolerance; the product is
 * formed in fp32 and d2 is the fp32 squared distance of csrc/point_tri.h (closest_on_tri on the triangle record's own words), exactly as
 * rt_query_points_device has them.  The answer is defined without the tree and does not depend on it.
 *   rt_count_neighbors_device: count_out_dev[i] (n i32, may be NULL) = |near(i)|; offsets_out_dev (n + 1 i64, may be NULL): [i] = the
 * exclusive prefix sum of the counts, [n] = their total; at least one of the two is required.
 *   rt_fill_neighbors_device: the neighbours of point i, sorted ascending by (d2, original triangle index), into elements
 * [offsets_in_dev[i], offsets_in_dev[i + 1]) of dist_out_dev (f32: sqrt(d2), correctly rounded, so non-decreasing along a slice) and
 * tri_out_dev (i32), arrays of `capacity` elements; offsets_in_dev (n + 1 i64) is read on the stream.  Entry 0 of a slice is bit for bit
 * what rt_query_points_device answers for the same point and rmax.  A point whose slice ends beyond the arrays (offsets[i + 1] >
 * capacity) writes NOTHING; every other point's slice is complete and sorted: what a too small capacity leaves out never depends on the
 * tree.  The caller sees offsets[n] > capacity, grows the arrays and calls this step again.  The step is memory-safe against offsets
 * that it did not make: point i writes its entry number j only while 0 <= offsets[i] and offsets[i] + j < offsets[i + 1] <= capacity; a
 * slice shorter than its point's list keeps the first entries in (d2, index) order and the others are counted in slice_overflow, which
 * is 0 whenever the offsets are the count step's for the same points, radii and mesh.  capacity == 0: dist_out_dev / tri_out_dev may be
 * NULL, nothing is written.
 *   rt_list_neighbors_device is exactly rt_count_neighbors_device(..., count_out_dev, offsets_out_dev) followed by
 * rt_fill_neighbors_device(..., offsets_out_dev, capacity, dist_out_dev, tri_out_dev); everything that can refuse either step - and
 * the first-use allocations of both - comes before the first step is enqueued, so a refused call has written nothing.
 * A point with a non-finite component, a NaN rmax, or a component beyond 32 x max(1, largest |vertex coordinate| of the mesh) -
 * rt_query_points_device's rule - is not walked: count_out = RT_POINT_INVALID, it adds 0 to the offsets, writes no entry, and is counted
 * in invalid_points.  !(rmax > 0), and an rmax so small that its square underflows to 0, give count 0 without a walk; rmax = +inf is
 * valid and lists every triangle whose d2 is finite.  A list is built by insertion into its slice, O(k^2) for k entries: meant for
 * lists of tens to a few hundred.  Nothing beyond element n - 1 of count_out_dev, n of offsets_out_dev and capacity - 1 of the entry
 * arrays is written.  The caller keeps all arrays alive until the stream has passed the call; lifetime rules against rt_set_mesh* are
 * rt_render_pt_device's.  Works on every mesh (host-built single- and two-level, device-built, refitted, with surfaces); reads the mesh
 * only, so a shared mesh stays shared.  Errors, all before anything is enqueued or written: RT_ERR_INVALID (a NULL context; a NULL
 * (where not allowed), host or other-device pointer, an allocation shorter than n / n + 1 / capacity rows, n above 2^30, capacity above
 * 2^40, count_traversal above 1, tune_refill_min above 64, tune_blocks_per_cu above 8, tune_lds_stack above 78, a mesh beyond
 * 2^RT_PT_MAX_COORD_LOG2 (the domain at the head of this section)), RT_ERR_STATE (no mesh), RT_ERR_OOM (scratch: 8 bytes per point
 * for the scan, shared with the all-hits queries, grown by size class).  n == 0: RT_OK, nothing is done. */
typedef struct rt_neighbor_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_ray_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_neighbor_query_params;
typedef struct rt_neighbor_query_stats {
    uint64_t points, invalid_points;     /* the last call with n > 0: points asked, points answered RT_POINT_INVALID */
    uint64_t neighbors;                  /* sum of |near(i)| over the valid points */
    uint64_t neighbors_written;          /* fill step: entries written into the entry arrays */
    uint64_t incomplete_points;          /* fill step: points with neighbours whose slice did not fit (offsets[i + 1] > capacity): nothing written */
    uint64_t slice_overflow;             /* fill step: neighbours beyond the length of their point's slice; 0 with the count step's offsets */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangles tested, over all walks of the call */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that call: 1 per walk, 3 for the scan */
    float ms;                            /* HIP-event time from the first to the last launch of the call */
} rt_neighbor_query_stats;
int rt_default_neighbor_query_params(rt_neighbor_query_params* p);
int rt_count_neighbors_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, float rmax_all, uint32_t n,
                              const rt_neighbor_query_params* params /* NULL = defaults */, void* count_out_dev /* may be NULL */,
                              void* offsets_out_dev /* may be NULL */);
int rt_fill_neighbors_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, float rmax_all, uint32_t n,
                             const rt_neighbor_query_params* params /* NULL = defaults */, const void* offsets_in_dev, uint64_t capacity,
                             void* dist_out_dev, void* tri_out_dev);
int rt_list_neighbors_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, float rmax_all, uint32_t n,
                             const rt_neighbor_query_params* params /* NULL = defaults */, void* count_out_dev /* may be NULL */,
                             void* offsets_out_dev, uint64_t capacity, void* dist_out_dev, void* tri_out_dev);
int rt_get_neighbor_query_stats(rt_ctx* ctx, rt_neighbor_query_stats* stats); /* synchronises the stream; the last call */
/* Overlap queries on device arrays: EVERY triangle of the current mesh that each of n caller-supplied triangles
 * intersects, counted and listed with the edges that pierce.  Enqueued on the context's stream behind the work already there; no host
 * synchronisation, and no allocation after the first query of a size class.  Query triangle i is tris_dev[i] (n x 9 f32: the vertices
 * A0, A1, A2, rt_set_mesh's vertex layout), device memory of the context's device, only read.  The arithmetic is csrc/tri_overlap.h,
 * fp32 only.  With F1 = A1 - A0, F2 = A2 - A0, Q = the box of the three vertices, and for mesh triangle T its record's v0, e1, e2 and
 * B = the box of v0, fl(v0 + e1), fl(v0 + e2):  cand(i, T) = Q and B overlap (closed, on all three axes);
 * seg(o, d, w0, g1, g2) = the ray / triangle test of rt_query_rays_device (csrc/ray_parity.h: ray_tri_t) accepts with 0 < t < 1, strict
 * at both ends;  mask(i, T) = bit 0: seg(A0, A1 - A0, v0, e1, e2), bit 1: seg(A1, A2 - A1, v0, e1, e2), bit 2: seg(A2, A0 - A2, v0, e1,
 * e2), bit 3: seg(v0, e1, A0, F1, F2), bit 4: seg(fl(v0 + e1), e2 - e1, A0, F1, F2), bit 5: seg(v0, e2, A0, F1, F2) - bits 0-2: an edge
 * of the query triangle pierces T, bits 3-5: an edge of T pierces the query triangle.  overlaps(i) = the triangles with cand and
 * mask != 0.  The answer is defined without the tree and does not depend on it.  In exact arithmetic two triangles that are not
 * coplanar intersect exactly when an edge of one pierces the other; coplanar pairs (det == 0) are never reported; the test is not
 * watertight (passes near an edge or a vertex inherit §6.3's leaks); pairs that share a vertex or an edge get whatever the arithmetic
 * gives, deterministically; a query triangle without area still answers as its three segments through bits 0-2, which are, given
 * cand, exactly membership in hits() of rt_count_ray_hits_device for the ray (o, d, tmax = 1).
 *   rt_count_overlaps_device: count_out_dev[i] (n i32, may be NULL) = |overlaps(i)|; offsets_out_dev (n + 1 i64, may be NULL): [i] = the
 * exclusive prefix sum of the counts, [n] = their total; at least one of the two is required.
 *   rt_fill_overlaps_device: the overlaps of triangle i, sorted ascending by original triangle index, into elements [offsets_in_dev[i],
 * offsets_in_dev[i + 1]) of tri_out_dev (i32) and edges_out_dev (i32: the mask), arrays of `capacity` elements; offsets_in_dev (n + 1
 * i64) is read on the stream.  A triangle whose slice ends beyond the arrays (offsets[i + 1] > capacity) writes NOTHING; every other
 * triangle's slice is complete and sorted: what a too small capacity leaves out never depends on the tree.  The caller sees
 * offsets[n] > capacity, grows the arrays and calls this step again.  The step is memory-safe against offsets that it did not make:
 * triangle i writes its entry number j only while 0 <= offsets[i] and offsets[i] + j < offsets[i + 1] <= capacity; a slice shorter
 * than its triangle's list keeps the entries with the lowest indices and the others are counted in slice_overflow, which is 0
 * whenever the offsets are the count step's for the same triangles and mesh.  capacity == 0: tri_out_dev / edges_out_dev may be NULL,
 * nothing is written.
 *   rt_list_overlaps_device is exactly rt_count_overlaps_device(..., count_out_dev, offsets_out_dev) followed by
 * rt_fill_overlaps_device(..., offsets_out_dev, capacity, tri_out_dev, edges_out_dev); everything that can refuse either step - and
 * the first-use allocations of both - comes before the first step is enqueued, so a refused call has written nothing.
 * A query triangle with a non-finite coordinate, or a coordinate beyond 32 x max(1, largest |vertex coordinate| of the mesh), is not
 * walked: count_out = RT_RAY_INVALID, it adds 0 to the offsets, writes no entry, and is counted in invalid_triangles.  A list is built
 * by insertion into its slice, O(k^2) for k entries: meant for lists of tens to a few hundred.  Nothing beyond element n - 1 of
 * count_out_dev, n of offsets_out_dev and capacity - 1 of the entry arrays is written.  The caller keeps all arrays alive until the
 * stream has passed the call; lifetime rules against rt_set_mesh* are rt_render_pt_device's.  Works on every mesh (host-built single-
 * and two-level, device-built, refitted, with surfaces); reads the mesh only, so a shared mesh stays shared.  Errors, all before
 * anything is enqueued or written: RT_ERR_INVALID (a NULL context; a NULL (where not allowed), host or other-device pointer, an
 * allocation shorter than n / n + 1 / capacity rows, n above 2^30, capacity above 2^40, count_traversal above 1, tune_refill_min above
 * 64, tune_blocks_per_cu above 8, tune_lds_stack above 78, a mesh beyond 2^RT_PT_MAX_COORD_LOG2 (the domain at the head of this
 * section)), RT_ERR_STATE (no mesh), RT_ERR_OOM (scratch: 8 bytes per triangle for the scan, shared with the other listing queries,
 * grown by size class).  n == 0: RT_OK, nothing is done. */
typedef struct rt_overlap_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_ray_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_overlap_query_params;
typedef struct rt_overlap_query_stats {
    uint64_t triangles, invalid_triangles; /* the last call with n > 0: triangles asked, triangles answered RT_RAY_INVALID */
    uint64_t overlaps;                     /* sum of |overlaps(i)| over the valid triangles */
    uint64_t overlaps_written;             /* fill step: entries written into the entry arrays */
    uint64_t incomplete_triangles;         /* fill step: triangles with overlaps whose slice did not fit (offsets[i + 1] > capacity): nothing written */
    uint64_t slice_overflow;               /* fill step: overlaps beyond the length of their triangle's slice; 0 with the count step's offsets */
    uint64_t nodes_visited, tris_tested;   /* count_traversal = 1 only: node records fetched, triangle records fetched, over all walks of the call */
    uint32_t stack_overflow;               /* must be 0 */
    uint32_t launches;                     /* kernel launches of that call: 1 per walk, 3 for the scan */
    float ms;                              /* HIP-event time from the first to the last launch of the call */
} rt_overlap_query_stats;
int rt_default_overlap_query_params(rt_overlap_query_params* p);
int rt_count_overlaps_device(rt_ctx* ctx, const void* tris_dev, uint32_t n, const rt_overlap_query_params* params /* NULL = defaults */,
                             void* count_out_dev /* may be NULL */, void* offsets_out_dev /* may be NULL */);
int rt_fill_overlaps_device(rt_ctx* ctx, const void* tris_dev, uint32_t n, const rt_overlap_query_params* params /* NULL = defaults */,
                            const void* offsets_in_dev, uint64_t capacity, void* tri_out_dev, void* edges_out_dev);
int rt_list_overlaps_device(rt_ctx* ctx, const void* tris_dev, uint32_t n, const rt_overlap_query_params* params /* NULL = defaults */,
                            void* count_out_dev /* may be NULL */, void* offsets_out_dev, uint64_t capacity, void* tri_out_dev,
                            void* edges_out_dev);
int rt_get_overlap_query_stats(rt_ctx* ctx, rt_overlap_query_stats* stats); /* synchronises the stream; the last call */
/* Overlap segments on device arrays: WHERE each pair of an overlap list intersects - one segment per entry of the
 * list that rt_list_overlaps_device / rt_fill_overlaps_device wrote for the same n query triangles and the same mesh.  Enqueued on the
 * context's stream behind the work already there (a list call, a refit), no host synchronisation, and no allocation after the first
 * call of a size class.  tris_dev (n x 9 f32), offsets_dev (n + 1 i64) and tri_dev (capacity i32) are the list call's arrays, device
 * memory of the context's device, only read; offsets_dev[n] is read on the stream.  The arithmetic is csrc/tri_section.h, fp32 only,
 * on the resident record words v0, e1, e2 of mesh triangle T = tri_dev[k] and the vertices of the query triangle i that owns entry k
 * (offsets[i] <= k < offsets[i + 1]):  m = cand(i, T) ? mask(i, T) : 0, recomputed - the stored masks are not an input, and on a list
 * the library wrote m is the stored mask;  for each set bit b, with (o, d, ...) the arguments of that bit's seg() above and t_b the t
 * of its ray / triangle test, P_b = (fma(t_b, d.x, o.x), fma(t_b, d.y, o.y), fma(t_b, d.z, o.z));  one bit set: both endpoints are P_b
 * (a touch);  two or more: the pair b < c of set bits with the largest fp32 |P_c - P_b|^2, ties to the first pair in lexicographic
 * (b, c) order, the segment is (P_b, P_c) in that order.  seg_out_dev[k] (capacity x 6 f32) = the two endpoints; ends_out_dev[k]
 * (capacity i32, may be NULL) = b | (c << 3), c = b for a touch: the edge each endpoint lies on (bits as in the mask).  In exact
 * arithmetic this is the intersection segment of two triangles that are not coplanar; it inherits the list's caveats (coplanar pairs
 * are never listed, the test is not watertight, pairs that share an edge or a vertex get what the arithmetic gives).
 *   Entries k < min(offsets[n], capacity) are visited, nothing else is read or written.  An entry of a slice that ends beyond the
 * capacity (offsets[i + 1] > capacity: the list call wrote nothing there) is left untouched and counted in skipped_incomplete.  The
 * call is memory-safe against arrays it did not make: an entry that no slice owns (offsets that do not ascend), with tri_dev[k]
 * outside [0, triangles of the mesh), with an invalid query triangle (rt_count_overlaps_device's rule) or with m == 0 gets six NaNs
 * and ends = -1 and is counted in bad_entries; 0 on a list the library wrote for these triangles and this mesh.
 *   Works on every mesh (host-built single- and two-level, device-built, refitted, updated by chunk, with surfaces).  The records are
 * in leaf order, so every call first writes the map original index -> leaf position (4 bytes per mesh triangle) into scratch of the
 * context's own, from the records themselves: nothing to invalidate, and the mesh is only read, so a shared mesh stays shared.
 * Errors, all before anything is enqueued or written: RT_ERR_INVALID (a NULL context; a NULL, host or other-device tris_dev,
 * offsets_dev, tri_dev or seg_out_dev, a host or other-device ends_out_dev, an allocation shorter than n / n + 1 / capacity rows, n
 * above 2^30, capacity above 2^40, a mesh beyond 2^RT_PT_MAX_COORD_LOG2), RT_ERR_STATE (no mesh), RT_ERR_OOM (the scratch, grown by
 * size class).  n == 0 or capacity == 0: RT_OK, nothing is done. */
typedef struct rt_overlap_segment_stats {
    uint64_t entries;            /* the last call with n > 0 and capacity > 0: entries visited, min(offsets[n], capacity) */
    uint64_t segments;           /* entries with two or more bits: a segment between two different edges */
    uint64_t touches;            /* entries with one bit: the same point twice */
    uint64_t skipped_incomplete; /* entries of slices that end beyond the capacity: untouched */
    uint64_t bad_entries;        /* entries answered with NaNs; entries = segments + touches + skipped_incomplete + bad_entries */
    uint32_t launches;           /* kernel launches of that call: the map and the segments */
    float ms;                    /* HIP-event time from the first to the last launch of the call */
} rt_overlap_segment_stats;
int rt_overlap_segments_device(rt_ctx* ctx, const void* tris_dev, uint32_t n, const void* offsets_dev /* n + 1 int64 */, uint64_t capacity,
                               const void* tri_dev /* int32 */, void* seg_out_dev /* capacity x 6 f32 */,
                               void* ends_out_dev /* capacity int32, may be NULL */);
int rt_get_overlap_segment_stats(rt_ctx* ctx, rt_overlap_segment_stats* stats); /* synchronises the stream; the last call */
/* Clearance queries on device arrays: how far is each of n caller-supplied triangles from the current mesh, which
 * mesh triangle is nearest, and where are the two nearest points?  Enqueued on the context's stream behind the work already there;
 * no host synchronisation, and no allocation after the first query of a mesh or size class.  tris_dev: n x 9 f32 (the three vertices,
 * rt_set_mesh's layout), rmax_dev: n f32 or NULL, device memory of the context's device, only read.  The arithmetic is
 * csrc/tri_dist.h, fp32 only, on the resident record words v0, e1, e2 of each mesh triangle T and the vertices A0, A1, A2 of query
 * triangle i, F1 = A1 - A0, F2 = A2 - A0:  a pair's d2 is the smallest d2 = |a - c|^2 (fp32) of up to twenty-one candidates, with
 * a = A0 + uq F1 + vq F2 and c = v0 + um e1 + vm e2 points of the two closed triangles, the earlier candidate winning a tie - where
 * one of the six segment tests of rt_list_overlaps_device accepts (cand and its mask bit), the point at t on that edge and the point
 * at (u / det, v / det) in the pierced triangle: for triangles that intersect, the pierce point twice and d2 = 0 or a rounding of it;
 * each corner of one triangle against the other (csrc/point_tri.h's closest_on_tri); each edge of one against each edge of the other
 * (the closest points of two clamped segments).  A test only proposes its pair: what counts is the d2 the pair evaluates to, so a
 * query triangle without area (a segment, a point), whose tests decide on rounding noise, is answered as well.  The answer for triangle i is the
 * lexicographic minimum of (d2, original triangle index) over all mesh triangles with d2 < rmax[i] * rmax[i] (strict; the product is
 * formed in fp32; without rmax_dev the limit is +inf).  tri_out_dev[i] = the original triangle index (i32); dist_out_dev[i] =
 * sqrt(d2), correctly rounded; point_query_out_dev / point_mesh_out_dev (n x 3 f32 each, either may be NULL) = a and c.  A miss
 * (nothing within the limit) is RT_POINT_MISS, +inf and NaNs; !(rmax > 0) and an rmax whose square underflows to 0 miss without a
 * walk.  A triangle with a non-finite coordinate, a NaN rmax, or a coordinate beyond 32 x max(1, largest |vertex coordinate| of the
 * mesh) is not answered: tri_out = RT_RAY_INVALID, NaNs, counted in invalid_triangles.  Coplanar pairs that overlap are not "cut"
 * (the overlap test refuses them): their distance is the candidates', which is 0 or a rounding of it.  Nothing beyond element n - 1
 * of an output is written.  Lifetime rules, meshes (every kind; the mesh is only read, a shared mesh stays shared) and errors are
 * rt_query_points_device's, all before anything is enqueued or written.  n == 0: RT_OK, nothing is done. */
typedef struct rt_clearance_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_point_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_clearance_query_params;
typedef struct rt_clearance_query_stats {
    uint64_t queries, invalid_triangles; /* the last query with n > 0: triangles asked, triangles answered RT_RAY_INVALID */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangle records fetched, over all queries */
    uint32_t stack_overflow;             /* must be 0 */
    float ms;                            /* HIP-event time of its launch */
} rt_clearance_query_stats;
int rt_default_clearance_query_params(rt_clearance_query_params* p);
int rt_query_clearance_device(rt_ctx* ctx, const void* tris_dev, const void* rmax_dev /* may be NULL */, uint32_t n,
                              const rt_clearance_query_params* params /* NULL = defaults */, void* tri_out_dev /* i32 n */,
                              void* dist_out_dev /* f32 n */, void* point_query_out_dev /* f32 3n, may be NULL */,
                              void* point_mesh_out_dev /* f32 3n, may be NULL */);
int rt_get_clearance_query_stats(rt_ctx* ctx, rt_clearance_query_stats* stats); /* synchronises the stream; the last query */
/* k-nearest queries on device arrays: the k triangles of the current mesh nearest to each of n caller-supplied
 * points, sorted, as rectangular n x k outputs from one walk.  Enqueued on the context's stream behind the work already there; no
 * host synchronisation, and no allocation after the first query of a mesh or size class.  points_dev: n x 3 f32, rmax_dev: n f32 or
 * NULL, device memory of the context's device, only read.  With limit2 = rmax[i] * rmax[i] (one fp32 product; +inf without
 * rmax_dev), near(i) is rt_list_neighbors_device's list: every triangle with d2 < limit2 (strictly), d2 = the fp32 squared distance
 * of csrc/point_tri.h on the resident record, sorted ascending by (d2, original triangle index).  Row i is the first
 * count = min(k, |near(i)|) entries of that list: dist_out_dev[i * k + j] = sqrt(d2), correctly rounded, tri_out_dev[i * k + j] =
 * the original triangle index (i32); an exact tie at the cut keeps the lower index; only triangles with a finite d2 appear.  k = 1 is
 * bit for bit rt_query_points_device's (dist, tri); every row is a prefix of rt_list_neighbors_device's slice for the same rmax.
 * Entries at and beyond count are +inf and RT_POINT_MISS (k above the number of triangles is valid: its rows are short).
 * count_out_dev (n i32, may be NULL) = count.  !(rmax > 0) and an rmax whose square underflows to 0 give count 0 without a walk.  A
 * point with a non-finite component, a NaN rmax, or a component beyond 32 x max(1, largest |vertex coordinate| of the mesh) is not
 * answered: count = RT_POINT_INVALID, its whole row NaN and RT_POINT_INVALID, counted in invalid_points.  Every element of rows
 * 0 .. n - 1 is written, nothing outside them; rows are addressed with 64 bits (n x k reaches 2^40).  Lifetime rules, meshes (every
 * kind; the mesh is only read, a shared mesh stays shared) and errors are rt_query_points_device's, and RT_ERR_INVALID also for
 * k == 0, k above RT_KNN_MAX_K and an output allocation shorter than n x k elements - all before anything is enqueued or written.
 * n == 0: RT_OK, nothing is done. */
#define RT_KNN_MAX_K 1024u
typedef struct rt_knn_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_point_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_knn_query_params;
typedef struct rt_knn_query_stats {
    uint64_t points, invalid_points;     /* the last query with n > 0: points asked, points answered RT_POINT_INVALID */
    uint64_t neighbors;                  /* entries listed over all rows: the sum of max(count, 0) */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangles tested, over all points */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that query */
    float ms;                            /* HIP-event time of its launch */
} rt_knn_query_stats;
int rt_default_knn_query_params(rt_knn_query_params* p);
int rt_query_knn_device(rt_ctx* ctx, const void* points_dev, const void* rmax_dev /* may be NULL */, uint32_t n, uint32_t k,
                        const rt_knn_query_params* params /* NULL = defaults */, void* dist_out_dev /* n x k f32 */,
                        void* tri_out_dev /* n x k i32 */, void* count_out_dev /* n i32, may be NULL */);
int rt_get_knn_query_stats(rt_ctx* ctx, rt_knn_query_stats* stats); /* synchronises the stream; the last query */
/* Sphere-cast (sweep) queries on device arrays: a sphere of radius r[i] starts with its centre at o[i] and moves
 * along d[i]; how far does it get before it touches the current mesh, which triangle does it touch first, and where?  Enqueued on
 * the context's stream behind the work already there; no host synchronisation, and no allocation after the first query of a mesh or
 * size class.  origins_dev, dirs_dev: n x 3 f32; radius_dev: n f32; tmax_dev: n f32 or NULL (+inf); device memory of the context's
 * device, only read.  d is not normalised: t is in units of |d|, as for rt_query_rays_device, and the centre at t is o + t d, one
 * fma per component.  The arithmetic is csrc/sweep_tri.h, fp32 only, on the resident record words v0, e1, e2 of each triangle T:
 * toi(T) = 0 when the start touches, closest_on_tri(o, T).d2 <= r * r (csrc/point_tri.h; the product in fp32); otherwise the
 * smallest accepted candidate among the entry times into the seven features of the sphere-swept triangle - the face's plane offset
 * by r towards the origin's side, the three edge cylinders where the contact parameter lies in [0, 1], the three vertex spheres -
 * each only where the centre approaches the feature, a candidate at or below 0 raised to the smallest positive normal float.  A
 * candidate t is accepted when the centre at t evaluates to a distance of at most r + 2^-21 S from T with closest_on_tri, S =
 * max(|o|_inf, r, |v0|_inf + max(|e1|_inf, |e2|_inf)): a feature proposes, the evaluated distance decides, so a needle cannot
 * pick a wrong feature and a triangle without area is the capsules and spheres it consists of.  A zero direction touches only at
 * t = 0; r = 0 is a ray against the closed triangle.  The answer for item i is the lexicographic minimum of (toi, original triangle
 * index) over all triangles with toi < tmax[i] (strictly) and toi <= FLT_MAX: among several triangles touched at the start the
 * lowest index wins.  t_out_dev[i] = toi (f32), tri_out_dev[i] = the original triangle index (i32), point_out_dev (n x 3 f32, may be
 * NULL) = the contact point: closest_on_tri of the centre at t against that triangle.  A miss is +inf, RT_RAY_MISS and NaNs;
 * !(tmax > 0) misses without a walk.  An item with a non-finite component of o or d, a radius that is NaN, negative or above
 * 32 x max(1, largest |vertex coordinate| of the mesh), a NaN tmax, or an origin component beyond that same reach is not answered:
 * tri_out = RT_RAY_INVALID, NaNs, counted in invalid_sweeps.  d . d must neither overflow nor underflow to 0 in fp32, else the item
 * is answered from its start alone.  Nothing beyond element n - 1 of an output is written.  Lifetime rules, meshes (every kind; the
 * mesh is only read, a shared mesh stays shared) and errors are rt_query_points_device's, all before anything is enqueued or
 * written.  n == 0: RT_OK, nothing is done. */
typedef struct rt_sweep_query_params {
    uint32_t tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks; /* as rt_point_query_params */
    uint32_t count_traversal;                                                      /* 1: fill nodes_visited / tris_tested */
} rt_sweep_query_params;
typedef struct rt_sweep_query_stats {
    uint64_t sweeps, invalid_sweeps;     /* the last query with n > 0: items asked, items answered RT_RAY_INVALID */
    uint64_t hits;                       /* items answered with a triangle */
    uint64_t nodes_visited, tris_tested; /* count_traversal = 1 only: node records fetched, triangle records fetched, over all items */
    uint32_t stack_overflow;             /* must be 0 */
    uint32_t launches;                   /* kernel launches of that query */
    float ms;                            /* HIP-event time of its launch */
} rt_sweep_query_stats;
int rt_default_sweep_query_params(rt_sweep_query_params* p);
int rt_query_sweeps_device(rt_ctx* ctx, const void* origins_dev, const void* dirs_dev, const void* radius_dev, const void* tmax_dev /* may be NULL */,
                           uint32_t n, const rt_sweep_query_params* params /* NULL = defaults */, void* t_out_dev /* f32 n */,
                           void* tri_out_dev /* i32 n */, void* point_out_dev /* f32 3n, may be NULL */);
int rt_get_sweep_query_stats(rt_ctx* ctx, rt_sweep_query_stats* stats); /* synchronises the stream; the last query */
/* Test hook (the product entry is rt_query_rays_device): trace n caller-supplied rays (host arrays, n*3 each).  any_hit = 0: closest hit,
 * t_out[i] = distance (inf on miss), tri_out[i] = original triangle index or -1;
 * any_hit = 1: tri_out[i] = 1 if the open segment (o, o + 0.999*d) is occluded. */
int rt_trace_rays(rt_ctx* ctx, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out, int32_t* tri_out);
/* Test hook: as rt_trace_rays, and counts_out[2i], counts_out[2i+1] (may be NULL) receive the number of BVH
 * nodes fetched and triangles tested for ray i by the traversal step functions the render kernels run:
 * tests/native/bvh8_walk.cpp walks the same tree on the host and must reproduce them exactly, which is what
 * entitles bench.py to quote rt_pt_stats.nodes_visited / tris_tested. */
int rt_trace_rays_counted(rt_ctx* ctx, const float* origins, const float* dirs, uint32_t n, int any_hit, float* t_out, int32_t* tri_out,
                          uint32_t* counts_out);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
