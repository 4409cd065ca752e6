// path_b.hip — wavefront path tracer over a triangle BVH (BASELINE.json configs[2..4]): the stages that are not a tree walk.
//
// NO REFERENCE COUNTERPART: the reference has no triangles, BVH, RNG, spp or bounces (SURVEY.md
// §0); only the camera model is the reference's (shaders/fragment.glsl:129-133,
// shaders/utilities.glsl:26-29).  Path B implements the specification of DESIGN.md §6; parity
// is against oracle B and is "unpinned by the reference".
//
// Structure (one launch per ray stage, all queue sizes stay on the device):
//   pt_generate       camera rays for every (pixel, sample) of the owned tiles -> path state + queue 0                      (this file)
//   pt_trace_packet*  camera rays of a 4x4-pixel block walk the tree as one wave, generate stage fused                      (pt_packet.hip)
//   pt_trace<closest> persistent waves with per-lane refill from the device-resident queue; traversal                     (pt_trace.hip)
//                     of a compressed 8-wide BVH (80-byte nodes, five 16-byte fetches per node) with a
//                     per-lane stack of node groups in LDS, ray/triangle tests, writes (t, triangle)
//   pt_shade          emission / sky / next-event estimation / cosine bounce; survivors are appended to                    (this file)
//                     the next queue and shadow rays to the shadow queue with wave ballot +
//                     prefix-popcount compaction (one atomic per 1024-thread workgroup)
//   pt_trace<any>     shadow rays: any-hit traversal, unoccluded contributions added to the path                           (pt_trace.hip)
//   pt_resolve        per pixel: samples summed in index order, divided by spp                                             (this file)
//   pt_query_rays     rt_query_rays_device: the refilling loop of pt_trace on caller-supplied rays in device arrays (section 6.13)      (pt_trace.hip)
//   pt_query_points   rt_query_points_device: the same loop around a nearest-first walk for the closest triangle to a point (section 6.14)  (pt_point_query.hip)
// Shared device headers: pt_traverse.h (the lane's walk of the BVH8), pt_queue.h (the stream queue as a wave sees it), pt_camera.h
// (RNG, pixel slots, camera ray); pt_launch.h for the launchers.  Every unit ends with the launchers of its own kernels.
// Memory: path state is SoA of float4 (16 B per lane per array = widest coalesced access), BVH nodes
// are 80-byte quantised records (bvh_node.h), triangles 48-byte records in leaf order.
#include "pt_camera.h"

namespace rt {
using namespace rtk;

// ---- spec §6.5: sin/cos(2*pi*u) from fma polynomials only ----------------------------------------
__device__ __forceinline__ void sincos_2pi(float u, float& s_out, float& c_out) {
    const float t = u * 4.0f;
    uint32_t q = (uint32_t)t;
    if (q > 3u) q = 3u;
    const float th = ((t - (float)q) - 0.5f) * 1.57079632679f;
    const float th2 = th * th;
    const float ps = __builtin_fmaf(th2, __builtin_fmaf(th2, __builtin_fmaf(th2, __builtin_fmaf(th2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f), 1.0f);
    const float s = th * ps;
    const float c = __builtin_fmaf(th2, __builtin_fmaf(th2, __builtin_fmaf(th2, __builtin_fmaf(th2, 2.4801587e-5f, -1.3888889e-3f), 4.1666667e-2f), -0.5f), 1.0f);
    const float R = 0.70710678f;
    const float cA = (q == 0u || q == 3u) ? R : -R;
    const float sA = (q < 2u) ? R : -R;
    c_out = __builtin_fmaf(cA, c, -(sA * s));
    s_out = __builtin_fmaf(sA, c, cA * s);
}

__device__ __forceinline__ v3 cosine_dir(v3 n, float u1, float u2) {
    const float r = __builtin_sqrtf(u1);
    float s, c;
    sincos_2pi(u2, s, c);
    const float x = r * c, y = r * s, z = __builtin_sqrtf(fmax_(0.0f, 1.0f - u1));
    const float sign = n.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + n.z);
    const float b = (n.x * n.y) * a;
    const v3 b1 = mk(__builtin_fmaf(sign, (n.x * n.x) * a, 1.0f), sign * b, -sign * n.x);
    const v3 b2 = mk(b, __builtin_fmaf(n.y * n.y, a, sign), -n.y);
    return mk(__builtin_fmaf(n.x, z, __builtin_fmaf(b2.x, y, b1.x * x)), __builtin_fmaf(n.y, z, __builtin_fmaf(b2.y, y, b1.y * x)),
              __builtin_fmaf(n.z, z, __builtin_fmaf(b2.z, y, b1.z * x)));
}

// ---- spec §6.11: mirror and glass vertices ---------------------------------------------------------
// w = the triangle's surface word (albedo.w): < 0 mirror, >= 1 glass of index w.  n = the shading normal, already turned
// against d (flipped: it was; the ray leaves the glass then).  u = rnd(key, depth, 7).  Returns the continuation
// direction; below = true for a refraction, whose origin lies on the far side of the surface.
__device__ __forceinline__ v3 delta_dir(v3 d, v3 n, float w, bool flipped, float u, bool& below) {
    const float c = -dot(n, d);
    below = false;
    if (w > 0.0f) {
        const float eta = flipped ? w : 1.0f / w;
        const float s2 = (eta * eta) * __builtin_fmaf(-c, c, 1.0f);
        if (s2 < 1.0f) {  // otherwise total internal reflection
            const float ct = __builtin_sqrtf(1.0f - s2);
            const float a = eta * c, b = eta * ct;
            const float rs = (a - ct) / (a + ct), rp = (c - b) / (c + b);
            const float F = __builtin_fmaf(rs, rs, rp * rp) * 0.5f;
            if (!(u < F)) {
                below = true;
                const float k = a - ct;
                return mk(__builtin_fmaf(n.x, k, eta * d.x), __builtin_fmaf(n.y, k, eta * d.y), __builtin_fmaf(n.z, k, eta * d.z));
            }
        }
    }
    return fma3(n, c + c, d);
}

// Queue append with workgroup-level aggregation: ballot + prefix popcount inside each wave, the wave
// totals meet in LDS, ONE atomic per workgroup reserves the range (a single hot counter serves only
// ~90 atomics/us chip-wide, so one atomic per wave made the compaction kernels atomic-bound).
// Must be called by every thread of the workgroup (two barriers inside).
constexpr uint32_t kAppendThreads = 1024;
__device__ __forceinline__ uint32_t block_append(bool want, uint32_t* counter, uint32_t* lds /* >= 17 words */) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const unsigned long long mask = __ballot(want);
    if (lane == 0) lds[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < n_waves; w++) total += lds[w];
        uint32_t base = total ? atomicAdd(counter, total) : 0u;
        for (uint32_t w = 0; w < n_waves; w++) {
            const uint32_t c = lds[w];
            lds[w] = base;
            base += c;
        }
    }
    __syncthreads();
    const uint32_t idx = lds[wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // lds is reused by the next append
    return idx;
}

// Queue append with a sort inside the workgroup ("rays compacted and sorted in LDS"): the rays a workgroup
// emits are reserved as one contiguous range (one atomic, as block_append) and placed inside it in key
// order by an LDS counting sort (histogram with returning LDS atomics -> rank in bin, exclusive scan over
// the bins, position = bin start + rank).  key < kSortBins; the order inside a bin is arrival order (not
// deterministic, and irrelevant: the queue order never changes a result).  Rays that
// sit next to each other in the queue are picked up by the same wave of pt_trace.
// Must be called by every thread of the workgroup.  lds: kSortBins + 40 words.
constexpr uint32_t kSortBins = 512;
template <uint32_t BINS = kSortBins>
__device__ __forceinline__ uint32_t block_append_sorted(bool want, uint32_t key, uint32_t* counter, uint32_t* lds) {
    static_assert(BINS % 64u == 0u && BINS <= kSortBins, "whole waves of bins");
    uint32_t* hist = lds;               // BINS
    uint32_t* wsum = lds + kSortBins;   // 16 wave sums of the scan + 1 base
    // The thread index as a value the compiler cannot follow: what this function derives from it (lane masks of the scan, LDS
    // addresses) is then made where it is used, not kept in registers through the caller's loop, which seldom comes here.
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    for (uint32_t i = tid; i < BINS; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    uint32_t rank = 0;
    if (want) rank = atomicAdd(&hist[key], 1u);
    __syncthreads();
    // exclusive scan of the BINS counts by the first BINS threads (wave scan + wave sums)
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    uint32_t v = 0, incl = 0;
    if (tid < BINS) {
        v = hist[tid];
        incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if ((int)lane >= off) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < BINS / 64u; w++) {
            const uint32_t c = wsum[w];
            wsum[w] = total;
            total += c;
        }
        wsum[16] = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    if (tid < BINS) hist[tid] = wsum[wave] + incl - v;  // bin start inside the workgroup's range
    __syncthreads();
    const uint32_t idx = want ? wsum[16] + hist[key] + rank : 0u;
    __syncthreads();  // lds is reused by the next append
    return idx;
}

// Sort key of a ray: direction octant (3 bits, major) and the cell of its origin in a 4 x 4 x 4 grid over the
// BVH root's quantisation frame (6 bits).
__device__ __forceinline__ uint32_t ray_sort_key(const float4* __restrict__ nodes, v3 o, v3 d) {
    const float4 n0 = nodes[0];  // root: p.xyz, exponent bytes
    const uint32_t w3 = __float_as_uint(n0.w);
    const float ex = __uint_as_float((((w3 & 0xffu) + 6u) & 0xffu) << 23), ey = __uint_as_float(((((w3 >> 8) & 0xffu) + 6u) & 0xffu) << 23),
                ez = __uint_as_float(((((w3 >> 16) & 0xffu) + 6u) & 0xffu) << 23);  // 64 quantisation steps = a quarter of the frame
    const int cx = (int)((o.x - n0.x) / ex), cy = (int)((o.y - n0.y) / ey), cz = (int)((o.z - n0.z) / ez);
    const uint32_t ux = (uint32_t)(cx < 0 ? 0 : cx > 3 ? 3 : cx), uy = (uint32_t)(cy < 0 ? 0 : cy > 3 ? 3 : cy), uz = (uint32_t)(cz < 0 ? 0 : cz > 3 ? 3 : cz);
    const uint32_t oct = (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 31) << 1) | ((__float_as_uint(d.z) >> 31) << 2);
    return (oct << 6) | (uz << 4) | (uy << 2) | ux;
}

// Sort keys that predict WORK rather than locality (tune_sort_rays = 2; 64 bins): rays that sit next to each other in the queue are
// taken by the same wave's refill, and lanes whose rays end at about the same time leave fewer lanes waiting for the next refill.
// Shadow rays: the segment's length in quarter-octaves (a segment is traversed end to end unless it is occluded; its node count
// grows with its length).  Bounce rays: how steeply the direction leaves the scene's long axis (rays along the soup's slab cross
// more of it) - the largest |component| of the direction picks the axis, its magnitude 16 steps.
__device__ __forceinline__ uint32_t shadow_work_key(v3 d) {
    const float l2 = dot(d, d);                                             // squared length: two quarter-octave steps per octave of length
    const int e = (int)((__float_as_uint(l2) >> 21) & 0x3ffu) - (125 << 2);  // exponent and two mantissa bits, offset so that |d| = 0.5 .. 128 maps to 0 .. 63
    return (uint32_t)(e < 0 ? 0 : e > 63 ? 63 : e);
}
__device__ __forceinline__ uint32_t bounce_work_key(v3 d) {
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    const uint32_t axis = ax >= ay && ax >= az ? 0u : ay >= az ? 1u : 2u;
    const float m = axis == 0u ? ax : axis == 1u ? ay : az;  // 0.577 .. 1
    const int q = (int)((m - 0.5f) * 32.0f);
    return axis * 16u + (uint32_t)(q < 0 ? 0 : q > 15 ? 15 : q);
}

// ---- generate -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAppendThreads) void pt_generate(const PtFrame f, PtState st, uint32_t* __restrict__ queue, uint32_t* __restrict__ ctr) {
    __shared__ uint32_t lds[32];
    const uint32_t pid = blockIdx.x * kAppendThreads + threadIdx.x;
    bool alive = false;
    if (pid < f.n_paths) {
        const uint32_t slot = pid / f.spp_batch, s = f.sample0 + (pid - slot * f.spp_batch);
        uint32_t px, py, lx, ly, k;
        if (slot_pixel(f, slot, px, py, lx, ly, k)) {
            alive = true;
            const v3 d = camera_dir(f, px, py, s);
            st.ray_o[pid] = make_float4(f.cam.pos[0], f.cam.pos[1], f.cam.pos[2], 0.0f);
            st.ray_d[pid] = make_float4(d.x, d.y, d.z, 0.0f);
            st.thr[pid] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        }
        st.rad[pid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const uint32_t idx = block_append(alive, &ctr[PT_CTR_COUNT], lds);
    if (alive) queue[idx] = pid;
}

// ---- shade ----------------------------------------------------------------------------------------
// SURF = false: every triangle is a Lambert reflector or a light (§6.4).  SURF = true: also mirror and glass triangles
// (§6.11, albedo.w != 0); thr.w = 1 marks a path whose last vertex was one of them, so the light it hits next is counted.
//
// The stage is bound by memory latency, so an item waits for memory three times, once per true dependency, and every load of a
// level is issued before the first wait of that level:
//   1. queue[i] -> pid                       (not behind the packet kernel: there the items are the path ids)
//   2. hit / ray_d / ray_o / thr / rad of the path
//   3. the whole record of the hit triangle (the emissive flag arrives with it) and its albedo, as one batch
// emission[li] of the hit triangle stays behind the flag: only the rare path that ends on a light reads it.
// The sampled light, TAB = true (at most kShadeLightTable lights, the launcher decides): every workgroup copies lights[k], the
// record and the emission of each light into LDS once, before its first item, and the sample reads them there - no wait on
// memory.  TAB = false: lights[kk] needs the path id alone and is loaded with level 2; the light's record and emission are one
// more batch inside the estimation (64 VGPRs do not reach to start it before the hit triangle has arrived).  Both ways the
// sample runs the same operations on the same values.
constexpr uint32_t kShadeLightTable = 32;  // lights held in LDS: four float4 each (2 KiB)
// An empty statement that reads and writes x in a vector register: the load that produces x cannot move below it.
__device__ __forceinline__ void keep_here(float& x) { asm volatile("" : "+v"(x)); }
// The light of a path's next-event estimation at this depth: lights[min(floor(u N_L), N_L - 1)], from the path id alone.
__device__ __forceinline__ uint32_t light_pick(const PtScene& sc, const PtFrame& f, uint32_t pid, uint32_t depth) {
    const uint32_t slot = pid / f.spp_batch, s = f.sample0 + (pid - slot * f.spp_batch);
    uint32_t px, py, lx, ly, k;
    slot_pixel(f, slot, px, py, lx, ly, k);
    const uint32_t kk = (uint32_t)(rnd(path_key(py * f.width + px, s, f.seed), depth, 2) * (float)sc.n_lights);
    return kk > sc.n_lights - 1 ? sc.n_lights - 1 : kk;
}
template <bool SURF, bool TAB>
__global__ __launch_bounds__(kAppendThreads, 8) void pt_shade(const PtScene sc, const PtFrame f, PtState st, const uint32_t* __restrict__ queue,
                                                           const uint32_t* __restrict__ count_ptr, uint32_t depth, uint32_t* __restrict__ next_queue,
                                                           uint32_t* __restrict__ next_ctr, uint32_t sort_rays) {
    __shared__ uint32_t lds[kSortBins + 40];
    __shared__ float4 light_tab[kShadeLightTable * 4];  // per light: the three float4 of its record, then emission.xyz with lights[k] in w
    // queue == nullptr (depth 0 behind the packet kernel, which has no generate stage and no queue): the items are the
    // path ids themselves; origin = camera, throughput 1, radiance 0 are known and not read from the path state
    const bool direct = queue == nullptr;
    const uint32_t n = direct ? f.n_paths : *count_ptr;
    const uint32_t stride = gridDim.x * kAppendThreads;
    if (TAB) {
        if (threadIdx.x < sc.n_lights * 4u) {
            const uint32_t lt = sc.lights[threadIdx.x >> 2], j = threadIdx.x & 3u;
            float4 v = j < 3u ? sc.tris[(size_t)lt * 3 + j] : sc.emission[lt];
            if (j == 3u) v.w = __uint_as_float(lt);
            light_tab[threadIdx.x] = v;
        }
        __syncthreads();
    }
    // grid-stride over whole workgroups: the trip count is workgroup-uniform (barriers in block_append)
    for (uint32_t base = blockIdx.x * kAppendThreads; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool bounce = false, shadow = false;
        uint32_t pid = 0;
        float4 so = {}, sd = {}, scn = {};
        bool item = i < n;
        uint32_t px = 0, py = 0, lx, ly, k;
        if (item && direct) item = slot_pixel(f, i / f.spp_batch, px, py, lx, ly, k);
        if (item) {
            pid = direct ? i : queue[i];
            // ---- level 2: everything that hangs on pid alone
            const float2 hrec = st.hit[pid];
            uint32_t lt = 0;
            if (!TAB) lt = sc.lights[light_pick(sc, f, pid, depth)];
            const float4 rd = st.ray_d[pid];
            const float4 ro = direct ? make_float4(f.cam.pos[0], f.cam.pos[1], f.cam.pos[2], 0.0f) : st.ray_o[pid];
            const float4 T = direct ? make_float4(1.0f, 1.0f, 1.0f, 0.0f) : st.thr[pid];
            float4 L = direct ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : st.rad[pid];
            // ---- level 3: the hit triangle's record and albedo in one batch (a path that left the scene reads triangle 0 and
            // ignores it)
            const int li = __float_as_int(hrec.y);
            const size_t lr = li < 0 ? 0 : (size_t)li;
            float4 ta = sc.tris[lr * 3 + 0], tb = sc.tris[lr * 3 + 1], tc = sc.tris[lr * 3 + 2];
            float4 alb = sc.albedo[lr];
            // left alone, the compiler sinks these loads into the branches below, the flag word first and the rest behind its wait
            keep_here(tc.z), keep_here(ta.w), keep_here(tb.x), keep_here(tb.y), keep_here(tb.z), keep_here(tb.w), keep_here(tc.x);
            keep_here(alb.x), keep_here(alb.y), keep_here(alb.z);
            if (SURF) keep_here(alb.w);
            const v3 o = mk(ro.x, ro.y, ro.z), d = mk(rd.x, rd.y, rd.z);
            // depth 0 behind the packet kernel: rad[pid] is stored once per path - zero (the shadow stage and pt_resolve read
            // it), the sky term or the emission term
            if (li < 0) {  // left the scene
                L.x = __builtin_fmaf(T.x, f.sky[0], L.x);
                L.y = __builtin_fmaf(T.y, f.sky[1], L.y);
                L.z = __builtin_fmaf(T.z, f.sky[2], L.z);
                st.rad[pid] = L;
            } else {
                if (__float_as_uint(tc.z) != 0u) {  // emissive (flag in the triangle record); lights are seen directly only by camera rays
                    const bool seen = depth == 0 || (SURF && T.w != 0.0f);  // and by rays that leave a mirror or glass vertex
                    if (seen) {
                        const float4 em = sc.emission[li];
                        L.x = __builtin_fmaf(T.x, em.x, L.x);
                        L.y = __builtin_fmaf(T.y, em.y, L.y);
                        L.z = __builtin_fmaf(T.z, em.z, L.z);
                    }
                    if (seen || direct) st.rad[pid] = L;
                } else {
                    if (direct) st.rad[pid] = L;
                    v3 nrm = normalize(cross(mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x)));
                    const bool flipped = dot(nrm, d) > 0.0f;
                    if (flipped) nrm = -nrm;
                    const v3 pt = fma3(d, hrec.x, o);
                    const v3 po = fma3(nrm, f.ray_eps, pt);
                    // path id -> rng key
                    const uint32_t slot = pid / f.spp_batch, s = f.sample0 + (pid - slot * f.spp_batch);
                    slot_pixel(f, slot, px, py, lx, ly, k);
                    const uint32_t key = path_key(py * f.width + px, s, f.seed);
                    const bool delta = SURF && alb.w != 0.0f;  // mirror or glass: no next-event estimation; on as a bounce ray or the path ends
                    if (delta && depth < f.bounces) {
                        bool below;
                        const v3 nd = delta_dir(d, nrm, alb.w, flipped, rnd(key, depth, 7), below);
                        const v3 no = below ? fma3(nrm, -f.ray_eps, pt) : po;
                        bounce = true;
                        st.ray_o[pid] = make_float4(no.x, no.y, no.z, 0.0f);
                        st.ray_d[pid] = make_float4(nd.x, nd.y, nd.z, 0.0f);
                        st.thr[pid] = make_float4(T.x * alb.x, T.y * alb.y, T.z * alb.z, 1.0f);
                    }
                    if (!delta && sc.n_lights > 0) {  // next-event estimation
                        float4 la, lb, lc, le;
                        if (TAB) {
                            uint32_t kk = (uint32_t)(rnd(key, depth, 2) * (float)sc.n_lights);
                            if (kk > sc.n_lights - 1) kk = sc.n_lights - 1;
                            la = light_tab[kk * 4u + 0u], lb = light_tab[kk * 4u + 1u], lc = light_tab[kk * 4u + 2u];
                            le = light_tab[kk * 4u + 3u];
                        } else {  // the record and the emission in one batch: the registers do not reach to start it before the hit triangle is there
                            la = sc.tris[(size_t)lt * 3 + 0], lb = sc.tris[(size_t)lt * 3 + 1], lc = sc.tris[(size_t)lt * 3 + 2];
                            le = sc.emission[lt];
                            keep_here(le.x), keep_here(le.y), keep_here(le.z);
                        }
                        const float su = __builtin_sqrtf(rnd(key, depth, 3)), u2 = rnd(key, depth, 4);
                        const float b1 = su * (1.0f - u2), b2 = su * u2;
                        const v3 lv0 = mk(la.x, la.y, la.z), le1 = mk(la.w, lb.x, lb.y), le2 = mk(lb.z, lb.w, lc.x);
                        const v3 q = mk(__builtin_fmaf(le2.x, b2, __builtin_fmaf(le1.x, b1, lv0.x)), __builtin_fmaf(le2.y, b2, __builtin_fmaf(le1.y, b1, lv0.y)),
                                        __builtin_fmaf(le2.z, b2, __builtin_fmaf(le1.z, b1, lv0.z)));
                        const v3 wi = q - po;
                        const float d2 = dot(wi, wi);
                        const v3 nl = cross(le1, le2);
                        const float cs = dot(nrm, wi), cl = __builtin_fabsf(dot(nl, wi));
                        const float d4 = d2 * d2;  // underflows to 0 for a light closer than about 2^-37 (d2 > 0 still): no sample, not a division by 0
                        if (cs > 0.0f && cl > 0.0f && d4 > 0.0f) {
                            const float w = ((cs * cl) * ((float)sc.n_lights * 0.15915494f)) / d4;
                            shadow = true;
                            so = make_float4(po.x, po.y, po.z, __uint_as_float(pid));
                            sd = make_float4(wi.x, wi.y, wi.z, 0.0f);
                            scn = make_float4(((T.x * alb.x) * le.x) * w, ((T.y * alb.y) * le.y) * w, ((T.z * alb.z) * le.z) * w, 0.0f);
                        }
                    }
                    if (!delta && depth < f.bounces) {
                        const v3 nd = cosine_dir(nrm, rnd(key, depth, 5), rnd(key, depth, 6));
                        bounce = true;
                        st.ray_o[pid] = make_float4(po.x, po.y, po.z, 0.0f);
                        st.ray_d[pid] = make_float4(nd.x, nd.y, nd.z, 0.0f);
                        st.thr[pid] = make_float4(T.x * alb.x, T.y * alb.y, T.z * alb.z, 0.0f);
                    }
                }
            }
        }
        uint32_t bi, si;
        if (sort_rays == 2u) {  // wave-uniform
            uint32_t kb = 0, ks = 0;
            if (bounce) {
                const float4 rd = st.ray_d[pid];
                kb = bounce_work_key(mk(rd.x, rd.y, rd.z));
            }
            if (shadow) ks = shadow_work_key(mk(sd.x, sd.y, sd.z));
            bi = block_append_sorted<64>(bounce, kb, &next_ctr[PT_CTR_COUNT], lds);
            si = block_append_sorted<64>(shadow, ks, &next_ctr[PT_CTR_SHADOW_COUNT], lds);
        } else if (sort_rays) {
            uint32_t kb = 0, ks = 0;
            if (bounce) {
                const float4 ro = st.ray_o[pid], rd = st.ray_d[pid];
                kb = ray_sort_key(sc.nodes, mk(ro.x, ro.y, ro.z), mk(rd.x, rd.y, rd.z));
            }
            if (shadow) ks = ray_sort_key(sc.nodes, mk(so.x, so.y, so.z), mk(sd.x, sd.y, sd.z));
            bi = block_append_sorted(bounce, kb, &next_ctr[PT_CTR_COUNT], lds);
            si = block_append_sorted(shadow, ks, &next_ctr[PT_CTR_SHADOW_COUNT], lds);
        } else {
            bi = block_append(bounce, &next_ctr[PT_CTR_COUNT], lds);
            si = block_append(shadow, &next_ctr[PT_CTR_SHADOW_COUNT], lds);
        }
        if (bounce) next_queue[bi] = pid;
        if (shadow) {
            st.sh_o[si] = so;
            st.sh_d[si] = sd;
            st.sh_c[si] = scn;
        }
    }
}

// ---- resolve --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_resolve(const PtFrame f, PtState st, float* __restrict__ acc, float* __restrict__ dst, uint32_t tile_major) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= f.n_slots) return;
    uint32_t px, py, lx, ly, k;
    if (!slot_pixel(f, slot, px, py, lx, ly, k)) return;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (f.sample0 > 0) {
        r = acc[(size_t)slot * 3 + 0];
        g = acc[(size_t)slot * 3 + 1];
        b = acc[(size_t)slot * 3 + 2];
    }
    for (uint32_t s = 0; s < f.spp_batch; s++) {  // spec §6.6: samples are summed in index order
        const float4 L = st.rad[(size_t)slot * f.spp_batch + s];
        r += L.x;
        g += L.y;
        b += L.z;
    }
    if (f.sample0 + f.spp_batch < f.spp_total) {
        acc[(size_t)slot * 3 + 0] = r;
        acc[(size_t)slot * 3 + 1] = g;
        acc[(size_t)slot * 3 + 2] = b;
        return;
    }
    const float inv = (float)f.spp_total;
    const size_t idx = tile_major ? ((size_t)k * (RT_TILE * RT_TILE) + (size_t)ly * RT_TILE + lx) : ((size_t)py * f.width + px);
    dst[idx * 3 + 0] = r / inv;
    dst[idx * 3 + 1] = g / inv;
    dst[idx * 3 + 2] = b / inv;
}

// ---- surfaces (rt_set_mesh_surfaces, §6.11) -------------------------------------------------------
// albedo.w of every leaf position from the surface words in original triangle order: word 9 of the triangle record names
// the triangle, whichever builder wrote the records.  surf == nullptr: every triangle Lambert (0)
__global__ __launch_bounds__(256) void pt_scatter_surfaces(const float4* __restrict__ tris, const float* __restrict__ surf, float4* __restrict__ albedo,
                                                           uint32_t n) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= n) return;
    const uint32_t t = __float_as_uint(tris[(size_t)li * 3 + 2].y);
    reinterpret_cast<float*>(albedo)[(size_t)li * 4 + 3] = surf && t < n ? surf[t] : 0.0f;
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_generate(Ctx* c, const PtFrame& f, const PtState& st, uint32_t* queue, uint32_t* ctr) {
    hipLaunchKernelGGL(pt_generate, dim3((f.n_paths + kAppendThreads - 1u) / kAppendThreads), dim3(kAppendThreads), 0, c->stream, f, st, queue, ctr);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int launch_pt_shade(Ctx* c, const PtScene& sc, const PtFrame& f, const PtState& st, const uint32_t* queue, const uint32_t* count_ptr,
                    uint32_t depth, uint32_t* next_queue, uint32_t* next_ctr, uint32_t grid, uint32_t sort_rays, bool surfaces) {
    const bool tab = sc.n_lights <= kShadeLightTable;
    auto kernel = surfaces ? (tab ? pt_shade<true, true> : pt_shade<true, false>) : (tab ? pt_shade<false, true> : pt_shade<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kAppendThreads), 0, c->stream, sc, f, st, queue, count_ptr, depth, next_queue, next_ctr, sort_rays);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int launch_pt_scatter_surfaces(Ctx* c, const float4* tris, const float* surf, float4* albedo, uint32_t n) {
    hipLaunchKernelGGL(pt_scatter_surfaces, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, tris, surf, albedo, n);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int launch_pt_resolve(Ctx* c, const PtFrame& f, const PtState& st, float* acc, float* dst, int tile_major) {
    hipLaunchKernelGGL(pt_resolve, dim3((f.n_slots + 255u) / 256u), dim3(256), 0, c->stream, f, st, acc, dst, (uint32_t)(tile_major ? 1 : 0));
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

}  // namespace rt
