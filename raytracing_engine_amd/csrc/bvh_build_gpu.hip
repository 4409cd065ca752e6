// bvh_build_gpu.hip — path B's BVH built on the GPU from device-resident triangles (rt_set_mesh_device).
//
// Produces exactly the node format of bvh_node.h (80-byte compressed 8-wide nodes, one triangle per leaf slot,
// breadth-first order, inner children and leaf triangles consecutive per node), so the traversal kernels cannot tell
// the difference.  The tree itself is an LBVH (Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees,
// and k-d Trees", HPG 2012) collapsed top-down into 8-wide nodes; stages and their launches: DESIGN.md §6.9.  The refit of a
// single-level tree, host- or device-built, to new vertices (rt_refit_mesh_device) is here too: it shares the
// validation with the build, and the quantiser (bvh_node.h) with the build and with the host builder.
//
// Rules every kernel here keeps:
//  - no data passes between workgroups inside a launch: every dependency is a launch boundary (no flags, no look-back,
//    no grid barriers); the only global atomics add histogram counts, whose sums do not depend on order;
//  - the output is a deterministic function of the input: keys are (30-bit Morton code, triangle index), unique, and
//    every reduction is a min / max / integer sum;
//  - every index a kernel derives from another kernel's output is bounds-checked before it is used to store.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "bvh_node.h"
#include "rt_internal.h"

namespace rt {
namespace {

constexpr int kThreads = 256;                          // every kernel: 256-thread workgroups (four waves of 64)
constexpr uint32_t kSortTile = kThreads * 16u;         // keys per workgroup of one radix pass
constexpr uint32_t kScanTile = kThreads * 16u;         // elements per workgroup of a scan
constexpr uint32_t kReduceBlocks = 1024;               // workgroups of the grid-stride reductions
constexpr uint32_t kTopLevelNodes = 4096;              // segment-tree levels this small are built by one workgroup
constexpr int32_t kEmpty = INT_MIN;                    // empty child slot in a plan
constexpr uint32_t kMaxLevels = 128;                   // the binary tree is at most 62 deep (key bits); a guard only

struct Plan {  // one 8-wide node: child reference per slot (>= 0 binary inner node, < 0 ~sorted leaf position, kEmpty)
    int32_t slot[8];
};

// padded box of triangle t, its edges formed in fp32 as set_mesh_impl forms them for build_bvh
__device__ __forceinline__ Box tri_box_at(const float* __restrict__ v, uint32_t t, float pad) {
    const float* p = v + 9 * (size_t)t;
    float e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
    }
    return tri_box(p, e1, e2, pad);
}

template <class T, class Op>
__device__ T block_reduce(T v, Op op) {
    __shared__ T s[kThreads];
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] = op(s[tid], s[tid + o]);
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}

template <class T>
__device__ T block_exclusive(T v, T* total) {
    __shared__ T s[kThreads];
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const T x = tid >= o ? s[tid - o] : T(0);
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    *total = s[kThreads - 1];
    const T r = s[tid] - v;
    __syncthreads();
    return r;
}

struct FMax {
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct FMin {
    __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct UOr {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; }
};
template <class T>
struct Sum {
    __device__ T operator()(T a, T b) const { return a + b; }
};

// ---- 1. validate and measure -------------------------------------------------------------------------------------------
// per workgroup: largest |v0|, |v0 + e1|, |v0 + e2| (build_bvh's maxabs) and whether any input coordinate is not finite
__global__ __launch_bounds__(kThreads) void bvhd_validate(const float* __restrict__ v, uint32_t n, float* __restrict__ part_max,
                                                          uint32_t* __restrict__ part_bad) {
    float m = 0.0f;
    uint32_t bad = 0;
    for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (size_t)gridDim.x * kThreads) {
        const float* p = v + 9 * t;
        float x[9];
        for (int i = 0; i < 9; i++) {
            x[i] = p[i];
            bad |= isfinite(x[i]) ? 0u : 1u;
        }
        for (int a = 0; a < 3; a++) {
            const float p0 = x[a], p1 = p0 + (x[3 + a] - p0), p2 = p0 + (x[6 + a] - p0);
            m = fmaxf(m, fmaxf(fabsf(p0), fmaxf(fabsf(p1), fabsf(p2))));
        }
    }
    m = block_reduce(m, FMax{});
    bad = block_reduce(bad, UOr{});
    if (threadIdx.x == 0) {
        part_max[blockIdx.x] = m;
        part_bad[blockIdx.x] = bad;
    }
}

// ---- 2. centroid bounds ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bvhd_bounds(const float* __restrict__ v, uint32_t n, float pad, float* __restrict__ part) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (size_t)gridDim.x * kThreads) {
        const Box b = tri_box_at(v, (uint32_t)t, pad);
        for (int a = 0; a < 3; a++) {
            const float c = 0.5f * (b.lo[a] + b.hi[a]);
            lo[a] = fminf(lo[a], c);
            hi[a] = fmaxf(hi[a], c);
        }
    }
    for (int a = 0; a < 3; a++) {
        const float l = block_reduce(lo[a], FMin{}), h = block_reduce(hi[a], FMax{});
        if (threadIdx.x == 0) {
            part[a * gridDim.x + blockIdx.x] = l;
            part[(3 + a) * gridDim.x + blockIdx.x] = h;
        }
    }
}

__global__ __launch_bounds__(kThreads) void bvhd_bounds_final(const float* __restrict__ part, uint32_t parts, float* __restrict__ bounds) {
    for (int k = 0; k < 6; k++) {
        float x = k < 3 ? INFINITY : -INFINITY;
        for (uint32_t i = threadIdx.x; i < parts; i += kThreads) x = k < 3 ? fminf(x, part[k * parts + i]) : fmaxf(x, part[k * parts + i]);
        x = k < 3 ? block_reduce(x, FMin{}) : block_reduce(x, FMax{});
        if (threadIdx.x == 0) bounds[k] = x;
    }
}

// ---- 3. keys -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t x) {  // 10 bits -> every third bit of 30
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// key = 30-bit Morton code of the box centroid over the centroid bounds (high word) | triangle index (low word): unique
__global__ __launch_bounds__(kThreads) void bvhd_keys(const float* __restrict__ v, uint32_t n, float pad, const float* __restrict__ bounds,
                                                      unsigned long long* __restrict__ keys) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    const Box b = tri_box_at(v, t, pad);
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float c = 0.5f * (b.lo[a] + b.hi[a]), lo = bounds[a], ext = bounds[3 + a] - lo;
        // a zero-extent axis (flat meshes, walls) contributes 0 bits of information: every centroid maps to cell 0
        q[a] = ext > 0.0f ? (uint32_t)fminf(fmaxf((c - lo) / ext * 1024.0f, 0.0f), 1023.0f) : 0u;
    }
    const uint32_t morton = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    keys[t] = ((unsigned long long)morton << 32) | t;
}

// ---- 4. LSD radix sort, 8-bit digits -----------------------------------------------------------------------------------
// whole-array histograms of all eight digits (order-independent sums): a digit whose keys all fall into one bucket is skipped
__global__ __launch_bounds__(kThreads) void bvhd_digit_hist(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ ghist) {
    __shared__ uint32_t h[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += kThreads) h[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const unsigned long long k = keys[i];
        for (int p = 0; p < 8; p++) atomicAdd(&h[p * 256 + (uint32_t)((k >> (8 * p)) & 255u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += kThreads)
        if (h[i]) atomicAdd(&ghist[i], h[i]);
}

// per-workgroup digit counts, digit-major (hist[d * blocks + b]) so that one exclusive scan gives every scatter base
__global__ __launch_bounds__(kThreads) void bvhd_sort_hist(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t shift,
                                                           uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortTile / kThreads; r++) {
        const size_t i = base + (size_t)r * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// stable scatter: rounds of 256 consecutive keys; inside a round a key's rank = keys of its digit in earlier waves + earlier
// lanes of its own wave (lanes of equal digit found with eight ballots)
__global__ __launch_bounds__(kThreads) void bvhd_sort_scatter(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                              uint32_t n, uint32_t shift, const uint32_t* __restrict__ offs) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcnt[kThreads / 64][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    base[tid] = offs[(size_t)tid * gridDim.x + blockIdx.x];
    for (int w = 0; w < kThreads / 64; w++) wcnt[w][tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const size_t tile = (size_t)blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortTile / kThreads; r++) {
        const size_t i = tile + (size_t)r * kThreads + tid;
        const bool valid = i < n;
        const unsigned long long k = valid ? in[i] : 0ull;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
            for (int w = 0; w < wave; w++) pos += wcnt[w][d];
            if (pos < n) out[pos] = k;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < kThreads / 64; w++) {
            add += wcnt[w][tid];
            wcnt[w][tid] = 0;
        }
        base[tid] += add;
        __syncthreads();
    }
}

// ---- exclusive scan (three launches: tile sums, one workgroup over the sums, tiles) ---------------------------------------
template <class T>
__global__ __launch_bounds__(kThreads) void bvhd_scan_reduce(const T* __restrict__ in, size_t count, T* __restrict__ sums) {
    const size_t t0 = (size_t)blockIdx.x * kScanTile, t1 = std::min(count, t0 + kScanTile);
    T s = 0;
    for (size_t i = t0 + threadIdx.x; i < t1; i += kThreads) s += in[i];
    s = block_reduce(s, Sum<T>{});
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

template <class T>
__global__ __launch_bounds__(kThreads) void bvhd_scan_top(T* __restrict__ sums, uint32_t parts, T* __restrict__ total) {
    T carry = 0;
    for (uint32_t c0 = 0; c0 < parts; c0 += kThreads) {
        const uint32_t i = c0 + threadIdx.x;
        const T x = i < parts ? sums[i] : T(0);
        T tot;
        const T ex = block_exclusive(x, &tot);
        if (i < parts) sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class T>
__global__ __launch_bounds__(kThreads) void bvhd_scan_down(const T* __restrict__ in, size_t count, const T* __restrict__ sums, T* __restrict__ out) {
    constexpr int kPer = 4;
    const size_t t0 = (size_t)blockIdx.x * kScanTile, t1 = std::min(count, t0 + kScanTile);
    T carry = sums[blockIdx.x];
    for (size_t c0 = t0; c0 < t1; c0 += (size_t)kThreads * kPer) {
        const size_t i0 = c0 + (size_t)threadIdx.x * kPer;
        T x[kPer], local = 0;
        for (int j = 0; j < kPer; j++) {
            x[j] = i0 + j < t1 ? in[i0 + j] : T(0);
            local += x[j];
        }
        T tot;
        T run = carry + block_exclusive(local, &tot);
        for (int j = 0; j < kPer; j++) {
            if (i0 + j < t1) out[i0 + j] = run;
            run += x[j];
        }
        carry += tot;
    }
}

// ---- 5. binary radix tree (Karras 2012): internal node i, children and leaf range -----------------------------------------
__device__ __forceinline__ int key_delta(const unsigned long long* __restrict__ k, long long n, long long i, long long j) {
    if (j < 0 || j >= n) return -1;
    return __clzll(k[i] ^ k[j]);  // keys are unique: the xor is never 0
}

// child reference: >= 0 internal node, < 0 ~(sorted leaf position)
__global__ __launch_bounds__(kThreads) void bvhd_karras(const unsigned long long* __restrict__ keys, uint32_t n, int2* __restrict__ child,
                                                        uint2* __restrict__ range) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)n - 1) return;
    const long long nn = n;
    const int d = key_delta(keys, nn, i, i + 1) - key_delta(keys, nn, i, i - 1) > 0 ? 1 : -1;
    const int dmin = key_delta(keys, nn, i, i - d);
    long long lmax = 2;
    while (key_delta(keys, nn, i, i + lmax * d) > dmin) lmax <<= 1;
    long long l = 0;
    for (long long t = lmax >> 1; t >= 1; t >>= 1)
        if (key_delta(keys, nn, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = key_delta(keys, nn, i, j);
    long long s = 0, step = l;
    do {
        step = (step + 1) >> 1;
        if (s + step < l && key_delta(keys, nn, i, i + (s + step) * d) > dnode) s += step;
    } while (step > 1);
    const long long gamma = i + s * d + (d < 0 ? -1 : 0);
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    child[i] = make_int2(lo == gamma ? ~(int)gamma : (int)gamma, hi == gamma + 1 ? ~(int)(gamma + 1) : (int)(gamma + 1));
    range[i] = make_uint2((uint32_t)lo, (uint32_t)hi);
}

// ---- 6. boxes: a min/max segment tree over the sorted leaf boxes (tree[n + i] = leaf i, tree[k] = tree[2k] u tree[2k+1]) --
__global__ __launch_bounds__(kThreads) void bvhd_leaf_boxes(const float* __restrict__ v, const unsigned long long* __restrict__ keys, uint32_t n,
                                                            float pad, Box* __restrict__ tree) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) tree[(size_t)n + i] = tri_box_at(v, (uint32_t)keys[i], pad);
}

__global__ __launch_bounds__(kThreads) void bvhd_box_level(Box* __restrict__ tree, uint32_t k0, uint32_t k1) {
    const uint32_t k = k0 + blockIdx.x * kThreads + threadIdx.x;
    if (k >= k1) return;
    Box b = tree[2 * (size_t)k];
    b.grow(tree[2 * (size_t)k + 1]);
    tree[k] = b;
}

// the small top levels [1, 2^(jtop+1)) by one workgroup, level after level (a barrier between levels, no other workgroup involved)
__global__ __launch_bounds__(kThreads) void bvhd_box_top(Box* __restrict__ tree, uint32_t n, int jtop) {
    for (int j = jtop; j >= 0; j--) {
        const uint32_t k1 = std::min<uint32_t>(2u << j, n);
        for (uint32_t k = (1u << j) + threadIdx.x; k < k1; k += kThreads) {
            Box b = tree[2 * (size_t)k];
            b.grow(tree[2 * (size_t)k + 1]);
            tree[k] = b;
        }
        __syncthreads();
    }
}

// box of internal node i = union of its leaf range, composed from O(log n) segment-tree pieces (min / max: exact)
__global__ __launch_bounds__(kThreads) void bvhd_inner_boxes(const Box* __restrict__ tree, const uint2* __restrict__ range, uint32_t n,
                                                             Box* __restrict__ ibox) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i + 1 >= n) return;
    const uint2 r = range[i];
    size_t lo = (size_t)r.x + n, hi = (size_t)r.y + n + 1;
    Box b = Box::empty();
    while (lo < hi) {
        if (lo & 1) b.grow(tree[lo++]);
        if (hi & 1) b.grow(tree[--hi]);
        lo >>= 1;
        hi >>= 1;
    }
    ibox[i] = b;
}

// ---- 7. collapse to 8-wide nodes, one level at a time -----------------------------------------------------------------------
struct TreeView {
    const int2* child;
    const Box* ibox;
    const Box* tree;
    uint32_t n;
    __device__ Box box(int32_t ref) const { return ref >= 0 ? ibox[ref] : tree[(size_t)n + (uint32_t)~ref]; }
};

// children of one 8-wide node and their slots (assign_slots, as the host builder's plan()); counts = inner << 32 | leaves
__global__ __launch_bounds__(kThreads) void bvhd_plan(TreeView tv, const int32_t* __restrict__ level, uint32_t count, Plan* __restrict__ plan,
                                                      unsigned long long* __restrict__ counts) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= count) return;
    int32_t ch[8];
    int k;
    if (tv.n == 1) {  // the whole mesh is one triangle: a root with a single leaf child, as the host builds it
        ch[0] = ~0;
        k = 1;
    } else {
        const int2 c = tv.child[level[w]];
        ch[0] = c.x;
        ch[1] = c.y;
        k = 2;
        // open the inner child with the largest surface area until there are eight children or only leaves
        while (k < 8) {
            int best = -1;
            float best_a = -1.0f;
            for (int i = 0; i < k; i++) {
                if (ch[i] < 0) continue;
                const float a = tv.ibox[ch[i]].half_area();
                if (a > best_a) {
                    best_a = a;
                    best = i;
                }
            }
            if (best < 0) break;
            const int2 cc = tv.child[ch[best]];
            ch[best] = cc.x;
            ch[k++] = cc.y;
        }
    }
    Box cb[8], nb = Box::empty();
    for (int i = 0; i < k; i++) {
        cb[i] = tv.box(ch[i]);
        nb.grow(cb[i]);
    }
    int child_in[8];
    assign_slots(cb, k, nb, child_in);
    Plan p;
    uint32_t inner = 0, leaves = 0;
    for (int s = 0; s < 8; s++) {
        p.slot[s] = child_in[s] >= 0 ? ch[child_in[s]] : kEmpty;
        if (child_in[s] < 0) continue;
        if (p.slot[s] >= 0) inner++;
        else leaves++;
    }
    plan[w] = p;
    counts[w] = ((unsigned long long)inner << 32) | leaves;
}

// node words (quantise()), the next level's binary nodes and the leaf order
__global__ __launch_bounds__(kThreads) void bvhd_write(TreeView tv, const Plan* __restrict__ plan, const unsigned long long* __restrict__ excl,
                                                       uint32_t count, uint32_t level_base, uint32_t tri_before, uint32_t node_cap,
                                                       const unsigned long long* __restrict__ keys, uint32_t* __restrict__ nodes,
                                                       int32_t* __restrict__ next_level, uint32_t* __restrict__ order) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= count) return;
    const Plan p = plan[w];
    const unsigned long long ex = excl[w];
    const uint32_t inner0 = (uint32_t)(ex >> 32), child_base = level_base + count + inner0, tri_base = tri_before + (uint32_t)ex;
    Box cb[8], nb = Box::empty();
    uint32_t imask = 0, leafmask = 0, rank = 0, off = 0;
    for (int s = 0; s < 8; s++) {
        const int32_t r = p.slot[s];
        if (r == kEmpty) continue;
        cb[s] = tv.box(r);
        nb.grow(cb[s]);
        if (r >= 0) {
            imask |= 1u << s;
            const uint32_t at = inner0 + rank++;
            if (at < node_cap) next_level[at] = r;
        } else {
            leafmask |= 1u << s;
            const uint32_t li = tri_base + off++;
            if (li < tv.n) order[li] = (uint32_t)keys[(uint32_t)~r];  // low word of the key: original triangle index
        }
    }
    uint32_t wd[kNodeWords];
    quantise(nb, cb, imask | leafmask, wd);
    node_set_topology(wd, imask, child_base, tri_base, leafmask);
    const uint32_t node = level_base + w;
    if (node >= node_cap) return;
    uint4* dst = reinterpret_cast<uint4*>(node_at(nodes, node));
    for (uint32_t i = 0; i < kNodeWords / 4; i++) dst[i] = make_uint4(wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3]);
}

// ---- 8. leaf-order payload and the light list -----------------------------------------------------------------------------
__device__ __forceinline__ void load_record(const float4* __restrict__ tris, uint32_t li, float r[kTriWords]) {
    for (uint32_t i = 0; i < kTriWords / 4; i++) {
        const float4 x = tris[(kTriWords / 4) * (size_t)li + i];
        r[4 * i] = x.x;
        r[4 * i + 1] = x.y;
        r[4 * i + 2] = x.z;
        r[4 * i + 3] = x.w;
    }
}

__device__ __forceinline__ void store_record(float4* __restrict__ tris, uint32_t li, const float r[kTriWords]) {
    for (uint32_t i = 0; i < kTriWords / 4; i++) tris[(kTriWords / 4) * (size_t)li + i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}

__global__ __launch_bounds__(kThreads) void bvhd_payload(const float* __restrict__ v, const float* __restrict__ albedo, const float* __restrict__ emission,
                                                         const uint32_t* __restrict__ order, uint32_t n, float4* __restrict__ tris,
                                                         float4* __restrict__ alb, float4* __restrict__ emi, uint32_t* __restrict__ leaf_pos,
                                                         uint32_t* __restrict__ light_flag) {
    const uint32_t li = blockIdx.x * kThreads + threadIdx.x;
    if (li >= n) return;
    const uint32_t t = order[li];
    if (t >= n) return;
    leaf_pos[t] = li;
    const float* p = v + 9 * (size_t)t;
    float e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
    }
    const float* em = emission + 3 * (size_t)t;
    const float* al = albedo + 3 * (size_t)t;
    const uint32_t light = is_emissive(em) ? 1u : 0u;
    float r[kTriWords];
    pack_tri_record(p, e1, e2, t, light != 0u, r);
    store_record(tris, li, r);
    alb[li] = make_float4(al[0], al[1], al[2], 0.0f);
    emi[li] = make_float4(em[0], em[1], em[2], 0.0f);
    light_flag[t] = light;
}

// lights in ascending original index, as leaf positions: an ordered compaction through the exclusive scan of the flags
__global__ __launch_bounds__(kThreads) void bvhd_lights(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ leaf_pos,
                                                        uint32_t n, uint32_t n_lights, uint32_t* __restrict__ lights) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < n && flag[t] && slot[t] < n_lights) lights[slot[t]] = leaf_pos[t];
}

// ---- refit (rt_refit_mesh_device): new vertices, the same topology and leaf order; DESIGN.md §6.10 ------------------------------
constexpr int kRefitTopThreads = 512;  // the top levels: one workgroup, a barrier between levels (512: 256 VGPRs, no spill)
constexpr uint32_t kRefitTopNodes = 1024;  // levels from the root down that hold at most this many nodes each are refitted by it
constexpr uint32_t kRefitTopMax = 16;

struct RefitTop {  // level j of the top = nodes [start[j], start[j + 1]), j < levels
    uint32_t start[kRefitTopMax + 1];
    uint32_t levels;
};

// triangle record of leaf position li: packed again from the new vertices of its triangle t = word 9 (edges formed in fp32 as in
// bvhd_payload / set_mesh_impl), index and light flag as they were.  Coalesced record traffic, gathered vertex reads
__global__ __launch_bounds__(kThreads) void bvhr_tris(const float* __restrict__ v, uint32_t n, float4* __restrict__ tris) {
    const uint32_t li = blockIdx.x * kThreads + threadIdx.x;
    if (li >= n) return;
    const float4 last = tris[(kTriWords / 4) * (size_t)li + kTriIdWord / 4];
    const uint32_t t = __float_as_uint(last.y), light = __float_as_uint(last.z);
    static_assert(kTriIdWord % 4 == 1 && kTriLightWord == kTriIdWord + 1, "index and light flag are .y and .z of the record's last float4");
    if (t >= n) return;
    const float* p = v + 9 * (size_t)t;
    float x[9];
    for (int i = 0; i < 9; i++) x[i] = p[i];
    float e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
        e1[a] = x[3 + a] - x[a];
        e2[a] = x[6 + a] - x[a];
    }
    float r[kTriWords];
    pack_tri_record(x, e1, e2, t, light != 0u, r);
    store_record(tris, li, r);
}

// padded box of the triangle at leaf position li, from its record
__device__ __forceinline__ Box record_box(const float4* __restrict__ tris, uint32_t li, float pad) {
    float r[kTriWords];
    load_record(tris, li, r);
    return tri_box(r, r + 3, r + 6, pad);
}

// node k: every slot's exact box (a leaf slot's padded triangle box, an inner slot's box as its child stored it one level deeper),
// their union, the quantised frame and planes (words 0-3 with imask kept, words 8-19; words 4-7 untouched) and the node's exact
// box for its parent.  Indices come from the node's own words and are checked before they are used
__device__ __forceinline__ void refit_node(uint32_t* __restrict__ nodes, const float4* __restrict__ tris, uint32_t n, uint32_t n_nodes, float pad,
                                           Box* __restrict__ box, uint32_t k) {
    uint4* nd = reinterpret_cast<uint4*>(node_at(nodes, k));
    const uint4 h0 = nd[0], h1 = nd[1];
    uint32_t wd[kNodeWords] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    const uint32_t imask = node_imask(wd), leafmask = node_leafmask(wd) & ~imask, child_base = node_child_base(wd), tri_base = node_tri_base(wd);
    Box cb[8], nb = Box::empty();
    uint32_t rank = 0, off = 0;
    for (int s = 0; s < 8; s++) {
        cb[s] = Box::empty();
        if ((imask >> s) & 1u) {
            const uint32_t ch = child_base + rank++;
            if (ch < n_nodes) cb[s] = box[ch];
        } else if ((leafmask >> s) & 1u) {
            const uint32_t li = tri_base + off++;
            if (li < n) cb[s] = record_box(tris, li, pad);
        } else {
            continue;
        }
        nb.grow(cb[s]);
    }
    quantise(nb, cb, imask | leafmask, wd);
    node_set_topology(wd, imask, child_base, tri_base, leafmask);  // quantise() cleared the imask; words 4-7 are not stored
    nd[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    nd[2] = make_uint4(wd[8], wd[9], wd[10], wd[11]);
    nd[3] = make_uint4(wd[12], wd[13], wd[14], wd[15]);
    nd[4] = make_uint4(wd[16], wd[17], wd[18], wd[19]);
    box[k] = nb;
}

// one level [k0, k1), one thread per node; the level below was finished by the previous launch
__global__ __launch_bounds__(kThreads) void bvhr_level(uint32_t* __restrict__ nodes, const float4* __restrict__ tris, uint32_t n, uint32_t n_nodes,
                                                       float pad, Box* __restrict__ box, uint32_t k0, uint32_t k1) {
    const uint32_t k = k0 + blockIdx.x * kThreads + threadIdx.x;
    if (k < k1 && k < n_nodes) refit_node(nodes, tris, n, n_nodes, pad, box, k);
}

// the top levels, deepest first, by one workgroup (a barrier between levels, no other workgroup involved)
__global__ __launch_bounds__(kRefitTopThreads) void bvhr_top(uint32_t* __restrict__ nodes, const float4* __restrict__ tris, uint32_t n, uint32_t n_nodes,
                                                             float pad, Box* __restrict__ box, RefitTop top) {
    for (int j = (int)top.levels - 1; j >= 0; j--) {
        const uint32_t k1 = min(top.start[j + 1], n_nodes);
        for (uint32_t k = top.start[j] + threadIdx.x; k < k1; k += kRefitTopThreads) refit_node(nodes, tris, n, n_nodes, pad, box, k);
        __syncthreads();
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
uint32_t blocks_for(size_t items) { return (uint32_t)((items + kThreads - 1) / kThreads); }

struct Bump {  // carves the one scratch allocation
    char* base = nullptr;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base ? base + used : nullptr);
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

struct Scratch {
    float* part_max;
    uint32_t* part_bad;
    float* part_bounds;
    float* bounds;
    unsigned long long* keys[2];
    uint32_t* ghist;
    uint32_t* hist;
    uint32_t* hist_off;
    unsigned long long* sums;  // scan tile sums (u32 scans use the same storage)
    unsigned long long* total;
    int2* child;
    uint2* range;
    Box* ibox;
    Box* tree;
    int32_t* level[2];
    Plan* plan;
    unsigned long long* counts;
    unsigned long long* excl;
    uint32_t* nodes;
    uint32_t* order;
    uint32_t* leaf_pos;
    uint32_t* flag;
    uint32_t* flag_excl;
};

void carve(Bump& b, Scratch& s, size_t n) {
    const size_t m = std::max<size_t>(n - 1, 1), sort_blocks = (n + kSortTile - 1) / kSortTile;
    const size_t scan_max = std::max<size_t>(n, 256 * sort_blocks);
    s.part_max = b.take<float>(kReduceBlocks);
    s.part_bad = b.take<uint32_t>(kReduceBlocks);
    s.part_bounds = b.take<float>(6 * kReduceBlocks);
    s.bounds = b.take<float>(8);
    s.keys[0] = b.take<unsigned long long>(n);
    s.keys[1] = b.take<unsigned long long>(n);
    s.ghist = b.take<uint32_t>(8 * 256);
    s.hist = b.take<uint32_t>(256 * sort_blocks);
    s.hist_off = b.take<uint32_t>(256 * sort_blocks);
    s.sums = b.take<unsigned long long>((scan_max + kScanTile - 1) / kScanTile + 1);
    s.total = b.take<unsigned long long>(1);
    s.child = b.take<int2>(m);
    s.range = b.take<uint2>(m);
    s.ibox = b.take<Box>(m);
    s.tree = b.take<Box>(2 * n);
    s.level[0] = b.take<int32_t>(m);
    s.level[1] = b.take<int32_t>(m);
    s.plan = b.take<Plan>(m);
    s.counts = b.take<unsigned long long>(m);
    s.excl = b.take<unsigned long long>(m);
    s.nodes = b.take<uint32_t>(kNodeWords * m);
    s.order = b.take<uint32_t>(n);
    s.leaf_pos = b.take<uint32_t>(n);
    s.flag = b.take<uint32_t>(n);
    s.flag_excl = b.take<uint32_t>(n);
}

#define BVHD_LAUNCH(ctx)                                                                           \
    do {                                                                                           \
        hipError_t e_ = hipGetLastError();                                                         \
        if (e_ != hipSuccess) return (ctx)->fail(RT_ERR_HIP, "device BVH build: %s", hipGetErrorString(e_)); \
    } while (0)

// exclusive scan of count elements; the sum of all of them lands in *total (device)
template <class T>
int scan(Ctx* c, const T* in, T* out, size_t count, T* sums, T* total) {
    const uint32_t parts = (uint32_t)((count + kScanTile - 1) / kScanTile);
    hipLaunchKernelGGL(bvhd_scan_reduce<T>, dim3(parts), dim3(kThreads), 0, c->stream, in, count, sums);
    hipLaunchKernelGGL(bvhd_scan_top<T>, dim3(1), dim3(kThreads), 0, c->stream, sums, parts, total);
    hipLaunchKernelGGL(bvhd_scan_down<T>, dim3(parts), dim3(kThreads), 0, c->stream, in, count, (const T*)sums, out);
    BVHD_LAUNCH(c);
    return RT_OK;
}

template <class T>
int read_back(Ctx* c, T* host, const T* dev, size_t count) {
    RT_HIP(c, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int build(Ctx* c, const float* verts, const float* albedo, const float* emission, uint32_t n, DeviceMesh* out, DevPtr<char>& scratch, Event (&ev)[2]) {
    const size_t m = std::max<uint32_t>(n - 1u, 1u);
    Bump sizing;
    Scratch s{};
    carve(sizing, s, n);
    if (!dalloc(scratch, sizing.used)) return c->fail(RT_ERR_OOM, "device BVH build: %zu bytes of scratch for %u triangles", sizing.used, n);
    Bump bump{scratch.get(), 0};
    carve(bump, s, n);
    for (Event& e : ev) RT_HIP(c, make_event(e));
    const uint32_t red_blocks = std::min<uint32_t>(kReduceBlocks, blocks_for(n));

    // 1. validate and measure: the only step that can refuse the input
    RT_HIP(c, hipEventRecord(ev[0].get(), c->stream));
    hipLaunchKernelGGL(bvhd_validate, dim3(red_blocks), dim3(kThreads), 0, c->stream, verts, n, s.part_max, s.part_bad);
    BVHD_LAUNCH(c);
    std::vector<float> pmax(red_blocks);
    std::vector<uint32_t> pbad(red_blocks);
    if (int rc = read_back(c, pmax.data(), s.part_max, red_blocks)) return rc;
    if (int rc = read_back(c, pbad.data(), s.part_bad, red_blocks)) return rc;
    float maxabs = 0.0f;
    uint32_t bad = 0;
    for (uint32_t b = 0; b < red_blocks; b++) {
        maxabs = std::max(maxabs, pmax[b]);
        bad |= pbad[b];
    }
    if (bad) return c->fail(RT_ERR_INVALID, "vertex data is not finite");
    out->maxabs = std::max(maxabs, 1.0f);
    out->pad = 2e-5f * out->maxabs;  // build_bvh's padding
    const float pad = out->pad;

    // 2.-3. centroid bounds, keys
    hipLaunchKernelGGL(bvhd_bounds, dim3(red_blocks), dim3(kThreads), 0, c->stream, verts, n, pad, s.part_bounds);
    hipLaunchKernelGGL(bvhd_bounds_final, dim3(1), dim3(kThreads), 0, c->stream, (const float*)s.part_bounds, red_blocks, s.bounds);
    hipLaunchKernelGGL(bvhd_keys, dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, verts, n, pad, (const float*)s.bounds, s.keys[0]);
    BVHD_LAUNCH(c);

    // 4. sort: digits that are constant over all keys are skipped
    RT_HIP(c, hipMemsetAsync(s.ghist, 0, 8 * 256 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(bvhd_digit_hist, dim3(red_blocks), dim3(kThreads), 0, c->stream, (const unsigned long long*)s.keys[0], n, s.ghist);
    BVHD_LAUNCH(c);
    std::vector<uint32_t> gh(8 * 256);
    if (int rc = read_back(c, gh.data(), s.ghist, gh.size())) return rc;
    const uint32_t sort_blocks = (n + kSortTile - 1) / kSortTile;
    int cur = 0;
    for (int p = 0; p < 8; p++) {
        if (*std::max_element(gh.begin() + 256 * p, gh.begin() + 256 * (p + 1)) == n) continue;
        const uint32_t shift = 8u * (uint32_t)p;
        hipLaunchKernelGGL(bvhd_sort_hist, dim3(sort_blocks), dim3(kThreads), 0, c->stream, (const unsigned long long*)s.keys[cur], n, shift, s.hist);
        BVHD_LAUNCH(c);
        if (int rc = scan<uint32_t>(c, s.hist, s.hist_off, (size_t)256 * sort_blocks, reinterpret_cast<uint32_t*>(s.sums), reinterpret_cast<uint32_t*>(s.total))) return rc;
        hipLaunchKernelGGL(bvhd_sort_scatter, dim3(sort_blocks), dim3(kThreads), 0, c->stream, (const unsigned long long*)s.keys[cur], s.keys[cur ^ 1], n, shift,
                           (const uint32_t*)s.hist_off);
        BVHD_LAUNCH(c);
        cur ^= 1;
    }
    const unsigned long long* keys = s.keys[cur];

    // 5.-6. binary tree and its boxes
    hipLaunchKernelGGL(bvhd_leaf_boxes, dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, verts, keys, n, pad, s.tree);
    if (n > 1) {
        hipLaunchKernelGGL(bvhd_karras, dim3(blocks_for(n - 1)), dim3(kThreads), 0, c->stream, keys, n, s.child, s.range);
        int j = 31 - __builtin_clz(n - 1);  // level of node n - 1: levels [2^j, 2^(j+1)) hold nodes 1 .. n - 1
        for (; j >= 0 && (1u << j) > kTopLevelNodes; j--) {
            const uint32_t k0 = 1u << j, k1 = std::min<uint32_t>(2u << j, n);
            hipLaunchKernelGGL(bvhd_box_level, dim3(blocks_for(k1 - k0)), dim3(kThreads), 0, c->stream, s.tree, k0, k1);
        }
        if (j >= 0) hipLaunchKernelGGL(bvhd_box_top, dim3(1), dim3(kThreads), 0, c->stream, s.tree, n, j);
        hipLaunchKernelGGL(bvhd_inner_boxes, dim3(blocks_for(n - 1)), dim3(kThreads), 0, c->stream, (const Box*)s.tree, (const uint2*)s.range, n, s.ibox);
    }
    BVHD_LAUNCH(c);

    // 7. collapse, level by level: plan, scan of (inner, leaf) counts in node order, write
    const TreeView tv{s.child, s.ibox, s.tree, n};
    const int32_t root = 0;
    RT_HIP(c, hipMemcpyAsync(s.level[0], &root, sizeof root, hipMemcpyHostToDevice, c->stream));
    uint32_t level_base = 0, level_size = 1, tri_count = 0, depth = 0;
    int lv = 0;
    out->level_start.assign(1, 0u);
    while (level_size) {
        if (++depth > kMaxLevels || (size_t)level_base + level_size > m) return c->fail(RT_ERR_STATE, "device BVH build: the collapse did not converge (internal error)");
        hipLaunchKernelGGL(bvhd_plan, dim3(blocks_for(level_size)), dim3(kThreads), 0, c->stream, tv, (const int32_t*)s.level[lv], level_size, s.plan, s.counts);
        BVHD_LAUNCH(c);
        if (int rc = scan<unsigned long long>(c, s.counts, s.excl, level_size, s.sums, s.total)) return rc;
        hipLaunchKernelGGL(bvhd_write, dim3(blocks_for(level_size)), dim3(kThreads), 0, c->stream, tv, (const Plan*)s.plan, (const unsigned long long*)s.excl,
                           level_size, level_base, tri_count, (uint32_t)m, keys, s.nodes, s.level[lv ^ 1], s.order);
        BVHD_LAUNCH(c);
        unsigned long long tot = 0;
        if (int rc = read_back(c, &tot, s.total, 1)) return rc;
        level_base += level_size;
        out->level_start.push_back(level_base);
        level_size = (uint32_t)(tot >> 32);
        tri_count += (uint32_t)tot;
        lv ^= 1;
    }
    if (tri_count != n) return c->fail(RT_ERR_STATE, "device BVH build: %u of %u triangles placed (internal error)", tri_count, n);
    out->n_nodes = level_base;
    out->depth = depth;
    out->stack_need = depth + 1;  // at most one pending sibling group per level (bvh_build.cpp)

    // 8. the mesh's own arrays
    if (!dalloc(out->nodes, (size_t)out->n_nodes * (kNodeWords / 4)) || !dalloc(out->tris, (size_t)n * (kTriWords / 4)) || !dalloc(out->albedo, n) || !dalloc(out->emission, n))
        return c->fail(RT_ERR_OOM, "mesh of %u triangles", n);
    out->cap_nodes = out->n_nodes;
    float4 *nodes = out->nodes.get(), *tris = out->tris.get(), *alb = out->albedo.get(), *emi = out->emission.get();
    RT_HIP(c, hipMemcpyAsync(nodes, s.nodes, (size_t)out->n_nodes * kNodeWords * 4, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(bvhd_payload, dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, verts, albedo, emission, (const uint32_t*)s.order, n, tris, alb, emi,
                       s.leaf_pos, s.flag);
    BVHD_LAUNCH(c);
    if (int rc = scan<uint32_t>(c, s.flag, s.flag_excl, n, reinterpret_cast<uint32_t*>(s.sums), reinterpret_cast<uint32_t*>(s.total))) return rc;
    uint32_t n_lights = 0;
    if (int rc = read_back(c, &n_lights, reinterpret_cast<const uint32_t*>(s.total), 1)) return rc;
    if (!dalloc(out->lights, std::max<uint32_t>(n_lights, 1u))) return c->fail(RT_ERR_OOM, "light list of %u triangles", n_lights);
    hipLaunchKernelGGL(bvhd_lights, dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, (const uint32_t*)s.flag, (const uint32_t*)s.flag_excl,
                       (const uint32_t*)s.leaf_pos, n, n_lights, out->lights.get());
    BVHD_LAUNCH(c);
    RT_HIP(c, hipEventRecord(ev[1].get(), c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    RT_HIP(c, hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()));
    out->build_ms = ms;
    out->n_tris = n;
    out->n_lights = n_lights;
    return RT_OK;
}

size_t refit_scratch_bytes(uint32_t n_nodes) {
    Bump b;
    b.take<float>(kReduceBlocks);
    b.take<uint32_t>(kReduceBlocks);
    b.take<Box>(n_nodes);
    return b.used;
}

}  // namespace

size_t refit_scratch_size(uint32_t n_nodes) { return refit_scratch_bytes(n_nodes); }

// the build's own three-launch scan for callers outside this unit (the hit queries' offsets, rt_abi_query.hip)
size_t scan_u64_sums_words(size_t count) { return (count + kScanTile - 1) / kScanTile + 1; }
int scan_u64_device(Ctx* c, const unsigned long long* in, unsigned long long* out, size_t count, unsigned long long* sums, unsigned long long* total) {
    return scan<unsigned long long>(c, in, out, count, sums, total);
}

int refit_measure(Ctx* c, const float* verts, uint32_t n, void* scratch, hipEvent_t begin, float* maxabs) {
    Bump bump{static_cast<char*>(scratch), 0};
    float* part_max = bump.take<float>(kReduceBlocks);
    uint32_t* part_bad = bump.take<uint32_t>(kReduceBlocks);
    const uint32_t red_blocks = std::min<uint32_t>(kReduceBlocks, blocks_for(n));
    RT_HIP(c, hipEventRecord(begin, c->stream));
    hipLaunchKernelGGL(bvhd_validate, dim3(red_blocks), dim3(kThreads), 0, c->stream, verts, n, part_max, part_bad);
    BVHD_LAUNCH(c);
    // ONE read-back: the two partial arrays are adjacent in the scratch (part_bad starts 4 * kReduceBlocks bytes after part_max)
    static_assert((kReduceBlocks * sizeof(float)) % 256 == 0, "part_bad must follow part_max directly");
    std::vector<uint32_t> part(2 * kReduceBlocks);
    if (int rc = read_back(c, part.data(), reinterpret_cast<const uint32_t*>(part_max), part.size())) return rc;
    float m = 0.0f;
    uint32_t bad = 0;
    for (uint32_t b = 0; b < red_blocks; b++) {
        float x;
        std::memcpy(&x, &part[b], 4);
        m = std::max(m, x);
        bad |= part[kReduceBlocks + b];
    }
    if (bad) return c->fail(RT_ERR_INVALID, "vertex data is not finite");
    *maxabs = m;
    return RT_OK;
}

int refit_write(Ctx* c, const float* verts, uint32_t n, float pad, uint32_t n_nodes, float4* nodes, float4* tris, const std::vector<uint32_t>& level_start,
                void* scratch, hipEvent_t begin, hipEvent_t end, float* ms) {
    const uint32_t levels = (uint32_t)level_start.size() - 1u;
    if (level_start.size() < 2 || level_start.front() != 0 || level_start.back() != n_nodes)
        return c->fail(RT_ERR_STATE, "refit: the mesh's level ranges do not describe its %u nodes (internal error)", n_nodes);
    Bump bump{static_cast<char*>(scratch), 0};
    (void)bump.take<float>(kReduceBlocks);
    (void)bump.take<uint32_t>(kReduceBlocks);
    Box* box = bump.take<Box>(n_nodes);
    uint32_t* words = reinterpret_cast<uint32_t*>(nodes);
    hipLaunchKernelGGL(bvhr_tris, dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, verts, n, tris);
    RefitTop top{};
    while (top.levels < levels && top.levels < kRefitTopMax && level_start[top.levels + 1] - level_start[top.levels] <= kRefitTopNodes) top.levels++;
    for (uint32_t j = 0; j <= top.levels; j++) top.start[j] = level_start[j];
    for (uint32_t j = levels; j-- > top.levels;) {
        const uint32_t k0 = level_start[j], k1 = level_start[j + 1];
        hipLaunchKernelGGL(bvhr_level, dim3(blocks_for(k1 - k0)), dim3(kThreads), 0, c->stream, words, (const float4*)tris, n, n_nodes, pad, box, k0, k1);
    }
    if (top.levels) hipLaunchKernelGGL(bvhr_top, dim3(1), dim3(kRefitTopThreads), 0, c->stream, words, (const float4*)tris, n, n_nodes, pad, box, top);
    BVHD_LAUNCH(c);
    RT_HIP(c, hipEventRecord(end, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    RT_HIP(c, hipEventElapsedTime(ms, begin, end));
    return RT_OK;
}

int build_bvh_device(Ctx* c, const float* verts, const float* albedo, const float* emission, uint32_t n, DeviceMesh* out) {
    DevPtr<char> scratch;  // freed here; the mesh's own arrays go to *out
    Event ev[2];
    const int rc = build(c, verts, albedo, emission, n, out, scratch, ev);
    if (rc != RT_OK) {
        (void)hipStreamSynchronize(c->stream);  // nothing enqueued may still use the scratch or the arrays when they are freed
        *out = DeviceMesh{};
    }
    return rc;
}

}  // namespace rt
