// pt_overlap_segments.hip — path B: where each listed triangle pair intersects (rt_overlap_segments_device).
// Two flat kernels, no tree walk, no LDS stack, no queue heads: pt_scatter_tri_inverse writes the map from a triangle's original index
// to its leaf position, pt_overlap_segments runs one lane per entry of an overlap list (the CSR that rt_list_overlaps_device wrote),
// gathers the entry's query triangle and mesh record and computes the segment with tri_section.h, the arithmetic the tests' CPU
// reference shares.
#include <algorithm>

#include "pt_launch.h"
#include "tri_section.h"

namespace rt {

// the sum of v over the wave, in lane 0 (add_wave_total's reduction, pt_queue.h)
__device__ __forceinline__ unsigned long long wave_total(uint32_t v) {
    unsigned long long a = v;
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    return a;
}

// inv[original index] = leaf position, from the records themselves (word 9 of a record is the original index): every mesh kind keeps
// that word, so there is nothing to invalidate when a mesh is set, built on the device, refitted, updated by chunk or shared.
__global__ __launch_bounds__(256) void pt_scatter_tri_inverse(const float4* __restrict__ tris, uint32_t n_tris, uint32_t* __restrict__ inv) {
    for (uint32_t li = blockIdx.x * 256u + threadIdx.x; li < n_tris; li += gridDim.x * 256u) {
        const uint32_t t = __float_as_uint(tris[(size_t)li * 3 + 2].y);
        if (t < n_tris) inv[t] = li;  // (always, on a record the library wrote; inv holds n_tris words)
    }
}

// One lane per entry k < K = min(offsets[n], capacity), 64 consecutive entries per wave and round.  Per entry: the owner i by binary
// search (it halves [lo, hi) whatever the offsets hold: at most 32 steps), checked against k; a slice that ends beyond the capacity
// was never written and is left alone; T = tri[k], the nine coordinates, inv[T], the record - each read only behind its bound
// check - then tri_section.h.  An entry without an owner, with T outside the mesh, with an invalid query triangle or with no bit set
// gets the NaN segment.  The 24-byte rows go through 1.5 KiB of the wave's own LDS, so that each of the six stores of a round
// writes 256 contiguous bytes instead of four bytes in every 24.
__global__ __launch_bounds__(256) void pt_overlap_segments(const PtScene sc, const SegmentQuery q, const uint32_t* __restrict__ inv,
                                                           unsigned long long* __restrict__ stats) {
    __shared__ float stage[4][64 * 6];
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* st = stage[wave];
    const long long total = q.offsets[q.n];
    const long long K = total < 0 ? 0 : total < q.capacity ? total : q.capacity;
    const long long stride = (long long)gridDim.x * 256;
    uint32_t touches = 0, skipped = 0, bad = 0;  // what this lane has met

    for (long long base = (long long)blockIdx.x * 256 + wave * 64u; base < K; base += stride) {  // (wave-uniform)
        const long long k = base + lane;
        Section s = section_none();
        bool write = false;
        if (k < K) {
            uint32_t lo = 0u, hi = q.n;  // the last i in [0, n) with offsets[i] <= k, where the offsets ascend
            while (hi - lo > 1u) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (q.offsets[mid] <= k) lo = mid;
                else hi = mid;
            }
            const long long a = q.offsets[lo], b = q.offsets[lo + 1u];
            const bool owned = a <= k && k < b;
            if (owned && b > q.capacity) {
                skipped++;
            } else {
                write = true;
                const int T = q.tri[k];
                bool ok = owned && T >= 0 && (uint32_t)T < sc.n_tris;
                QueryTri A{P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}, P3{0.0f, 0.0f, 0.0f}};
                if (ok) {
                    const float* tp = q.tris + (size_t)lo * 9u;
                    A = QueryTri{P3{tp[0], tp[1], tp[2]}, P3{tp[3], tp[4], tp[5]}, P3{tp[6], tp[7], tp[8]}};
                    ok = tri_in_reach(A, q.reach);
                }
                uint32_t li = 0u;
                if (ok) {
                    li = inv[T];
                    ok = li < sc.n_tris;
                }
                if (ok) {
                    const float4* rp = sc.tris + (size_t)li * 3;
                    const float4 ra = rp[0], rb = rp[1], rc = rp[2];
                    if (__float_as_uint(rc.y) == (uint32_t)T)  // (the map is the records' own)
                        s = overlap_section(A, query_box(A), P3{ra.x, ra.y, ra.z}, P3{ra.w, rb.x, rb.y}, P3{rb.z, rb.w, rc.x});
                }
                if (s.ends < 0) bad++;
                else if ((s.ends & 7) == (s.ends >> 3)) touches++;
            }
        }
        // rows to columns: lane l's six words lie at 6 l .. 6 l + 5, store j of the round writes words 64 j .. 64 j + 63
        st[lane * 6u + 0u] = s.p0.x, st[lane * 6u + 1u] = s.p0.y, st[lane * 6u + 2u] = s.p0.z;
        st[lane * 6u + 3u] = s.p1.x, st[lane * 6u + 4u] = s.p1.y, st[lane * 6u + 5u] = s.p1.z;
        const unsigned long long wmask = __ballot(write);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        float* row = q.seg_out + base * 6;
#pragma unroll
        for (uint32_t j = 0; j < 6u; j++) {
            const uint32_t w = j * 64u + lane;
            if ((wmask >> (w / 6u)) & 1ull) row[w] = st[w];  // a word of an entry that is written: below K x 6
        }
        if (write && q.ends_out) q.ends_out[k] = s.ends;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();  // the next round's rows wait for this round's reads
    }
    // The counters: a wave total each (add_wave_total's reduction), then one atomic per workgroup and counter, and none for a total of 0 -
    // on a list the library wrote only `touches` is ever met.  A hot word answers some 90 atomics a microsecond (rt_internal.h), and a
    // grid of 2 048 workgroups adding five words per wave would wait 0.45 ms for them, as long as the rest of the call.
    __shared__ unsigned long long totals[4][3];
    const unsigned long long t0 = wave_total(touches), t1 = wave_total(skipped), t2 = wave_total(bad);
    if (lane == 0u) totals[wave][0] = t0, totals[wave][1] = t1, totals[wave][2] = t2;
    __syncthreads();  // (every thread arrives: the loop above has no early exit)
    if (threadIdx.x < 3u) {
        const unsigned long long sum = totals[0][threadIdx.x] + totals[1][threadIdx.x] + totals[2][threadIdx.x] + totals[3][threadIdx.x];
        if (sum) atomicAdd(&stats[SG_STAT_TOUCHES + threadIdx.x], sum);
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) stats[SG_STAT_ENTRIES] = (unsigned long long)K;  // entries visited; segments = the rest (the host subtracts)
}

// ---- launchers ------------------------------------------------------------------------------------
int launch_pt_tri_inverse(Ctx* c, const PtScene& sc, uint32_t* inv) {
    const uint32_t grid = std::max(1u, std::min((sc.n_tris + 255u) / 256u, (uint32_t)c->n_cus * 8u));
    hipLaunchKernelGGL(pt_scatter_tri_inverse, dim3(grid), dim3(256), 0, c->stream, sc.tris, sc.n_tris, inv);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

// the grid is sized from the capacity: the host never learns offsets[n]
int launch_pt_overlap_segments(Ctx* c, const PtScene& sc, const SegmentQuery& q, const uint32_t* inv, unsigned long long* stats) {
    const unsigned long long blocks = ((unsigned long long)q.capacity + 255ull) / 256ull;
    const uint32_t grid = (uint32_t)std::max(1ull, std::min(blocks, (unsigned long long)c->n_cus * 8ull));
    hipLaunchKernelGGL(pt_overlap_segments, dim3(grid), dim3(256), 0, c->stream, sc, q, inv, stats);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

}  // namespace rt
