// pt_queue.h — path B, device side: a device-resident queue of PT_HEADS interleaved streams (rt_internal.h) as a persistent wave
// sees it: where a stream's entries lie, which stream a wave starts on, the cursor that reserves entries with one atomic per refill
// and moves on when a stream is dry.  Used by the per-lane trace kernels and the ray queries (pt_trace.hip), by the shared query loop
// (pt_query_loop.h: six of the eight query kinds), the closest-point and the all-hits queries (pt_point_query.hip, pt_hit_query.hip); pt_overlap_segments.hip uses add_wave_total.  The queries' queue is implicit.  The atomics here are aggregated by hand: see the Makefile for the flag that keeps them as written.
#pragma once
#include "pt_traverse.h"

namespace rt {
using namespace rtk;

// Stream-local entry j of stream k is queue entry ((j / 64) * PT_HEADS + k) * 64 + j % 64 (rt_internal.h).
__device__ __forceinline__ uint32_t stream_entry(uint32_t stream, uint32_t j) { return (((j >> 6) * PT_HEADS + stream) << 6) | (j & 63u); }

// The stream a wave starts to pull from.
// (readfirstlane: threadIdx.x >> 6 is wave-uniform, but only this tells the compiler, and everything the stream index touches -
// the dry-stream test, `exhausted`, the refill branch - would otherwise live in vector registers under lane masks)
__device__ __forceinline__ uint32_t home_stream() { return uniform((blockIdx.x * 4u + (threadIdx.x >> 6)) & (PT_HEADS - 1u)); }

// Where a wave stands in a queue (all wave-uniform): it pulls from one stream until it finds it dry, then from the next one.
struct QueueCursor {
    uint32_t n;     // entries in the queue
    uint32_t* head;  // the queue's PT_HEADS stream heads
    uint32_t stream, dry_streams;
    __device__ __forceinline__ uint32_t* head_word() const { return head + stream * PT_HEAD_STRIDE; }
    // One returning atomic on the wave's stream head reserves `want` stream-local entries; the first one is returned to every lane.
    __device__ __forceinline__ uint32_t reserve(uint32_t want, uint32_t lane) const {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(head_word(), want);
        return uniform(base);
    }
    // je = the end of a reservation.  Past the queue's end the stream is dry (entries grow with j) and the wave moves on; returns
    // true when that was the last stream, i.e. the queue is dry.
    __device__ __forceinline__ bool advance_if_dry(uint32_t je) {
        if (stream_entry(stream, je) < n) return false;
        stream = (stream + 1u) & (PT_HEADS - 1u);
        return ++dry_streams >= PT_HEADS;
    }
};

// rt_pt_params.tune_refill_min, byte 1: triangle tests per round of the inline schedules
__device__ __forceinline__ int tris_per_round_of(uint32_t refill_min) { return (int)((refill_min >> 8) & 0xffu) ? (int)((refill_min >> 8) & 0xffu) : kTrisPerRound; }

__device__ __forceinline__ void add_wave_total(unsigned long long* word, uint32_t v, uint32_t lane) {  // one atomic per wave
    unsigned long long a = v;
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (lane == 0) atomicAdd(word, a);
}

}  // namespace rt
