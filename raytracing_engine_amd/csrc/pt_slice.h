// pt_slice.h — path B, device side: what the kernels of the listing queries share beside their loop and their walk - the sorted
// slice that a lane keeps in global memory (insert_hit), where that slice lies (open_slice), the lane's slice record with the
// sink's accounting (ListSlice), the count step's answer (write_count) and the wave totals (add_listing_totals).  Used by the
// all-hits ray queries (pt_hit_query.hip: keys are t; its kernel keeps the record's fields and the sink's arithmetic as its own
// text), by the neighbour queries (pt_neighbor_query.hip: keys are d2) and by the overlap queries (pt_overlap_query.hip: (index,
// mask) pairs with insert_pair); the k-nearest queries (pt_knn_query.hip) use insert_hit on their rows.
#pragma once
#include "pt_queue.h"

namespace rt {

// Hit (t, id) into the slice ts / ids, which holds the min(found, room) smallest hits met so far in ascending (t, id) order: larger
// entries move up by one; with the slice full its last entry falls off (or the new hit, if it is no smaller).  A lane reads back
// only what it stored itself, so program order is all the ordering this needs.  Writes only elements below room.
__device__ __forceinline__ void insert_hit(float* ts, int* ids, uint32_t room, uint32_t found, float t, int id) {
    uint32_t j = found < room ? found : room;  // entries held
    if (j == room) {
        if (room == 0u) return;
        const float tl = ts[room - 1u];
        if (!(t < tl || (t == tl && id < ids[room - 1u]))) return;
        j = room - 1u;
    }
    while (j > 0u) {
        const float tp = ts[j - 1u];
        const int ip = ids[j - 1u];
        if (!(tp > t || (tp == t && ip > id))) break;
        ts[j] = tp;
        ids[j] = ip;
        j--;
    }
    ts[j] = t;
    ids[j] = id;
}

// The fill step: the slice of item i as the offsets give it - where it starts, its own length (saturated at 2^32 - 1), and the
// entries it may hold: written only if 0 <= lo <= hi <= capacity, and then only below hi - lo (room 0: it does not fit, nothing is
// written).  Returned by value: the same function filling three references changed the kernels' code (profiles/refactor_listing.txt).
struct Slice {
    long long lo;
    uint32_t len, room;
};
__device__ __forceinline__ Slice open_slice(const long long* offsets, uint32_t i, long long capacity) {
    const long long lo = offsets[i], hi = offsets[(size_t)i + 1u];
    const long long span = hi > lo ? hi - lo : 0ll;
    const uint32_t len = span < 0xffffffffll ? (uint32_t)span : 0xffffffffu;
    return Slice{lo, len, (lo >= 0ll && hi <= capacity) ? len : 0u};
}

// The count step: the answer of an item whose count is known - the caller's 32-bit column and the scan's 64-bit one (max(count, 0));
// either may be absent
__device__ __forceinline__ void write_count(int* count_out, unsigned long long* count64, uint32_t i, int count, unsigned long long scanned) {
    if (count_out) count_out[i] = count;
    if (count64) count64[i] = scanned;
}

// What a listing lane holds of its list beside the walk: the slice of the item under way and the lane's totals.
struct ListSlice {
    long long lo = 0;    // FILL: where the slice starts
    uint32_t room = 0;   // FILL: entries it may hold (0: it does not fit, nothing is written)
    uint32_t len = 0;    // FILL: its own length
    uint32_t found = 0;  // the item's entries so far
    uint32_t invalid = 0, total = 0, written = 0, incomplete = 0, beyond = 0;  // what this lane has met
    // on admission, FILL: open_slice's answer
    __device__ __forceinline__ void open(const long long* offsets, uint32_t i, long long capacity) {
        const Slice s = open_slice(offsets, i, capacity);
        lo = s.lo, len = s.len, room = s.room;
    }
    // The sink: the item's entries into the totals; returns how many of them the slice holds.
    template <bool FILL>
    __device__ __forceinline__ uint32_t close() {
        const uint32_t kept = found < room ? found : room;
        total += found;
        if (FILL) {
            written += kept;
            incomplete += (found != 0u && room != len) ? 1u : 0u;
            beyond += found > len ? found - len : 0u;
        }
        return kept;
    }
};

// A wave's totals into the step's LQ_STEP_WORDS counters, one atomic per word
template <bool COUNT, bool FILL>
__device__ __forceinline__ void add_listing_totals(unsigned long long* stats, uint32_t lane, uint32_t invalid, uint32_t found, uint32_t written, uint32_t incomplete,
                                                   uint32_t beyond, const TravCounters& tc) {
    add_wave_total(&stats[LQ_STAT_INVALID], invalid, lane);
    add_wave_total(&stats[LQ_STAT_FOUND], found, lane);
    if (FILL) {
        add_wave_total(&stats[LQ_STAT_WRITTEN], written, lane);
        add_wave_total(&stats[LQ_STAT_INCOMPLETE], incomplete, lane);
        add_wave_total(&stats[LQ_STAT_SLICE_OVERFLOW], beyond, lane);
    }
    if (COUNT) {
        add_wave_total(&stats[LQ_STAT_NODES], tc.nodes, lane);
        add_wave_total(&stats[LQ_STAT_TRIS], tc.tris, lane);
    }
    if (tc.overflow) atomicOr((unsigned int*)&stats[LQ_STAT_OVERFLOW], 1u);
}
template <bool COUNT, bool FILL>
__device__ __forceinline__ void add_listing_totals(unsigned long long* stats, uint32_t lane, const ListSlice& sl, const TravCounters& tc) {
    add_listing_totals<COUNT, FILL>(stats, lane, sl.invalid, sl.total, sl.written, sl.incomplete, sl.beyond, tc);
}

// The overlap queries' slice (pt_overlap_query.hip): pairs (id, word) in ascending id order, ids distinct.  insert_hit's protocol
// with the id as the only key: the slice holds the min(found, room) smallest ids met so far, larger entries move up by one, with
// the slice full its last entry falls off (or the new pair, if its id is no smaller).  Writes only elements below room.
__device__ __forceinline__ void insert_pair(int* ids, int* words, uint32_t room, uint32_t found, int id, int word) {
    uint32_t j = found < room ? found : room;  // entries held
    if (j == room) {
        if (room == 0u) return;
        if (!(id < ids[room - 1u])) return;
        j = room - 1u;
    }
    while (j > 0u) {
        const int ip = ids[j - 1u];
        if (!(ip > id)) break;
        ids[j] = ip;
        words[j] = words[j - 1u];
        j--;
    }
    ids[j] = id;
    words[j] = word;
}

}  // namespace rt
