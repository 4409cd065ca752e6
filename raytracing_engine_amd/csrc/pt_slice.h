// pt_slice.h — path B, device side: the sorted slice that a lane of a listing query keeps in global memory.  Used by the all-hits ray
// queries (pt_hit_query.hip: keys are t) and by the neighbour queries (pt_neighbor_query.hip: keys are d2).
#pragma once
#include <cstdint>

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

}  // namespace rt
