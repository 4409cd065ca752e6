// pt_query_loop.h — path B, device side: what the persistent query kernels share: the refilling loop
// over pt_queue.h's streams (RT_QUERY_LOOP), and the two walks that a kind puts inside it - the nearest-first walk (clearance,
// k-nearest, sphere casts) and the group walk (sides, neighbours, overlaps; the ray queries' round is pt_traverse.h's inline_round).
// Used by pt_query_rays (pt_trace.hip) and by pt_side_query.hip, pt_neighbor_query.hip, pt_overlap_query.hip,
// pt_clearance_query.hip, pt_knn_query.hip and pt_sweep_query.hip.  pt_query_points and pt_query_hits keep their own text of the loop and of their
// walks: as lanes they were slower (profiles/refactor_query_loop.txt).  The render loops of pt_trace.hip (two queues, a
// software-pipelined head) are their own.
#pragma once
#include "point_tri.h"
#include "pt_queue.h"

namespace rt {
using namespace rtk;

// ---- the loop ---------------------------------------------------------------------------------------------------------------------
// A persistent wave answers the items 0 .. n - 1 of an implicit queue (entry i is item i of the caller's arrays) that is cut into
// PT_HEADS streams.  A kind supplies a lane object:
//   void retire()           the sink: called for an idle lane that still holds an item; writes that item's answer
//   bool admit(uint32_t i)  the source: loads item i, writes the answer of an item that needs no walk (invalid, empty interval) and
//                           returns whether the lane now walks.  A refill may therefore hand out 64 entries and leave no lane alive
//   bool step(bool alive)   one round of the kind's walk; returns whether the lane still has work (by value: see inline_round)
// The sink stands before the source: what a lane holds when retire() runs is the retiring item's.
// A refill happens when every lane is idle, or when at least refill_min are and the queue is not dry: one returning atomic reserves
// exactly what the idle lanes need, assigned by ballot + prefix popcount.  With few workgroups a stream may have no wave that started
// on it, so a wave leaves only when it has found the last stream dry AND holds no live lane.  That test sits inside the refill block:
// `idle == ~0` is the only way there once the queue is dry, and the idle lanes have retired just above it, so every answer of the
// wave is written when it breaks.
// A kernel body is four things: make the stack, construct the lane, RT_QUERY_LOOP(lane, q.n, head, refill_min, lane_id), add the wave
// totals.  The loop is a macro and not a function template: as a __forceinline__ function the same text spilled vector registers in
// pt_query_sides (profiles/refactor_query_loop.txt).  `lane` is an lvalue; the other arguments are evaluated once.
#define RT_QUERY_LOOP(lane, n_items, head_words, refill_min_lanes, lane_id)                                                                   \
    do {                                                                                                                                        \
        bool has_item_ = false, alive_ = false;                                                                                                 \
        QueueCursor qc_{(n_items), (head_words), home_stream(), 0u};                                                                            \
        const uint32_t refill_min_ = (refill_min_lanes), lane_id_ = (lane_id);                                                                  \
        bool exhausted_ = qc_.n == 0u; /* every stream has been found dry */                                                                    \
        for (;;) {                                                                                                                              \
            const unsigned long long idle_ = __ballot(!alive_);                                                                                 \
            if (idle_ == ~0ull || (!exhausted_ && (uint32_t)__popcll(idle_) >= refill_min_)) {                                                  \
                if (!alive_ && has_item_) {                                                                                                     \
                    (lane).retire();                                                                                                            \
                    has_item_ = false;                                                                                                          \
                }                                                                                                                               \
                if (!exhausted_) {                                                                                                              \
                    const uint32_t want_ = (uint32_t)__popcll(idle_);                                                                           \
                    const uint32_t base_ = qc_.reserve(want_, lane_id_);                                                                        \
                    /* the idle lanes below this one, counted by v_mbcnt: a lane mask held through the walk is two registers */                 \
                    const uint32_t rank_ = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_, 0u));   \
                    const uint32_t i_ = !alive_ ? stream_entry(qc_.stream, base_ + rank_) : qc_.n; /* >= n: nothing for this lane */            \
                    if (!alive_ && i_ < qc_.n) has_item_ = alive_ = (lane).admit(i_);                                                           \
                    exhausted_ = qc_.advance_if_dry(base_ + want_);                                                                             \
                }                                                                                                                               \
                if (__ballot(alive_) == 0ull && exhausted_) break;                                                                              \
            }                                                                                                                                   \
            alive_ = (lane).step(alive_);                                                                                                       \
        }                                                                                                                                       \
    } while (0)

// ---- the nearest-first walk -----------------------------------------------------------------------------------------------------------
// A lane holds the node it visits next (kNoNode: pop one) and a bound on d2 that shrinks as the walk goes.  Stack entries are
// (node index, lb2 bits) in TravStack's 8-byte slots: one pending sibling each, so an entry whose bound the walk has passed
// meanwhile is dropped without fetching its node.  Worst case 7 entries per level below the root (point_stack_need, rt_internal.h).
constexpr uint32_t kNoNode = 0xffffffffu;

struct Nearest {
    float d2;
    uint32_t id;  // original triangle index (tie-break)
    int li;       // leaf-order triangle index, -1 = none
};

// The eight lower bounds of node nd's child boxes against p (child_lb2 of point_tri.h on the decoded record).  They stay in
// registers: every loop that indexes them is unrolled.
__device__ __forceinline__ void point_child_lb2(const NodeRec& nd, P3 p, float (&lb)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float gx = axis_gap(p.x, nd.ox, nd.sx, plane_q(nd.lx, i), plane_q(nd.hx, i));
        const float gy = axis_gap(p.y, nd.oy, nd.sy, plane_q(nd.ly, i), plane_q(nd.hy, i));
        const float gz = axis_gap(p.z, nd.oz, nd.sz, plane_q(nd.lz, i), plane_q(nd.hz, i));
        lb[i] = gap_lb2(gx, gy, gz);
    }
}

// bit s: lb[s] is not beyond the bound (strictly, and written so that a NaN is entered; empty slots: the callers mask them)
__device__ __forceinline__ uint32_t within_bound(const float (&lb)[8], float bound) {
    uint32_t pass = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) pass |= !(lb[i] > bound) ? 1u << i : 0u;
    return pass;
}

// The nearest pending sibling that the bound has not passed; kNoNode: the stack is empty, the walk is over.
__device__ __forceinline__ uint32_t pop_within(TravStack& stk, float bound) {
#pragma unroll 1
    while (stk.sp) {
        const Group e = stk.pop();
        if (!(__uint_as_float(e.y) > bound)) return e.x;
    }
    return kNoNode;
}

// Of node nd's inner children that the bound has not passed, the nearest is returned (lmin: its lb2; kNoNode: there is none) and
// the others are pushed as (node, lb2).
__device__ __forceinline__ uint32_t descend_nearest(const NodeRec& nd, const float (&lb)[8], float bound, float& lmin, TravStack& stk, uint32_t& overflow) {
    uint32_t go = 0, smin = 0;  // inner children still to be entered, the nearest of them
    lmin = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((nd.imask >> i) & 1u) && !(lb[i] > bound)) {
            if (go == 0u || lb[i] < lmin) {
                lmin = lb[i];
                smin = (uint32_t)i;
            }
            go |= 1u << i;
        }
    }
    if (go == 0u) return kNoNode;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (((go >> i) & 1u) && (uint32_t)i != smin) stk.push(Group{nd.child((uint32_t)i), __float_as_uint(lb[i])}, overflow);
    }
    return nd.child(smin);
}

// ---- the group walk -------------------------------------------------------------------------------------------------------------------
// The walks whose test does not change as they go (a ray that never learns anything, a fixed radius, a fixed box) enter every child
// that passes, in any order: the passing inner children of a node are ONE group (child base + mask, pt_traverse.h's Group) and
// node_step's protocol holds - a node visit takes one child out of the current group and pushes what is left of it, so the stack
// holds at most one group per level below the root.
// Take the highest pending inner child out of node group G, push the remaining siblings; returns the child's node index.
__device__ __forceinline__ uint32_t take_child(Group& G, TravStack& stk, uint32_t& overflow) {
    const uint32_t pend = G.y;
    const uint32_t bit = 31u - (uint32_t)__builtin_clz(pend);
    G.y &= ~(1u << bit);
    if (has_nodes(G)) stk.push(G, overflow);
    return G.x + (uint32_t)__builtin_popcount(pend & ~(0xffffffffu << (bit - 24u)));  // low byte of pend = imask
}
// The verdicts on node nd's eight slots become the new node group and the triangle group (empty slots: masked here).
__device__ __forceinline__ void enter_node(const NodeRec& nd, uint32_t pass, Group& G, Group& T) {
    G = Group{nd.child_base, ((pass & nd.imask) << 24) | nd.imask};
    T = Group{nd.tri_base, (pass & nd.leafmask) | (nd.leafmask << 8)};
}
// Take the lowest pending leaf slot out of triangle group T (the caller checked has_tris); returns the triangle's leaf-order index.
__device__ __forceinline__ uint32_t take_tri(Group& T) {
    const uint32_t bit = (uint32_t)__builtin_ctz(T.y);
    T.y &= T.y - 1u;
    return T.x + (uint32_t)__builtin_popcount((T.y >> 8) & ~(0xffffffffu << bit));
}

// One round: the node phase - a lane without pending triangles visits its next node and pops a group when none is pending; with an
// empty stack the walk is over and walk_over() says whether the lane goes on (the sides start their next walk there) - then the
// triangle phase: one test.  alive goes in and out by value, as in inline_round.
template <class NodeStep, class TriStep, class WalkOver>
__device__ __forceinline__ bool group_round(Group& G, Group& T, TravStack& stk, bool alive, NodeStep node_step, TriStep tri_step, WalkOver walk_over) {
    if (alive && !has_tris(T)) {
        if (!has_nodes(G)) {
            if (stk.sp) G = stk.pop();
            else alive = walk_over();
        }
        if (alive) node_step();
    }
    if (alive && has_tris(T)) tri_step();
    return alive;
}

}  // namespace rt
