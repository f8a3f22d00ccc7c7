// omg_segment_body.h — what the kernels of omg_segment.hip do for one node: the foreground test, the backward neighbours of a
// node, find and union on a table of parent links, and the rule of a cropped output node, as functions that also compile for
// the host, so that the phases can be stepped through run by run and compared with omg-planner_amd/segmentation.py without a
// GPU.  Integers only.  The only HIP built-ins are the two accesses of the link table below; on the host they are plain.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SEG_HD __host__ __device__ __forceinline__
#else
#define SEG_HD inline
#endif

#define SEG_FREE 0
#define SEG_SURFACE 1
#define SEG_UNKNOWN 2
#define SEG_BACKGROUND (-1)
// Where a link table lives: the LDS of one workgroup, or global memory that workgroups on other XCDs change in the same launch.
// SEG_SCOPE_PLAIN: a table that nobody changes during the launch, read with plain loads.
#define SEG_SCOPE_WORKGROUP 0
#define SEG_SCOPE_AGENT 1
#define SEG_SCOPE_PLAIN 2

// The two accesses of a link table while other threads change it: a relaxed atomic load and a relaxed atomic minimum that
// returns what the cell held.  Agent scope keeps the load out of the caches that another XCD's atomic does not reach.
template <int SCOPE>
SEG_HD int32_t seg_load(const int32_t* cell) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (SCOPE == SEG_SCOPE_PLAIN) return *cell;
    return SCOPE == SEG_SCOPE_AGENT ? __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    return *cell;
#endif
}
template <int SCOPE>
SEG_HD int32_t seg_fetch_min(int32_t* cell, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return SCOPE == SEG_SCOPE_AGENT ? __hip_atomic_fetch_min(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : __hip_atomic_fetch_min(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    const int32_t old = *cell;
    if (v < old) *cell = v;
    return old;
#endif
}

// select bit 0: SURFACE nodes; bit 1: nodes that are neither FREE nor SURFACE.
SEG_HD bool seg_foreground(uint8_t state, int select) {
    return state == SEG_SURFACE ? (select & 1) != 0 : state != SEG_FREE && (select & 2) != 0;
}

// 6 / 18 / 26 -> the most axes a neighbour's offset may move along.
SEG_HD int seg_order(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }

// The backward neighbours of a node: the 13 offsets (di, dj, dk) before (0, 0, 0) in x-major order, n = 0 .. 12:
// di = -1 with dj, dk in -1 .. 1 (n = 0 .. 8), then (0, -1, dk) (n = 9 .. 11), then (0, 0, -1).
#define SEG_BACKWARD 13
SEG_HD void seg_offset(int n, int* d) {
    if (n < 9) d[0] = -1, d[1] = n / 3 - 1, d[2] = n % 3 - 1;
    else if (n < 12) d[0] = 0, d[1] = -1, d[2] = n - 10;
    else d[0] = 0, d[1] = 0, d[2] = -1;
}
// Is backward neighbour n of node (i, j, k) a neighbour under `order` and inside the grid?  *Lq: its linear index, always
// smaller than the node's own.
SEG_HD bool seg_neighbour(int n, int order, const int32_t* dims, int i, int j, int k, int64_t* Lq) {
    int d[3];
    seg_offset(n, d);
    if ((d[0] != 0) + (d[1] != 0) + (d[2] != 0) > order) return false;
    const int qi = i + d[0], qj = j + d[1], qk = k + d[2];
    if (qi < 0 || qj < 0 || qj >= dims[1] || qk < 0 || qk >= dims[2]) return false;
    *Lq = ((int64_t)qi * dims[1] + qj) * dims[2] + qk;
    return true;
}

// The links of the foreground nodes of one run or one volume: parent[x] <= x is a node of x's tree, a root has
// parent[x] == x, the root of a tree is its smallest node.
//
// Termination, whatever other threads do to the table meanwhile.  A cell only ever changes through seg_fetch_min with a value
// smaller than its own index (the initial parent[x] = x aside), so a link points to a smaller index and never grows.
//   find:  every turn replaces x by parent[x] < x: an integer >= 0 that strictly decreases.
//   union: a turn ends the loop or goes on with (old, b), where old < a and b < a for the a of this turn: max(a, b) strictly
//          decreases.
// So both end after at most x (max(a, b)) turns; nothing here waits for another thread.  A stale read gives a link the cell
// held earlier: an older ancestor, a node of the same component (a link is only ever replaced by a link to a node that the
// replacing union goes on to join with the old one), which costs a turn and never a wrong answer.
template <int SCOPE>
SEG_HD int32_t seg_find(const int32_t* parent, int32_t x) {
    for (int32_t p = seg_load<SCOPE>(parent + x); p != x; p = seg_load<SCOPE>(parent + x)) x = p;
    return x;
}
template <int SCOPE>
SEG_HD void seg_union(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = seg_find<SCOPE>(parent, a), b = seg_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b, b = t; }              // a: the larger root, which gets the link
        const int32_t old = seg_fetch_min<SCOPE>(parent + a, b);
        if (old == a) return;                                          // a was still a root: it hangs under b now
        a = old;                                                       // someone linked a first: parent[a] = min(old, b); join old's tree and b's
    }
}

// A record of a component: (count, first_L, lo_i, lo_j, lo_k, hi_i, hi_j, hi_k).
#define SEG_RECORD 8
SEG_HD bool seg_in_box(const int32_t* rec, int i, int j, int k) {
    return i >= rec[2] && i <= rec[5] && j >= rec[3] && j <= rec[6] && k >= rec[4] && k <= rec[7];
}

// The state of an output node whose source node has `state` and `label`, for the component with the local rank `rank` and
// the record `rec`.  in_grid: the source node exists.
SEG_HD uint8_t seg_pick_state(bool in_grid, uint8_t state, int32_t label, int32_t rank, const int32_t* rec, int i, int j, int k, int mode) {
    if (!in_grid) return SEG_FREE;
    const bool mine = label == rank;
    const bool hidden = state != SEG_FREE && state != SEG_SURFACE && seg_in_box(rec, i, j, k);
    if (mode == 0) return mine ? SEG_SURFACE : hidden ? SEG_UNKNOWN : SEG_FREE;
    return mine || hidden ? SEG_FREE : state;
}
