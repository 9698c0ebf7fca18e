// lk_cluster.h - the arithmetic of the clustering of map clouds (lk_clouds_cluster_dev, lk_cluster_kernels.h) that the device route and its CPU twin
// (tools/probes/cluster_host.cc, tests/test_cluster_host.py) share: the three visitors (count, link, nearest core) that lk_c2c.h's walk calls per
// candidate record, and the union-find over the core points.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): every decision is lk_c2c_d2(i, j) <= reach * reach, and by the argument at the head
// of lk_c2c.h every record within reach lies in the 27 cells that lk_c2c_walk visits.  Everything here is whole numbers and comparisons of d2,
// so the walk's order leaves no trace: n_i is a count, the nearest core candidate minimises (d2, index), and the union-find ends with the same roots
// whatever order the unions arrive in.
//
// The union-find.  parent[] is indexed by a record's input position within the call and starts as parent[i] = i.  A root is an entry that points
// at itself.  find follows parents and halves the path behind it; unite hooks the LARGER of two roots under the SMALLER with a compare-and-swap
// that succeeds only while the larger is still a root, and goes on from the value the swap returns otherwise.  Every write lowers an entry
// (atomic min, or the swap of i for something below i), so an entry only ever decreases, every chain of parents descends strictly, and every loop
// ends.  A component's root is the smallest position among its members: nothing smaller is ever hooked under anything.  On the device several
// XCDs work on parent[] at once and their L2s are not coherent with each other: every read is a relaxed atomic load of agent scope and every write
// a device-scope atomic, so a stale value is a hint that the swap validates, never a decision.  No thread waits for another.
// Plain C++ that compiles for the host as it stands (there the accesses are plain loads and stores: the twin runs one record after the other).
#pragma once
#include "lk_c2c.h"

#define LK_CLUSTER_NONE 0xffffffffu

LK_C2C_HD unsigned int lk_cluster_load(const unsigned int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
// *p = min(*p, v)
LK_C2C_HD void lk_cluster_lower(unsigned int* p, unsigned int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
// *p = v if *p == expect; the value found
LK_C2C_HD unsigned int lk_cluster_swap(unsigned int* p, unsigned int expect, unsigned int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const unsigned int old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}

// the root of i, with path halving: an entry on the way takes its grandparent, which is below its parent
LK_C2C_HD unsigned int lk_cluster_find(unsigned int* parent, unsigned int i) {
    for (;;) {
        const unsigned int p = lk_cluster_load(parent + i);
        if (p == i) return i;
        const unsigned int gp = lk_cluster_load(parent + p);
        if (gp != p) lk_cluster_lower(parent + i, gp);
        i = gp;
    }
}
// the root of i when nothing changes parent[] any more (after the link kernel): no write
LK_C2C_HD unsigned int lk_cluster_root(const unsigned int* parent, unsigned int i) {
    for (;;) {
        const unsigned int p = parent[i];
        if (p == i) return i;
        i = p;
    }
}
LK_C2C_HD void lk_cluster_unite(unsigned int* parent, unsigned int x, unsigned int y) {
    for (;;) {
        x = lk_cluster_find(parent, x), y = lk_cluster_find(parent, y);
        if (x == y) return;
        const unsigned int hi = x > y ? x : y, lo = x > y ? y : x;
        const unsigned int old = lk_cluster_swap(parent + hi, hi, lo);
        if (old == hi) return;
        x = old, y = lo;   // hi was hooked elsewhere in the meantime: on from where it points now
    }
}

// The visitors of lk_c2c_walk, one point of a cloud against the cloud itself (the walk calls them for every record of the 27 cells, the query itself
// included).  n_i: the records within reach, the point itself and its duplicates among them
struct LkClusterCount {
    double reach2;
    unsigned int n;
    LK_C2C_HD void operator()(unsigned int, const LkC2cRec&, double d2) { n += lk_c2c_matched(d2, reach2) ? 1u : 0u; }
};
LK_C2C_HD bool lk_cluster_is_core(unsigned int n_i, unsigned int min_pts) { return n_i >= min_pts; }
// a CORE query united with every core candidate of a smaller index: each edge is taken once, from its larger end.  core: a flag per sorted place of
// the cloud; parent: the call's, base = the cloud's first input position
struct LkClusterLink {
    double reach2;
    const unsigned char* core;
    unsigned int* parent;
    unsigned int base, qidx;
    LK_C2C_HD void operator()(unsigned int a, const LkC2cRec& r, double d2) {
        if (r.idx < qidx && core[a] && lk_c2c_matched(d2, reach2)) lk_cluster_unite(parent, base + qidx, base + r.idx);
    }
};
// the core candidate that minimises (d2, index): C2C's rule
struct LkClusterNearest {
    double reach2;
    const unsigned char* core;
    double best;
    unsigned int j;
    LK_C2C_HD void operator()(unsigned int a, const LkC2cRec& r, double d2) {
        if (core[a] && lk_c2c_matched(d2, reach2) && (d2 < best || (d2 == best && r.idx < j))) best = d2, j = r.idx;
    }
};

// a cluster of `size` members against the bounds (min_size 0 and 1 mean the same: a cluster has a member; max_size 0xffffffff: no bound)
LK_C2C_HD bool lk_cluster_in_bounds(unsigned int size, unsigned int min_size, unsigned int max_size) { return size >= min_size && size <= max_size; }
// (size, id) of a cluster against the best so far: the larger size, the smaller id among equals.  none: best_id == LK_CLUSTER_NONE
LK_C2C_HD bool lk_cluster_larger(unsigned int size, unsigned int id, unsigned int best_size, unsigned int best_id) {
    return best_id == LK_CLUSTER_NONE || size > best_size || (size == best_size && id < best_id);
}
