// lk_cluster_kernels.h - DBSCAN over many map clouds (lk_clouds_cluster_dev; the arithmetic is lk_cluster.h's, shared with the host probe): a label, a
// kind and a neighbour count per point, a size and a first core index per cluster, and the points of the clusters whose size is in bounds written
// out in input order.  The chain in front is lk_c2c_kernels.h's, launched as it is with the reach as the cell edge and every non-empty cloud in use.
// Every phase boundary is a kernel boundary; inside a kernel no thread waits for another.
//   lk_cluster_count_kernel   one thread per SORTED record, for lk_mme_kernels.h's reason.  n_i and the kind (core / not yet anything) go to the
//                             input position, the core flag to the SORTED place, where the later walks read it beside the record; parent[] starts;
//   lk_cluster_link_kernel    one thread per sorted CORE record: every core candidate of a smaller index is united with it (lk_cluster.h);
//   lk_cluster_assign_kernel  one thread per sorted record.  parent[] no longer changes: a core point takes its root, another point the root of the
//                             core candidate that minimises (d2, index) and becomes a border point, or stays noise;
//   lk_cluster_rootflag_kernel  a word per input position, 1 at a root; lk_prim_exclusive_scan over them numbers the clusters of the call in
//                             ascending order of their smallest core position - per cloud that is the definition's order - and, read at the
//                             cloud starts, gives cl_off;
//   lk_cluster_label_kernel   one thread per input position: the label, the cluster's member count (atomicAdd: integers, any order gives the same
//                             bits), at a root the cluster's first core index;
//   lk_cluster_record_kernel  one block per cloud: the counts, `largest` with its tie rule, the clusters in bounds and the one that is kept under
//                             LK_CLUSTER_KEEP_LARGEST;
//   lk_cluster_flag_kernel    a keep word per record; the scan, the output offsets and the scatter behind it are lk_c2c_kernels.h's compaction tail.
// DESIGN.md section 4q says what was measured.
#pragma once
#include "lk_cluster.h"

struct LkClusterCall {
    const unsigned int* off;      // [n_clouds + 1], counted from the first record
    const unsigned int* status;   // [n_clouds]
    const LkC2cGrid* grid;        // [n_clouds]
    const unsigned int* keys;     // sorted, all clouds
    const LkC2cRec* recs;         // in that order
    unsigned char* core;          // [total] SORTED order: 1 where the record at that place is a core point
    unsigned int* parent;         // [total] input order
    unsigned int* root;           // [total] input order: the root's position, from the label kernel on the cluster's number within the call; NONE = noise
    unsigned int* n;              // [total] input order (the caller's or ours)
    unsigned char* kind;          // [total] input order (the caller's or ours)
    unsigned int* label;          // [total] input order, may be null
    unsigned int* rflag;          // [total + 1] 1 at a root, the last one 0
    unsigned int* rscan;          // [total + 1] their exclusive prefix sum
    unsigned int* size;           // [total] members per cluster of the call, zeroed before the label kernel
    unsigned int* first;          // [total] smallest core index per cluster of the call
    unsigned int* cl_size;        // the caller's tables, may be null: the first rscan[total] entries of size / first
    unsigned int* cl_first;
    unsigned int* cl_off;         // [n_clouds + 1]
    unsigned int* kept_id;        // [n_clouds] under KEEP_LARGEST the cluster of the call that is kept, NONE = none
    unsigned int* flag;           // [total + 1] keep words, the last one 0
    double reach2;
    unsigned int n_clouds, total, min_pts, min_size, max_size, keep_largest;
    lk_cluster* out;              // [n_clouds], device
};

__global__ void __launch_bounds__(256) lk_cluster_count_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    unsigned int pos = g, n = 0u;   // a status cloud's records were not gathered: each sorted place takes the entry of the same number
    bool core = false;
    if (a.status[c] == 0u) {
        const LkC2cRec q = a.recs[g];
        LkClusterCount v = {a.reach2, 0u};
        lk_c2c_walk(q.x, q.y, q.z, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, v, nullptr);
        pos = b + q.idx, n = v.n, core = lk_cluster_is_core(n, a.min_pts);
    }
    a.n[pos] = n, a.kind[pos] = core ? 2 : 0, a.core[g] = core ? 1 : 0, a.parent[pos] = pos;
}

__global__ void __launch_bounds__(256) lk_cluster_link_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total || !a.core[g]) return;   // (a status cloud has no core point)
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    const LkC2cRec q = a.recs[g];
    LkClusterLink v = {a.reach2, a.core + b, a.parent, b, q.idx};
    lk_c2c_walk(q.x, q.y, q.z, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, v, nullptr);
}

__global__ void __launch_bounds__(256) lk_cluster_assign_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    unsigned int pos = g, root = LK_CLUSTER_NONE;
    if (a.status[c] == 0u) {
        const LkC2cRec q = a.recs[g];
        pos = b + q.idx;
        if (a.core[g]) {
            root = lk_cluster_root(a.parent, pos);
        } else {
            LkClusterNearest v = {a.reach2, a.core + b, INFINITY, LK_CLUSTER_NONE};
            lk_c2c_walk(q.x, q.y, q.z, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, v, nullptr);
            if (v.j != LK_CLUSTER_NONE) root = lk_cluster_root(a.parent, b + v.j), a.kind[pos] = 1;
        }
    }
    a.root[pos] = root;
}

// a word per input position and one 0 behind the last, so that the exclusive scan ends with the number of clusters
__global__ void __launch_bounds__(256) lk_cluster_rootflag_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total) return;
    a.rflag[g] = (g < a.total && a.root[g] == g) ? 1u : 0u;   // (only a core point is its own root: a border point's root is a core point)
}

__global__ void __launch_bounds__(256) lk_cluster_label_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int r = a.root[g];
    unsigned int id = LK_CLUSTER_NONE, label = LK_CLUSTER_NONE;
    if (r != LK_CLUSTER_NONE) {
        const unsigned int b = a.off[lk_c2c_cloud_of(a.off, a.n_clouds, g)];
        id = a.rscan[r], label = id - a.rscan[b];
        atomicAdd(a.size + id, 1u);
        if (r == g) a.first[id] = g - b;
    }
    if (a.label) a.label[g] = label;
    a.root[g] = id;   // (entry g is read by this thread alone)
}

// one block per cloud; whole numbers throughout, so the order of the sums is free
struct LkClusterPart {
    unsigned long long core, border, kept_pts;
    unsigned int in_bounds, best_size, best_id, keep_size, keep_id;   // best: of all clusters, keep: of those in bounds; ids of the call, NONE = none
};
__device__ __forceinline__ void lk_cluster_merge(LkClusterPart& x, const LkClusterPart& y) {
    x.core += y.core, x.border += y.border, x.kept_pts += y.kept_pts, x.in_bounds += y.in_bounds;
    if (y.best_id != LK_CLUSTER_NONE && lk_cluster_larger(y.best_size, y.best_id, x.best_size, x.best_id)) x.best_size = y.best_size, x.best_id = y.best_id;
    if (y.keep_id != LK_CLUSTER_NONE && lk_cluster_larger(y.keep_size, y.keep_id, x.keep_size, x.keep_id)) x.keep_size = y.keep_size, x.keep_id = y.keep_id;
}
__global__ void __launch_bounds__(256) lk_cluster_record_kernel(LkClusterCall a) {
    __shared__ LkClusterPart sh[256];
    const unsigned int c = blockIdx.x, t = threadIdx.x, b = a.off[c], n = a.off[c + 1] - b;
    const unsigned int k0 = a.rscan[b], k1 = a.rscan[a.off[c + 1]];
    LkClusterPart p = {0ull, 0ull, 0ull, 0u, 0u, LK_CLUSTER_NONE, 0u, LK_CLUSTER_NONE};
    for (unsigned int i = t; i < n; i += 256u) {
        const unsigned int kind = a.kind[b + i];
        p.core += kind == 2 ? 1ull : 0ull, p.border += kind == 1 ? 1ull : 0ull;
    }
    for (unsigned int k = k0 + t; k < k1; k += 256u) {
        const unsigned int s = a.size[k];
        if (lk_cluster_larger(s, k, p.best_size, p.best_id)) p.best_size = s, p.best_id = k;
        if (!lk_cluster_in_bounds(s, a.min_size, a.max_size)) continue;
        p.in_bounds += 1u, p.kept_pts += s;
        if (lk_cluster_larger(s, k, p.keep_size, p.keep_id)) p.keep_size = s, p.keep_id = k;
    }
    sh[t] = p;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkClusterPart x = sh[t];
            lk_cluster_merge(x, sh[t + o]);
            sh[t] = x;
        }
        __syncthreads();
    }
    if (t != 0) return;
    p = sh[0];
    const bool one = a.keep_largest != 0u, any = p.keep_id != LK_CLUSTER_NONE;
    lk_cluster r;
    r.n_points = n, r.n_core = p.core, r.n_border = p.border, r.n_noise = a.status[c] ? 0ull : n - p.core - p.border;
    r.n_kept = one ? (any ? p.keep_size : 0ull) : p.kept_pts;
    r.n_clusters = k1 - k0, r.n_kept_clusters = one ? (any ? 1u : 0u) : p.in_bounds;
    r.largest = p.best_id != LK_CLUSTER_NONE ? p.best_id - k0 : 0u, r.largest_size = p.best_id != LK_CLUSTER_NONE ? p.best_size : 0u;
    r.status = a.status[c], r.pad = 0u;
    a.out[c] = r;
    a.kept_id[c] = p.keep_id;
}

// cl_off, and the caller's tables: the first rscan[total] entries of ours
__global__ void __launch_bounds__(256) lk_cluster_tables_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g <= a.n_clouds) a.cl_off[g] = a.rscan[a.off[g]];
    if (g >= a.rscan[a.total]) return;
    if (a.cl_size) a.cl_size[g] = a.size[g];
    if (a.cl_first) a.cl_first[g] = a.first[g];
}

// a keep word per record and one 0 behind the last, so that the exclusive scan ends with the number of kept records
__global__ void __launch_bounds__(256) lk_cluster_flag_kernel(LkClusterCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total) return;
    unsigned int kept = 0u;
    const unsigned int id = g < a.total ? a.root[g] : LK_CLUSTER_NONE;
    if (id != LK_CLUSTER_NONE)
        kept = a.keep_largest ? (id == a.kept_id[lk_c2c_cloud_of(a.off, a.n_clouds, g)] ? 1u : 0u) : (lk_cluster_in_bounds(a.size[id], a.min_size, a.max_size) ? 1u : 0u);
    a.flag[g] = kept;
}
