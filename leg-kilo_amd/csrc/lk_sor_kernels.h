// lk_sor_kernels.h - the statistical outlier filter of many map clouds (lk_clouds_sor_dev; the arithmetic is lk_sor.h's, shared with the host probe):
// per point the mean distance to its k nearest neighbours within a reach, per cloud the mean and deviation of those, and the points that pass
// mu + n_sigma * sigma written out in input order.  The chain in front is lk_c2c_kernels.h's, launched as it is with the reach as the cell edge and
// every non-empty cloud in use: bounds, grids, keys, the stable segmented sort, the gather into cell order.  Then
//   lk_sor_point_kernel<CAP>  one thread per SORTED record, for lk_mme_kernels.h's reason: the 64 lanes of a wave sit in the same or adjacent cells
//                             and walk nearly the same key ranges.  The list of the CAP smallest d2 is indexed by constants only and stays in
//                             registers (lk_sor.h); CAP is chosen from k on the host.  cnt_i and dbar_i go to position rec.idx - input order;
//   lk_sor_stats_kernel       one block per cloud over dbar in input order, lk_mme_reduce_kernel's scheme - lane-strided partial sums, then a fixed
//                             tree - twice: the mean first, the centred squares second; then the counts under the threshold, and the record;
//   lk_sor_flag_kernel        a keep word per record (and the caller's d_keep byte).  What follows is lk_c2c_kernels.h's compaction tail, shared
//                             with clustering and plane extraction: lk_prim_exclusive_scan over the keep words gives every kept record its place
//                             and, read at the cloud starts, the offsets of the output clouds; the scatter moves the kept records there.
// DESIGN.md section 4p says what was measured.
#pragma once
#include "lk_sor.h"

struct LkSorCall {
    const unsigned int* off;      // [n_clouds + 1], counted from the first record
    const unsigned int* status;   // [n_clouds]
    const LkC2cGrid* grid;        // [n_clouds]
    const unsigned int* keys;     // sorted, all clouds
    const LkC2cRec* recs;         // in that order
    unsigned int* cnt;            // per-point arrays, input order, [total]; cnt and keep may be null
    double* dbar;
    unsigned char* keep;
    unsigned int* flag;           // [total + 1] keep words, the last one 0
    double* thr;                  // [n_clouds]
    double reach2, n_sigma;
    unsigned int n_clouds, k, total;
    lk_sor* out;                  // [n_clouds], device
};

template <int CAP>
__global__ void __launch_bounds__(256) lk_sor_point_kernel(LkSorCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    unsigned int pos = g, cnt = 0u;   // a status cloud's records were not gathered: each sorted place takes the entry of the same number
    double dbar = __longlong_as_double(0x7ff8000000000000ll);
    if (a.status[c] == 0u) {
        const LkC2cRec q = a.recs[g];
        LkSorList<CAP> list;
        lk_sor_walk(q.x, q.y, q.z, q.idx, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, a.reach2, &list, nullptr);
        dbar = lk_sor_finish(list, a.k);
        pos = b + q.idx, cnt = list.cnt;
    }
    if (a.cnt) a.cnt[pos] = cnt;
    a.dbar[pos] = dbar;
}

// one block per cloud.  Lane t takes the points t, t + 256, ... in ascending order, then the 256 partial sums meet in a fixed tree: the order depends
// on the cloud's size alone.  worst: the largest dbar, the smallest index among equals.
struct LkSorPart {
    double s, mx;
    unsigned long long ns, iso;
    unsigned int worst;
};
__device__ __forceinline__ void lk_sor_merge(LkSorPart& x, const LkSorPart& y) {
    if (y.ns && (!x.ns || y.mx > x.mx || (y.mx == x.mx && y.worst < x.worst))) x.mx = y.mx, x.worst = y.worst;
    x.s = x.s + y.s, x.ns += y.ns, x.iso += y.iso;
}
__global__ void __launch_bounds__(256) lk_sor_stats_kernel(LkSorCall a) {
    __shared__ LkSorPart sh[256];
    __shared__ double sq[256];
    __shared__ unsigned long long kept_all;
    const unsigned int c = blockIdx.x, t = threadIdx.x, b = a.off[c], n = a.off[c + 1] - b;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // pass 1: the mean, the counts, the worst point
    LkSorPart p = {0.0, 0.0, 0ull, 0ull, 0u};
    for (unsigned int i = t; i < n; i += 256u) {
        const double d = a.dbar[b + i];
        if (d == d) {
            p.s = p.s + d;
            if (!p.ns || d > p.mx) p.mx = d, p.worst = i;
            p.ns += 1ull;
        } else {
            p.iso += 1ull;
        }
    }
    sh[t] = p;
    if (t == 0) kept_all = 0ull;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkSorPart x = sh[t];
            lk_sor_merge(x, sh[t + o]);
            sh[t] = x;
        }
        __syncthreads();
    }
    p = sh[0];
    const double mu = p.ns ? p.s / (double)p.ns : nan;
    // pass 2: the centred squares, in the same order
    double q = 0.0;
    for (unsigned int i = t; i < n; i += 256u) {
        const double d = a.dbar[b + i];
        if (d == d) {
            const double e = d - mu;
            q = q + e * e;
        }
    }
    sq[t] = q;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) sq[t] = sq[t] + sq[t + o];
        __syncthreads();
    }
    const unsigned int st = a.status[c];
    const bool any = st == 0u && p.ns;
    const double sigma = any ? lk_sor_sigma(sq[0], p.ns) : nan;
    const double thr = any ? lk_sor_thr(mu, sigma, a.n_sigma) : nan;
    // the points under the threshold: whole numbers, any order
    unsigned long long kept = 0ull;
    for (unsigned int i = t; i < n; i += 256u) kept += lk_sor_kept(a.dbar[b + i], thr) ? 1ull : 0ull;
    if (kept) atomicAdd(&kept_all, kept);
    __syncthreads();
    if (t != 0) return;
    lk_sor r;
    r.mu = any ? mu : nan, r.sigma = sigma, r.thr = thr;
    r.n_points = n, r.n_isolated = st ? 0ull : p.iso, r.n_kept = st ? 0ull : kept_all, r.n_outliers = st ? 0ull : p.ns - kept_all;
    r.worst = any ? p.worst : 0u, r.status = st;
    a.out[c] = r;
    a.thr[c] = thr;
}

// a keep word per record and one 0 behind the last, so that the exclusive scan ends with the number of kept records
__global__ void __launch_bounds__(256) lk_sor_flag_kernel(LkSorCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total) return;
    if (g == a.total) {
        a.flag[g] = 0u;
        return;
    }
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g);
    const unsigned int kept = lk_sor_kept(a.dbar[g], a.thr[c]) ? 1u : 0u;
    a.flag[g] = kept;
    if (a.keep) a.keep[g] = (unsigned char)kept;
}
