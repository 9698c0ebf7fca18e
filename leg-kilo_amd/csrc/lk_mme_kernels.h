// lk_mme_kernels.h - reference-free scores of many map clouds (lk_clouds_mme_dev; the arithmetic is lk_mme.h's, shared with the host probe): mean map
// entropy and mean plane variance.  The chain in front is lk_c2c_kernels.h's, launched as it is with the radius as the reach and every non-empty
// cloud in use: bounds, grids, keys, the stable segmented sort, the gather into cell order.  Then
//   lk_mme_point_kernel   one thread per SORTED record: the 64 lanes of a wave sit in the same or adjacent cells, take nearly the same nine lower
//                         bounds and walk nearly the same key ranges, so their record loads hit the same cache lines and the wave diverges little.
//                         (lk_c2c_query_kernel runs a thread per INPUT record, whose lanes lie anywhere.)  The count and nine sums stay in registers,
//                         lk_mme_finish runs in the same thread, the results go to position rec.idx of the per-point arrays - input order;
//   lk_mme_reduce_kernel  one block per cloud over the per-point arrays in input order: lane-strided partial sums, then a fixed tree, so a cloud's
//                         record depends on that cloud alone.
// DESIGN.md section 4m says what was measured.
#pragma once
#include "lk_mme.h"

struct LkMmeCall {
    const unsigned int* off;      // [n_clouds + 1], counted from the first record
    const unsigned int* status;   // [n_clouds]
    const LkC2cGrid* grid;        // [n_clouds]
    const unsigned int* keys;     // sorted, all clouds
    const LkC2cRec* recs;         // in that order
    unsigned int* n;              // per-point arrays, input order, [off[n_clouds]]
    double *h, *lmin;
    double reach2;
    unsigned int n_clouds, min_pts, total;
    lk_mme* out;                  // [n_clouds], device
};

__global__ void __launch_bounds__(256) lk_mme_point_kernel(LkMmeCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    unsigned int pos = g, n = 0u;   // a status cloud's records were not gathered: each sorted place takes the entry of the same number
    double h = __longlong_as_double(0x7ff8000000000000ll), lmin = h;
    if (a.status[c] == 0u) {
        const LkC2cRec q = a.recs[g];
        LkMmeAcc acc;
        unsigned int cls;
        lk_mme_walk(q.x, q.y, q.z, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, a.reach2, &acc, nullptr);
        lk_mme_finish(acc, a.min_pts, &cls, &h, &lmin);
        pos = b + q.idx, n = acc.n;
    }
    a.n[pos] = n, a.h[pos] = h, a.lmin[pos] = lmin;
}

// one block per cloud.  Lane t takes the points t, t + 256, ... in ascending order, then the 256 partial sums meet in a fixed tree: the order depends
// on the cloud's size alone.  worst: the largest h, the smallest index among equals.
struct LkMmePart {
    double sh, sl, mx;
    unsigned long long pairs, dense, scored;
    unsigned int worst;
};
__device__ __forceinline__ void lk_mme_merge(LkMmePart& x, const LkMmePart& y) {
    if (y.scored && (!x.scored || y.mx > x.mx || (y.mx == x.mx && y.worst < x.worst))) x.mx = y.mx, x.worst = y.worst;
    x.sh = x.sh + y.sh, x.sl = x.sl + y.sl, x.pairs += y.pairs, x.dense += y.dense, x.scored += y.scored;
}
__global__ void __launch_bounds__(256) lk_mme_reduce_kernel(LkMmeCall a) {
    __shared__ LkMmePart sh[256];
    const unsigned int c = blockIdx.x, t = threadIdx.x, b = a.off[c], n = a.off[c + 1] - b;
    LkMmePart p = {0.0, 0.0, 0.0, 0ull, 0ull, 0ull, 0u};
    for (unsigned int i = t; i < n; i += 256u) {
        const double h = a.h[b + i], l = a.lmin[b + i];
        p.pairs += a.n[b + i];
        if (l == l) p.sl = p.sl + l, p.dense += 1ull;
        if (h == h) {
            p.sh = p.sh + h;
            if (!p.scored || h > p.mx) p.mx = h, p.worst = i;
            p.scored += 1ull;
        }
    }
    sh[t] = p;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkMmePart x = sh[t];
            lk_mme_merge(x, sh[t + o]);
            sh[t] = x;
        }
        __syncthreads();
    }
    if (t != 0) return;
    p = sh[0];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned int st = a.status[c];
    lk_mme r;
    r.mme = (st == 0u && p.scored) ? p.sh / (double)p.scored : nan;
    r.mpv = (st == 0u && p.dense) ? p.sl / (double)p.dense : nan;
    r.h_max = (st == 0u && p.scored) ? p.mx : nan;
    r.n_points = n, r.n_dense = st ? 0ull : p.dense, r.n_scored = st ? 0ull : p.scored, r.n_pairs = st ? 0ull : p.pairs;
    r.worst = (st == 0u && p.scored) ? p.worst : 0u, r.status = st;
    a.out[c] = r;
}
