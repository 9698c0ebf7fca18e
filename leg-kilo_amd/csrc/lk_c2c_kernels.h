// lk_c2c_kernels.h - cloud-to-cloud nearest-neighbour distance of many pairs of clouds (lk_clouds_c2c_dev; the arithmetic is lk_c2c.h's, shared with
// the host probe).  Per call: bounds and status words of the clouds a pair names, on both sides, a grid per reference cloud (lk_c2c_grid: edge max_dist, doubled
// until the cloud's cells fit 31 bits), a cell key per reference record, rocPRIM's stable segmented radix sort with a segment per reference cloud, a
// gather of the records into cell order with their index in the cloud; then one thread per (pair, query point) searches the 27 cells around its point
// (lk_c2c_search: nine lower bounds in the cloud's sorted keys, each followed by a walk over the row's records) and writes (j, d2); last, one block
// per pair reduces its points in a fixed order.
// The streaming kernels run 256 threads with a record per lane.  The query kernel is SUPPOSED to be bound by the latency of its dependent loads -
// nine bisections of ~log2(n) steps, then records gathered 16 bytes at a time - and by divergence where heavy cells lie beside empty ones; DESIGN.md
// section 4l says what was measured.
#pragma once
#include "lk_c2c.h"

struct LkC2cQuery {
    const float4* q_pts;                   // the query buffer as given (offsets below are absolute)
    const unsigned long long* q_off;       // [n_q + 1]
    const unsigned int* r_off;             // [n_r + 1], counted from the first reference record
    const unsigned int *pair_q, *pair_r;   // [n_pairs]
    const unsigned long long* nn_off;      // [n_pairs + 1]
    const unsigned int *q_status, *r_status;
    const LkC2cGrid* grid;                 // [n_r]
    const unsigned int* keys;              // sorted, all reference clouds
    const LkC2cRec* recs;                  // in that order
    unsigned int* nn_idx;
    double* nn_d2;
    double reach2, thr2[4];
    unsigned int n_pairs, n_thr;
    lk_c2c* out;                           // [n_pairs], device
};

__device__ __forceinline__ int lk_c2c_f2ord(float f) {   // order-preserving int image of a float (lk_pre_kernels.h's lk_f2ord; this unit does not see that header)
    const int i = __float_as_int(f);
    return i >= 0 ? i : (i ^ 0x7fffffff);
}
__device__ __forceinline__ float lk_c2c_ord2f(int i) { return __int_as_float(i >= 0 ? i : (i ^ 0x7fffffff)); }

__global__ void __launch_bounds__(256) lk_c2c_init_kernel(int* __restrict__ mm, unsigned int* __restrict__ status, unsigned int n) {
    const unsigned int c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) mm[6 * c + k] = 0x7fffffff, mm[6 * c + 3 + k] = (int)0x80000000;
    status[c] = 0u;
}
// bounds and status of the clouds of one side: blockIdx.x = cloud (of the `used` ones only: a cloud no pair names is not read), gridDim.y blocks
// stride over its records.  atomicMin / atomicMax / atomicOr are order-free: the words do not depend on the schedule.
__global__ void __launch_bounds__(256) lk_c2c_bounds_kernel(const float4* __restrict__ pts, const unsigned long long* __restrict__ off,
                                                            const unsigned int* __restrict__ used, double max_dist, int* mm, unsigned int* status) {
    const unsigned int c = used[blockIdx.x];
    const unsigned long long e = off[c + 1];
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    unsigned int bad = 0u;
    for (unsigned long long i = off[c] + blockIdx.y * 256ull + threadIdx.x; i < e; i += gridDim.y * 256ull) {
        const float4 p = pts[i];
        const float q[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!isfinite(q[k])) bad |= LK_C2C_NONFINITE;
            else if (lk_c2c_out_of_range(q[k], max_dist)) bad |= LK_C2C_RANGE;
            const int v = lk_c2c_f2ord(q[k]);
            lo[k] = min(lo[k], v), hi[k] = max(hi[k], v);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = min(lo[k], __shfl_xor(lo[k], o, 64));
            hi[k] = max(hi[k], __shfl_xor(hi[k], o, 64));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicMin(&mm[6 * c + k], lo[k]), atomicMax(&mm[6 * c + 3 + k], hi[k]);
        if (bad) atomicOr(&status[c], bad);
    }
}
// the grid of every reference cloud; an empty, unused or refused one gets the grid of nothing (a refused cloud's bounds mean nothing)
__global__ void __launch_bounds__(256) lk_c2c_grid_kernel(const int* __restrict__ mm, const unsigned int* __restrict__ status, double max_dist, unsigned int n,
                                                          LkC2cGrid* __restrict__ grid) {
    const unsigned int c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n) return;
    LkC2cGrid g;
    if (status[c] == 0u && mm[6 * c] <= mm[6 * c + 3]) {
        const float lo[3] = {lk_c2c_ord2f(mm[6 * c]), lk_c2c_ord2f(mm[6 * c + 1]), lk_c2c_ord2f(mm[6 * c + 2])};
        const float hi[3] = {lk_c2c_ord2f(mm[6 * c + 3]), lk_c2c_ord2f(mm[6 * c + 4]), lk_c2c_ord2f(mm[6 * c + 5])};
        lk_c2c_grid(lo, hi, max_dist, &g);
    } else {
        lk_c2c_grid_of_nothing(max_dist, &g);
    }
    grid[c] = g;
}
__device__ __forceinline__ unsigned int lk_c2c_cloud_of(const unsigned int* __restrict__ off, unsigned int n, unsigned int i) {
    unsigned int lo = 0, hi = n;   // off[lo] <= i < off[hi]; among empty clouds the last one that starts at or before i
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// cell key of every reference record under its cloud's grid; records of an unused or refused cloud get key 0 (nothing searches them)
__global__ void __launch_bounds__(256)
    lk_c2c_keys_kernel(const float4* __restrict__ pts, unsigned int n, const unsigned int* __restrict__ r_off, unsigned int n_r, const LkC2cGrid* __restrict__ grid,
                       const unsigned int* __restrict__ status, const int* __restrict__ mm, unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = lk_c2c_cloud_of(r_off, n_r, i);
    unsigned int key = 0u;
    if (status[c] == 0u && mm[6 * c] <= mm[6 * c + 3]) {
        const float4 p = pts[i];
        key = lk_c2c_key(p.x, p.y, p.z, grid[c]);
    }
    keys[i] = key, vals[i] = i;
}
// the records into cell order, each with its index in its own cloud (the sort keeps a record inside its cloud's segment)
__global__ void __launch_bounds__(256)
    lk_c2c_gather_kernel(const float4* __restrict__ pts, const unsigned int* __restrict__ order, unsigned int n, const unsigned int* __restrict__ r_off,
                         unsigned int n_r, const unsigned int* __restrict__ status, const int* __restrict__ mm, LkC2cRec* __restrict__ recs) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = lk_c2c_cloud_of(r_off, n_r, i);
    LkC2cRec r = {0.f, 0.f, 0.f, 0u};
    if (status[c] == 0u && mm[6 * c] <= mm[6 * c + 3]) {   // (an unused cloud's records are not read)
        const unsigned int src = order[i];
        const float4 p = pts[src];
        r.x = p.x, r.y = p.y, r.z = p.z, r.idx = src - r_off[c];
    }
    recs[i] = r;
}
// one thread per (pair, query point): entry nn_off[k] + i of the two nn arrays
__global__ void __launch_bounds__(256) lk_c2c_query_kernel(LkC2cQuery a, unsigned long long total) {
    const unsigned long long g = blockIdx.x * 256ull + threadIdx.x;
    if (g >= total) return;
    unsigned int lo = 0, hi = a.n_pairs;   // nn_off[lo] <= g < nn_off[hi]
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (a.nn_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    const unsigned int qc = a.pair_q[lo], rc = a.pair_r[lo];
    unsigned int j = 0xffffffffu;
    double d2 = INFINITY;
    if ((a.q_status[qc] | a.r_status[rc]) == 0u) {
        const float4 q = a.q_pts[a.q_off[qc] + (g - a.nn_off[lo])];
        const unsigned int b = a.r_off[rc];
        lk_c2c_search(q.x, q.y, q.z, a.grid[rc], a.keys + b, a.recs + b, a.r_off[rc + 1] - b, a.reach2, &j, &d2, nullptr);
    }
    a.nn_idx[g] = j, a.nn_d2[g] = d2;
}

// one block per pair over its nn entries.  Lane t adds the points t, t + 256, ... in ascending order, then the 256 partial sums meet in a fixed tree:
// the order depends on the pair's query size alone.  worst: the largest d2, the smallest index among equals.
struct LkC2cPart {
    double s2, s1, mx;
    unsigned long long n, w[4];
    unsigned int worst;
};
__device__ __forceinline__ void lk_c2c_merge(LkC2cPart& x, const LkC2cPart& y) {
    if (y.n && (!x.n || y.mx > x.mx || (y.mx == x.mx && y.worst < x.worst))) x.mx = y.mx, x.worst = y.worst;
    x.s2 = x.s2 + y.s2, x.s1 = x.s1 + y.s1, x.n += y.n;
#pragma unroll
    for (int k = 0; k < 4; ++k) x.w[k] += y.w[k];
}
__global__ void __launch_bounds__(256) lk_c2c_reduce_kernel(LkC2cQuery a) {
    __shared__ LkC2cPart sh[256];
    const unsigned int k = blockIdx.x, t = threadIdx.x;
    const unsigned long long b = a.nn_off[k], n = a.nn_off[k + 1] - b;
    LkC2cPart p = {0.0, 0.0, 0.0, 0ull, {0ull, 0ull, 0ull, 0ull}, 0u};
    for (unsigned long long i = t; i < n; i += 256ull) {
        if (a.nn_idx[b + i] == 0xffffffffu) continue;
        const double d2 = a.nn_d2[b + i];
        p.s2 = p.s2 + d2, p.s1 = p.s1 + sqrt(d2);
        if (!p.n || d2 > p.mx) p.mx = d2, p.worst = (unsigned int)i;
        p.n += 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) p.w[c] += (c < (int)a.n_thr && d2 <= a.thr2[c]) ? 1ull : 0ull;
    }
    sh[t] = p;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkC2cPart x = sh[t];
            lk_c2c_merge(x, sh[t + o]);
            sh[t] = x;
        }
        __syncthreads();
    }
    if (t != 0) return;
    p = sh[0];
    lk_c2c r;
    const unsigned int st = a.q_status[a.pair_q[k]] | a.r_status[a.pair_r[k]];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool none = st != 0u || p.n == 0ull;
    r.rmse = none ? nan : sqrt(p.s2 / (double)p.n);
    r.mean = none ? nan : p.s1 / (double)p.n;
    r.max = none ? nan : sqrt(p.mx);
    r.n_query = n, r.n_matched = none ? 0ull : p.n;
#pragma unroll
    for (int c = 0; c < 4; ++c) r.n_within[c] = none ? 0ull : p.w[c];
    r.worst = none ? 0u : p.worst, r.status = st;
    a.out[k] = r;
}

// The compaction tail of the families that write kept records out as clouds (outlier filter, clustering, plane extraction): each brings its own keep
// words, lk_prim_exclusive_scan over them gives every kept record its place, and these two kernels do the rest.
struct LkCompactCall {
    const unsigned int* off;    // [n_clouds + 1], counted from the first record
    unsigned int n_clouds, total;
    const unsigned int* flag;   // [total + 1] keep words, the last one 0
    unsigned int* scan;         // [total + 1] their exclusive prefix sum
    unsigned int* out_off;      // [n_clouds + 1]
    const uint4* in;            // the call's first record: input order, [total]
    uint4* out_pts;             // may be null
    unsigned int* src_idx;      // may be null
};
// the output offsets: kept records in front of every cloud's first record
__global__ void __launch_bounds__(256) lk_c2c_compact_offsets_kernel(LkCompactCall a) {
    const unsigned int c = blockIdx.x * 256u + threadIdx.x;
    if (c <= a.n_clouds) a.out_off[c] = a.scan[a.off[c]];
}
// the kept records to their places, all 16 bytes as they are (four 32-bit words: a NaN payload survives), and their indices within their input clouds
__global__ void __launch_bounds__(256) lk_c2c_compact_scatter_kernel(LkCompactCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total || !a.flag[g]) return;
    const unsigned int j = a.scan[g];
    if (a.out_pts) a.out_pts[j] = a.in[g];
    if (a.src_idx) a.src_idx[j] = g - a.off[lk_c2c_cloud_of(a.off, a.n_clouds, g)];
}
