// lk_normals_kernels.h - per-point normals of many clouds (lk_clouds_normals_dev; the arithmetic is lk_normals.h's, shared with the host probe).
// The chain in front is lk_c2c_kernels.h's, launched as lk_clouds_mme_dev launches it with the radius as the reach and every non-empty cloud in
// use.  Then
//   lk_normals_point_kernel   lk_mme_point_kernel's shape: one thread per SORTED record, lk_mme_walk as it stands (so n_i is MME's d_n),
//                             lk_normals_finish in the same thread, the 16-byte record to position rec.idx - input order;
//   lk_normals_count_kernel   one block per cloud: the valid records (nx == nx) counted, the cloud's lk_normals record.
// DESIGN.md section 4o says what was measured.
#pragma once
#include "lk_normals.h"

struct LkNormalsCall {
    const unsigned int* off;      // [n_clouds + 1], counted from the first record
    const unsigned int* status;   // [n_clouds]
    const LkC2cGrid* grid;        // [n_clouds]
    const unsigned int* keys;     // sorted, all clouds
    const LkC2cRec* recs;         // in that order
    float4* normals;              // per-point records, input order, [off[n_clouds]]
    double reach2, min_planarity;
    unsigned int n_clouds, min_pts, total;
    lk_normals* out;              // [n_clouds], device
};

__global__ void __launch_bounds__(256) lk_normals_point_kernel(LkNormalsCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g), b = a.off[c];
    unsigned int pos = g;   // a status cloud's records were not gathered: each sorted place takes the entry of the same number
    const float nan = __int_as_float(0x7fc00000);
    float rec[4] = {nan, nan, nan, nan};
    if (a.status[c] == 0u) {
        const LkC2cRec q = a.recs[g];
        LkMmeAcc acc;
        lk_mme_walk(q.x, q.y, q.z, a.grid[c], a.keys + b, a.recs + b, a.off[c + 1] - b, a.reach2, &acc, nullptr);
        lk_normals_finish(acc, a.min_pts, a.min_planarity, rec);
        pos = b + q.idx;
    }
    a.normals[pos] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

__global__ void __launch_bounds__(256) lk_normals_count_kernel(LkNormalsCall a) {
    __shared__ unsigned long long sh[256];
    const unsigned int c = blockIdx.x, t = threadIdx.x, b = a.off[c], n = a.off[c + 1] - b;
    unsigned long long v = 0ull;
    for (unsigned int i = t; i < n; i += 256u) {
        const float x = a.normals[b + i].x;
        v += x == x ? 1ull : 0ull;
    }
    sh[t] = v;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t != 0) return;
    lk_normals r;
    r.n_points = n, r.n_valid = a.status[c] ? 0ull : sh[0], r.status = a.status[c], r.pad = 0u;
    a.out[c] = r;
}
