// lk_align_kernels.h - rigid alignment (point-to-point ICP) of many pairs of clouds, the loop around lk_c2c_kernels.h's search and lk_horn.h's solve
// (lk_clouds_align_dev; the arithmetic is lk_align.h's, shared with the host probe), and the streaming kernel that writes moved clouds
// (lk_clouds_transform_dev).  Per call the reference side is indexed once (c2c_index); then max_iter + 1 search launches with max_iter solve
// launches between them go onto the stream back to back, and lk_c2c_reduce_kernel makes the final lk_c2c record from the last nn arrays.
// A pair's state lives in device memory: its record (rot / trans are the current T) and a `done` word -
//     0  running: the search runs, the solve that follows takes a step
//     1  converged: the search that follows is the final one, the solve after it only closes the pair
//     2  closed: the nn entries hold the final search; search and solve return at once
// Only the solve kernel (and the init kernel) write `done`, between two searches, so every thread of a search reads the same word.
// The search kernel has lk_c2c_query_kernel's shape and is SUPPOSED to be bound as that one is, by its dependent loads.
// One block per pair in the solve: a single pair of tens of millions of points is slow there, as it is in lk_c2c_reduce_kernel.
#pragma once
#include "lk_align.h"
#include "lk_c2c_kernels.h"

struct LkAlignCall {
    LkC2cQuery q;                          // the clouds' tables, the reference index, the nn arrays, the final lk_c2c records
    const float4* r_pts;                   // the reference buffer as given (absolute offsets), for the solve's gather in original order
    const unsigned long long* r_off64;     // [n_r + 1]
    const double* T0;                      // [12 n_pairs]
    lk_align* rec;                         // [n_pairs], device
    unsigned int* done;                    // [n_pairs]
    double max_dist, eps_rot, eps_trans;
};

// a pair's record and done word before the first search: T = T0; a status of the input clouds or a non-finite T0 closes the pair
__global__ void __launch_bounds__(256) lk_align_init_kernel(LkAlignCall a) {
    const unsigned int k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.q.n_pairs) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    lk_align r;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = a.T0[12 * k + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) r.rot[i] = T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) r.trans[i] = T[9 + i];
    r.rmse_first = nan, r.step_rot = nan, r.step_trans = nan, r.n_matched_first = 0ull, r.iters = 0u;
    r.status = (a.q.q_status[a.q.pair_q[k]] | a.q.r_status[a.q.pair_r[k]]) | (lk_align_finite12(T) ? 0u : LK_ALIGN_BAD_T0);
    a.rec[k] = r;
    a.done[k] = r.status ? 2u : 0u;
}

// one thread per (pair, query point): entry nn_off[k] + i of the two nn arrays under the pair's current T.  first: the launch in front of every
// solve, where a closed pair (a status) still gets its unmatched entries written
__global__ void __launch_bounds__(256) lk_align_search_kernel(LkAlignCall a, unsigned long long total, int first) {
    const unsigned long long g = blockIdx.x * 256ull + threadIdx.x;
    if (g >= total) return;
    unsigned int lo = 0, hi = a.q.n_pairs;   // nn_off[lo] <= g < nn_off[hi]
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (a.q.nn_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    const bool closed = a.done[lo] == 2u;
    if (closed && !first) return;
    unsigned int j = 0xffffffffu;
    double d2 = INFINITY;
    if (!closed) {
        const unsigned int qc = a.q.pair_q[lo], rc = a.q.pair_r[lo];
        const float4 p = a.q.q_pts[a.q.q_off[qc] + (g - a.q.nn_off[lo])];
        const unsigned int b = a.q.r_off[rc];
        const lk_align* r = a.rec + lo;
        double T[12];
#pragma unroll
        for (int i = 0; i < 9; ++i) T[i] = r->rot[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) T[9 + i] = r->trans[i];
        lk_align_search(T, p.x, p.y, p.z, a.max_dist, a.q.grid[rc], a.q.keys + b, a.q.recs + b, a.q.r_off[rc + 1] - b, a.q.reach2, &j, &d2);
    }
    a.q.nn_idx[g] = j, a.q.nn_d2[g] = d2;
}

// one block per pair over its nn entries, built like lk_c2c_reduce_kernel: lane t adds the points t, t + 256, ... in ascending order, then the 256
// partial sums meet in a fixed tree - the order depends on the pair's query size alone.  First the count, the sum of d2 and the two centroids; after a
// barrier the nine centred products, r_j gathered from the reference buffer in its original order; then thread 0 solves and decides.
__global__ void __launch_bounds__(256) lk_align_solve_kernel(LkAlignCall a) {
    __shared__ union {
        LkAlignSums sums[256];
        double cov[256][9];
    } sh;
    __shared__ double bar[6];
    const unsigned int k = blockIdx.x, t = threadIdx.x;
    const unsigned int was = a.done[k];
    __syncthreads();   // (every thread has read the word before thread 0 may write it)
    if (was != 0u) {
        if (t == 0u && was == 1u) a.done[k] = 2u;   // the search in front of this launch was the final one
        return;
    }
    const unsigned int qc = a.q.pair_q[k], rc = a.q.pair_r[k];
    const unsigned long long b = a.q.nn_off[k], n = a.q.nn_off[k + 1] - b;
    const float4* qp = a.q.q_pts + a.q.q_off[qc];
    const float4* rp = a.r_pts + a.r_off64[rc];
    LkAlignSums s;
    lk_align_sums_zero(&s);
    for (unsigned long long i = t; i < n; i += 256ull) {
        const unsigned int j = a.q.nn_idx[b + i];
        if (j == 0xffffffffu) continue;
        const float4 p = qp[i], r = rp[j];
        lk_align_sums_term(&s, a.q.nn_d2[b + i], p.x, p.y, p.z, r.x, r.y, r.z);
    }
    sh.sums[t] = s;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkAlignSums x = sh.sums[t];
            lk_align_sums_merge(&x, sh.sums[t + o]);
            sh.sums[t] = x;
        }
        __syncthreads();
    }
    s = sh.sums[0];
    lk_align* rec = a.rec + k;
    if (t == 0u) {
        if (rec->iters == 0u) {   // the search under T0
            rec->n_matched_first = s.n;
            rec->rmse_first = s.n ? sqrt(s.s2 / (double)s.n) : __longlong_as_double(0x7ff8000000000000ll);
        }
        if (s.n < 3ull) rec->status |= LK_ALIGN_FEW, a.done[k] = 2u;   // that search is final and T stays
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) bar[c] = s.p[c] / (double)s.n, bar[3 + c] = s.r[c] / (double)s.n;
        }
    }
    if (s.n < 3ull) return;
    __syncthreads();   // (sh.sums has been read by everyone, bar is written)
    double pbar[3], rbar[3], S[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) pbar[c] = bar[c], rbar[c] = bar[3 + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) S[c] = 0.0;
    for (unsigned long long i = t; i < n; i += 256ull) {
        const unsigned int j = a.q.nn_idx[b + i];
        if (j == 0xffffffffu) continue;
        const float4 p = qp[i], r = rp[j];
        lk_align_cov_term(S, pbar, rbar, p.x, p.y, p.z, r.x, r.y, r.z);
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) sh.cov[t][c] = S[c];
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int c = 0; c < 9; ++c) sh.cov[t][c] = sh.cov[t][c] + sh.cov[t + o][c];
        }
        __syncthreads();
    }
    if (t != 0u) return;
    double T[12], Tn[12], step_rot, step_trans;
#pragma unroll
    for (int c = 0; c < 9; ++c) S[c] = sh.cov[0][c], T[c] = rec->rot[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) T[9 + c] = rec->trans[c];
    lk_align_solve(S, pbar, rbar, Tn);
    lk_align_step(T, Tn, pbar, &step_rot, &step_trans);
#pragma unroll
    for (int c = 0; c < 9; ++c) rec->rot[c] = Tn[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) rec->trans[c] = Tn[9 + c];
    rec->step_rot = step_rot, rec->step_trans = step_trans, rec->iters += 1u;
    if (lk_align_converged(step_rot, step_trans, a.eps_rot, a.eps_trans)) rec->status |= LK_ALIGN_CONVERGED, a.done[k] = 1u;
}

// max_iter == 0: no solve has looked at the one search, so its figures come from the final lk_c2c record
__global__ void __launch_bounds__(256) lk_align_first_is_last_kernel(LkAlignCall a) {
    const unsigned int k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.q.n_pairs || a.rec[k].status != 0u) return;
    a.rec[k].n_matched_first = a.q.out[k].n_matched, a.rec[k].rmse_first = a.q.out[k].rmse;
}

// record off[c] + i of `in` -> entry rel[c] + i of `out` (rel = off - off[0]; in_first = in + off[0]): x y z moved under the cloud's T and rounded
// once to float32, w copied bit for bit.  One record per lane; a lane reads and writes the same index, so out == in_first is in place.
__global__ void __launch_bounds__(256) lk_clouds_transform_kernel(const float4* in_first, const unsigned long long* __restrict__ rel, unsigned int n_clouds,
                                                                  const double* __restrict__ T, float4* out, unsigned long long total) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= total) return;
    unsigned int lo = 0, hi = n_clouds;   // rel[lo] <= i < rel[hi]; among empty clouds the last one that starts at or before i
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (rel[mid] <= i) lo = mid;
        else hi = mid;
    }
    const float4 p = in_first[i];
    double m[3];
    lk_align_move(T + 12ull * lo, (double)p.x, (double)p.y, (double)p.z, m);
    out[i] = make_float4((float)m[0], (float)m[1], (float)m[2], p.w);
}
