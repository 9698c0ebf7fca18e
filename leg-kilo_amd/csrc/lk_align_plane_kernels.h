// lk_align_plane_kernels.h - the solve of the point-to-plane alignment (lk_clouds_align_plane_dev; the arithmetic is lk_align_plane.h's, shared with
// the host probe).  The loop, the pair's record and `done` word, lk_align_init_kernel, lk_align_search_kernel and the final lk_c2c_reduce_kernel are
// lk_align_kernels.h's as they stand: matching ignores the normals.  What differs is the kernel between two searches, and that it also runs after
// the LAST search of the call (`last`), because every pair's final search gets its plane figures from a first pass:
//     done 0, not last   first pass; fewer than 6 used points or an unobserved direction close the pair (this search was its final one, T stays),
//                        otherwise the second pass, the solve, the step and the stop decision
//     done 0, last       first pass only, the pair is closed
//     done 1             the search in front was the final one: first pass only, the pair is closed
//     done 2             nothing
// One block of 256 threads per pair, built like lk_align_solve_kernel: lane t adds the points t, t + 256, ... in ascending order, then a fixed tree;
// thread 0 solves.  27 doubles a lane in the second pass: 55 296 B of LDS.
#pragma once
#include "lk_align_kernels.h"
#include "lk_align_plane.h"

__global__ void __launch_bounds__(256) lk_align_plane_solve_kernel(LkAlignCall a, const float4* r_nrm, lk_align_plane* pl, int first, int last) {
    __shared__ union {
        LkPlaneSums sums[256];
        double hg[256][27];
    } sh;
    __shared__ double bar[3];
    __shared__ double Tsh[12];
    const unsigned int k = blockIdx.x, t = threadIdx.x;
    const unsigned int was = a.done[k];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    lk_align* rec = a.rec + k;
    if (t < 12u) Tsh[t] = t < 9u ? rec->rot[t] : rec->trans[t - 9u];
    __syncthreads();   // (every thread has read the word and T before thread 0 may write either)
    if (first && t == 0u) pl[k].rmse_plane_first = nan, pl[k].rmse_plane = nan, pl[k].n_used_first = 0ull, pl[k].n_used = 0ull;
    if (was == 2u) return;
    const unsigned int qc = a.q.pair_q[k], rc = a.q.pair_r[k];
    const unsigned long long b = a.q.nn_off[k], n = a.q.nn_off[k + 1] - b;
    const float4* qp = a.q.q_pts + a.q.q_off[qc];
    const float4* rp = a.r_pts + a.r_off64[rc];
    const float4* np = r_nrm + a.r_off64[rc];
    double T[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) T[c] = Tsh[c];
    LkPlaneSums s;
    lk_plane_sums_zero(&s);
    for (unsigned long long i = t; i < n; i += 256ull) {
        const unsigned int j = a.q.nn_idx[b + i];
        if (j == 0xffffffffu) continue;
        const float4 p = qp[i], r = rp[j], nr = np[j];
        lk_plane_sums_term(&s, T, a.q.nn_d2[b + i], p.x, p.y, p.z, r.x, r.y, r.z, nr.x, nr.y, nr.z);
    }
    sh.sums[t] = s;
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            LkPlaneSums x = sh.sums[t];
            lk_plane_sums_merge(&x, sh.sums[t + o]);
            sh.sums[t] = x;
        }
        __syncthreads();
    }
    s = sh.sums[0];
    const bool closing = was == 1u || last != 0;
    const bool few = s.nu < LK_ALIGN_PLANE_MIN_USED;
    if (t == 0u) {
        const double rp1 = s.nu ? sqrt(s.e2 / (double)s.nu) : nan;
        if (rec->iters == 0u) {   // the search under T0
            rec->n_matched_first = s.n;
            rec->rmse_first = s.n ? sqrt(s.s2 / (double)s.n) : nan;
            pl[k].rmse_plane_first = rp1, pl[k].n_used_first = s.nu;
        }
        if (closing || few) {   // this search is the pair's final one
            pl[k].rmse_plane = rp1, pl[k].n_used = s.nu;
            if (!closing) rec->status |= LK_ALIGN_FEW;
            a.done[k] = 2u;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) bar[c] = s.m[c] / (double)s.nu;
        }
    }
    if (closing || few) return;
    __syncthreads();   // (sh.sums has been read by everyone, bar is written)
    double mbar[3], Hg[27];
#pragma unroll
    for (int c = 0; c < 3; ++c) mbar[c] = bar[c];
#pragma unroll
    for (int c = 0; c < 27; ++c) Hg[c] = 0.0;
    for (unsigned long long i = t; i < n; i += 256ull) {
        const unsigned int j = a.q.nn_idx[b + i];
        if (j == 0xffffffffu) continue;
        const float4 p = qp[i], r = rp[j], nr = np[j];
        lk_plane_rows_term(Hg, T, mbar, p.x, p.y, p.z, r.x, r.y, r.z, nr.x, nr.y, nr.z);
    }
#pragma unroll
    for (int c = 0; c < 27; ++c) sh.hg[t][c] = Hg[c];
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int c = 0; c < 27; ++c) sh.hg[t][c] = sh.hg[t][c] + sh.hg[t + o][c];
        }
        __syncthreads();
    }
    if (t != 0u) return;
    double x[6], Tn[12], pbar[3], step_rot, step_trans;
#pragma unroll
    for (int c = 0; c < 27; ++c) Hg[c] = sh.hg[0][c];
    if (!lk_plane_solve(Hg, x)) {   // an unobserved direction: this search is final and T stays
        rec->status |= LK_ALIGN_DEGENERATE;
        pl[k].rmse_plane = s.nu ? sqrt(s.e2 / (double)s.nu) : nan, pl[k].n_used = s.nu;
        a.done[k] = 2u;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pbar[c] = s.p[c] / (double)s.nu;
    lk_plane_update(T, x, mbar, Tn);
    lk_align_step(T, Tn, pbar, &step_rot, &step_trans);
#pragma unroll
    for (int c = 0; c < 9; ++c) rec->rot[c] = Tn[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) rec->trans[c] = Tn[9 + c];
    rec->step_rot = step_rot, rec->step_trans = step_trans, rec->iters += 1u;
    if (lk_align_converged(step_rot, step_trans, a.eps_rot, a.eps_trans)) rec->status |= LK_ALIGN_CONVERGED, a.done[k] = 1u;
}
