// lk_traj_kernels.h - absolute trajectory error of many trajectories against ground truth, on the device (lk_traj_ate_dev, lk_runs_ate_dev):
// tum.associate + tum.ate of leg-kilo_amd/tum.py without the trip of the trajectories to the host - and, further down, their relative pose error
// (lk_traj_rpe_dev, lk_runs_rpe_dev: tum.rpe).  Compiled in lk_traj.hip only.
//
// One workgroup of one wave per trajectory; lane l owns the estimate samples l, l + 64, l + 128, ... in every pass, so a sum is the lanes' partial
// sums (each in ascending sample order) added by wave_sum / wave_sum_n: an order that depends on the trajectory's own samples alone - not on n_traj,
// not on where the trajectory stands in the call.  The passes of one launch:
//   stamps     both sides finite and not decreasing, else the trajectory is reported through LkTrajTab::bad and left out;
//   pair       partner j(i) = the ground-truth sample that minimises fabs(t_est[i] - t_gt[j]), the earliest on equal distance (a lower bound over the
//              sorted stamps, the two neighbours compared, then the first sample that is as close as the winner); kept when that distance is
//              <= max_dt; the partner index goes to scratch (4 bytes per sample, re-read by the lane that wrote it), the later passes do not search again;
//   centroid   means of the paired g and p, summed relative to the FIRST pair's positions (the sums stay small where the trajectory lies 600 km out);
//   covariance the 3 x 3 cross-covariance of the centred pairs (never sum xy - n mean mean);
//   solve      lk_horn.h on wave-uniform values (every lane computes the same R: no broadcast, and no lane waits less than the one that would solve);
//   residual   e_i = |(g_i - cg) - R (p_i - cp)|: sum of squares, sum, maximum with its first index.
// Without LK_ATE_ALIGN only pair and residual run, with e_i = |g_i - p_i| on the values as they lie.
#pragma once
#include "lk_horn.h"
#include "lk_relpose.h"

#define LK_TRAJ_NONE 0xffffffffu   // partner word of an estimate sample without a pair

struct LkTrajTab {   // what both kernels read the same way (LkTraj, LkTrajRpe: this and their own members)
    const unsigned char *est_t, *est_p, *gt_t, *gt_p;   // first sample's stamp / position of either side
    unsigned long long est_stride, gt_stride;           // bytes from sample to sample
    const unsigned long long *est_off, *gt_off;         // [n_traj + 1] sample ranges (device copies of the caller's tables)
    unsigned long long part_base;                       // est_off[0]: partner[] starts at the call's first estimate sample
    unsigned int* partner;                              // [est_off[n_traj] - est_off[0]]
    unsigned int* bad;                                  // min over the refused trajectories of 2 r + side (0 estimate, 1 ground truth); 0xffffffff: none
    double max_dt;
};
struct LkTraj {
    LkTrajTab t;
    lk_ate* out;   // [n_traj]
    unsigned int flags;
};

__device__ __forceinline__ double traj_ld(const unsigned char* base, unsigned long long stride, unsigned long long k, int c = 0) {
    return reinterpret_cast<const double*>(base + k * stride)[c];
}
__device__ __forceinline__ unsigned long long traj_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, LK_WAVE);
    return v;
}
__device__ __forceinline__ unsigned long long traj_wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, LK_WAVE);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ double traj_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, LK_WAVE));
    return v;
}
// the first index that holds the wave's maximum: v, i - the lane's own maximum and its first index (~0: none), wmax - traj_wave_max(v)
__device__ __forceinline__ unsigned long long traj_wave_first_max(double v, double wmax, unsigned long long i) { return traj_wave_min_u64(v == wmax ? i : ~0ull); }
__device__ __forceinline__ bool traj_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// stamps of one side: finite and not decreasing (whole wave; the answer is uniform)
__device__ __forceinline__ bool traj_stamps_ok(const unsigned char* t, unsigned long long stride, unsigned long long n, int lane) {
    bool bad = false;
    for (unsigned long long i = lane; i < n; i += LK_WAVE) {
        const double v = traj_ld(t, stride, i);
        bad = bad || !traj_finite(v) || (i > 0 && v < traj_ld(t, stride, i - 1));
    }
    return __ballot(bad) == 0;
}

// first k in [0, n) with t[k] >= v (n: none)
__device__ __forceinline__ unsigned long long traj_lower_bound(const unsigned char* t, unsigned long long stride, unsigned long long n, double v) {
    unsigned long long lo = 0, hi = n;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (traj_ld(t, stride, mid) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// partner of the stamp te among m >= 1 sorted ground-truth stamps: the minimiser of fabs(te - t[j]), the earliest of equals; *dist: that distance
__device__ __forceinline__ unsigned long long traj_partner(const unsigned char* t, unsigned long long stride, unsigned long long m, double te, double* dist) {
    const unsigned long long lb = traj_lower_bound(t, stride, m, te);
    if (lb == 0) {
        *dist = fabs(te - traj_ld(t, stride, 0));
        return 0;
    }
    const double db = fabs(te - traj_ld(t, stride, lb - 1));
    if (lb < m) {
        const double da = fabs(te - traj_ld(t, stride, lb));
        if (da < db) {   // every sample in front of lb is at least db away
            *dist = da;
            return lb;
        }
    }
    // lb - 1 wins.  In front of it the rounded distances do not increase with the index, so the first sample that is exactly as close - an equal
    // stamp, or one the subtraction cannot tell from it - is found by bisection
    unsigned long long lo = 0, hi = lb - 1;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (fabs(te - traj_ld(t, stride, mid)) > db) lo = mid + 1; else hi = mid;
    }
    *dist = db;
    return lo;
}

// ---- the prologue both kernels share
struct LkTrajRange {   // trajectory r of a call: its sample counts and strides, its first sample on either side, its partner words
    unsigned long long e0, ne, g0, ng, se, sg;
    const unsigned char *et, *ep, *gt, *gp;
    unsigned int* part;
};
__device__ __forceinline__ LkTrajRange traj_range(const LkTrajTab& t, unsigned int r) {
    const unsigned long long e0 = t.est_off[r], g0 = t.gt_off[r], se = t.est_stride, sg = t.gt_stride;
    return {e0, t.est_off[r + 1] - e0, g0, t.gt_off[r + 1] - g0, se, sg, t.est_t + e0 * se, t.est_p + e0 * se, t.gt_t + g0 * sg, t.gt_p + g0 * sg,
            t.partner + (e0 - t.part_base)};
}
// the stamps pass; false (uniform): refused through LkTrajTab::bad - the caller writes its empty record from lane 0 and leaves
__device__ __forceinline__ bool traj_stamps(const LkTrajTab& t, const LkTrajRange& v, unsigned int r, int lane) {
    const bool ok_e = traj_stamps_ok(v.et, v.se, v.ne, lane), ok_g = traj_stamps_ok(v.gt, v.sg, v.ng, lane);
    if (ok_e && ok_g) return true;
    if (lane == 0) atomicMin(t.bad, 2u * r + (ok_e ? 1u : 0u));
    return false;
}
// the partner word of estimate sample i: traj_partner, kept when it lies within max_dt
__device__ __forceinline__ unsigned int traj_partner_word(const LkTrajRange& v, double max_dt, unsigned long long i) {
    if (!v.ng) return LK_TRAJ_NONE;
    double d;
    const unsigned long long j = traj_partner(v.gt, v.sg, v.ng, traj_ld(v.et, v.se, i), &d);
    return d <= max_dt ? (unsigned int)j : LK_TRAJ_NONE;
}

__device__ __forceinline__ void traj_write(lk_ate* o, double rmse, double mean, double mx, const double* R, const double* tr, unsigned long long n_pairs,
                                           unsigned int worst, unsigned int status) {
    o->rmse = rmse, o->mean = mean, o->max = mx;
#pragma unroll
    for (int k = 0; k < 9; ++k) o->rot[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o->trans[k] = tr[k];
    o->n_pairs = n_pairs, o->worst = worst, o->status = status;
}

__global__ void __launch_bounds__(LK_WAVE) lk_traj_ate_kernel(LkTraj a) {
    const unsigned int r = blockIdx.x;
    const int lane = threadIdx.x;
    const LkTrajRange v = traj_range(a.t, r);
    const unsigned long long ne = v.ne, se = v.se, sg = v.sg;
    const unsigned char *ep = v.ep, *gp = v.gp;
    unsigned int* part = v.part;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tr[3] = {0.0, 0.0, 0.0};

    // ---- stamps
    if (!traj_stamps(a.t, v, r, lane)) {
        if (lane == 0) traj_write(&a.out[r], nan, nan, nan, R, tr, 0, 0, 0);
        return;
    }

    // ---- pair: partner words, the pair count, whether a paired position is not finite, and the lane's first pair
    unsigned long long cnt = 0, first = ~0ull;
    bool nonfinite = false;
    double fg[3] = {0.0, 0.0, 0.0}, fp[3] = {0.0, 0.0, 0.0};
    for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
        const unsigned int w = traj_partner_word(v, a.t.max_dt, i);
        part[i] = w;
        if (w != LK_TRAJ_NONE) {
            double g[3], p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = traj_ld(gp, sg, w, c), p[c] = traj_ld(ep, se, i, c);
            nonfinite = nonfinite || !(traj_finite(g[0]) && traj_finite(g[1]) && traj_finite(g[2]) && traj_finite(p[0]) && traj_finite(p[1]) && traj_finite(p[2]));
            if (cnt == 0) {
                first = i;
#pragma unroll
                for (int c = 0; c < 3; ++c) fg[c] = g[c], fp[c] = p[c];
            }
            ++cnt;
        }
    }
    const unsigned long long n_pairs = traj_wave_sum_u64(cnt);
    if (n_pairs == 0 || __ballot(nonfinite) != 0) {
        if (lane == 0) traj_write(&a.out[r], nan, nan, nan, R, tr, n_pairs, 0, n_pairs ? LK_ATE_NONFINITE : 0u);
        return;
    }
    const double inv_n = 1.0 / (double)n_pairs;

    // what the residual pass takes off g and p, in the two steps of the covariance pass; without LK_ATE_ALIGN all of it is zero and R the identity,
    // and (g - 0 - 0) - (1 p + 0 + 0) is g - p to the bit
    double og[3] = {0.0, 0.0, 0.0}, op[3] = {0.0, 0.0, 0.0}, mg[3] = {0.0, 0.0, 0.0}, mp[3] = {0.0, 0.0, 0.0};
    if (a.flags & LK_ATE_ALIGN) {
        // ---- centroid, relative to the first pair's positions (its lane hands them to the others)
        const int src = (int)(traj_wave_min_u64(first) & (LK_WAVE - 1));
#pragma unroll
        for (int c = 0; c < 3; ++c) og[c] = __shfl(fg[c], src, LK_WAVE), op[c] = __shfl(fp[c], src, LK_WAVE);
        double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
            const unsigned int w = part[i];
            if (w == LK_TRAJ_NONE) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) s6[c] += traj_ld(gp, sg, w, c) - og[c], s6[3 + c] += traj_ld(ep, se, i, c) - op[c];
        }
        wave_sum_n<6>(s6);
#pragma unroll
        for (int c = 0; c < 3; ++c) mg[c] = s6[c] * inv_n, mp[c] = s6[3 + c] * inv_n;
        // ---- cross-covariance of the centred pairs: S[3 a + b] = sum p_a g_b
        double s9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
            const unsigned int w = part[i];
            if (w == LK_TRAJ_NONE) continue;
            double g[3], p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = (traj_ld(gp, sg, w, c) - og[c]) - mg[c], p[c] = (traj_ld(ep, se, i, c) - op[c]) - mp[c];
#pragma unroll
            for (int k = 0; k < 9; ++k) s9[k] += p[k / 3] * g[k % 3];
        }
        wave_sum_n<9>(s9);
        // ---- solve (uniform), t = cg - R cp with the centroids cg = og + mg, cp = op + mp
        lk_horn_rotation(s9, R);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double cp0 = op[0] + mp[0], cp1 = op[1] + mp[1], cp2 = op[2] + mp[2];
            tr[c] = (og[c] + mg[c]) - ((R[3 * c] * cp0 + R[3 * c + 1] * cp1) + R[3 * c + 2] * cp2);
        }
    }
    // ---- residual: e_i = |(g_i - cg) - R (p_i - cp)|
    double s2 = 0.0, s1 = 0.0, emax = -1.0;
    unsigned long long imax = ~0ull;
    for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
        const unsigned int w = part[i];
        if (w == LK_TRAJ_NONE) continue;
        double g[3], p[3], d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = (traj_ld(gp, sg, w, c) - og[c]) - mg[c], p[c] = (traj_ld(ep, se, i, c) - op[c]) - mp[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = g[c] - ((R[3 * c] * p[0] + R[3 * c + 1] * p[1]) + R[3 * c + 2] * p[2]);
        const double e2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], e = sqrt(e2);
        s2 += e2, s1 += e;
        if (e > emax) emax = e, imax = i;   // (ascending i: the lane's first of equal maxima)
    }
    s2 = wave_sum(s2), s1 = wave_sum(s1);
    const double wmax = traj_wave_max(emax);
    const unsigned long long worst = traj_wave_first_max(emax, wmax, imax);
    if (lane == 0) traj_write(&a.out[r], sqrt(s2 * inv_n), s1 * inv_n, wmax, R, tr, n_pairs, (unsigned int)worst, 0);
}

// ---- relative pose error (lk_traj_rpe_dev, lk_runs_rpe_dev): the same launch shape, lane ownership and helpers; the per-term arithmetic is lk_relpose.h.
// The passes of one launch:
//   stamps     as above;
//   pair       partner words to scratch, n_pairs counted (no pose is read here: a sample's pose is touched only by a term it takes part in);
//   -- __syncthreads(): the term pass reads the partner word of sample k(i), which ANOTHER lane wrote.  One wave is the whole workgroup, so the
//      workgroup barrier with its workgroup-scope fence orders that store before the load (both lanes sit on one CU and share its L1: no agent scope)
//   terms      k(i): in seconds mode the first sample behind i with t_est[k] >= t_est[i] + delta (traj_lower_bound over the samples behind i - never i
//              itself or an earlier equal stamp), in index mode i + step; a term when i and k both have partners.  The estimate's two poses are
//              loaded and reduced to their motion (12 doubles) before the ground truth's two are loaded: at most two poses are live beside a motion;
//   combine    wave_sum of the lanes' sums (each in ascending i), the maxima by shuffles, the worst index by traj_wave_first_max - the ATE kernel's idiom, once
//              per figure.
struct LkTrajRpe {
    LkTrajTab t;
    const unsigned char *est_r, *gt_r;   // first sample's rotation of either side
    lk_rpe* out;                         // [n_traj]
    double delta;
    unsigned long long step;   // LK_RPE_INDEX: (uint64)delta
    unsigned int flags;
};

__device__ __forceinline__ void traj_rpe_write(lk_rpe* o, const double* fig, unsigned long long n_terms, unsigned long long n_pairs, unsigned int worst_t,
                                               unsigned int worst_r, unsigned int status) {
    o->trans_rmse = fig[0], o->trans_mean = fig[1], o->trans_max = fig[2];
    o->rot_rmse = fig[3], o->rot_mean = fig[4], o->rot_max = fig[5];
    o->n_terms = n_terms, o->n_pairs = n_pairs;
    o->worst_trans = worst_t, o->worst_rot = worst_r, o->status = status, o->reserved = 0;
}

// one pose: 3 position and 9 rotation doubles; false when one of them is not finite
__device__ __forceinline__ bool traj_ld_pose(const unsigned char* p, const unsigned char* r, unsigned long long stride, unsigned long long k, double* pos, double* rot) {
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = traj_ld(p, stride, k, c), fin = fin && traj_finite(pos[c]);
#pragma unroll
    for (int c = 0; c < 9; ++c) rot[c] = traj_ld(r, stride, k, c), fin = fin && traj_finite(rot[c]);
    return fin;
}

__global__ void __launch_bounds__(LK_WAVE) lk_traj_rpe_kernel(LkTrajRpe a) {
    const unsigned int r = blockIdx.x;
    const int lane = threadIdx.x;
    const LkTrajRange v = traj_range(a.t, r);
    const unsigned long long ne = v.ne, se = v.se, sg = v.sg;
    const unsigned char *et = v.et, *ep = v.ep, *er = a.est_r + v.e0 * se, *gp = v.gp, *gr = a.gt_r + v.g0 * sg;
    unsigned int* part = v.part;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double fig[6] = {nan, nan, nan, nan, nan, nan};

    // ---- stamps
    if (!traj_stamps(a.t, v, r, lane)) {
        if (lane == 0) traj_rpe_write(&a.out[r], fig, 0, 0, 0, 0, 0);
        return;
    }

    // ---- pair
    unsigned long long cnt = 0;
    for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
        const unsigned int w = traj_partner_word(v, a.t.max_dt, i);
        part[i] = w;
        cnt += w != LK_TRAJ_NONE;
    }
    const unsigned long long n_pairs = traj_wave_sum_u64(cnt);
    __syncthreads();   // part[k(i)] below is another lane's word (the exit above is uniform: every lane of the wave arrives)

    // ---- terms
    unsigned long long terms = 0, imax_t = ~0ull, imax_r = ~0ull;
    double t2 = 0.0, t1 = 0.0, tmax = -1.0, r2 = 0.0, r1 = 0.0, rmax = -1.0;
    bool nonfinite = false;
    for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
        unsigned long long k;
        if (a.flags & LK_RPE_INDEX) {
            k = i + a.step;
        } else {
            const double target = traj_ld(et, se, i) + a.delta;
            k = (i + 1) + traj_lower_bound(et + (i + 1) * se, se, ne - (i + 1), target);
        }
        if (k >= ne) continue;
        const unsigned int wa = part[i], wb = part[k];
        if (wa == LK_TRAJ_NONE || wb == LK_TRAJ_NONE) continue;
        ++terms;
        double dRe[9], dpe[3], dRg[9], dpg[3], e_t, s, c;
        bool fin;
        {
            double p0[3], R0[9], p1[3], R1[9];
            fin = traj_ld_pose(ep, er, se, i, p0, R0);
            fin = traj_ld_pose(ep, er, se, k, p1, R1) && fin;
            lk_relpose_motion(R0, p0, R1, p1, dRe, dpe);
        }
        {
            double p0[3], R0[9], p1[3], R1[9];
            fin = traj_ld_pose(gp, gr, sg, wa, p0, R0) && fin;
            fin = traj_ld_pose(gp, gr, sg, wb, p1, R1) && fin;
            lk_relpose_motion(R0, p0, R1, p1, dRg, dpg);
        }
        if (!fin) {
            nonfinite = true;
            continue;
        }
        lk_relpose_term(dRe, dpe, dRg, dpg, &e_t, &s, &c);
        const double e_r = atan2(s, c);
        t2 += e_t * e_t, t1 += e_t;
        r2 += e_r * e_r, r1 += e_r;
        if (e_t > tmax) tmax = e_t, imax_t = i;   // (ascending i: the lane's first of equal maxima)
        if (e_r > rmax) rmax = e_r, imax_r = i;
    }
    const unsigned long long n_terms = traj_wave_sum_u64(terms);
    if (n_terms == 0 || __ballot(nonfinite) != 0) {
        if (lane == 0) traj_rpe_write(&a.out[r], fig, n_terms, n_pairs, 0, 0, n_terms ? LK_RPE_NONFINITE : 0u);
        return;
    }

    // ---- combine
    const double inv_n = 1.0 / (double)n_terms;
    t2 = wave_sum(t2), t1 = wave_sum(t1), r2 = wave_sum(r2), r1 = wave_sum(r1);
    const double wt = traj_wave_max(tmax), wr = traj_wave_max(rmax);
    const unsigned long long worst_t = traj_wave_first_max(tmax, wt, imax_t), worst_r = traj_wave_first_max(rmax, wr, imax_r);
    fig[0] = sqrt(t2 * inv_n), fig[1] = t1 * inv_n, fig[2] = wt;
    fig[3] = sqrt(r2 * inv_n), fig[4] = r1 * inv_n, fig[5] = wr;
    if (lane == 0) traj_rpe_write(&a.out[r], fig, n_terms, n_pairs, (unsigned int)worst_t, (unsigned int)worst_r, 0);
}
