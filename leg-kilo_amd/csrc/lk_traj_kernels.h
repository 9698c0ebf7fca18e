// lk_traj_kernels.h - absolute trajectory error of many trajectories against ground truth, on the device (lk_traj_ate_dev, lk_runs_ate_dev):
// tum.associate + tum.ate of leg-kilo_amd/tum.py without the trip of the trajectories to the host.  Compiled in lk_traj.hip only.
//
// One workgroup of one wave per trajectory; lane l owns the estimate samples l, l + 64, l + 128, ... in every pass, so a sum is the lanes' partial
// sums (each in ascending sample order) added by wave_sum / wave_sum_n: an order that depends on the trajectory's own samples alone - not on n_traj,
// not on where the trajectory stands in the call.  The passes of one launch:
//   stamps     both sides finite and not decreasing, else the trajectory is reported through LkTraj::bad and left out;
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

#define LK_TRAJ_NONE 0xffffffffu   // partner word of an estimate sample without a pair

struct LkTraj {
    const unsigned char *est_t, *est_p, *gt_t, *gt_p;   // first sample's stamp / position of either side
    unsigned long long est_stride, gt_stride;           // bytes from sample to sample
    const unsigned long long *est_off, *gt_off;         // [n_traj + 1] sample ranges (device copies of the caller's tables)
    unsigned long long part_base;                       // est_off[0]: partner[] starts at the call's first estimate sample
    unsigned int* partner;                              // [est_off[n_traj] - est_off[0]]
    lk_ate* out;                                        // [n_traj]
    unsigned int* bad;                                  // min over the refused trajectories of 2 r + side (0 estimate, 1 ground truth); 0xffffffff: none
    double max_dt;
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
    const unsigned long long e0 = a.est_off[r], ne = a.est_off[r + 1] - e0, g0 = a.gt_off[r], ng = a.gt_off[r + 1] - g0;
    const unsigned long long se = a.est_stride, sg = a.gt_stride;
    const unsigned char *et = a.est_t + e0 * se, *ep = a.est_p + e0 * se, *gt = a.gt_t + g0 * sg, *gp = a.gt_p + g0 * sg;
    unsigned int* part = a.partner + (e0 - a.part_base);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tr[3] = {0.0, 0.0, 0.0};

    // ---- stamps
    const bool ok_e = traj_stamps_ok(et, se, ne, lane), ok_g = traj_stamps_ok(gt, sg, ng, lane);
    if (!ok_e || !ok_g) {
        if (lane == 0) {
            atomicMin(a.bad, 2u * r + (ok_e ? 1u : 0u));
            traj_write(&a.out[r], nan, nan, nan, R, tr, 0, 0, 0);
        }
        return;
    }

    // ---- pair: partner words, the pair count, whether a paired position is not finite, and the lane's first pair
    unsigned long long cnt = 0, first = ~0ull;
    bool nonfinite = false;
    double fg[3] = {0.0, 0.0, 0.0}, fp[3] = {0.0, 0.0, 0.0};
    for (unsigned long long i = lane; i < ne; i += LK_WAVE) {
        unsigned int w = LK_TRAJ_NONE;
        if (ng) {
            double d;
            const unsigned long long j = traj_partner(gt, sg, ng, traj_ld(et, se, i), &d);
            if (d <= a.max_dt) w = (unsigned int)j;
        }
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
    double wmax = emax;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o, LK_WAVE));
    const unsigned long long worst = traj_wave_min_u64(emax == wmax ? imax : ~0ull);
    if (lane == 0) traj_write(&a.out[r], sqrt(s2 * inv_n), s1 * inv_n, wmax, R, tr, n_pairs, (unsigned int)worst, 0);
}
