// lk_relpose.h - one term of the relative pose error (lk_traj_rpe_dev / lk_runs_rpe_dev, lk_traj_kernels.h): the motion between two poses of the
// estimate against the motion between their two ground-truth partners, both expressed in the FIRST pose's own frame, so that one fixed rigid
// transform of a whole trajectory drops out.
//
// With (R, p) row-major body -> world:  dR = R_i^T R_k,  dp = R_i^T (p_k - p_i)                                       (lk_relpose_motion)
// and of the two motions (dRe, dpe), (dRg, dpg):  e_t = |dpe - dpg|,  E = dRg^T dRe,
//     s = 0.5 |(E21 - E12, E02 - E20, E10 - E01)|,  c = 0.5 (E00 + E11 + E22 - 1),  e_r = atan2(s, c)                  (lk_relpose_term)
// The matrices are used as given - no re-orthonormalisation: the figure is this formula on those bits.  atan2 of sine and cosine, not acos of the
// cosine alone: near c = 1 acos resolves 1.5e-8 rad, atan2 the angle itself.
// BOTH motions go through the one helper, a product always as a^T b with the sum ((k = 0) + (k = 1)) + (k = 2): equal poses on both sides give equal
// motions to the bit, E = D^T D then has E[i][j] and E[j][i] from the same products in the same order, s = 0 and e_t = 0 exactly.  No FMA is spelled
// out and the units that include this build with -ffp-contract=off, so the host build (tools/probes/relpose_host.cc, tests/test_rpe_host.py) rounds
// as the device does up to sqrt and atan2.  Plain C++ that compiles for the host as it stands, like lk_horn.h.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define LK_RELPOSE_HD __host__ __device__ __forceinline__
#define LK_RELPOSE_UNROLL _Pragma("unroll")
#else
#define LK_RELPOSE_HD inline
#define LK_RELPOSE_UNROLL
#endif

// out = a^T b (3 x 3, row-major)
LK_RELPOSE_HD void lk_relpose_atb(const double* a, const double* b, double* out) {
LK_RELPOSE_UNROLL
    for (int i = 0; i < 3; ++i) {
LK_RELPOSE_UNROLL
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
    }
}

// the motion from pose (R0, p0) to pose (R1, p1) in the first pose's frame
LK_RELPOSE_HD void lk_relpose_motion(const double* R0, const double* p0, const double* R1, const double* p1, double* dR, double* dp) {
    lk_relpose_atb(R0, R1, dR);
    const double d0 = p1[0] - p0[0], d1 = p1[1] - p0[1], d2 = p1[2] - p0[2];
LK_RELPOSE_UNROLL
    for (int i = 0; i < 3; ++i) dp[i] = (R0[i] * d0 + R0[3 + i] * d1) + R0[6 + i] * d2;
}

// the estimate's motion against the ground truth's: translation error, sine and cosine of the rotation error
LK_RELPOSE_HD void lk_relpose_term(const double* dRe, const double* dpe, const double* dRg, const double* dpg, double* e_t, double* s, double* c) {
    const double x = dpe[0] - dpg[0], y = dpe[1] - dpg[1], z = dpe[2] - dpg[2];
    *e_t = sqrt((x * x + y * y) + z * z);
    double E[9];
    lk_relpose_atb(dRg, dRe, E);
    const double v0 = E[7] - E[5], v1 = E[2] - E[6], v2 = E[3] - E[1];
    *s = 0.5 * sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    *c = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
}

// four poses in - estimate i, estimate k, ground truth a, ground truth b - e_t, s, c out
LK_RELPOSE_HD void lk_relpose_eval(const double* Ri, const double* pi, const double* Rk, const double* pk, const double* Qa, const double* ga,
                                   const double* Qb, const double* gb, double* e_t, double* s, double* c) {
    double dRe[9], dpe[3], dRg[9], dpg[3];
    lk_relpose_motion(Ri, pi, Rk, pk, dRe, dpe);
    lk_relpose_motion(Qa, ga, Qb, gb, dRg, dpg);
    lk_relpose_term(dRe, dpe, dRg, dpg, e_t, s, c);
}
