// lk_align.h - the arithmetic of the rigid alignment of a query cloud to a reference cloud (lk_clouds_align_dev / lk_clouds_transform_dev,
// lk_align_kernels.h) that the device route and its CPU twin (tools/probes/align_host.cc, tests/test_align_host.py) share: the move of a point under
// T = (R, t), the nearest-neighbour search of lk_c2c.h for a query coordinate that is a DOUBLE (the moved point is never rounded to float32), the
// terms of the two passes of a solve (centroids first, centred products second), the step between two transforms and the stop decision.
//
// The search is lk_c2c.h's: its walk and its visitor take the query coordinate as it comes, and the double-coordinate overloads of lk_c2c_cell,
// lk_c2c_axis and lk_c2c_d2 stand there in front of the walk, with the reason why the 27-cell argument does not ask how many bits the query
// coordinate has.  What this header adds to the search is the move in front of it and the guard: a moved point is searched only when it is finite
// and |m / max_dist| < 2^30 per axis (lk_align_in_range), so its cell and a difference of two cells stay inside a long long and an int as there.
// No FMA is spelled out and the units that include this build with -ffp-contract=off; the host build rounds as the device does up to sqrt and atan2.
// Plain C++ that compiles for the host as it stands, like lk_c2c.h.
#pragma once
#include "lk_c2c.h"
#include "lk_horn.h"
#if defined(__HIPCC__)
#define LK_ALIGN_UNROLL _Pragma("unroll")
#else
#define LK_ALIGN_UNROLL
#endif

// m = R p + t, T = nine row-major doubles of R, then t: two products summed, the third added, then t - each rounded
LK_C2C_HD void lk_align_move(const double* T, double x, double y, double z, double* m) {
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) m[a] = ((T[3 * a] * x + T[3 * a + 1] * y) + T[3 * a + 2] * z) + T[9 + a];
}
// the range guard of a moved point: finite and below 2^30 cells of max_dist on every axis (false for NaN and infinity)
LK_C2C_HD bool lk_align_in_range(const double* m, double max_dist) {
    return fabs(m[0] / max_dist) < 1073741824.0 && fabs(m[1] / max_dist) < 1073741824.0 && fabs(m[2] / max_dist) < 1073741824.0;
}
LK_C2C_HD bool lk_align_finite12(const double* T) {
    bool ok = true;
    for (int k = 0; k < 12; ++k) ok = ok && (fabs(T[k]) <= 1.79769313486231570815e308);
    return ok;
}

// one query point under T against one reference cloud: moved, guarded, searched (lk_c2c_search on the double coordinates).
// LK_ALIGN_NO_GUARD (test aid of the host probe only): the search without the range guard.  By brute force the guard changes no result (a float32
// reference point in range lies 64 max_dist or more inside the bound); what it protects is lk_c2c_cell's conversion of floor(m / edge) to an
// integer, which is undefined from 2^63 on - the probe's sanitizers tell.
LK_C2C_HD void lk_align_search(const double* T, float x, float y, float z, double max_dist, const LkC2cGrid& g, const unsigned int* keys,
                               const LkC2cRec* recs, unsigned int n, double reach2, unsigned int* j, double* d2) {
    double m[3];
    lk_align_move(T, (double)x, (double)y, (double)z, m);
    *j = 0xffffffffu, *d2 = INFINITY;
#ifdef LK_ALIGN_NO_GUARD
    lk_c2c_search(m[0], m[1], m[2], g, keys, recs, n, reach2, j, d2);
#else
    if (lk_align_in_range(m, max_dist)) lk_c2c_search(m[0], m[1], m[2], g, keys, recs, n, reach2, j, d2);
#endif
}

// ---- the solve.  First pass, per matched point: the count, d2 (the figures of that search) and the two coordinate sums of the ORIGINAL points
struct LkAlignSums {
    double s2, p[3], r[3];
    unsigned long long n;
};
LK_C2C_HD void lk_align_sums_zero(LkAlignSums* s) {
    s->s2 = 0.0, s->n = 0ull;
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) s->p[a] = 0.0, s->r[a] = 0.0;
}
LK_C2C_HD void lk_align_sums_term(LkAlignSums* s, double d2, float px, float py, float pz, float rx, float ry, float rz) {
    s->s2 = s->s2 + d2, s->n += 1ull;
    s->p[0] = s->p[0] + (double)px, s->p[1] = s->p[1] + (double)py, s->p[2] = s->p[2] + (double)pz;
    s->r[0] = s->r[0] + (double)rx, s->r[1] = s->r[1] + (double)ry, s->r[2] = s->r[2] + (double)rz;
}
LK_C2C_HD void lk_align_sums_merge(LkAlignSums* x, const LkAlignSums& y) {
    x->s2 = x->s2 + y.s2, x->n += y.n;
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) x->p[a] = x->p[a] + y.p[a], x->r[a] = x->r[a] + y.r[a];
}
// second pass, per matched point: S[3a + b] += (p - pbar)_a (r - rbar)_b
LK_C2C_HD void lk_align_cov_term(double* S, const double* pbar, const double* rbar, float px, float py, float pz, float rx, float ry, float rz) {
    const double u[3] = {(double)px - pbar[0], (double)py - pbar[1], (double)pz - pbar[2]};
    const double v[3] = {(double)rx - rbar[0], (double)ry - rbar[1], (double)rz - rbar[2]};
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) {
LK_ALIGN_UNROLL
        for (int b = 0; b < 3; ++b) S[3 * a + b] = S[3 * a + b] + u[a] * v[b];
    }
}
// T' from the centroids and the centred products: R' = lk_horn_rotation(S), t' = rbar - R' pbar
LK_C2C_HD void lk_align_solve(const double* S, const double* pbar, const double* rbar, double* T) {
    lk_horn_rotation(S, T);
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) T[9 + a] = rbar[a] - ((T[3 * a] * pbar[0] + T[3 * a + 1] * pbar[1]) + T[3 * a + 2] * pbar[2]);
}
// the step from T to T' (Tn): the angle of E = R' R^T with lk_relpose.h's atan2 form - s = 0.5 |(E21 - E12, E02 - E20, E10 - E01)|,
// c = 0.5 (trace E - 1) - and the distance the query centroid moves.  T' == T to the bit gives E[i][j] and E[j][i] from the same products in the
// same order: both steps are exactly 0.
LK_C2C_HD void lk_align_step(const double* T, const double* Tn, const double* pbar, double* step_rot, double* step_trans) {
    double E[9];
LK_ALIGN_UNROLL
    for (int i = 0; i < 3; ++i) {
LK_ALIGN_UNROLL
        for (int j = 0; j < 3; ++j) E[3 * i + j] = (Tn[3 * i] * T[3 * j] + Tn[3 * i + 1] * T[3 * j + 1]) + Tn[3 * i + 2] * T[3 * j + 2];
    }
    const double v0 = E[7] - E[5], v1 = E[2] - E[6], v2 = E[3] - E[1];
    const double s = 0.5 * sqrt((v0 * v0 + v1 * v1) + v2 * v2), c = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
    *step_rot = atan2(s, c);
    double a[3], b[3];
    lk_align_move(Tn, pbar[0], pbar[1], pbar[2], a);
    lk_align_move(T, pbar[0], pbar[1], pbar[2], b);
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    *step_trans = sqrt((x * x + y * y) + z * z);
}
// the stop decision: both steps at or below their eps
LK_C2C_HD bool lk_align_converged(double step_rot, double step_trans, double eps_rot, double eps_trans) {
    return step_rot <= eps_rot && step_trans <= eps_trans;
}
