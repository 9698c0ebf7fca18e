// lk_align_plane.h - the arithmetic of the point-to-plane alignment of a query cloud to a reference cloud with per-point normals
// (lk_clouds_align_plane_dev, lk_align_plane_kernels.h) that the device route and its CPU twin (tools/probes/align_plane_host.cc,
// tests/test_plane_host.py) share, over lk_align.h: the search, the move, the step and the stop decision are that file's, unchanged.  Here: the
// terms of the two passes of a linearised solve (centroids and the plane residual first, the 6 x 6 normal equations about the moved centroid
// second), the scaled Cholesky solve that reports an unobserved direction instead of stepping along it, and the update of T.
//
// A matched point is USED when its reference normal has three finite components; the normal is taken as given (not normalised, w never read).
//   e_i = (nx*dx + ny*dy) + nz*dz, d = m_i - r_j(i) per axis, m_i = lk_align_move(T, p_i)
//   a_i = (c_i x n, n), c_i = m_i - mbar;  H = sum a a^T (21 upper terms, row-major),  g = sum a e
//   x = -D (D H D)^-1 D g = (omega, v),  D = diag(H)^(-1/2): the increment is the rotation omega ABOUT mbar, then the shift v
// The rows are centred on mbar, so the sums carry rounding of order 2^-53 extent^2 wherever the clouds lie.
// No FMA is spelled out and the units that include this build with -ffp-contract=off.  Plain C++ that compiles for the host as it stands.
#pragma once
#include "lk_align.h"

#define LK_ALIGN_PLANE_MIN_USED 6ull
#define LK_ALIGN_PLANE_PIVOT 9.5367431640625e-07   // 2^-20: a pivot of the scaled matrix at or below it is an unobserved direction

// first pass: over the matched points n and s2 as lk_align.h's first pass takes them; over the used ones the count, the sums of the moved and
// of the ORIGINAL points and the sum of e^2
struct LkPlaneSums {
    double s2, e2, m[3], p[3];
    unsigned long long n, nu;
};
LK_C2C_HD void lk_plane_sums_zero(LkPlaneSums* s) {
    s->s2 = 0.0, s->e2 = 0.0, s->n = 0ull, s->nu = 0ull;
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) s->m[a] = 0.0, s->p[a] = 0.0;
}
LK_C2C_HD bool lk_plane_normal_finite(float nx, float ny, float nz) {
    return fabsf(nx) <= 3.40282346638528859812e38f && fabsf(ny) <= 3.40282346638528859812e38f && fabsf(nz) <= 3.40282346638528859812e38f;
}
// the plane residual of a moved point against its reference point and that point's normal
LK_C2C_HD double lk_plane_residual(const double* m, float rx, float ry, float rz, float nx, float ny, float nz) {
    const double dx = m[0] - (double)rx, dy = m[1] - (double)ry, dz = m[2] - (double)rz;
    return ((double)nx * dx + (double)ny * dy) + (double)nz * dz;
}
LK_C2C_HD void lk_plane_sums_term(LkPlaneSums* s, const double* T, double d2, float px, float py, float pz, float rx, float ry, float rz, float nx, float ny, float nz) {
    s->s2 = s->s2 + d2, s->n += 1ull;
    if (!lk_plane_normal_finite(nx, ny, nz)) return;
    double m[3];
    lk_align_move(T, (double)px, (double)py, (double)pz, m);
    const double e = lk_plane_residual(m, rx, ry, rz, nx, ny, nz);
    s->nu += 1ull, s->e2 = s->e2 + e * e;
    s->m[0] = s->m[0] + m[0], s->m[1] = s->m[1] + m[1], s->m[2] = s->m[2] + m[2];
    s->p[0] = s->p[0] + (double)px, s->p[1] = s->p[1] + (double)py, s->p[2] = s->p[2] + (double)pz;
}
LK_C2C_HD void lk_plane_sums_merge(LkPlaneSums* x, const LkPlaneSums& y) {
    x->s2 = x->s2 + y.s2, x->e2 = x->e2 + y.e2, x->n += y.n, x->nu += y.nu;
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) x->m[a] = x->m[a] + y.m[a], x->p[a] = x->p[a] + y.p[a];
}
// second pass, per used point: Hg[0 .. 20] += a_i a_j (i <= j, row-major upper triangle), Hg[21 + i] += a_i e
LK_C2C_HD void lk_plane_rows_term(double* Hg, const double* T, const double* mbar, float px, float py, float pz, float rx, float ry, float rz, float nx, float ny, float nz) {
    if (!lk_plane_normal_finite(nx, ny, nz)) return;
    double m[3];
    lk_align_move(T, (double)px, (double)py, (double)pz, m);
    const double e = lk_plane_residual(m, rx, ry, rz, nx, ny, nz);
    const double n0 = (double)nx, n1 = (double)ny, n2 = (double)nz;
#ifdef LK_ALIGN_PLANE_ORIGIN   // (test aid of the host probe only: the rows about the origin; lk_plane_update then carries v over to the turn about mbar)
    const double c0 = m[0], c1 = m[1], c2 = m[2];
    (void)mbar;
#else
    const double c0 = m[0] - mbar[0], c1 = m[1] - mbar[1], c2 = m[2] - mbar[2];
#endif
    const double a[6] = {c1 * n2 - c2 * n1, c2 * n0 - c0 * n2, c0 * n1 - c1 * n0, n0, n1, n2};
    int k = 0;
LK_ALIGN_UNROLL
    for (int i = 0; i < 6; ++i) {
LK_ALIGN_UNROLL
        for (int j = i; j < 6; ++j, ++k) Hg[k] = Hg[k] + a[i] * a[j];
    }
LK_ALIGN_UNROLL
    for (int i = 0; i < 6; ++i) Hg[21 + i] = Hg[21 + i] + a[i] * e;
}

// x = -D (D H D)^-1 D g by Cholesky in natural order without pivoting; false (x untouched) for a diagonal entry <= 0 or a pivot <= 2^-20
LK_C2C_HD bool lk_plane_solve(const double* Hg, double* x) {
    double d[6], L[6][6], y[6];
    bool ok = true;
    int k = 0;
LK_ALIGN_UNROLL
    for (int i = 0; i < 6; ++i) {
LK_ALIGN_UNROLL
        for (int j = i; j < 6; ++j, ++k) {
            L[j][i] = Hg[k];   // the lower triangle takes H for now
            if (j == i) {
                ok = ok && (Hg[k] > 0.0);
                d[i] = 1.0 / sqrt(Hg[k]);
            }
        }
    }
    if (!ok) return false;
LK_ALIGN_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = (L[j][j] * d[j]) * d[j];
LK_ALIGN_UNROLL
        for (int q = 0; q < j; ++q) s = s - L[j][q] * L[j][q];
        if (!(s > LK_ALIGN_PLANE_PIVOT)) return false;
        const double piv = sqrt(s);
        L[j][j] = piv;
LK_ALIGN_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = (L[i][j] * d[j]) * d[i];
LK_ALIGN_UNROLL
            for (int q = 0; q < j; ++q) v = v - L[i][q] * L[j][q];
            L[i][j] = v / piv;
        }
    }
LK_ALIGN_UNROLL
    for (int i = 0; i < 6; ++i) {   // L y = D g
        double v = d[i] * Hg[21 + i];
LK_ALIGN_UNROLL
        for (int q = 0; q < i; ++q) v = v - L[i][q] * y[q];
        y[i] = v / L[i][i];
    }
LK_ALIGN_UNROLL
    for (int i = 5; i >= 0; --i) {   // L^T z = y
        double v = y[i];
LK_ALIGN_UNROLL
        for (int q = i + 1; q < 6; ++q) v = v - L[q][i] * y[q];
        y[i] = v / L[i][i];
    }
LK_ALIGN_UNROLL
    for (int i = 0; i < 6; ++i) x[i] = -(d[i] * y[i]);
    return true;
}

// the proper rotation nearest a matrix that is one up to rounding: lk_horn_rotation of the TRANSPOSE (S[3a + b] = sum p_a g_b with g = R p and
// sum p p^T = 1 is R^T), so a rotation comes back as itself
LK_C2C_HD void lk_plane_nearest_rotation(const double* R1, double* R) {
    double S[9];
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) {
LK_ALIGN_UNROLL
        for (int b = 0; b < 3; ++b) S[3 * a + b] = R1[3 * b + a];
    }
    lk_horn_rotation(S, R);
}
// T' from T and x = (omega, v): dR = the rotation of omega, R' = nearest rotation of dR R, t' = dR (t - mbar) + (mbar + v)
LK_C2C_HD void lk_plane_update(const double* T, const double* x, const double* mbar, double* Tn) {
    const double theta = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    double dR[9], R1[9];
    if (theta == 0.0) lk_quat_to_rot(1.0, 0.0, 0.0, 0.0, dR);
    else {
        const double h = theta / 2.0, s = sin(h);
        lk_quat_to_rot(cos(h), s * x[0] / theta, s * x[1] / theta, s * x[2] / theta, dR);
    }
LK_ALIGN_UNROLL
    for (int i = 0; i < 3; ++i) {
LK_ALIGN_UNROLL
        for (int j = 0; j < 3; ++j) R1[3 * i + j] = (dR[3 * i] * T[j] + dR[3 * i + 1] * T[3 + j]) + dR[3 * i + 2] * T[6 + j];
    }
#ifdef LK_ALIGN_PLANE_NO_ORTHO   // (test aid of the host probe only: the product kept as it is)
    for (int c = 0; c < 9; ++c) Tn[c] = R1[c];
#else
    lk_plane_nearest_rotation(R1, Tn);
#endif
#ifdef LK_ALIGN_PLANE_ORIGIN   // (the same step in exact arithmetic: v about mbar = v about the origin + omega x mbar)
    const double v[3] = {x[3] + (x[1] * mbar[2] - x[2] * mbar[1]), x[4] + (x[2] * mbar[0] - x[0] * mbar[2]), x[5] + (x[0] * mbar[1] - x[1] * mbar[0])};
#else
    const double v[3] = {x[3], x[4], x[5]};
#endif
    const double u[3] = {T[9] - mbar[0], T[10] - mbar[1], T[11] - mbar[2]}, w[3] = {mbar[0] + v[0], mbar[1] + v[1], mbar[2] + v[2]};
LK_ALIGN_UNROLL
    for (int a = 0; a < 3; ++a) Tn[9 + a] = ((dR[3 * a] * u[0] + dR[3 * a + 1] * u[1]) + dR[3 * a + 2] * u[2]) + w[a];
}
