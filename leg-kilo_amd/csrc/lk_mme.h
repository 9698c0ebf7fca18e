// lk_mme.h - the arithmetic of the reference-free map scores (lk_clouds_mme_dev, lk_mme_kernels.h) that the device route and its CPU twin
// (tools/probes/mme_host.cc, tests/test_mme_host.py) share: the second moments of a point's neighbourhood about the point itself, the covariance with
// its determinant, the flatness floor, the entropy and the smallest eigenvalue, and the visitor that sums them on lk_c2c.h's walk.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): N_i holds every record j of the cloud with lk_c2c_d2(i, j) <= r * r, i itself among
// them.  The grid and the walk are lk_c2c.h's with the radius as the reach (lk_c2c_walk; the argument at the head of that file is why every member
// lies in the 27 cells around the point's own).  The offsets u_j = p_j - p_i are bounded by r whatever the cloud's coordinates, so the sums carry
// rounding of order 2^-53 r^2.  The order of a sum is the walk's: rows of cells in ascending (z, y), keys ascending inside a row, records of equal
// key in input order - a function of the cloud's own records and of the radius.
// No FMA is spelled out and the units that include this build with -ffp-contract=off.  Plain C++ that compiles for the host as it stands.
#pragma once
#include "lk_c2c.h"
#include "lk_eig3.h"

#define LK_MME_SPARSE 0u   // fewer than min_pts records within the radius: no figure
#define LK_MME_FLAT   1u   // dense, det <= 2^-30 (tr / 3)^3: lmin only
#define LK_MME_SCORED 2u   // dense and not flat: h and lmin

struct LkMmeAcc {
    unsigned int n;   // records within the radius, the point itself among them
    double s[3];      // sum u
    double m[6];      // sum u u^T: xx xy xz yy yz zz
};
LK_C2C_HD void lk_mme_clear(LkMmeAcc* a) {
    a->n = 0u;
    for (int k = 0; k < 3; ++k) a->s[k] = 0.0;
    for (int k = 0; k < 6; ++k) a->m[k] = 0.0;
}
// record r against the query q: a member when lk_c2c_d2 <= reach2, then its offset about q joins the sums (each product and each sum rounded)
LK_C2C_HD void lk_mme_add(LkMmeAcc* a, float qx, float qy, float qz, float rx, float ry, float rz, double reach2) {
    if (!lk_c2c_matched(lk_c2c_d2(qx, qy, qz, rx, ry, rz), reach2)) return;
    const double ux = (double)rx - (double)qx, uy = (double)ry - (double)qy, uz = (double)rz - (double)qz;
    a->n += 1u;
    a->s[0] = a->s[0] + ux, a->s[1] = a->s[1] + uy, a->s[2] = a->s[2] + uz;
    a->m[0] = a->m[0] + ux * ux, a->m[1] = a->m[1] + ux * uy, a->m[2] = a->m[2] + ux * uz;
    a->m[3] = a->m[3] + uy * uy, a->m[4] = a->m[4] + uy * uz, a->m[5] = a->m[5] + uz * uz;
}
// the covariance of a neighbourhood of two records or more from its sums (lk_normals.h takes it too): C = (M - s s^T / n) / (n - 1): xx xy xz yy yz zz
LK_C2C_HD void lk_mme_cov(const LkMmeAcc& a, double* c) {
    const double n = (double)a.n, n1 = (double)(a.n - 1u);
    c[0] = (a.m[0] - a.s[0] * a.s[0] / n) / n1, c[1] = (a.m[1] - a.s[0] * a.s[1] / n) / n1, c[2] = (a.m[2] - a.s[0] * a.s[2] / n) / n1;
    c[3] = (a.m[3] - a.s[1] * a.s[1] / n) / n1, c[4] = (a.m[4] - a.s[1] * a.s[2] / n) / n1, c[5] = (a.m[5] - a.s[2] * a.s[2] / n) / n1;
}
// class and figures of one point from its sums; h is NaN unless SCORED, lmin NaN when SPARSE.  min_pts >= 4 (below four points det is 0 by rank).
LK_C2C_HD void lk_mme_finish(const LkMmeAcc& a, unsigned int min_pts, unsigned int* cls, double* h, double* lmin) {
    *cls = LK_MME_SPARSE, *h = NAN, *lmin = NAN;
    if (a.n < min_pts) return;
    double c[6];
    lk_mme_cov(a, c);
    const double tr = (c[0] + c[3]) + c[5];
    const double det = (c[0] * (c[3] * c[5] - c[4] * c[4]) - c[1] * (c[1] * c[5] - c[4] * c[2])) + c[2] * (c[1] * c[4] - c[3] * c[2]);
    const double t = tr / 3.0;
    double ev[3];
    lk_eig_sym3_vals(c, ev);
    const double e = fmin(ev[0], fmin(ev[1], ev[2]));
    *lmin = e > 0.0 ? e : 0.0;
    if (det <= 9.31322574615478515625e-10 * ((t * t) * t)) {   // 2^-30: the floor under which det is the rounding of the storage format
        *cls = LK_MME_FLAT;
        return;
    }
    *cls = LK_MME_SCORED;
    *h = 0.5 * (8.5136311992280364508 + log(det));   // 3 ln(2 pi e) = 8.51363119922803645...
}

// One point of a cloud against the cloud itself: lk_c2c_walk with every record within reach ADDED where the search keeps the minimum (lk_mme_add
// takes its own d2: the walk's expression, the walk's bits).  *seen (may be null): records whose distance was evaluated.
struct LkMmeVisit {
    LkMmeAcc* acc;
    float qx, qy, qz;
    double reach2;
    LK_C2C_HD void operator()(unsigned int, const LkC2cRec& r, double) { lk_mme_add(acc, qx, qy, qz, r.x, r.y, r.z, reach2); }
};
LK_C2C_HD void lk_mme_walk(float qx, float qy, float qz, const LkC2cGrid& g, const unsigned int* keys, const LkC2cRec* recs, unsigned int n, double reach2,
                           LkMmeAcc* acc, unsigned int* seen) {
    lk_mme_clear(acc);
    LkMmeVisit v = {acc, qx, qy, qz, reach2};
    lk_c2c_walk(qx, qy, qz, g, keys, recs, n, v, seen);
}
