// lk_normals.h - the arithmetic of the per-point normals of a cloud (lk_clouds_normals_dev, lk_normals_kernels.h) that the device route and its CPU
// twin (tools/probes/align_plane_host.cc, tests/test_plane_host.py) share: from the sums of a point's neighbourhood (lk_mme.h's walk and
// accumulator, as they stand) the covariance, its eigenvalues in ascending order, the planarity and the unit eigenvector of the smallest one.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): N_i, s, M and C are lk_clouds_mme_dev's, so a point's n_i is that entry's d_n.
//   planarity  w = (l1 - l0) / l2 of the sorted eigenvalues l0 <= l1 <= l2, 0 when l2 <= 0 (all duplicates)
//   validity   n_i >= min_pts and w >= min_planarity
//   normal     the unit eigenvector of l0; its sign makes the float64 component of largest magnitude positive, the first such component on ties;
//              then each component is rounded once to float32
// A point that is not valid gets NaN in nx ny nz; it keeps its w when it is dense (n_i >= min_pts), a sparse one gets NaN there too.
// No FMA is spelled out and the units that include this build with -ffp-contract=off.  Plain C++ that compiles for the host as it stands.
#pragma once
#include "lk_mme.h"

// +-1: the sign rule on the float64 vector.  LK_NORMALS_SIGN_F32 (test aid of the host probe only): the rule on the ROUNDED components, where two
// components a float32 apart in float64 tie and the first of them decides
LK_C2C_HD double lk_normals_sign(double x, double y, double z) {
#ifdef LK_NORMALS_SIGN_F32
    const double a0 = fabs((double)(float)x), a1 = fabs((double)(float)y), a2 = fabs((double)(float)z);
#else
    const double a0 = fabs(x), a1 = fabs(y), a2 = fabs(z);
#endif
    double lead = x, big = a0;
    if (a1 > big) lead = y, big = a1;
    if (a2 > big) lead = z, big = a2;
    return lead < 0.0 ? -1.0 : 1.0;
}

// rec = (nx, ny, nz, w) of one point from its sums; returns whether the point is valid.  min_pts >= 3.
LK_C2C_HD bool lk_normals_finish(const LkMmeAcc& a, unsigned int min_pts, double min_planarity, float* rec) {
    rec[0] = NAN, rec[1] = NAN, rec[2] = NAN, rec[3] = NAN;
    if (a.n < min_pts) return false;
    double c[6], ev[3], v0[3], v1[3], v2[3];
    lk_mme_cov(a, c);
    lk_eig_sym3_cols(c, ev, v0, v1, v2);
    // sorted as scalars beside the choice of the vector (lk_eig3.h: ev may leave ascending order by rounding when two coincide, and a vector picked
    // by an index costs memory on the device); the first of equal smallest eigenvalues gives the normal
    double l0 = ev[0], nx = v0[0], ny = v0[1], nz = v0[2];
    if (ev[1] < l0) l0 = ev[1], nx = v1[0], ny = v1[1], nz = v1[2];
    if (ev[2] < l0) l0 = ev[2], nx = v2[0], ny = v2[1], nz = v2[2];
    const double l2 = fmax(ev[0], fmax(ev[1], ev[2]));
    const double l1 = fmax(fmin(ev[0], ev[1]), fmin(fmax(ev[0], ev[1]), ev[2]));   // the median of three
    const double w = l2 > 0.0 ? (l1 - l0) / l2 : 0.0;
    rec[3] = (float)w;
    if (!(w >= min_planarity)) return false;
    const double sg = lk_normals_sign(nx, ny, nz);   // (a product with +-1 is exact)
    rec[0] = (float)(sg * nx), rec[1] = (float)(sg * ny), rec[2] = (float)(sg * nz);
    return true;
}
