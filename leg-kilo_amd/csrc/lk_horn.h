// lk_horn.h - the proper rotation that best maps one centred point set onto another (absolute orientation, Horn 1987: "Closed-form solution of
// absolute orientation using unit quaternions"), the solve of the trajectory error entries (lk_traj_kernels.h).
//
// Given the cross-covariance S[3 a + b] = sum_i p_a g_b of the CENTRED pairs, the rotation R that minimises sum |g_i - R p_i|^2 over det R = +1 is
// the one of the unit quaternion q = (w, x, y, z) that maximises q^T N q, N the symmetric 4 x 4 matrix below: its eigenvector of the largest
// eigenvalue.  Every unit quaternion is a proper rotation, so there is no reflection case to correct (an SVD's U V^T is a reflection for a mirrored
// trajectory), and a rank-1 or rank-2 S (collinear, planar, two points) only makes the largest eigenvalue multiple: every vector of its eigenspace is
// a minimiser, and cyclic Jacobi hands back an orthonormal basis whatever the multiplicities.  S = 0 (one pair, coincident points): the identity.
// The eigenvector comes from cyclic Jacobi with Rutishauser's rotation formulas - one solve per trajectory, so its ~6 sweeps of 6 rotations do not matter.
// Plain C++ that compiles for the host as it stands (tools/probes/horn_host.cc, tests/test_ate_host.py), like lk_eig3.h.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define LK_HORN_HD __host__ __device__ inline
#define LK_HORN_UNROLL _Pragma("unroll")   // constant indices: the two 4 x 4 arrays stay in registers on the device
#else
#define LK_HORN_HD inline
#define LK_HORN_UNROLL
#endif

// unit quaternion (w, x, y, z) -> row-major rotation matrix
LK_HORN_HD void lk_quat_to_rot(double w, double x, double y, double z, double* R) {
    R[0] = (w * w + x * x) - (y * y + z * z), R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z), R[4] = (w * w + y * y) - (x * x + z * z), R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = (w * w + z * z) - (x * x + y * y);
}

// S: row-major, S[3 a + b] = sum p_a g_b over the centred pairs.  R: row-major, g ~ R p, det R = +1.  A non-finite S gives the identity.
LK_HORN_HD void lk_horn_rotation(const double* S, double* R) {
    double mx = 0.0;
    bool finite = true;
    for (int k = 0; k < 9; ++k) {
        const double v = fabs(S[k]);
        finite = finite && (v <= 1.79769313486231570815e308);   // false for NaN and infinity
        mx = v > mx ? v : mx;
    }
    if (!finite || !(mx > 0.0)) {
        lk_quat_to_rot(1.0, 0.0, 0.0, 0.0, R);
        return;
    }
    const double inv = 1.0 / mx;   // N is homogeneous in S: the scale only keeps the products away from the ends of the exponent range
    const double Sxx = S[0] * inv, Sxy = S[1] * inv, Sxz = S[2] * inv, Syx = S[3] * inv, Syy = S[4] * inv, Syz = S[5] * inv, Szx = S[6] * inv,
                 Szy = S[7] * inv, Szz = S[8] * inv;
    double a[4][4], v[4][4];
    a[0][0] = Sxx + Syy + Szz, a[0][1] = Syz - Szy, a[0][2] = Szx - Sxz, a[0][3] = Sxy - Syx;
    a[1][1] = Sxx - Syy - Szz, a[1][2] = Sxy + Syx, a[1][3] = Szx + Sxz;
    a[2][2] = -Sxx + Syy - Szz, a[2][3] = Syz + Szy;
    a[3][3] = -Sxx - Syy + Szz;
LK_HORN_UNROLL
    for (int i = 0; i < 4; ++i) {
LK_HORN_UNROLL
        for (int j = 0; j < 4; ++j) {
            v[i][j] = (i == j) ? 1.0 : 0.0;
            if (j < i) a[i][j] = a[j][i];
        }
    }
    for (int sweep = 0; sweep < 40; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (off == 0.0) break;
LK_HORN_UNROLL
        for (int p = 0; p < 3; ++p) {
LK_HORN_UNROLL
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                const double g = 100.0 * fabs(apq);
                // an element that no longer changes either diagonal neighbour is dropped (from the fourth sweep on, as in Rutishauser's procedure)
                if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
                    a[p][q] = a[q][p] = 0.0;
                } else if (apq != 0.0) {
                    const double h = a[q][q] - a[p][p];
                    double t;
                    if (fabs(h) + g == fabs(h)) {
                        t = apq / h;
                    } else {
                        const double theta = 0.5 * h / apq;
                        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                    }
                    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                    a[p][p] -= t * apq;
                    a[q][q] += t * apq;
                    a[p][q] = a[q][p] = 0.0;
LK_HORN_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        if (r != p && r != q) {
                            const double x = a[r][p], y = a[r][q];
                            a[r][p] = a[p][r] = x - s * (y + x * tau);
                            a[r][q] = a[q][r] = y + s * (x - y * tau);
                        }
                        const double x = v[r][p], y = v[r][q];
                        v[r][p] = x - s * (y + x * tau);
                        v[r][q] = y + s * (x - y * tau);
                    }
                }
            }
        }
    }
    // the column of the largest eigenvalue (the first of equal ones), selected without a run-time index
    double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
    if (a[1][1] > best) best = a[1][1], w = v[0][1], x = v[1][1], y = v[2][1], z = v[3][1];
    if (a[2][2] > best) best = a[2][2], w = v[0][2], x = v[1][2], y = v[2][2], z = v[3][2];
    if (a[3][3] > best) best = a[3][3], w = v[0][3], x = v[1][3], y = v[2][3], z = v[3][3];
    const double n = sqrt((w * w + x * x) + (y * y + z * z));
    if (!(n > 0.0)) {
        lk_quat_to_rot(1.0, 0.0, 0.0, 0.0, R);
        return;
    }
    lk_quat_to_rot(w / n, x / n, y / n, z / n, R);
}
