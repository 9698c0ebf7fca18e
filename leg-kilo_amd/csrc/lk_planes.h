// lk_planes.h - the arithmetic of the plane extraction of map clouds (lk_clouds_planes_dev, lk_planes_kernels.h) that the device route and its CPU
// twin (tools/probes/planes_host.cc, tests/test_planes_host.py) share: the sampler, a hypothesis from three records, the test of one record against
// it, the winner's order, and what turns the sums over a plane's inliers into its reported coefficients.
//
// The RESULT is defined in include/legkilo_hip.h.  Every decision is a comparison of float64 values that were formed from the float32 coordinates
// with one rounding per operation (the library is built with -ffp-contract=off; the twin too), without a square root and without a division, and a
// score is a whole number: the order in which records are counted leaves no trace.  Nothing here knows which cloud of a call it works on.
// Plain C++ that compiles for the host as it stands.
#pragma once
#include <math.h>
#include <stdint.h>
#include "lk_eig3.h"
#if defined(__HIPCC__)
#define LK_PLANES_HD __host__ __device__ __forceinline__
#else
#define LK_PLANES_HD inline
#endif

#define LK_PLANES_HYP_LIMIT 4096u   // include/legkilo_hip.h's LK_PLANES_MAX_HYP: the sampler's counter is laid out by it
#define LK_PLANES_GROUP 64u         // hypotheses of one block of the score kernel: a lane each
#define LK_PLANES_TILE 256u         // records staged in LDS at a time
#define LK_PLANES_CHUNK 2048u       // records of the remainder that one block of the score kernel tests
#define LK_PLANES_NONE 0xffffffffu  // no plane: a label, a winner

LK_PLANES_HD uint64_t lk_planes_mix(uint64_t x) {   // splitmix64: the state advanced by the golden gamma, then the finaliser
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
LK_PLANES_HD uint64_t lk_planes_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// three distinct positions below m (m >= 3) for hypothesis h of round r
LK_PLANES_HD void lk_planes_sample(uint64_t seed, uint32_t r, uint32_t h, uint32_t m, uint32_t* i) {
    const uint64_t ctr = ((uint64_t)r * LK_PLANES_HYP_LIMIT + h) * 4ull;
    const uint32_t i0 = (uint32_t)lk_planes_mulhi(lk_planes_mix(seed + ctr), m);
    uint32_t i1 = (uint32_t)lk_planes_mulhi(lk_planes_mix(seed + ctr + 1ull), m - 1u);
    uint32_t i2 = (uint32_t)lk_planes_mulhi(lk_planes_mix(seed + ctr + 2ull), m - 2u);
    i1 += i1 >= i0 ? 1u : 0u;
    const uint32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    i2 += i2 >= lo ? 1u : 0u;
    i2 += i2 >= hi ? 1u : 0u;
    i[0] = i0, i[1] = i1, i[2] = i2;
}

struct LkPlanesAxis {   // the caller's axis and cos_max_angle * cos_max_angle; given == 0: no axis
    double x, y, z, aa, c2;
    unsigned int given;
};
LK_PLANES_HD LkPlanesAxis lk_planes_axis(const double* axis, double cos_max_angle) {
    LkPlanesAxis a = {0.0, 0.0, 0.0, 0.0, cos_max_angle * cos_max_angle, axis ? 1u : 0u};
    if (axis) a.x = axis[0], a.y = axis[1], a.z = axis[2], a.aa = (axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2];
    return a;
}

// a hypothesis: its first sample point, u x v, and dist^2 * |u x v|^2.  t2q is -1 for a skipped hypothesis: no s * s is at or below it
struct LkPlanesHyp {
    double ax, ay, az, mx, my, mz, t2q;
};
LK_PLANES_HD LkPlanesHyp lk_planes_hyp(const float* a, const float* b, const float* c, double dist2, const LkPlanesAxis& ax) {
    LkPlanesHyp h;
    h.ax = a[0], h.ay = a[1], h.az = a[2];
    const double ux = (double)b[0] - h.ax, uy = (double)b[1] - h.ay, uz = (double)b[2] - h.az;
    const double vx = (double)c[0] - h.ax, vy = (double)c[1] - h.ay, vz = (double)c[2] - h.az;
    h.mx = uy * vz - uz * vy, h.my = uz * vx - ux * vz, h.mz = ux * vy - uy * vx;
    const double q = (h.mx * h.mx + h.my * h.my) + h.mz * h.mz;
    bool ok = q > 0.0 && q <= 1.7976931348623157e308;   // (a NaN fails both)
    if (ok && ax.given) {
        const double g = (h.mx * ax.x + h.my * ax.y) + h.mz * ax.z;
        ok = !(g * g < (ax.c2 * q) * ax.aa);
    }
    h.t2q = ok ? dist2 * q : -1.0;
    return h;
}
LK_PLANES_HD bool lk_planes_inlier(const LkPlanesHyp& h, double px, double py, double pz) {
    const double ex = px - h.ax, ey = py - h.ay, ez = pz - h.az;
    const double s = (h.mx * ex + h.my * ey) + h.mz * ez;
    return s * s <= h.t2q;
}
// (score, h) against the best so far: the larger score, the smaller h among equals.  none yet: best_h == LK_PLANES_NONE
LK_PLANES_HD bool lk_planes_better(unsigned int score, unsigned int h, unsigned int best_score, unsigned int best_h) {
    return best_h == LK_PLANES_NONE || score > best_score || (score == best_score && h < best_h);
}
// a round runs on a remainder of m records
LK_PLANES_HD bool lk_planes_runs(unsigned int m, unsigned int min_inliers) { return m >= (min_inliers > 3u ? min_inliers : 3u); }

// the reported coefficients from a plane's n inliers: s = their coordinate sums' centroid, cov = the six centred sums (xx xy xz yy yz zz)
struct LkPlanesFit {
    double normal[3], d, centroid[3], eig[3], rmse;
};
LK_PLANES_HD void lk_planes_fit(const double* centroid, const double* csum, unsigned int n, const LkPlanesAxis& ax, LkPlanesFit* f) {
    const double dn = (double)n;
    const double A[6] = {csum[0] / dn, csum[1] / dn, csum[2] / dn, csum[3] / dn, csum[4] / dn, csum[5] / dn};
    double ev[3], v0[3], v1[3], v2[3];
    lk_eig_sym3_cols(A, ev, v0, v1, v2);
    // sorted as scalars beside the choice of the vector (lk_eig3.h: ev may leave ascending order by rounding when two coincide, and a vector picked
    // by an index costs memory on the device); the first of equal smallest eigenvalues gives the normal
    double l0 = ev[0], nx = v0[0], ny = v0[1], nz = v0[2];
    if (ev[1] < l0) l0 = ev[1], nx = v1[0], ny = v1[1], nz = v1[2];
    if (ev[2] < l0) l0 = ev[2], nx = v2[0], ny = v2[1], nz = v2[2];
    const double l2 = fmax(ev[0], fmax(ev[1], ev[2]));
    const double l1 = fmax(fmin(ev[0], ev[1]), fmin(fmax(ev[0], ev[1]), ev[2]));   // the median of three
    bool flip;
    if (ax.given) {
        flip = !((nx * ax.x + ny * ax.y) + nz * ax.z >= 0.0);
    } else {
        const double m0 = fabs(nx), m1 = fabs(ny), m2 = fabs(nz);
        const double big = (m0 >= m1 && m0 >= m2) ? nx : (m1 >= m2 ? ny : nz);   // the first among equal magnitudes
        flip = big < 0.0;
    }
    f->normal[0] = flip ? -nx : nx, f->normal[1] = flip ? -ny : ny, f->normal[2] = flip ? -nz : nz;
    f->centroid[0] = centroid[0], f->centroid[1] = centroid[1], f->centroid[2] = centroid[2];
    f->eig[0] = l0, f->eig[1] = l1, f->eig[2] = l2;
    f->d = -((f->normal[0] * centroid[0] + f->normal[1] * centroid[1]) + f->normal[2] * centroid[2]);
    f->rmse = sqrt(l0 > 0.0 ? l0 : 0.0);
}
