// lk_sor.h - the arithmetic of the statistical outlier filter of map clouds (lk_clouds_sor_dev, lk_sor_kernels.h) that the device route and its CPU
// twin (tools/probes/sor_host.cc, tests/test_sor_host.py) share: the list of the k smallest squared distances of a point, the walk of one point
// through the sorted cells of its own cloud that fills it, the mean neighbour distance, the threshold and the keep test.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): the candidates of point i are the records j != i of its cloud with
// lk_c2c_d2(i, j) <= reach * reach, and lk_c2c.h's argument holds word for word - every candidate lies in the 27 cells around the point's own.  The k
// smallest of a multiset do not depend on the order in which its members arrive, so the walk's order leaves no trace in dbar_i.
// The list is LkSorList<CAP>: CAP doubles in ascending order, +inf where nothing was entered yet.  Every index into it is a compile-time constant
// (the loops below unroll fully), so on the device it lives in registers; a list indexed by a runtime k would go to scratch.  CAP >= k, and the
// list keeps the CAP smallest - the k smallest are its first k.  The instantiations are LK_SOR_CAPS.
// No FMA is spelled out and the units that include this build with -ffp-contract=off.  Plain C++ that compiles for the host as it stands.
#pragma once
#include "lk_c2c.h"

#define LK_SOR_CAP_SMALL 8    // k <= 8
#define LK_SOR_CAP_MID   16   // k <= 16
#define LK_SOR_CAP_BIG   32   // k <= 32 = LK_SOR_MAX_K
LK_C2C_HD int lk_sor_cap_of(unsigned int k) { return k <= LK_SOR_CAP_SMALL ? LK_SOR_CAP_SMALL : k <= LK_SOR_CAP_MID ? LK_SOR_CAP_MID : LK_SOR_CAP_BIG; }

template <int CAP>
struct LkSorList {
    double v[CAP];      // the CAP smallest candidate d2 so far, ascending; +inf = not taken
    unsigned int cnt;   // candidates in all
};
template <int CAP>
LK_C2C_HD void lk_sor_clear(LkSorList<CAP>* l) {
    l->cnt = 0u;
#pragma unroll
    for (int s = 0; s < CAP; ++s) l->v[s] = INFINITY;
}
// d enters the ascending list: every place above its own takes its lower neighbour's value, the last one drops out.  Among equal values the new one
// goes last - they are equal, so nobody can tell.  Places are visited from the top, so v[s - 1] is still the old one when place s reads it.
template <int CAP>
LK_C2C_HD void lk_sor_insert(LkSorList<CAP>* l, double d) {
#pragma unroll
    for (int s = CAP - 1; s > 0; --s) {
        const double below = l->v[s - 1], here = l->v[s];
        l->v[s] = d < below ? below : (d < here ? d : here);
    }
    l->v[0] = d < l->v[0] ? d : l->v[0];
}
// record r (index ridx within the cloud) against the query q (index qidx): a candidate when it is another record - by INDEX, a duplicate of q is one at
// distance 0 - and lk_c2c_d2 <= reach2; it enters the list when it is below the list's last place
template <int CAP>
LK_C2C_HD void lk_sor_add(LkSorList<CAP>* l, float qx, float qy, float qz, unsigned int qidx, float rx, float ry, float rz, unsigned int ridx, double reach2) {
    if (ridx == qidx) return;
    const double d2 = lk_c2c_d2(qx, qy, qz, rx, ry, rz);
    if (!lk_c2c_matched(d2, reach2)) return;
    l->cnt += 1u;
    if (d2 < l->v[CAP - 1]) lk_sor_insert(l, d2);
}
// dbar of a point from its list: NaN when it has fewer than k candidates (ISOLATED), else the mean of the roots of the k smallest d2, the sum taken
// in ascending order, one term after the other
template <int CAP>
LK_C2C_HD double lk_sor_finish(const LkSorList<CAP>& l, unsigned int k) {
    if (l.cnt < k) return NAN;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < CAP; ++s)
        if ((unsigned int)s < k) sum = sum + sqrt(l.v[s]);
    return sum / (double)k;
}
// sigma of n_s >= 1 values from the sum of their centred squares; thr from mu, sigma and n_sigma (+inf: no product is taken); the keep test
LK_C2C_HD double lk_sor_sigma(double ss, unsigned long long n_s) { return n_s > 1ull ? sqrt(ss / (double)(n_s - 1ull)) : 0.0; }
LK_C2C_HD double lk_sor_thr(double mu, double sigma, double n_sigma) { return n_sigma == INFINITY ? INFINITY : mu + n_sigma * sigma; }
LK_C2C_HD bool lk_sor_kept(double dbar, double thr) { return dbar <= thr; }   // (false for an isolated point's NaN, and under a status cloud's NaN thr)

// One point of a cloud against the cloud itself: lk_mme_walk's loops - the same 27 cells and nine lower bounds - with lk_sor_add in the place of
// lk_mme_add.  `keys` - the cloud's n cell keys in ascending order, `recs` - its records in that order.  *seen (may be null): records whose distance
// was evaluated or that were the query itself.
template <int CAP>
LK_C2C_HD void lk_sor_walk(float qx, float qy, float qz, unsigned int qidx, const LkC2cGrid& g, const unsigned int* keys, const LkC2cRec* recs, unsigned int n,
                           double reach2, LkSorList<CAP>* list, unsigned int* seen) {
    unsigned int count = 0;
    long long lo[3], hi[3];
    lk_sor_clear(list);
    const bool any = lk_c2c_axis(qx, g.edge, g.mn[0], g.dv[0], &lo[0], &hi[0]) & lk_c2c_axis(qy, g.edge, g.mn[1], g.dv[1], &lo[1], &hi[1]) &
                     lk_c2c_axis(qz, g.edge, g.mn[2], g.dv[2], &lo[2], &hi[2]);
    if (any && n) {
        for (long long i2 = lo[2]; i2 <= hi[2]; ++i2) {
            for (long long i1 = lo[1]; i1 <= hi[1]; ++i1) {
                const long long row = i1 * g.dv[0] + i2 * (long long)g.dv[0] * g.dv[1], k0 = row + lo[0], k1 = row + hi[0];
                unsigned int a = 0, b = n;   // the first record with key >= k0
                while (a < b) {
                    const unsigned int m = a + (b - a) / 2;
                    if ((long long)keys[m] < k0) a = m + 1;
                    else b = m;
                }
                for (; a < n && (long long)keys[a] <= k1; ++a) {
                    const LkC2cRec r = recs[a];
                    lk_sor_add(list, qx, qy, qz, qidx, r.x, r.y, r.z, r.idx, reach2);
                    ++count;
                }
            }
        }
    }
    if (seen) *seen = count;
}
