// lk_sor.h - the arithmetic of the statistical outlier filter of map clouds (lk_clouds_sor_dev, lk_sor_kernels.h) that the device route and its CPU
// twin (tools/probes/sor_host.cc, tests/test_sor_host.py) share: the list of the k smallest squared distances of a point, the visitor that fills it
// on lk_c2c.h's walk, the mean neighbour distance, the threshold and the keep test.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): the candidates of point i are the records j != i of its cloud with
// lk_c2c_d2(i, j) <= reach * reach, and by the argument at the head of lk_c2c.h every candidate lies in the 27 cells that lk_c2c_walk visits.  The k
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
// the walk's visitor.  Record r against the query (index qidx within the cloud): a candidate when it is another record - by INDEX, a duplicate of
// the query is one at distance 0 - and d2 <= reach2; it enters the list when it is below the list's last place
template <int CAP>
struct LkSorVisit {
    LkSorList<CAP>* l;
    unsigned int qidx;
    double reach2;
    LK_C2C_HD void operator()(unsigned int, const LkC2cRec& r, double d2) {
        if (r.idx == qidx || !lk_c2c_matched(d2, reach2)) return;
        l->cnt += 1u;
        if (d2 < l->v[CAP - 1]) lk_sor_insert(l, d2);
    }
};
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

// One point of a cloud against the cloud itself: lk_c2c_walk with that visitor.  *seen (may be null): records the walk visited, the query itself
// among them.
template <int CAP>
LK_C2C_HD void lk_sor_walk(float qx, float qy, float qz, unsigned int qidx, const LkC2cGrid& g, const unsigned int* keys, const LkC2cRec* recs, unsigned int n,
                           double reach2, LkSorList<CAP>* list, unsigned int* seen) {
    lk_sor_clear(list);
    LkSorVisit<CAP> v = {list, qidx, reach2};
    lk_c2c_walk(qx, qy, qz, g, keys, recs, n, v, seen);
}
