// lk_c2c.h - the arithmetic of the cloud-to-cloud distance (lk_clouds_c2c_dev, lk_c2c_kernels.h) that the device route and its CPU twin
// (tools/probes/c2c_host.cc, tests/test_c2c_host.py) share: the squared distance, the matched test, the cell of a point, the cell-edge rule, the
// clipped neighbour ranges, the walk of one query point through the sorted cells of one cloud (lk_c2c_walk - the ONE copy of it: lk_align.h, lk_mme.h,
// lk_sor.h and lk_cluster.h bring a visitor each) and the search of one query point on it.
//
// The RESULT is defined without a grid (include/legkilo_hip.h): j(i) minimises (d2, j) over the whole reference cloud, kept when d2 <= max_dist^2.
// The grid only has to hold every reference point with d2 <= max_dist^2 among the cells it visits.  It does: fl(dx*dx) <= d2 <= fl(max_dist^2) and
// squaring is strictly monotone on doubles, so |dx| <= max_dist <= edge per axis; p -> floor(p / edge) is monotone and moves by at most one over a
// distance of edge, so the reference point's cell is the query's or a neighbour, per axis: 27 cells.  (dx is the rounded difference of two floats; it
// is exact unless the coordinates' magnitudes lie more than 2^28 apart, and then rounds by less than 2^-53 of max_dist - the one place where "within
// max_dist" and "next cell" could part, for a reference point at exactly max_dist from a query coordinate 2^-28 of that size.)  Every edge >=
// max_dist does, so the edge rule is free to double: the result does not depend on it.
// No FMA is spelled out and the units that include this build with -ffp-contract=off; the host build rounds as the device does.
// Plain C++ that compiles for the host as it stands, like lk_relpose.h.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define LK_C2C_HD __host__ __device__ __forceinline__
#else
#define LK_C2C_HD inline
#endif

// a reference record in cell order: the coordinates and the record's index within its cloud (the place of w, which nothing reads)
struct alignas(16) LkC2cRec {
    float x, y, z;
    unsigned int idx;
};
// the grid of one reference cloud over its own bounds
struct LkC2cGrid {
    double edge;      // max_dist * 2^doublings
    int mn[3];        // cell of the cloud's smallest coordinate, per axis
    int dv[3];        // cells per axis; dv[0] * dv[1] * dv[2] < 2^31
    int doublings;
    int pad_;
};

// three products and two sums, each rounded
LK_C2C_HD double lk_c2c_d2(float qx, float qy, float qz, float rx, float ry, float rz) {
    const double dx = (double)qx - (double)rx, dy = (double)qy - (double)ry, dz = (double)qz - (double)rz;
    return (dx * dx + dy * dy) + dz * dz;
}
LK_C2C_HD double lk_c2c_reach2(double max_dist) { return max_dist * max_dist; }   // one rounded product
LK_C2C_HD bool lk_c2c_matched(double d2, double reach2) { return d2 <= reach2; }
// LK_C2C_RANGE: below 2^30 a cell coordinate, and a difference of two, stays inside an int under every edge >= max_dist
LK_C2C_HD bool lk_c2c_out_of_range(float p, double max_dist) { return !(fabs((double)p / max_dist) < 1073741824.0); }
// floor, not truncation: -1e-7 lies in cell -1
LK_C2C_HD long long lk_c2c_cell(float p, double edge) { return (long long)floor((double)p / edge); }

// The cell-edge rule: the edge starts at max_dist and doubles until the grid over the bounds lo .. hi holds fewer than 2^31 cells (a key is then an
// unsigned int below 2^31, what the radix sort is asked to sort).  Ends after at most 31 doublings: an axis holds at most 2^31 cells to begin with.
LK_C2C_HD void lk_c2c_grid(const float lo[3], const float hi[3], double max_dist, LkC2cGrid* g) {
    g->edge = max_dist, g->doublings = 0, g->pad_ = 0;
    for (;;) {
        for (int c = 0; c < 3; ++c) {
            const long long a = lk_c2c_cell(lo[c], g->edge);
            g->mn[c] = (int)a, g->dv[c] = (int)(lk_c2c_cell(hi[c], g->edge) - a + 1);
        }
        if ((double)g->dv[0] * (double)g->dv[1] * (double)g->dv[2] < 2147483648.0) return;
        g->edge = g->edge + g->edge, g->doublings += 1;
    }
}
LK_C2C_HD void lk_c2c_grid_of_nothing(double max_dist, LkC2cGrid* g) {   // an empty (or refused) cloud: one cell that holds no record
    g->edge = max_dist, g->doublings = 0, g->pad_ = 0;
    for (int c = 0; c < 3; ++c) g->mn[c] = 0, g->dv[c] = 1;
}
LK_C2C_HD unsigned int lk_c2c_key(float x, float y, float z, const LkC2cGrid& g) {
    const long long i0 = lk_c2c_cell(x, g.edge) - g.mn[0], i1 = lk_c2c_cell(y, g.edge) - g.mn[1], i2 = lk_c2c_cell(z, g.edge) - g.mn[2];
    return (unsigned int)(i0 + i1 * g.dv[0] + i2 * (long long)g.dv[0] * g.dv[1]);
}
// The cells i - 1 .. i + 1 of a query coordinate on one axis of a reference grid, CLIPPED to the grid: a query outside the reference's bounds sees
// only the cells that exist, and none (false) from two cells out on.
LK_C2C_HD bool lk_c2c_axis(float q, double edge, int mn, int dv, long long* lo, long long* hi) {
    const long long i = lk_c2c_cell(q, edge) - mn;
    *lo = i - 1 < 0 ? 0 : i - 1, *hi = i + 1 > dv - 1 ? dv - 1 : i + 1;
    return *lo <= *hi;
}

// The same for a query coordinate that is a DOUBLE (lk_align.h: a moved point is never rounded to float32): overloads, declared in front of the walk
// because its calls on fundamental types find only what is declared by then.  The 27-cell argument above holds for them unchanged - it never asks
// how many bits the query coordinate has; dx is then always a rounded difference, by less than 2^-53 of max_dist where it matters.
LK_C2C_HD double lk_c2c_d2(double qx, double qy, double qz, float rx, float ry, float rz) {
    const double dx = qx - (double)rx, dy = qy - (double)ry, dz = qz - (double)rz;
    return (dx * dx + dy * dy) + dz * dz;
}
LK_C2C_HD long long lk_c2c_cell(double p, double edge) { return (long long)floor(p / edge); }
LK_C2C_HD bool lk_c2c_axis(double q, double edge, int mn, int dv, long long* lo, long long* hi) {
    const long long i = lk_c2c_cell(q, edge) - mn;
    *lo = i - 1 < 0 ? 0 : i - 1, *hi = i + 1 > dv - 1 ? dv - 1 : i + 1;
    return *lo <= *hi;
}

// THE walk: one query point (Q = float or double) through the sorted cells of one cloud - `keys`: the cloud's n cell keys in ascending order, `recs`:
// its records in that order.  The three x-neighbours of a cell are consecutive keys, so a row is one range of keys: nine lower bounds cover the 27
// cells.  visit(a, r, lk_c2c_d2(q, r)) is called for every record r at sorted place a of those cells - rows in ascending (z, y), keys ascending
// within a row, records of equal key in input order - whatever its distance; *seen (may be null): records visited.  Every neighbourhood of the
// map-cloud families is this walk with a visitor: the nearest record (below, lk_align.h), the moments (lk_mme.h), the k smallest (lk_sor.h), the
// count, the link and the nearest core point (lk_cluster.h).
// LK_C2C_WRAP_BUG (test aid of the host probe c2c_host.cc only): the x range as plain i - 1 .. i + 1, so that a row's range runs on into the next
// row's first cells.  The distance test still rejects what lies there - the result stands, the work does not: `seen` tells.
template <class Q, class V>
LK_C2C_HD void lk_c2c_walk(Q qx, Q qy, Q qz, const LkC2cGrid& g, const unsigned int* keys, const LkC2cRec* recs, unsigned int n, V& visit, unsigned int* seen) {
    unsigned int count = 0;
    long long lo[3], hi[3];
    bool any = lk_c2c_axis(qy, g.edge, g.mn[1], g.dv[1], &lo[1], &hi[1]) & lk_c2c_axis(qz, g.edge, g.mn[2], g.dv[2], &lo[2], &hi[2]);
#ifdef LK_C2C_WRAP_BUG
    lo[0] = lk_c2c_cell(qx, g.edge) - g.mn[0] - 1, hi[0] = lo[0] + 2;
#else
    any &= lk_c2c_axis(qx, g.edge, g.mn[0], g.dv[0], &lo[0], &hi[0]);
#endif
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
                    visit(a, r, lk_c2c_d2(qx, qy, qz, r.x, r.y, r.z));
                    ++count;
                }
            }
        }
    }
    if (seen) *seen = count;
}

// the record that minimises (d2, index) among those with d2 <= reach2; none: j = 0xffffffff, best = +inf
struct LkC2cNearest {
    double reach2, best;
    unsigned int j;
    LK_C2C_HD void operator()(unsigned int, const LkC2cRec& r, double d2) {
        if (lk_c2c_matched(d2, reach2) && (d2 < best || (d2 == best && r.idx < j))) best = d2, j = r.idx;
    }
};
// One query point against one reference cloud: *j, *d2 - the minimiser, or 0xffffffff and +inf; *seen (may be null): records whose distance was evaluated
template <class Q>
LK_C2C_HD void lk_c2c_search(Q qx, Q qy, Q qz, const LkC2cGrid& g, const unsigned int* keys, const LkC2cRec* recs, unsigned int n, double reach2,
                             unsigned int* j, double* d2, unsigned int* seen = nullptr) {
    LkC2cNearest v = {reach2, INFINITY, 0xffffffffu};
    lk_c2c_walk(qx, qy, qz, g, keys, recs, n, v, seen);
    *j = v.j, *d2 = v.best;
}
