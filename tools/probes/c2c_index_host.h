// The host twin of the index that the map-cloud kernels search (lk_c2c_kernels.h: bounds, grid, keys, sort, gather), for the probes next to this
// file - c2c_host.cc, mme_host.cc, align_host.cc, align_plane_host.cc, sor_host.cc, cluster_host.cc: the status bits of a cloud's coordinates, its
// bounds, lk_c2c_grid, a key per record, and the records sorted by (key, index) - std::sort in the place of the device's stable radix sort.
// Host only.  Include it behind the arithmetic header under test (mme_host.cc redefines floor in front of that one).
#pragma once
#include "../../leg-kilo_amd/csrc/lk_c2c.h"
#include <algorithm>
#include <utility>
#include <vector>

struct HostIndex {
    LkC2cGrid g;
    std::vector<unsigned int> keys;   // ascending
    std::vector<LkC2cRec> recs;       // in that order
};

// the status bits of n x 3 coordinates: 1 = a non-finite one, 2 = one out of range under the cell edge `reach`
static unsigned int host_status(const std::vector<float>& p, double reach) {
    unsigned int status = 0;
    for (float v : p) status |= !isfinite(v) ? 1u : lk_c2c_out_of_range(v, reach) ? 2u : 0u;
    return status;
}

// the index of the n records of p with `reach` as the cell edge; ok false (a status bit is set) or n = 0: the grid of nothing, records of zeros
static void host_index(const std::vector<float>& p, unsigned int n, double reach, bool ok, HostIndex& x) {
    lk_c2c_grid_of_nothing(reach, &x.g);
    x.keys.assign(n, 0u), x.recs.assign(n, LkC2cRec{});
    if (!ok || !n) return;
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = p[c];
    for (unsigned int i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) lo[c] = std::min(lo[c], p[3 * i + c]), hi[c] = std::max(hi[c], p[3 * i + c]);
    lk_c2c_grid(lo, hi, reach, &x.g);
    std::vector<std::pair<unsigned int, unsigned int>> order(n);
    for (unsigned int i = 0; i < n; ++i) order[i] = {lk_c2c_key(p[3 * i], p[3 * i + 1], p[3 * i + 2], x.g), i};
    std::sort(order.begin(), order.end());
    for (unsigned int i = 0; i < n; ++i) {
        const unsigned int s = order[i].second;
        x.keys[i] = order[i].first, x.recs[i] = LkC2cRec{p[3 * s], p[3 * s + 1], p[3 * s + 2], s};
    }
}
