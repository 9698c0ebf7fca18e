// Host build of leg-kilo_amd/csrc/lk_sor.h for tests/test_sor_host.py - a program of its own, the CPU twin of the device route of
// lk_clouds_sor_dev (lk_sor_kernels.h): bounds, lk_c2c_grid with the reach as the cell edge, a key per record, the records sorted by (key, index) -
// std::sort in the place of the stable radix sort - lk_sor_walk and lk_sor_finish per record with the list capacity the device would take for k,
// and the cloud's statistics summed as lk_sor_stats_kernel sums them (256 lane-strided partial sums, then the halving tree; the mean first, the
// centred squares second).
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o sor_host sor_host.cc
//   sor_host file
// The file holds clouds one after the other, little endian: double reach, double n_sigma, uint64 n, uint64 k, n x 3 float32.  Per cloud a line
// "cloud <n> status <bits> edge <hex float> doublings <d> cells <dv0> <dv1> <dv2> cap <list capacity>" goes out, then a line
// "<cnt_i> <keep_i> <dbar_i> <seen>" per record in input order (dbar as a hex float, nan where the point is isolated; seen = records the walk
// looked at), then "record <mu> <sigma> <thr> <n_isolated> <n_outliers> <n_kept> <worst>".  A cloud with a status bit prints every point as
// "0 0 nan 0", as the device does.  A truncated file is an error (exit status 2).
#include <math.h>
#include <cmath>
#include "../../leg-kilo_amd/csrc/lk_sor.h"
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct Part {
    double s = 0.0, mx = 0.0;
    unsigned long long ns = 0, iso = 0;
    unsigned int worst = 0;
};
static void merge(Part& x, const Part& y) {
    if (y.ns && (!x.ns || y.mx > x.mx || (y.mx == x.mx && y.worst < x.worst))) x.mx = y.mx, x.worst = y.worst;
    x.s = x.s + y.s, x.ns += y.ns, x.iso += y.iso;
}

template <int CAP>
static void points(const LkC2cGrid& g, const std::vector<unsigned int>& keys, const std::vector<LkC2cRec>& recs, double reach2, unsigned int k,
                   std::vector<unsigned int>& cnt, std::vector<double>& dbar, std::vector<unsigned int>& seen) {
    const unsigned int n = (unsigned int)recs.size();
    for (unsigned int s = 0; s < n; ++s) {   // one sorted record after the other, as the device's threads take them
        const LkC2cRec q = recs[s];
        LkSorList<CAP> list;
        lk_sor_walk(q.x, q.y, q.z, q.idx, g, keys.data(), recs.data(), n, reach2, &list, &seen[q.idx]);
        dbar[q.idx] = lk_sor_finish(list, k), cnt[q.idx] = list.cnt;
    }
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: sor_host file\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "sor_host: cannot open %s\n", argv[1]);
        return 2;
    }
    for (;;) {
        double par[2];
        uint64_t hd[2];
        const size_t got = fread(par, 1, sizeof(par), f);
        if (got == 0) break;
        if (got != sizeof(par) || !read_exact(f, hd, sizeof(hd)) || hd[0] > 0x7fffffffu || hd[1] == 0 || hd[1] > LK_SOR_CAP_BIG) {
            fprintf(stderr, "sor_host: truncated or oversized cloud header\n");
            return 2;
        }
        const double reach = par[0], n_sigma = par[1];
        const unsigned int n = (unsigned int)hd[0], k = (unsigned int)hd[1];
        std::vector<float> p(3 * (size_t)n);
        if (!read_exact(f, p.data(), 4 * p.size())) {
            fprintf(stderr, "sor_host: truncated cloud\n");
            return 2;
        }
        const unsigned int status = host_status(p, reach);
        HostIndex x;
        host_index(p, n, reach, !status, x);
        const LkC2cGrid& g = x.g;
        const std::vector<unsigned int>& keys = x.keys;
        const std::vector<LkC2cRec>& recs = x.recs;
        const int cap = lk_sor_cap_of(k);
        printf("cloud %u status %u edge %a doublings %d cells %d %d %d cap %d\n", n, status, g.edge, g.doublings, g.dv[0], g.dv[1], g.dv[2], cap);
        const double reach2 = lk_c2c_reach2(reach);
        std::vector<unsigned int> cnt(n, 0u), seen(n, 0u);
        std::vector<double> dbar(n, NAN);
        if (!status) {
            if (cap == LK_SOR_CAP_SMALL) points<LK_SOR_CAP_SMALL>(g, keys, recs, reach2, k, cnt, dbar, seen);
            else if (cap == LK_SOR_CAP_MID) points<LK_SOR_CAP_MID>(g, keys, recs, reach2, k, cnt, dbar, seen);
            else points<LK_SOR_CAP_BIG>(g, keys, recs, reach2, k, cnt, dbar, seen);
        }
        std::vector<Part> part(256);
        for (unsigned int t = 0; t < 256; ++t)
            for (unsigned int i = t; i < n; i += 256) {
                Part& x = part[t];
                const double d = dbar[i];
                if (d == d) {
                    x.s = x.s + d;
                    if (!x.ns || d > x.mx) x.mx = d, x.worst = i;
                    x.ns += 1;
                } else {
                    x.iso += 1;
                }
            }
        for (unsigned int o = 128; o > 0; o >>= 1)
            for (unsigned int t = 0; t < o; ++t) merge(part[t], part[t + o]);
        const Part& r = part[0];
        const bool any = !status && r.ns;
        const double mu = any ? r.s / (double)r.ns : NAN;
        std::vector<double> sq(256, 0.0);
        for (unsigned int t = 0; t < 256; ++t)
            for (unsigned int i = t; i < n; i += 256)
                if (dbar[i] == dbar[i]) {
                    const double e = dbar[i] - mu;
                    sq[t] = sq[t] + e * e;
                }
        for (unsigned int o = 128; o > 0; o >>= 1)
            for (unsigned int t = 0; t < o; ++t) sq[t] = sq[t] + sq[t + o];
        const double sigma = any ? lk_sor_sigma(sq[0], r.ns) : NAN, thr = any ? lk_sor_thr(mu, sigma, n_sigma) : NAN;
        unsigned long long kept = 0;
        for (unsigned int i = 0; i < n; ++i) {
            const bool keep = lk_sor_kept(dbar[i], thr);
            kept += keep ? 1 : 0;
            printf("%u %u %a %u\n", cnt[i], keep ? 1u : 0u, dbar[i], seen[i]);
        }
        printf("record %a %a %a %llu %llu %llu %u\n", mu, sigma, thr, status ? 0ull : r.iso, status ? 0ull : r.ns - kept, kept, any ? r.worst : 0u);
    }
    fclose(f);
    return 0;
}
