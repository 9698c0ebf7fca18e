// Host build of leg-kilo_amd/csrc/lk_mme.h for tests/test_mme_host.py - a program of its own, the CPU twin of the device route of
// lk_clouds_mme_dev (lk_mme_kernels.h): bounds, lk_c2c_grid with the radius as the reach, a key per record, the records sorted by (key, index) -
// std::sort in the place of the stable radix sort - lk_mme_walk and lk_mme_finish per record, and the cloud's record summed as lk_mme_reduce_kernel
// sums it (256 lane-strided partial sums, then the halving tree).
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o mme_host mme_host.cc
//   mme_host file
// The file holds clouds one after the other, little endian: double radius, uint64 n, uint64 min_pts, n x 3 float32.  Per cloud a line
// "cloud <n> status <bits> edge <hex float> doublings <k> cells <dv0> <dv1> <dv2>" goes out, then a line "<n_i> <class> <h> <lmin> <seen>" per
// record in input order (h, lmin as hex floats, nan where the point has none; seen = records whose distance was evaluated), then
// "record <mme> <mpv> <h_max> <n_dense> <n_scored> <n_pairs> <worst>".  A cloud with a status bit prints every point as "0 0 nan nan 0", as the
// device does.  A truncated file is an error (exit status 2).
// -DMME_HOST_TRUNC (test aid): the cell of a coordinate by truncation instead of floor - the cell at 0 is then two edges wide, which the header
// line and `seen` of the around-zero case show.
#include <math.h>
#include <cmath>
#ifdef MME_HOST_TRUNC
#define floor trunc
#endif
#include "../../leg-kilo_amd/csrc/lk_mme.h"
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct Part {
    double sh = 0.0, sl = 0.0, mx = 0.0;
    unsigned long long pairs = 0, dense = 0, scored = 0;
    unsigned int worst = 0;
};
static void merge(Part& x, const Part& y) {
    if (y.scored && (!x.scored || y.mx > x.mx || (y.mx == x.mx && y.worst < x.worst))) x.mx = y.mx, x.worst = y.worst;
    x.sh = x.sh + y.sh, x.sl = x.sl + y.sl, x.pairs += y.pairs, x.dense += y.dense, x.scored += y.scored;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: mme_host file\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "mme_host: cannot open %s\n", argv[1]);
        return 2;
    }
    for (;;) {
        double radius;
        uint64_t hd[2];
        const size_t got = fread(&radius, 1, sizeof(radius), f);
        if (got == 0) break;
        if (got != sizeof(radius) || !read_exact(f, hd, sizeof(hd)) || hd[0] > 0x7fffffffu || hd[1] > 0xffffffffu) {
            fprintf(stderr, "mme_host: truncated or oversized cloud header\n");
            return 2;
        }
        const unsigned int n = (unsigned int)hd[0], min_pts = (unsigned int)hd[1];
        std::vector<float> p(3 * (size_t)n);
        if (!read_exact(f, p.data(), 4 * p.size())) {
            fprintf(stderr, "mme_host: truncated cloud\n");
            return 2;
        }
        const unsigned int status = host_status(p, radius);
        HostIndex x;
        host_index(p, n, radius, !status, x);
        const LkC2cGrid& g = x.g;
        const std::vector<unsigned int>& keys = x.keys;
        const std::vector<LkC2cRec>& recs = x.recs;
        printf("cloud %u status %u edge %a doublings %d cells %d %d %d\n", n, status, g.edge, g.doublings, g.dv[0], g.dv[1], g.dv[2]);
        const double reach2 = lk_c2c_reach2(radius);
        std::vector<unsigned int> cnt(n, 0u), cls(n, 0u), seen(n, 0u);
        std::vector<double> h(n, NAN), lmin(n, NAN);
        if (!status)
            for (unsigned int k = 0; k < n; ++k) {   // one sorted record after the other, as the device's threads take them
                const LkC2cRec q = recs[k];
                LkMmeAcc acc;
                lk_mme_walk(q.x, q.y, q.z, g, keys.data(), recs.data(), n, reach2, &acc, &seen[q.idx]);
                lk_mme_finish(acc, min_pts, &cls[q.idx], &h[q.idx], &lmin[q.idx]);
                cnt[q.idx] = acc.n;
            }
        for (unsigned int i = 0; i < n; ++i) printf("%u %u %a %a %u\n", cnt[i], cls[i], h[i], lmin[i], seen[i]);
        std::vector<Part> part(256);
        for (unsigned int t = 0; t < 256; ++t)
            for (unsigned int i = t; i < n; i += 256) {
                Part& x = part[t];
                x.pairs += cnt[i];
                if (lmin[i] == lmin[i]) x.sl = x.sl + lmin[i], x.dense += 1;
                if (h[i] == h[i]) {
                    x.sh = x.sh + h[i];
                    if (!x.scored || h[i] > x.mx) x.mx = h[i], x.worst = i;
                    x.scored += 1;
                }
            }
        for (unsigned int o = 128; o > 0; o >>= 1)
            for (unsigned int t = 0; t < o; ++t) merge(part[t], part[t + o]);
        const Part& r = part[0];
        printf("record %a %a %a %llu %llu %llu %u\n", r.scored ? r.sh / (double)r.scored : NAN, r.dense ? r.sl / (double)r.dense : NAN, r.scored ? r.mx : NAN, r.dense,
               r.scored, r.pairs, r.scored ? r.worst : 0u);
    }
    fclose(f);
    return 0;
}
