// Host build of leg-kilo_amd/csrc/lk_c2c.h for tests/test_c2c_host.py - a program of its own, the CPU twin of the device route of
// lk_clouds_c2c_dev (lk_c2c_kernels.h): bounds, lk_c2c_grid, a key per reference record, the records sorted by (key, index) - std::sort in the place of
// the stable radix sort - and lk_c2c_search per query point.
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o c2c_host c2c_host.cc
//   c2c_host file
// The file holds pairs of clouds one after the other, little endian: double max_dist, uint64 n_query, uint64 n_ref, n_query x 3 float32, n_ref x 3
// float32.  Per pair a line "pair <n_query> <n_ref> status <bits> edge <hex float> doublings <k> cells <dv0> <dv1> <dv2>" goes out and then a line
// "<j> <d2 as hex float> <seen>" per query point: j = 4294967295 and d2 = inf where the point is unmatched, seen = reference records whose distance
// was evaluated.  A pair with a status bit prints every point as unmatched, as the device does.  A truncated file is an error (exit status 2).
// -DLK_C2C_WRAP_BUG: see lk_c2c.h - the x range of a row unclipped; the test expects the wrap case's `seen` to show it.
#include "../../leg-kilo_amd/csrc/lk_c2c.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: c2c_host file\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "c2c_host: cannot open %s\n", argv[1]);
        return 2;
    }
    for (;;) {
        double max_dist;
        uint64_t n[2];
        const size_t got = fread(&max_dist, 1, sizeof(max_dist), f);
        if (got == 0) break;
        if (got != sizeof(max_dist) || !read_exact(f, n, sizeof(n)) || n[0] > 0x7fffffffu || n[1] > 0x7fffffffu) {
            fprintf(stderr, "c2c_host: truncated or oversized pair header\n");
            return 2;
        }
        std::vector<float> q(3 * n[0]), r(3 * n[1]);
        if (!read_exact(f, q.data(), 4 * q.size()) || !read_exact(f, r.data(), 4 * r.size())) {
            fprintf(stderr, "c2c_host: truncated cloud\n");
            return 2;
        }
        unsigned int status = 0;
        for (const std::vector<float>* c : {&q, &r})
            for (float v : *c) status |= !isfinite(v) ? 1u : lk_c2c_out_of_range(v, max_dist) ? 2u : 0u;
        const unsigned int nr = (unsigned int)n[1];
        LkC2cGrid g;
        lk_c2c_grid_of_nothing(max_dist, &g);
        std::vector<unsigned int> keys(nr);
        std::vector<LkC2cRec> recs(nr);
        if (!status && nr) {
            float lo[3], hi[3];
            for (int c = 0; c < 3; ++c) lo[c] = hi[c] = r[c];
            for (unsigned int i = 0; i < nr; ++i)
                for (int c = 0; c < 3; ++c) lo[c] = std::min(lo[c], r[3 * i + c]), hi[c] = std::max(hi[c], r[3 * i + c]);
            lk_c2c_grid(lo, hi, max_dist, &g);
            std::vector<std::pair<unsigned int, unsigned int>> order(nr);
            for (unsigned int i = 0; i < nr; ++i) order[i] = {lk_c2c_key(r[3 * i], r[3 * i + 1], r[3 * i + 2], g), i};
            std::sort(order.begin(), order.end());
            for (unsigned int i = 0; i < nr; ++i) {
                const unsigned int s = order[i].second;
                keys[i] = order[i].first, recs[i] = LkC2cRec{r[3 * s], r[3 * s + 1], r[3 * s + 2], s};
            }
        }
        printf("pair %llu %llu status %u edge %a doublings %d cells %d %d %d\n", (unsigned long long)n[0], (unsigned long long)n[1], status, g.edge, g.doublings,
               g.dv[0], g.dv[1], g.dv[2]);
        const double reach2 = lk_c2c_reach2(max_dist);
        for (uint64_t i = 0; i < n[0]; ++i) {
            unsigned int j = 0xffffffffu, seen = 0;
            double d2 = INFINITY;
            if (!status) lk_c2c_search(q[3 * i], q[3 * i + 1], q[3 * i + 2], g, keys.data(), recs.data(), nr, reach2, &j, &d2, &seen);
            printf("%u %a %u\n", j, d2, seen);
        }
    }
    fclose(f);
    return 0;
}
