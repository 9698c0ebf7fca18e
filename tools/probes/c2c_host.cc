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
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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
        const unsigned int status = host_status(q, max_dist) | host_status(r, max_dist), nr = (unsigned int)n[1];
        HostIndex x;
        host_index(r, nr, max_dist, !status, x);
        const LkC2cGrid& g = x.g;
        printf("pair %llu %llu status %u edge %a doublings %d cells %d %d %d\n", (unsigned long long)n[0], (unsigned long long)n[1], status, g.edge, g.doublings,
               g.dv[0], g.dv[1], g.dv[2]);
        const double reach2 = lk_c2c_reach2(max_dist);
        for (uint64_t i = 0; i < n[0]; ++i) {
            unsigned int j = 0xffffffffu, seen = 0;
            double d2 = INFINITY;
            if (!status) lk_c2c_search(q[3 * i], q[3 * i + 1], q[3 * i + 2], g, x.keys.data(), x.recs.data(), nr, reach2, &j, &d2, &seen);
            printf("%u %a %u\n", j, d2, seen);
        }
    }
    fclose(f);
    return 0;
}
