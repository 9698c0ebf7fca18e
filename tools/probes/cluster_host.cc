// Host build of leg-kilo_amd/csrc/lk_cluster.h for tests/test_cluster_host.py - a program of its own, the CPU twin of the device route of
// lk_clouds_cluster_dev (lk_cluster_kernels.h): bounds, lk_c2c_grid with the reach as the cell edge, a key per record, the records sorted by (key,
// index) - std::sort in the place of the stable radix sort - then the kernels' phases one sorted record after the other: lk_c2c_walk with the
// count visitor, with the link visitor over the union-find, the roots and the nearest core candidate of every other point, a number per root in
// ascending order, the sizes, the record and the keep flags.
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o cluster_host cluster_host.cc
//   cluster_host file
// The file holds clouds one after the other, little endian: double reach, uint64 n, min_pts, min_size, max_size, flags, n x 3 float32.  Per cloud a
// line "cloud <n> status <bits> edge <hex float> doublings <d> cells <dv0> <dv1> <dv2>" goes out, then a line "<n_i> <kind> <label> <keep> <seen>"
// per record in input order (seen = records the count walk looked at), then "clusters <k>" and a line "<size> <first>" per cluster, then
// "record <n_core> <n_border> <n_noise> <n_kept> <n_clusters> <n_kept_clusters> <largest> <largest_size>".  A cloud with a status bit prints every
// point as "0 0 4294967295 0 0", as the device does.  A truncated file is an error (exit status 2).
#include <math.h>
#include <cmath>
#include "../../leg-kilo_amd/csrc/lk_cluster.h"
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: cluster_host file\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cluster_host: cannot open %s\n", argv[1]);
        return 2;
    }
    for (;;) {
        double reach;
        uint64_t hd[5];
        const size_t got = fread(&reach, 1, sizeof(reach), f);
        if (got == 0) break;
        if (got != sizeof(reach) || !read_exact(f, hd, sizeof(hd)) || hd[0] > 0x7fffffffu || hd[1] == 0 || hd[1] > 0xffffffffu || hd[2] > hd[3] || hd[3] > 0xffffffffu || hd[4] > 1) {
            fprintf(stderr, "cluster_host: truncated or invalid cloud header\n");
            return 2;
        }
        const unsigned int n = (unsigned int)hd[0], min_pts = (unsigned int)hd[1], min_size = (unsigned int)hd[2], max_size = (unsigned int)hd[3];
        const bool keep_largest = hd[4] != 0;
        std::vector<float> p(3 * (size_t)n);
        if (!read_exact(f, p.data(), 4 * p.size())) {
            fprintf(stderr, "cluster_host: truncated cloud\n");
            return 2;
        }
        const unsigned int status = host_status(p, reach);
        HostIndex x;
        host_index(p, n, reach, !status, x);
        const LkC2cGrid& g = x.g;
        const std::vector<unsigned int>& keys = x.keys;
        const std::vector<LkC2cRec>& recs = x.recs;
        printf("cloud %u status %u edge %a doublings %d cells %d %d %d\n", n, status, g.edge, g.doublings, g.dv[0], g.dv[1], g.dv[2]);
        const double reach2 = lk_c2c_reach2(reach);
        std::vector<unsigned int> cnt(n, 0u), seen(n, 0u), parent(n), root(n, LK_CLUSTER_NONE);
        std::vector<unsigned char> core(n, 0), kind(n, 0);   // core: sorted order, kind: input order
        for (unsigned int i = 0; i < n; ++i) parent[i] = i;
        if (!status) {
            for (unsigned int s = 0; s < n; ++s) {   // count
                const LkC2cRec q = recs[s];
                LkClusterCount v = {reach2, 0u};
                lk_c2c_walk(q.x, q.y, q.z, g, keys.data(), recs.data(), n, v, &seen[q.idx]);
                cnt[q.idx] = v.n, core[s] = lk_cluster_is_core(v.n, min_pts) ? 1 : 0, kind[q.idx] = core[s] ? 2 : 0;
            }
            for (unsigned int s = 0; s < n; ++s) {   // link
                if (!core[s]) continue;
                const LkC2cRec q = recs[s];
                LkClusterLink v = {reach2, core.data(), parent.data(), 0u, q.idx};
                lk_c2c_walk(q.x, q.y, q.z, g, keys.data(), recs.data(), n, v, nullptr);
            }
            for (unsigned int s = 0; s < n; ++s) {   // assign
                const LkC2cRec q = recs[s];
                if (core[s]) {
                    root[q.idx] = lk_cluster_root(parent.data(), q.idx);
                    continue;
                }
                LkClusterNearest v = {reach2, core.data(), INFINITY, LK_CLUSTER_NONE};
                lk_c2c_walk(q.x, q.y, q.z, g, keys.data(), recs.data(), n, v, nullptr);
                if (v.j != LK_CLUSTER_NONE) root[q.idx] = lk_cluster_root(parent.data(), v.j), kind[q.idx] = 1;
            }
        }
        std::vector<unsigned int> scan(n + 1, 0u);   // ids: the exclusive scan of the root flags
        for (unsigned int i = 0; i < n; ++i) scan[i + 1] = scan[i] + (root[i] == i ? 1u : 0u);
        const unsigned int k = scan[n];
        std::vector<unsigned int> size(k, 0u), first(k, 0u), label(n, LK_CLUSTER_NONE);
        for (unsigned int i = 0; i < n; ++i) {
            if (root[i] == LK_CLUSTER_NONE) continue;
            label[i] = scan[root[i]], size[label[i]] += 1u;
            if (root[i] == i) first[label[i]] = i;
        }
        unsigned int best_id = LK_CLUSTER_NONE, best_size = 0, keep_id = LK_CLUSTER_NONE, keep_size = 0, in_bounds = 0;
        unsigned long long kept_pts = 0, n_core = 0, n_border = 0;
        for (unsigned int c = 0; c < k; ++c) {
            if (lk_cluster_larger(size[c], c, best_size, best_id)) best_size = size[c], best_id = c;
            if (!lk_cluster_in_bounds(size[c], min_size, max_size)) continue;
            in_bounds += 1, kept_pts += size[c];
            if (lk_cluster_larger(size[c], c, keep_size, keep_id)) keep_size = size[c], keep_id = c;
        }
        for (unsigned int i = 0; i < n; ++i) {
            const bool keep = label[i] != LK_CLUSTER_NONE && (keep_largest ? label[i] == keep_id : lk_cluster_in_bounds(size[label[i]], min_size, max_size));
            n_core += kind[i] == 2, n_border += kind[i] == 1;
            printf("%u %u %u %u %u\n", cnt[i], (unsigned int)kind[i], label[i], keep ? 1u : 0u, seen[i]);
        }
        printf("clusters %u\n", k);
        for (unsigned int c = 0; c < k; ++c) printf("%u %u\n", size[c], first[c]);
        const bool any = keep_id != LK_CLUSTER_NONE;
        printf("record %llu %llu %llu %llu %u %u %u %u\n", n_core, n_border, status ? 0ull : n - n_core - n_border,
               keep_largest ? (any ? (unsigned long long)keep_size : 0ull) : kept_pts, k, keep_largest ? (any ? 1u : 0u) : in_bounds, best_id != LK_CLUSTER_NONE ? best_id : 0u,
               best_id != LK_CLUSTER_NONE ? best_size : 0u);
    }
    fclose(f);
    return 0;
}
