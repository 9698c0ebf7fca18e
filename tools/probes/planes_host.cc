// Host build of leg-kilo_amd/csrc/lk_planes.h for tests/test_planes_host.py - a program of its own, the CPU twin of the device route of
// lk_clouds_planes_dev (lk_planes_kernels.h): the status word, then per round the remainder compacted in input order, lk_planes_sample and
// lk_planes_hyp per hypothesis, lk_planes_inlier per (hypothesis, record), lk_planes_better over the scores, the winner's test again per record; behind
// the rounds per plane the sums in the refit kernel's order - lane t of 256 takes the cloud's records t, t + 256, ..., a halving tree - and
// lk_planes_fit.
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o planes_host planes_host.cc
//   planes_host file
//   planes_host --sample seed r h0 count m
// The file holds clouds one after the other, little endian: double dist, cos_max_angle, axis[3]; uint64 n, n_hyp, max_planes, min_inliers, seed,
// flags (bit 0: LK_PLANES_KEEP_PLANES, bit 1: the axis is given); n x 3 float32.  Per cloud a line "cloud <n> status <bits>" goes out, then a line
// "round <r> m <m> winner <h> score <s>" per round that ran (winner 4294967295: none), then "<label> <keep>" per record in input order, then
// "planes <k>" and per plane "<n_inliers> <hyp>" followed by normal[3], d, centroid[3], eig[3], rmse as hexadecimal floats, then
// "record <n_on_planes> <n_rest> <n_kept>".  --sample prints "<i0> <i1> <i2>" for the hypotheses h0 .. h0 + count - 1 of round r on a remainder
// of m records.  A truncated file is an error (exit status 2).
#include "../../leg-kilo_amd/csrc/lk_planes.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

// v[0 .. n) in the refit kernel's order; take(i): whether record i takes part, val(i): its term
template <class Take, class Val>
static double tree_sum(unsigned int n, Take take, Val val) {
    double part[256];
    for (unsigned int t = 0; t < 256; ++t) {
        double s = 0.0;
        for (unsigned int i = t; i < n; i += 256u)
            if (take(i)) s = s + val(i);
        part[t] = s;
    }
    for (unsigned int o = 128; o > 0; o >>= 1)
        for (unsigned int t = 0; t < o; ++t) part[t] = part[t] + part[t + o];
    return part[0];
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "--sample")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0);
        const uint32_t r = (uint32_t)strtoul(argv[3], nullptr, 0), h0 = (uint32_t)strtoul(argv[4], nullptr, 0), count = (uint32_t)strtoul(argv[5], nullptr, 0);
        const uint32_t m = (uint32_t)strtoul(argv[6], nullptr, 0);
        if (m < 3) return 2;
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t i[3];
            lk_planes_sample(seed, r, h0 + k, m, i);
            printf("%u %u %u\n", i[0], i[1], i[2]);
        }
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: planes_host file | planes_host --sample seed r h0 count m\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "planes_host: cannot open %s\n", argv[1]);
        return 2;
    }
    for (;;) {
        double par[5];
        uint64_t hd[6];
        const size_t got = fread(par, 1, sizeof(par), f);
        if (got == 0) break;
        if (got != sizeof(par) || !read_exact(f, hd, sizeof(hd)) || hd[0] > 0x7fffffffu || hd[1] == 0 || hd[1] > LK_PLANES_HYP_LIMIT || hd[2] == 0 || hd[2] > 16 || hd[3] < 3 ||
            hd[3] > 0xffffffffu || hd[5] > 3) {
            fprintf(stderr, "planes_host: truncated or invalid cloud header\n");
            return 2;
        }
        const unsigned int n = (unsigned int)hd[0], n_hyp = (unsigned int)hd[1], max_planes = (unsigned int)hd[2], min_inliers = (unsigned int)hd[3];
        const uint64_t seed = hd[4];
        const bool keep_planes = hd[5] & 1u;
        const LkPlanesAxis axis = lk_planes_axis((hd[5] & 2u) ? par + 2 : nullptr, par[1]);
        const double dist2 = par[0] * par[0];
        std::vector<float> p(3 * (size_t)n);
        if (!read_exact(f, p.data(), 4 * p.size())) {
            fprintf(stderr, "planes_host: truncated cloud\n");
            return 2;
        }
        unsigned int status = 0;
        for (float v : p) status |= !isfinite(v) ? 1u : !(fabs((double)v) < 1073741824.0) ? 2u : 0u;
        printf("cloud %u status %u\n", n, status);
        std::vector<unsigned int> label(n, LK_PLANES_NONE), n_in, hyp_of;
        std::vector<unsigned char> alive(n, status ? 0 : 1);
        for (unsigned int r = 0; r < max_planes && !status; ++r) {
            std::vector<float> rem;   // the remainder, in input order
            for (unsigned int i = 0; i < n; ++i)
                if (alive[i]) rem.insert(rem.end(), p.begin() + 3 * (size_t)i, p.begin() + 3 * (size_t)i + 3);
            const unsigned int m = (unsigned int)(rem.size() / 3);
            if (!lk_planes_runs(m, min_inliers)) break;
            unsigned int best = 0, best_h = LK_PLANES_NONE;
            for (unsigned int h = 0; h < n_hyp; ++h) {
                uint32_t s[3];
                lk_planes_sample(seed, r, h, m, s);
                const LkPlanesHyp hy = lk_planes_hyp(&rem[3 * (size_t)s[0]], &rem[3 * (size_t)s[1]], &rem[3 * (size_t)s[2]], dist2, axis);
                unsigned int score = 0;
                for (unsigned int j = 0; j < m; ++j) score += lk_planes_inlier(hy, rem[3 * (size_t)j], rem[3 * (size_t)j + 1], rem[3 * (size_t)j + 2]) ? 1u : 0u;
                if (lk_planes_better(score, h, best, best_h)) best = score, best_h = h;
            }
            const bool none = best < min_inliers;
            printf("round %u m %u winner %u score %u\n", r, m, none ? LK_PLANES_NONE : best_h, best);
            if (none) break;
            uint32_t s[3];
            lk_planes_sample(seed, r, best_h, m, s);
            const LkPlanesHyp hy = lk_planes_hyp(&rem[3 * (size_t)s[0]], &rem[3 * (size_t)s[1]], &rem[3 * (size_t)s[2]], dist2, axis);
            for (unsigned int i = 0; i < n; ++i)
                if (alive[i] && lk_planes_inlier(hy, p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2])) alive[i] = 0, label[i] = r;
            n_in.push_back(best), hyp_of.push_back(best_h);
        }
        unsigned long long on = 0, kept = 0;
        for (unsigned int i = 0; i < n; ++i) {
            const bool keep = !status && (keep_planes ? label[i] != LK_PLANES_NONE : alive[i] != 0);
            on += label[i] != LK_PLANES_NONE, kept += keep;
            printf("%u %u\n", label[i], keep ? 1u : 0u);
        }
        printf("planes %zu\n", n_in.size());
        for (unsigned int r = 0; r < n_in.size(); ++r) {
            auto take = [&](unsigned int i) { return label[i] == r; };
            unsigned int cnt = 0;
            for (unsigned int i = 0; i < n; ++i) cnt += take(i);
            double cen[3], cs[6];
            for (int k = 0; k < 3; ++k) cen[k] = tree_sum(n, take, [&](unsigned int i) { return (double)p[3 * (size_t)i + k]; }) / (double)cnt;
            const int ij[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
            for (int k = 0; k < 6; ++k)
                cs[k] = tree_sum(n, take, [&](unsigned int i) { return ((double)p[3 * (size_t)i + ij[k][0]] - cen[ij[k][0]]) * ((double)p[3 * (size_t)i + ij[k][1]] - cen[ij[k][1]]); });
            LkPlanesFit ft;
            lk_planes_fit(cen, cs, cnt, axis, &ft);
            printf("%u %u %a %a %a %a %a %a %a %a %a %a %a\n", n_in[r], hyp_of[r], ft.normal[0], ft.normal[1], ft.normal[2], ft.d, ft.centroid[0], ft.centroid[1], ft.centroid[2],
                   ft.eig[0], ft.eig[1], ft.eig[2], ft.rmse);
        }
        printf("record %llu %llu %llu\n", on, status ? 0ull : n - on, kept);
    }
    fclose(f);
    return 0;
}
