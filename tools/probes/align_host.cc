// Host build of leg-kilo_amd/csrc/lk_align.h (with lk_c2c.h and lk_horn.h) for tests/test_align_host.py - a program of its own, the CPU twin of the
// device route of lk_clouds_align_dev (lk_align_kernels.h): bounds and status of the input clouds, lk_c2c_grid, the reference records sorted by
// (key, index), then the loop - lk_align_search per query point under T, the two passes of the solve with the device's summation order (256 lanes
// striding in ascending order, then the fixed tree), Horn, the step and the stop decision - and the final search's figures in
// lk_c2c_reduce_kernel's order.
//   g++ -O1 -g -ffp-contract=off -fno-builtin-floor -fsanitize=address,undefined,float-cast-overflow -o align_host align_host.cc
//   align_host file
// The file holds pairs one after the other, little endian: double max_dist, eps_rot, eps_trans, 12 doubles T0, uint64 max_iter, n_query, n_ref,
// n_query x 3 float32, n_ref x 3 float32.  Per pair a line
//   "pair <n_query> <n_ref> status <bits> iters <k> n_first <n> rmse_first <hex> step_rot <hex> step_trans <hex> n_last <n> rmse <hex> mean <hex> max <hex> worst <i>"
// goes out, a line "T" with the 12 entries as hex floats, and then a line "<j first search> <j final search> <d2 final as hex float>" per query
// point; j = 4294967295 and d2 = inf where the point is unmatched.  A truncated file is an error (exit status 2).
// -DLK_ALIGN_NO_GUARD: see lk_align.h - the search without the range guard; the test expects the sanitizers to stop the sheared case (guard_t0).
#include "../../leg-kilo_amd/csrc/lk_align.h"
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static void search_all(const double* T, const std::vector<float>& q, double max_dist, const HostIndex& x, std::vector<unsigned int>& j, std::vector<double>& d2) {
    const double reach2 = lk_c2c_reach2(max_dist);
    for (size_t i = 0; i < j.size(); ++i)
        lk_align_search(T, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, x.g, x.keys.data(), x.recs.data(), (unsigned int)x.recs.size(), reach2, &j[i], &d2[i]);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: align_host file\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "align_host: cannot open %s\n", argv[1]);
        return 2;
    }
    const double nan = NAN;
    for (;;) {
        double head[15];
        uint64_t n[3];
        const size_t got = fread(head, 1, sizeof(head), f);
        if (got == 0) break;
        if (got != sizeof(head) || !read_exact(f, n, sizeof(n)) || n[0] > 1000u || n[1] > 0x7fffffffu || n[2] > 0x7fffffffu) {
            fprintf(stderr, "align_host: truncated or oversized pair header\n");
            return 2;
        }
        const double max_dist = head[0], eps_rot = head[1], eps_trans = head[2];
        double T[12];
        memcpy(T, head + 3, sizeof(T));
        const uint64_t max_iter = n[0], nq = n[1];
        const unsigned int nr = (unsigned int)n[2];
        std::vector<float> q(3 * nq), r(3 * (size_t)nr);
        if (!read_exact(f, q.data(), 4 * q.size()) || !read_exact(f, r.data(), 4 * r.size())) {
            fprintf(stderr, "align_host: truncated cloud\n");
            return 2;
        }
        unsigned int status = host_status(q, max_dist) | host_status(r, max_dist);
        if (!lk_align_finite12(T)) status |= 16u;
        HostIndex x;
        host_index(r, nr, max_dist, !(status & 3u), x);
        std::vector<unsigned int> j(nq, 0xffffffffu), j_first(nq, 0xffffffffu);
        std::vector<double> d2(nq, INFINITY);
        uint64_t iters = 0, n_first = 0;
        double rmse_first = nan, step_rot = nan, step_trans = nan;
        bool stopped = false;
        for (bool first = true; first ? !status : true; first = false) {   // a status of the inputs or of T0: no search at all
            search_all(T, q, max_dist, x, j, d2);
            if (first) j_first = j;
            // the first pass: 256 lanes stride over the points in ascending order, then the fixed tree
            std::vector<LkAlignSums> part(256);
            for (unsigned int t = 0; t < 256; ++t) {
                lk_align_sums_zero(&part[t]);
                for (uint64_t i = t; i < nq; i += 256)
                    if (j[i] != 0xffffffffu)
                        lk_align_sums_term(&part[t], d2[i], q[3 * i], q[3 * i + 1], q[3 * i + 2], r[3 * (size_t)j[i]], r[3 * (size_t)j[i] + 1], r[3 * (size_t)j[i] + 2]);
            }
            for (unsigned int o = 128; o > 0; o >>= 1)
                for (unsigned int t = 0; t < o; ++t) lk_align_sums_merge(&part[t], part[t + o]);
            const LkAlignSums s = part[0];
            if (first) n_first = s.n, rmse_first = s.n ? sqrt(s.s2 / (double)s.n) : nan;
            if (iters == max_iter || stopped) break;
            if (s.n < 3) {
                status |= 4u;
                break;
            }
            double pbar[3], rbar[3];
            for (int c = 0; c < 3; ++c) pbar[c] = s.p[c] / (double)s.n, rbar[c] = s.r[c] / (double)s.n;
            std::vector<double> cov(256 * 9, 0.0);
            for (unsigned int t = 0; t < 256; ++t)
                for (uint64_t i = t; i < nq; i += 256)
                    if (j[i] != 0xffffffffu)
                        lk_align_cov_term(&cov[9 * t], pbar, rbar, q[3 * i], q[3 * i + 1], q[3 * i + 2], r[3 * (size_t)j[i]], r[3 * (size_t)j[i] + 1], r[3 * (size_t)j[i] + 2]);
            for (unsigned int o = 128; o > 0; o >>= 1)
                for (unsigned int t = 0; t < o; ++t)
                    for (int c = 0; c < 9; ++c) cov[9 * t + c] = cov[9 * t + c] + cov[9 * (t + o) + c];
            double Tn[12];
            lk_align_solve(cov.data(), pbar, rbar, Tn);
            lk_align_step(T, Tn, pbar, &step_rot, &step_trans);
            memcpy(T, Tn, sizeof(T));
            iters += 1;
            if (lk_align_converged(step_rot, step_trans, eps_rot, eps_trans)) status |= 8u, stopped = true;
        }
        // the final search's figures, in lk_c2c_reduce_kernel's order
        struct Part { double s2 = 0.0, s1 = 0.0, mx = 0.0; uint64_t n = 0; uint64_t worst = 0; };
        std::vector<Part> part(256);
        for (unsigned int t = 0; t < 256; ++t)
            for (uint64_t i = t; i < nq; i += 256) {
                if (j[i] == 0xffffffffu) continue;
                Part& p = part[t];
                p.s2 = p.s2 + d2[i], p.s1 = p.s1 + sqrt(d2[i]);
                if (!p.n || d2[i] > p.mx) p.mx = d2[i], p.worst = i;
                p.n += 1;
            }
        for (unsigned int o = 128; o > 0; o >>= 1)
            for (unsigned int t = 0; t < o; ++t) {
                Part &a = part[t], &b = part[t + o];
                if (b.n && (!a.n || b.mx > a.mx || (b.mx == a.mx && b.worst < a.worst))) a.mx = b.mx, a.worst = b.worst;
                a.s2 = a.s2 + b.s2, a.s1 = a.s1 + b.s1, a.n += b.n;
            }
        const Part& p = part[0];
        printf("pair %llu %u status %u iters %llu n_first %llu rmse_first %a step_rot %a step_trans %a n_last %llu rmse %a mean %a max %a worst %llu\n",
               (unsigned long long)nq, nr, status, (unsigned long long)iters, (unsigned long long)n_first, rmse_first, step_rot, step_trans, (unsigned long long)p.n,
               p.n ? sqrt(p.s2 / (double)p.n) : nan, p.n ? p.s1 / (double)p.n : nan, p.n ? sqrt(p.mx) : nan, (unsigned long long)(p.n ? p.worst : 0));
        printf("T");
        for (int c = 0; c < 12; ++c) printf(" %a", T[c]);
        printf("\n");
        for (uint64_t i = 0; i < nq; ++i) printf("%u %u %a\n", j_first[i], j[i], d2[i]);
    }
    fclose(f);
    return 0;
}
