// Host build of leg-kilo_amd/csrc/lk_align_plane.h and lk_normals.h (with lk_align.h, lk_mme.h, lk_eig3.h and lk_horn.h) for tests/test_plane_host.py
// - a program of its own, the CPU twin of the device routes of lk_clouds_align_plane_dev (lk_align_plane_kernels.h) and lk_clouds_normals_dev
// (lk_normals_kernels.h): bounds and status of the input clouds, lk_c2c_grid, the records sorted by (key, index), and then either the alignment loop
// - lk_align_search per query point under T, the two passes of the plane solve with the device's summation order (256 lanes striding in ascending
// order, then the fixed tree), the scaled Cholesky solve, the update, the step and the stop decision - or lk_mme_walk and lk_normals_finish per record.
//   g++ -O1 -g -ffp-contract=off -fno-builtin-floor -fsanitize=address,undefined,float-cast-overflow -o align_plane_host align_plane_host.cc
//   align_plane_host align file | align_plane_host normals file
// align: the file holds pairs one after the other, little endian: double max_dist, eps_rot, eps_trans, 12 doubles T0, uint64 max_iter, n_query, n_ref,
// n_query x 3 float32, n_ref x 3 float32, n_ref x 3 float32 normals.  Per pair a line
//   "pair <n_query> <n_ref> status <bits> iters <k> n_first <n> rmse_first <hex> step_rot <hex> step_trans <hex> n_last <n> rmse <hex> mean <hex> max <hex> worst <i>
//    used_first <n> plane_first <hex> used <n> plane <hex>"
// goes out, a line "T" with the 12 entries as hex floats, and then a line "<j first search> <j final search> <d2 final as hex float>" per query point.
// normals: clouds one after the other: double radius, double min_planarity, uint64 n, uint64 min_pts, n x 3 float32.  Per cloud a line
// "cloud <n> status <bits> valid <n_valid>", then "<n_i> <nx> <ny> <nz> <w>" per record in input order (hex floats).
// A truncated file is an error (exit status 2).
// Test aids: -DLK_ALIGN_PLANE_ORIGIN, -DLK_ALIGN_PLANE_NO_ORTHO (lk_align_plane.h), -DLK_NORMALS_SIGN_F32 (lk_normals.h).
#include "../../leg-kilo_amd/csrc/lk_align_plane.h"
#include "../../leg-kilo_amd/csrc/lk_normals.h"
#include "c2c_index_host.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static int run_normals(FILE* f) {
    for (;;) {
        double hd[2];
        uint64_t n2[2];
        const size_t got = fread(hd, 1, sizeof(hd), f);
        if (got == 0) break;
        if (got != sizeof(hd) || !read_exact(f, n2, sizeof(n2)) || n2[0] > 0x7fffffffu || n2[1] > 0xffffffffu) {
            fprintf(stderr, "align_plane_host: truncated or oversized cloud header\n");
            return 2;
        }
        const double radius = hd[0], min_planarity = hd[1];
        const unsigned int n = (unsigned int)n2[0], min_pts = (unsigned int)n2[1];
        std::vector<float> p(3 * (size_t)n);
        if (!read_exact(f, p.data(), 4 * p.size())) {
            fprintf(stderr, "align_plane_host: truncated cloud\n");
            return 2;
        }
        const unsigned int status = host_status(p, radius);
        HostIndex x;
        host_index(p, n, radius, !status, x);
        const double reach2 = lk_c2c_reach2(radius);
        std::vector<unsigned int> cnt(n, 0u);
        std::vector<float> rec(4 * (size_t)n, NAN);
        unsigned long long valid = 0;
        if (!status)
            for (unsigned int k = 0; k < n; ++k) {   // one sorted record after the other, as the device's threads take them
                const LkC2cRec q = x.recs[k];
                LkMmeAcc acc;
                lk_mme_walk(q.x, q.y, q.z, x.g, x.keys.data(), x.recs.data(), n, reach2, &acc, nullptr);
                valid += lk_normals_finish(acc, min_pts, min_planarity, &rec[4 * (size_t)q.idx]) ? 1u : 0u;
                cnt[q.idx] = acc.n;
            }
        printf("cloud %u status %u valid %llu\n", n, status, valid);
        for (unsigned int i = 0; i < n; ++i) printf("%u %a %a %a %a\n", cnt[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
    }
    return 0;
}

static int run_align(FILE* f) {
    const double nan = NAN;
    for (;;) {
        double head[15];
        uint64_t n[3];
        const size_t got = fread(head, 1, sizeof(head), f);
        if (got == 0) break;
        if (got != sizeof(head) || !read_exact(f, n, sizeof(n)) || n[0] > 1000u || n[1] > 0x7fffffffu || n[2] > 0x7fffffffu) {
            fprintf(stderr, "align_plane_host: truncated or oversized pair header\n");
            return 2;
        }
        const double max_dist = head[0], eps_rot = head[1], eps_trans = head[2];
        double T[12];
        memcpy(T, head + 3, sizeof(T));
        const uint64_t max_iter = n[0], nq = n[1];
        const unsigned int nr = (unsigned int)n[2];
        std::vector<float> q(3 * nq), r(3 * (size_t)nr), nm(3 * (size_t)nr);
        if (!read_exact(f, q.data(), 4 * q.size()) || !read_exact(f, r.data(), 4 * r.size()) || !read_exact(f, nm.data(), 4 * nm.size())) {
            fprintf(stderr, "align_plane_host: truncated cloud\n");
            return 2;
        }
        unsigned int status = host_status(q, max_dist) | host_status(r, max_dist);
        if (!lk_align_finite12(T)) status |= 16u;
        HostIndex x;
        host_index(r, nr, max_dist, !(status & 3u), x);
        const double reach2 = lk_c2c_reach2(max_dist);
        std::vector<unsigned int> j(nq, 0xffffffffu), j_first(nq, 0xffffffffu);
        std::vector<double> d2(nq, INFINITY);
        uint64_t iters = 0, n_first = 0, used_first = 0, used = 0;
        double rmse_first = nan, step_rot = nan, step_trans = nan, plane_first = nan, plane = nan;
        bool stopped = false;
        for (bool first = true; first ? !status : true; first = false) {   // a status of the inputs or of T0: no search at all
            for (size_t i = 0; i < nq; ++i)
                lk_align_search(T, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, x.g, x.keys.data(), x.recs.data(), nr, reach2, &j[i], &d2[i]);
            if (first) j_first = j;
            // the first pass: 256 lanes stride over the points in ascending order, then the fixed tree
            std::vector<LkPlaneSums> part(256);
            for (unsigned int t = 0; t < 256; ++t) {
                lk_plane_sums_zero(&part[t]);
                for (uint64_t i = t; i < nq; i += 256) {
                    if (j[i] == 0xffffffffu) continue;
                    const size_t k = 3 * (size_t)j[i];
                    lk_plane_sums_term(&part[t], T, d2[i], q[3 * i], q[3 * i + 1], q[3 * i + 2], r[k], r[k + 1], r[k + 2], nm[k], nm[k + 1], nm[k + 2]);
                }
            }
            for (unsigned int o = 128; o > 0; o >>= 1)
                for (unsigned int t = 0; t < o; ++t) lk_plane_sums_merge(&part[t], part[t + o]);
            const LkPlaneSums s = part[0];
            used = s.nu, plane = s.nu ? sqrt(s.e2 / (double)s.nu) : nan;
            if (first) n_first = s.n, rmse_first = s.n ? sqrt(s.s2 / (double)s.n) : nan, used_first = used, plane_first = plane;
            if (iters == max_iter || stopped) break;
            if (s.nu < LK_ALIGN_PLANE_MIN_USED) {
                status |= 4u;
                break;
            }
            double mbar[3], pbar[3];
            for (int c = 0; c < 3; ++c) mbar[c] = s.m[c] / (double)s.nu, pbar[c] = s.p[c] / (double)s.nu;
            std::vector<double> hg(256 * 27, 0.0);
            for (unsigned int t = 0; t < 256; ++t)
                for (uint64_t i = t; i < nq; i += 256) {
                    if (j[i] == 0xffffffffu) continue;
                    const size_t k = 3 * (size_t)j[i];
                    lk_plane_rows_term(&hg[27 * t], T, mbar, q[3 * i], q[3 * i + 1], q[3 * i + 2], r[k], r[k + 1], r[k + 2], nm[k], nm[k + 1], nm[k + 2]);
                }
            for (unsigned int o = 128; o > 0; o >>= 1)
                for (unsigned int t = 0; t < o; ++t)
                    for (int c = 0; c < 27; ++c) hg[27 * t + c] = hg[27 * t + c] + hg[27 * (t + o) + c];
            double xs[6], Tn[12];
            if (!lk_plane_solve(hg.data(), xs)) {
                status |= 32u;
                break;
            }
            lk_plane_update(T, xs, mbar, Tn);
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
        printf("pair %llu %u status %u iters %llu n_first %llu rmse_first %a step_rot %a step_trans %a n_last %llu rmse %a mean %a max %a worst %llu "
               "used_first %llu plane_first %a used %llu plane %a\n",
               (unsigned long long)nq, nr, status, (unsigned long long)iters, (unsigned long long)n_first, rmse_first, step_rot, step_trans, (unsigned long long)p.n,
               p.n ? sqrt(p.s2 / (double)p.n) : nan, p.n ? p.s1 / (double)p.n : nan, p.n ? sqrt(p.mx) : nan, (unsigned long long)(p.n ? p.worst : 0),
               (unsigned long long)used_first, plane_first, (unsigned long long)used, plane);
        printf("T");
        for (int c = 0; c < 12; ++c) printf(" %a", T[c]);
        printf("\n");
        for (uint64_t i = 0; i < nq; ++i) printf("%u %u %a\n", j_first[i], j[i], d2[i]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "align") && strcmp(argv[1], "normals"))) {
        fprintf(stderr, "usage: align_plane_host align|normals file\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        fprintf(stderr, "align_plane_host: cannot open %s\n", argv[2]);
        return 2;
    }
    const int rc = strcmp(argv[1], "align") ? run_normals(f) : run_align(f);
    fclose(f);
    return rc;
}
