// Stand-alone driver of leg-kilo_amd/csrc/lk_pcd_files.h - the file ranges of the map clouds from the run replays' tables (PcdSaver::workerLoop's
// counting) - meant to be built with -fsanitize=address,undefined and run on its own (tests/test_map_clouds_abi.py).  It prints, for every
// frames_per_file on its command line, one line `fpf n_files | file_off ... | file_run ...` that the test compares with binding.pcd_file_offsets.
// Buffers are heap allocations of EXACTLY the documented extents, so that an entry too many is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lk_pcd_files.h"

int main(int argc, char** argv) {
    // six runs of 3, 1, 4, 2, 1, 3 scans; a scan without points in the middle of run 2 and at the end of run 5; the first scan starts at record 13
    const uint32_t run_len[] = {3, 1, 4, 2, 1, 3};
    const uint32_t scan_len[] = {5, 7, 2, 9, 4, 0, 6, 1, 8, 3, 11, 2, 5, 0};
    const size_t R = sizeof(run_len) / sizeof(run_len[0]), S = sizeof(scan_len) / sizeof(scan_len[0]);
    std::vector<uint32_t> run_off(R + 1, 0);
    std::vector<uint64_t> scan_off(S + 1, 13);
    for (size_t r = 0; r < R; ++r) run_off[r + 1] = run_off[r] + run_len[r];
    for (size_t s = 0; s < S; ++s) scan_off[s + 1] = scan_off[s] + scan_len[s];
    if (run_off[R] != S) return 2;
    for (int a = 1; a < argc; ++a) {
        const int fpf = std::atoi(argv[a]);
        const size_t F = pcd_file_offsets(run_off.data(), R, scan_off.data(), fpf, nullptr, nullptr);   // counting only
        if (F > S) return 3;
        std::vector<uint64_t> file_off(F + 1, 0xdeadbeefull);
        std::vector<uint32_t> file_run(F, 0xdeadbeefu);
        if (pcd_file_offsets(run_off.data(), R, scan_off.data(), fpf, file_off.data(), file_run.data()) != F) return 4;
        if (pcd_file_offsets(run_off.data(), R, scan_off.data(), fpf, file_off.data(), nullptr) != F) return 5;   // either array is optional
        std::printf("%d %zu |", fpf, F);
        for (uint64_t v : file_off) std::printf(" %llu", (unsigned long long)v);
        std::printf(" |");
        for (uint32_t v : file_run) std::printf(" %u", v);
        std::printf("\n");
    }
    {   // no runs, and runs without a point: no file, nothing written but file_off[0]
        uint64_t one[1] = {99};
        const uint32_t ro0[1] = {0};
        const uint64_t so0[1] = {7};
        if (pcd_file_offsets(ro0, 0, so0, 2, one, nullptr) != 0 || one[0] != 99) return 6;
        const uint32_t ro1[2] = {0, 2};
        const uint64_t so1[3] = {7, 7, 7};
        if (pcd_file_offsets(ro1, 1, so1, 1, one, nullptr) != 0 || one[0] != 7) return 7;
    }
    std::puts("pcd files ok");
    return 0;
}
