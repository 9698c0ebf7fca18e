// Stand-alone driver of leg-kilo_amd/csrc/lk_cloud_layout.h - the host arithmetic of the _cloud run replays (bucket-table size, scan_bucket_off, the
// registration launch's grid, the getters' range check) - meant to be built with -fsanitize=address,undefined and run on its own
// (tests/test_runs_cloud_abi.py).  Buffers are heap allocations of EXACTLY the documented extents, so that an entry too many is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lk_cloud_layout.h"

#define REQUIRE(c)                                                     \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    const size_t REC = 144;
    // table bytes: plain products, the largest table a batch can have (2^32 - 1 buckets), and the overflow guard
    REQUIRE(lk_cloud_table_bytes(0, REC) == 0);
    REQUIRE(lk_cloud_table_bytes(1, REC) == 144);
    REQUIRE(lk_cloud_table_bytes(0xffffffffull, REC) == 0xffffffffull * 144ull);
    REQUIRE(lk_cloud_table_bytes(UINT64_MAX / 144 + 1, REC) == 0);
    REQUIRE(lk_cloud_table_bytes(UINT64_MAX, REC) == 0);
    // scan_bucket_off: six runs' scans with 1 .. 40 buckets each, counted from this call's first bucket
    for (uint32_t first : {0u, 7u, 0xfffffff0u - 500u}) {
        const uint32_t nb[] = {51, 1, 40, 50, 1, 49, 52, 3, 1, 50, 50, 40, 1, 2};
        const size_t S = sizeof(nb) / sizeof(nb[0]);
        std::vector<uint32_t> bs(S + 1), out(S + 1, 0xdeadbeefu);
        bs[0] = first;
        for (size_t s = 0; s < S; ++s) bs[s + 1] = bs[s] + nb[s];
        const uint64_t B = lk_cloud_scan_offsets(bs.data(), S, out.data());
        REQUIRE(B == (uint64_t)(bs[S] - first) && out[0] == 0 && out[S] == B);
        for (size_t s = 0; s < S; ++s) REQUIRE(out[s + 1] - out[s] == nb[s]);
        REQUIRE(lk_cloud_scan_offsets(bs.data(), S, nullptr) == B);   // the caller's array is optional
        REQUIRE(lk_cloud_table_bytes(B, REC) == (size_t)B * REC);
        bs[3] = bs[2];   // an empty scan cannot come out of the device's tables: reported, nothing written past it
        REQUIRE(lk_cloud_scan_offsets(bs.data(), S, out.data()) == UINT64_MAX);
    }
    {   // one scan of one bucket; the table of the largest batch
        const uint32_t bs[2] = {0, 1};
        uint32_t out[2] = {9, 9};
        REQUIRE(lk_cloud_scan_offsets(bs, 1, out) == 1 && out[0] == 0 && out[1] == 1);
        const uint32_t top[2] = {0, 0xffffffffu};
        REQUIRE(lk_cloud_scan_offsets(top, 1, out) == 0xffffffffull && out[1] == 0xffffffffu);
    }
    // tiles of the registration launch: every point in exactly one tile, none past the last point
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 4096ull, 0xffffffffull}) {
        const uint32_t tiles = lk_cloud_tiles(n);
        REQUIRE((uint64_t)tiles * LK_REG_TILE >= n && (uint64_t)(tiles - 1) * LK_REG_TILE < n);
    }
    REQUIRE(lk_cloud_tiles(0) == 0);
    // the getters' range check, where first + n would wrap
    REQUIRE(lk_cloud_range_ok(0, 0, 5) && lk_cloud_range_ok(0, 5, 5) && lk_cloud_range_ok(5, 0, 5) && lk_cloud_range_ok(2, 3, 5));
    REQUIRE(!lk_cloud_range_ok(0, 6, 5) && !lk_cloud_range_ok(5, 1, 5) && !lk_cloud_range_ok(6, 0, 5));
    REQUIRE(!lk_cloud_range_ok(UINT64_MAX, 2, 5) && !lk_cloud_range_ok(2, UINT64_MAX, 5) && !lk_cloud_range_ok(1ull << 63, 1ull << 63, 5));
    std::puts("cloud layout ok");
    return 0;
}
