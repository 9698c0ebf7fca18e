// lk_cloud_layout.h - host-side layout arithmetic of the bucket table and the registration launch of the _cloud run replays (legkilo_hip.hip).
// Plain C++ without HIP, so that tests/cloud_layout_main.cc can run it under the host sanitizers on its own.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef LK_REG_TILE
#define LK_REG_TILE 256   // points per workgroup of lk_register_cloud_kernel
#endif

// bytes of a table of B records of `rec` bytes each; 0 when the product does not fit a size_t
static inline size_t lk_cloud_table_bytes(uint64_t B, size_t rec) {
    if (rec && B > (uint64_t)(SIZE_MAX / rec)) return 0;
    return (size_t)B * rec;
}
// scan_bucket_off[0 .. S] from the scans' first flat buckets bs[0 .. S] of THIS call's tables (bs[0] is 0 there; a caller's copy counts from 0 in any
// case); returns the flat bucket count, or UINT64_MAX if bs is not strictly increasing (no scan is empty)
static inline uint64_t lk_cloud_scan_offsets(const uint32_t* bs, size_t S, uint32_t* scan_bucket_off) {
    for (size_t s = 0; s < S; ++s)
        if (bs[s + 1] <= bs[s]) return UINT64_MAX;
    if (scan_bucket_off)
        for (size_t s = 0; s <= S; ++s) scan_bucket_off[s] = bs[s] - bs[0];
    return (uint64_t)bs[S] - bs[0];
}
// workgroups of the registration launch over n points (n < 2^32: at most 2^24)
static inline uint32_t lk_cloud_tiles(uint64_t n) {
    return (uint32_t)((n + LK_REG_TILE - 1) / LK_REG_TILE);
}
// a record range of the getters lies inside a table of `count` records
static inline bool lk_cloud_range_ok(uint64_t first, uint64_t n, uint64_t count) {
    return first <= count && n <= count - first;
}
