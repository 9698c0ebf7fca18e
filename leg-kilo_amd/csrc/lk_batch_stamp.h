// lk_batch_stamp.h - the content stamp of a device-resident batch and what a replay does with it (lk_batch_order, legkilo_hip.hip).  The one thread of
// lk_batch_stamp_kernel that decides runs lk_stamp_decide; the host tests (tools/probes/batch_stamp_host.cc, tests/test_batch_stamp.py) compile the same
// header alone and drive it through sequences of replays.  Plain C++, no HIP header.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LK_STAMP_FN __host__ __device__ __forceinline__
#else
#define LK_STAMP_FN inline
#endif

#define LK_ORD_PROBE 0     // no copy (yet): count how often the content repeats
#define LK_ORD_CHECK 1     // a copy exists: use it if the buffer still holds what it was made from
#define LK_ORD_SET 2       // the copy has just been made from the buffer
#define LK_ORD_SORTED 1000000u

#define LK_STAMP_SAMPLES 4096   // points the stamp looks at: point k * lk_stamp_stride(total), k < 4096 (a batch of fewer points: all of them)
#define LK_ORD_RINGS 3          // streams the asynchronous batch entry rotates over: a decision word each

// The device words of one tracked batch (OrdEntry::d_ref), 64 bits each:
//   [LK_ORDW_COPY]  the stamp the library's copy was made from; 0: no copy.  Written by LK_ORD_SET alone.
//   [LK_ORDW_LAST]  the stamp of the replay before, for counting repeats; 0: no stamp yet.
//   [LK_ORDW_USE + 2 r], [.. + 1]   ring stream r's pair: this replay's stamp, and 1 if ITS residual launches read the copy (ResidualOut::alt_use
//                   points at the pair, alt_use[1] is the word read).  Replays on one stream are ordered, so a pair belongs to one replay at a time.
//   [LK_ORDW_SCRATCH]  the unsorted-pairs counter of lk_sort_check_kernel
#define LK_ORDW_COPY 0
#define LK_ORDW_LAST 1
#define LK_ORDW_USE 2
#define LK_ORDW_SCRATCH (LK_ORDW_USE + 2 * LK_ORD_RINGS)
#define LK_ORDW_COUNT (LK_ORDW_SCRATCH + 1)

LK_STAMP_FN size_t lk_stamp_stride(size_t total) { return total / LK_STAMP_SAMPLES ? total / LK_STAMP_SAMPLES : 1; }

// What point `idx` (its 16 bytes as four words) adds to the stamp.  The stamp is the SUM of these: the order the threads arrive in does not matter.
LK_STAMP_FN unsigned long long lk_stamp_mix(unsigned int x, unsigned int y, unsigned int z, unsigned int w, size_t idx) {
    unsigned long long m = ((unsigned long long)x | ((unsigned long long)y << 32)) ^ (0x9E3779B97F4A7C15ull * (idx + 1));
    m = (m ^ (m >> 31)) * 0xBF58476D1CE4E5B9ull;
    m ^= ((unsigned long long)z | ((unsigned long long)w << 32)) * 0x94D049BB133111EBull;
    m = (m ^ (m >> 29)) * 0xC2B2AE3D27D4EB4Full;
    return m ^ (m >> 32);
}
LK_STAMP_FN unsigned long long lk_stamp_finish(unsigned long long sum) { return sum | 1ull; }   // never 0: a word that holds 0 means "no stamp yet"

// The count the host reads: several replays of one batch may be in flight on different streams, so it is only ever exchanged or added to atomically.
LK_STAMP_FN unsigned int lk_stamp_seen_load(unsigned int* seen) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    return *seen;
#endif
}
LK_STAMP_FN void lk_stamp_seen_set(unsigned int* seen, unsigned int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_exchange(seen, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    *seen = v;
#endif
}
LK_STAMP_FN void lk_stamp_seen_add(unsigned int* seen) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(seen, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    *seen += 1u;
#endif
}

// One replay's decision.  st: its stamp (lk_stamp_finish: never 0); w: the batch's words; use: this replay's pair (w + LK_ORDW_USE + 2 * ring);
// seen: the count the host reads - replays in a row that found the same stamp, LK_ORD_SORTED while the copy is current.  Returns use[1].
//   - the copy is read ONLY by a replay whose stamp is the one the copy was made from (w[LK_ORDW_COPY], which no mismatch ever touches): a second
//     LK_ORD_CHECK on new content, enqueued while the host still saw LK_ORD_SORTED, reads the caller's buffer like the first one did;
//   - a mismatch brings the count below LK_ORD_SORTED, where it stays until the next LK_ORD_SET (the host then forgets the copy), and only
//     LK_ORD_PROBE launches that find the stamp of the replay before count upwards.
LK_STAMP_FN unsigned long long lk_stamp_decide(int mode, unsigned long long st, unsigned long long* w, unsigned long long* use, unsigned int* seen) {
    use[0] = st;
    if (mode == LK_ORD_SET) {
        w[LK_ORDW_COPY] = st, w[LK_ORDW_LAST] = st;
        lk_stamp_seen_set(seen, LK_ORD_SORTED);
        return use[1] = 1ull;
    }
    const bool copy_ok = mode == LK_ORD_CHECK && st == w[LK_ORDW_COPY];
    const unsigned int cur = lk_stamp_seen_load(seen);
    if (copy_ok && cur >= LK_ORD_SORTED) return use[1] = 1ull;   // the copy is current: nothing to count
    if (st != w[LK_ORDW_LAST] || cur >= LK_ORD_SORTED) {          // other content than last time: the count starts again
        w[LK_ORDW_LAST] = st;
        lk_stamp_seen_set(seen, 1u);
    } else if (mode == LK_ORD_PROBE) {
        lk_stamp_seen_add(seen);
    }
    return use[1] = copy_ok ? 1ull : 0ull;
}
