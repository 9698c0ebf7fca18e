// Host build of leg-kilo_amd/csrc/lk_batch_stamp.h for tests/test_batch_stamp.py:  g++ -O2 -std=c++17 -shared -fPIC -o batch_stamp_host.so batch_stamp_host.cc
// -DLK_STAMP_PARENT_LOGIC: the three branches lk_batch_stamp_kernel had BEFORE the copy's stamp got a word of its own, transcribed once - shared words
// ref[0] (last stamp) / ref[1] (decision) for every stream - so that the exhaustive sequence test can be shown to fail on them.  The library has no such build.
#include <cstdint>
#include <cstring>

#include "../../leg-kilo_amd/csrc/lk_batch_stamp.h"

// The words of one tracked batch as the device holds them, and the host-mapped count.
struct StampState {
    unsigned long long w[LK_ORDW_COUNT];
    unsigned int seen;
};

extern "C" {
int lk_stamp_host_layout(int* out6) {
    out6[0] = LK_ORDW_COPY, out6[1] = LK_ORDW_LAST, out6[2] = LK_ORDW_USE, out6[3] = LK_ORD_RINGS, out6[4] = LK_ORDW_COUNT, out6[5] = (int)LK_ORD_SORTED;
    return (int)sizeof(StampState);
}
void lk_stamp_host_reset(StampState* s) { std::memset(s, 0, sizeof(*s)); }

// One replay on ring stream `ring`: mode LK_ORD_PROBE / CHECK / SET with stamp st.  Returns 1 if the replay is told to read the copy.
int lk_stamp_host_step(StampState* s, int mode, unsigned long long st, int ring) {
#if defined(LK_STAMP_PARENT_LOGIC)
    (void)ring;
    unsigned long long* ref = s->w;
    if (mode == LK_ORD_SET) {
        ref[0] = st, ref[1] = 1ull, s->seen = LK_ORD_SORTED;
    } else if (st == ref[0]) {
        ref[1] = mode == LK_ORD_CHECK ? 1ull : 0ull;
        if (mode == LK_ORD_PROBE) s->seen = s->seen + 1u;
    } else {
        ref[0] = st, ref[1] = 0ull, s->seen = 1u;
    }
    return (int)ref[1];
#else
    unsigned long long* use = s->w + LK_ORDW_USE + 2 * ring;
    const unsigned long long r = lk_stamp_decide(mode, st, s->w, use, &s->seen);
    return r == use[1] ? (int)r : -1;   // what it returns is what the residual launches will read
#endif
}

// Every sequence of `len` replays over modes {PROBE, CHECK, SET} x stamps stamps3[0..2] after an initial SET(stamps3[0]), each replay on ring
// (position % n_rings).  For every step: a replay told to read the copy must carry the stamp of the last SET; a CHECK that carries it while the
// count stands at LK_ORD_SORTED must be told to (or the copy would never be read).  After every step: a mismatch (a non-SET replay with another stamp
// than the last SET's) since the last SET <=> count below LK_ORD_SORTED; and the count below LK_ORD_SORTED equals what a plain model gives -
// the CHECK or PROBE that starts a run of equal stamps counts 1, each further PROBE of that run +1, a further CHECK +0 - so only
// PROBE launches that saw the same stamp in a row raise it.  Returns the number of sequences that broke a rule (0: all hold); by_rule4[r]: how
// many broke rule r first (1 copy read on another stamp, 2 count, 3 current copy not read); first_bad[r]: the first of them as base-9 digits (mode * 3 +
// stamp index), first step in the lowest digit.
uint64_t lk_stamp_host_enumerate(int len, const unsigned long long* stamps3, int n_rings, uint64_t* first_bad, uint64_t* by_rule4) {
    uint64_t n_seq = 1, bad = 0;
    for (int r = 0; r < 4; ++r) by_rule4[r] = 0, first_bad[r] = 0;
    for (int i = 0; i < len; ++i) n_seq *= 9;
    for (uint64_t q = 0; q < n_seq; ++q) {
        StampState s;
        lk_stamp_host_reset(&s);
        lk_stamp_host_step(&s, LK_ORD_SET, stamps3[0], 0);
        unsigned long long set_st = stamps3[0], run_st = stamps3[0];
        bool mismatched = false;
        unsigned int model = LK_ORD_SORTED;
        int rule = 0;
        uint64_t d = q;
        for (int i = 0; i < len && !rule; ++i, d /= 9) {
            const int mode = (int)(d % 9) / 3;
            const unsigned long long st = stamps3[d % 3];
            const int use = lk_stamp_host_step(&s, mode, st, i % n_rings);
            if (mode == LK_ORD_SET) {
                set_st = st, run_st = st, mismatched = false, model = LK_ORD_SORTED;
                if (use != 1) rule = 3;
            } else {
                if (st != set_st) mismatched = true;
                if (mismatched) {
                    if (model >= LK_ORD_SORTED || st != run_st) model = 1, run_st = st;
                    else if (mode == LK_ORD_PROBE) ++model;
                } else if (mode == LK_ORD_PROBE) {   // (the host never probes while it holds a current copy; if it did: the same count rule)
                    mismatched = true, model = 1, run_st = st;
                }
                if (use != 0 && (use != 1 || st != set_st || mode != LK_ORD_CHECK)) rule = 1;
                else if (mode == LK_ORD_CHECK && st == set_st && s.seen >= LK_ORD_SORTED && use != 1) rule = 3;
            }
            if (!rule && s.seen != model) rule = 2;
#if !defined(LK_STAMP_PARENT_LOGIC)
            if (!rule && s.w[LK_ORDW_COPY] != set_st) rule = 1;   // the copy's word is the last SET's stamp, whatever came since
#endif
        }
        if (rule) {
            if (!by_rule4[rule]) first_bad[rule] = q;
            ++by_rule4[rule];
            ++bad;
        }
    }
    return bad;
}

// The stamp of `total` 16-byte points the way lk_batch_stamp_kernel takes it (the sum does not depend on the order).
unsigned long long lk_stamp_host_of(const uint32_t* pts4, size_t total) {
    const size_t stride = lk_stamp_stride(total);
    unsigned long long sum = 0ull;
    for (size_t k = 0; k < LK_STAMP_SAMPLES; ++k) {
        const size_t idx = k * stride;
        if (idx >= total) break;
        sum += lk_stamp_mix(pts4[4 * idx], pts4[4 * idx + 1], pts4[4 * idx + 2], pts4[4 * idx + 3], idx);
    }
    return lk_stamp_finish(sum);
}
}
