// Host build of leg-kilo_amd/csrc/lk_carve.h for tests/test_carve.py:  g++ -O2 -std=c++17 -shared -fPIC -o carve_host.so carve_host.cc
#include <cstdint>

#include "../../leg-kilo_amd/csrc/lk_carve.h"

namespace {
struct alignas(16) Rec16 {   // stands for lk_point / float4
    float v[4];
};
}  // namespace

// One layout description - array i holds count[i] elements of elem[i] bytes (1, 4, 8 or 16) - applied to `base` (0: the counting pass).
// addr[i]: where array i starts (0 while counting); returns the total, or (size_t)-1 for an element size it does not know.
extern "C" size_t lk_carve_host(uintptr_t base, size_t min_align, int n, const int* elem, const size_t* count, uintptr_t* addr) {
    LkCarve c(reinterpret_cast<void*>(base), min_align);
    for (int i = 0; i < n; ++i) {
        switch (elem[i]) {
            case 1: addr[i] = reinterpret_cast<uintptr_t>(c.take<unsigned char>(count[i])); break;
            case 4: addr[i] = reinterpret_cast<uintptr_t>(c.take<unsigned int>(count[i])); break;
            case 8: addr[i] = reinterpret_cast<uintptr_t>(c.take<double>(count[i])); break;
            case 16: addr[i] = reinterpret_cast<uintptr_t>(c.take<Rec16>(count[i])); break;
            default: return static_cast<size_t>(-1);
        }
    }
    return c.total();
}
