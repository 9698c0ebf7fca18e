// lk_carve.h - one buffer carved into typed arrays.  A layout is written ONCE, as a function that takes the arrays in order from an LkCarve:
// run over a null base it only counts (total() is what to reserve), run over a buffer it hands out the pointers, run over a second
// buffer (the pinned staging copy and the device copy of one table) it hands out the same offsets there.  An array is named in one
// place, so its offset, its alignment and its type cannot drift apart.  Plain C++17, no HIP header: the host tests compile it alone.
#pragma once
#include <cstddef>

class LkCarve {
public:
    // min_align: every array starts at a multiple of it (and of its element's own alignment); a power of two that the base honours
    explicit LkCarve(void* base, size_t min_align = 16) : base_(static_cast<unsigned char*>(base)), align_(min_align) {}
    // n elements of T (n = 0: an empty array that takes no room); nullptr while counting
    template <typename T>
    T* take(size_t n) {
        const size_t a = alignof(T) > align_ ? alignof(T) : align_;
        off_ = (off_ + a - 1) & ~(a - 1);
        T* r = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += sizeof(T) * n;
        return r;
    }
    size_t total() const { return (off_ + align_ - 1) & ~(align_ - 1); }   // bytes taken so far, rounded up to min_align

private:
    unsigned char* base_;
    size_t align_, off_ = 0;
};
