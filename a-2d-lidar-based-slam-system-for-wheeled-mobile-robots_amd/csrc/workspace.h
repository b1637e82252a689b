// The layout of one call's workspace: the call declares its pieces ONCE, each bound to the pointer that will address it;
// bytes() is what the whole needs and place() hands the pieces out inside a block of known size - so the sum that is
// reserved and the pieces that are used cannot disagree, and a layout that does not fit is an error, never a launch.
// Plain C++17 without a HIP include (as launch_shapes.h): the C-ABI layer (slam_abi.hip: the scratch arena of the device
// forms, the table of Staging) and the ray casts' launchers (grid_kernels.hip: TileScratch, WedgeScratch) share it.
#pragma once

#include <cstddef>

namespace slam {

class Layout {
public:
    static constexpr int kMaxPieces = 24;
    static constexpr size_t kAlign = 256;     // every piece starts on a multiple of it (from a base that does)

    // a piece of n elements of T; place() sets `ptr` (a zero-size piece gets the address the next one starts at)
    template <typename T> Layout &add(T *&ptr, size_t n)
    {
        ptr = nullptr;
        if (n_ == kMaxPieces) overflow_ = true;
        if (overflow_) return *this;
        const size_t bytes = n * sizeof(T);
        p_[n_++] = Piece{&ptr, &set_ptr<T>, size_, bytes};
        size_ += (bytes + kAlign - 1) / kAlign * kAlign;
        return *this;
    }
    // bytes of the whole: where the last piece ends, rounded up to kAlign
    size_t bytes() const { return size_; }
    // the pieces at base .. base + bytes(); false, and no pointer set, when that ends beyond cap or more than kMaxPieces were declared
    bool place(void *base, size_t cap) const
    {
        if (overflow_ || size_ > cap) return false;
        for (int i = 0; i < n_; ++i) p_[i].set(p_[i].ptr, static_cast<char *>(base) + p_[i].off);
        return true;
    }
    // the table, for a user that copies into or out of the pieces it added (Staging): piece i is the i-th add()
    int count() const { return n_; }
    size_t offset(int i) const { return p_[i].off; }
    size_t size(int i) const { return p_[i].bytes; }

private:
    struct Piece {
        void *ptr;                            // the caller's pointer (a T *), set by place()
        void (*set)(void *ptr, char *p);
        size_t off, bytes;
    };
    template <typename T> static void set_ptr(void *ptr, char *p) { *static_cast<T **>(ptr) = reinterpret_cast<T *>(p); }

    Piece p_[kMaxPieces];
    int n_ = 0;
    bool overflow_ = false;
    size_t size_ = 0;
};

}  // namespace slam
