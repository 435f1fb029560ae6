// How every module cuts the one opaque workspace its caller hands over into pieces (host only, no HIP: a plain C++
// compiler builds a test program against this file).  One policy: every piece starts on a 256-byte boundary, a NULL base
// means "only tell me the size", and because the size function and the launcher of a module run the SAME layout function
// -- once with NULL, once with the buffer -- the byte count and the pointers cannot drift apart.
#pragma once

#include <cstddef>
#include <cstdint>

namespace goi {

inline size_t round_up_256(size_t n) { return (n + 255) & ~(size_t)255; }

// A layout that has always given an empty array a piece of its own (mesh, texture: the size of an empty mesh's workspace
// counts them) says so where it takes the piece: c.take<T>(at_least_one(n)).
inline size_t at_least_one(size_t n) { return n ? n : 1; }

struct Carver {
    // base rounded up to 256 (a caller that could not align its buffer is given 256 bytes of slack by the size functions
    // that tolerate one); NULL stays NULL
    explicit Carver(void* base) : base_(reinterpret_cast<char*>(round_up_256(reinterpret_cast<uintptr_t>(base)))) {}
    // The next piece: the offset is rounded up to 256 BEFORE the piece, not after it, so the last piece is not padded.
    // A zero count takes nothing.  NULL when sizing.
    template <typename T>
    T* take(size_t count) {
        const size_t at = round_up_256(end_);
        if (count) end_ = at + count * sizeof(T);
        return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
    }
    size_t end() const { return end_; }                  // bytes used from the (rounded) base, the last piece not padded
    size_t bytes() const { return round_up_256(end_); }  // the same with the last piece padded

private:
    char* base_;
    size_t end_ = 0;
};

}  // namespace goi
