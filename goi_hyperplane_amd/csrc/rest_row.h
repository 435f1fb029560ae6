// What the kernels that walk a selection of Gaussians wave by wave share (edit.hip, pose.hip): the selection predicate and the
// LDS layout of a wave's 64 _features_rest rows.
#pragma once

#include "common.h"

namespace goi {

// selection [P] bytes: non-zero selects, with `invert` a zero byte does; NULL = every row
__device__ __forceinline__ bool edit_selected(const uint8_t* __restrict__ sel, int invert, long long i) {
    return !sel || ((sel[i] != 0) != (invert != 0));
}

// A wave's 64 rows of R floats in LDS, row r at r * STRIDE.
template <int R>
struct RestRow {
    static constexpr int STRIDE = (R % 2) ? R : R + 1;  // odd: 64 lanes reading their own rows hit 64 different banks
};

}  // namespace goi
