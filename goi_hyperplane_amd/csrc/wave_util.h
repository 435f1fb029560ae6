// Lane-level helpers shared by the stand-alone kernel families (field, mesh, texture, dbscan, knn, display, pca,
// codebook_init, photometric, masks): the ordered float key, the 64-lane butterfly reductions, wave_same and the union-find
// walk.  gfx950 only (wave64).
//
// Deliberately NOT here, and not to be folded in later:
//   * the DPP reductions of osh.hip (wave_sum) and codebook_loss.hip (wave_sum_u, wave_max_u, wave_min_u, row_sum, row_max,
//     row_min).  They add in another order than the butterfly below, and float sums are compared bit for bit (osh_path, the
//     fused loss's bit-reproducibility): they are different functions, not copies.
//   * blend_common.h, scan_sort.hip and the rasterizer's frame path (preprocess, binning, reduce_rows, render_*), which keep
//     their own helpers and do not include this file.
#pragma once

#include "common.h"

namespace goi {

// Order-preserving key of a float: a < b  <=>  ord_enc(a) < ord_enc(b) as unsigned (-0 < +0), so integer atomicMin / atomicMax
// on the key are float min / max.  ord_enc_bits takes the float's bits; ord_dec is the inverse.
__device__ __forceinline__ uint32_t ord_enc_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t ord_enc(float f) { return ord_enc_bits(__float_as_uint(f)); }
// (Branch-free on purpose: spelled as the select `(e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e`, mesh.hip does not compile --
// the gfx950 backend rejects its own v_cndmask with "Illegal instruction detected: Operand has incorrect register class".)
__device__ __forceinline__ float ord_dec(uint32_t e) {
    const uint32_t m = (uint32_t)((int32_t)e >> 31);  // all ones for an encoded non-negative value: clear its top bit; else ~e
    return __uint_as_float(e ^ (~m | 0x80000000u));
}

// Butterfly reductions over the wave's 64 lanes, offsets 32, 16, ..., 1 (a float or double sum has this one order); every lane
// gets the result.  Only the types somebody calls.  (The bounding-box kernels of field.hip, mesh.hip and pca.hip interleave a
// minimum and a maximum in one loop of their own: through these helpers the same instructions come out in another order.)
template <class T, class Op>
__device__ __forceinline__ T wave_butterfly(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    return wave_butterfly(v, [](float a, float b) { return fminf(a, b); });
}
__device__ __forceinline__ float wave_max(float v) {
    return wave_butterfly(v, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    return wave_butterfly(v, [](uint32_t a, uint32_t b) { return min(a, b); });
}
__device__ __forceinline__ float wave_sum(float v) {
    return wave_butterfly(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ double wave_sum(double v) {
    return wave_butterfly(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    return wave_butterfly(v, [](uint32_t a, uint32_t b) { return a + b; });
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    return wave_butterfly(v, [](unsigned long long a, unsigned long long b) { return a + b; });
}

// true when every active lane of the wave carries the same key (then one lane can speak for the wave)
__device__ __forceinline__ bool wave_same(bool active, uint32_t key) {
    const unsigned long long m = __ballot(active);
    if (!m) return false;
    const uint32_t lead = (uint32_t)__shfl((int)key, __builtin_ctzll(m));
    return __all(!active || key == lead);
}

// ---- union-find over parent[0 .. n): unions hook the larger root under the smaller with atomicCAS, so parents only decrease
__device__ __forceinline__ uint32_t load_parent(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // past the non-coherent L1
}
// root of x; the walk ends within n steps (the bound is a guard, never reached: overrunning it raises `bit` in *status)
__device__ __forceinline__ uint32_t find_root(const uint32_t* parent, uint32_t x, uint32_t n, uint32_t* status, uint32_t bit) {
    for (uint32_t it = 0; it <= n; it++) {
        const uint32_t p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
    atomicOr(status, bit);
    return x;
}

}  // namespace goi
