// Rigid edits of a selection of Gaussians, in place: x' = p + t + s R (x - p) with the covariance (the raw quaternion and
// log-scale) and the view-dependent colour (SH bands 1..3) turned along, and the Adam first moments with them.  What
// gui/main_edit.py:1512-1548 (obj_move) does for a translation only; DESIGN.md section 4.23.
//
//   edit_bounds_partial_k / edit_bounds_final_k   count, bounding box and float64 centroid of the selection, so that a pivot
//                     derived from the selection never comes back to the host.  Every thread sums the rows it owns (a fixed
//                     function of P), the wave butterfly and the waves in order give one partial per workgroup, and ONE
//                     workgroup sums the partials in the same fixed way: no float atomics, the same bits on every run.
//   edit_transform_k  one launch over parameters and moments.  A workgroup is ONE wave that owns 64 consecutive Gaussians and
//                     ballots their selection bytes; with nothing selected it has read those 64 bytes and nothing else.
//                     Position, quaternion and log-scale (12 / 16 / 12 B rows) are read and written by the owning lane and stay
//                     in registers.  _features_rest rows are 3 (M - 1) floats, only 4-byte aligned: the wave's 64 rows are one
//                     contiguous piece of memory, loaded with coalesced dword loads into LDS (an unselected row's lanes all read
//                     one word of a selected row instead: no traffic, no branch between the loads), each selected lane then
//                     reads ITS row at an odd stride (45, 25 for the 24-float rows of M = 9, 9: conflict-free), multiplies the
//                     bands by D1 / D2 / D3 -- 83 uniform numbers that arrive by value in the kernel arguments -- writes the row
//                     back to LDS, and the wave stores the selected rows coalesced.  The moments' rows go through the same
//                     function.
//
// This TU is compiled with -ffp-contract=off: every product and every sum below rounds once, in the order written, which is the
// order of tests/edit_reference.py.  No float atomics, no inline assembly.
// C entries, with the limits they enforce, at the end of the file: goi_edit_* (declared in include/goi_raster.h).
#include "entry.h"
#include "rest_row.h"
#include "wave_util.h"

namespace goi {

struct EditPointers {
    float *xyz, *rotation, *scaling, *rest;  // parameters (NULL: not written)
    float *m_xyz, *m_rotation, *m_rest;      // Adam first moments (NULL: none)
    const float* pivot_dev;                  // NULL: the pivot of the GoiEditTransform
};

namespace {

constexpr int BOUNDS_THREADS = 256;
constexpr int BOUNDS_WAVES = BOUNDS_THREADS / 64;
constexpr long long BOUNDS_MAX_BLOCKS = 1024;

struct BoundsPartial {
    double sum[3];
    unsigned long long n;
    float lo[3], hi[3];
};

__device__ __forceinline__ void bounds_add(BoundsPartial& a, const BoundsPartial& b) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.sum[k] = a.sum[k] + b.sum[k];
        a.lo[k] = fminf(a.lo[k], b.lo[k]);
        a.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    }
    a.n += b.n;
}

__device__ __forceinline__ BoundsPartial bounds_empty() {
    BoundsPartial b;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        b.sum[k] = 0.0;
        b.lo[k] = INFINITY;
        b.hi[k] = -INFINITY;
    }
    b.n = 0;
    return b;
}

// the workgroup's total in thread 0: butterfly inside each wave, then the waves in ascending order
__device__ __forceinline__ BoundsPartial bounds_block_reduce(BoundsPartial v, BoundsPartial* waves) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v.sum[k] = wave_sum(v.sum[k]);
        v.lo[k] = wave_min(v.lo[k]);
        v.hi[k] = wave_max(v.hi[k]);
    }
    v.n = wave_sum(v.n);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    BoundsPartial total = waves[0];
#pragma unroll
    for (int w = 1; w < BOUNDS_WAVES; w++) bounds_add(total, waves[w]);
    return total;
}

__global__ __launch_bounds__(BOUNDS_THREADS) void edit_bounds_partial_k(long long P, const float* __restrict__ xyz,
                                                                        const uint8_t* __restrict__ sel, int invert,
                                                                        BoundsPartial* __restrict__ partials) {
    __shared__ BoundsPartial waves[BOUNDS_WAVES];
    BoundsPartial v = bounds_empty();
    const long long stride = (long long)gridDim.x * BOUNDS_THREADS;
    for (long long i = (long long)blockIdx.x * BOUNDS_THREADS + threadIdx.x; i < P; i += stride) {
        if (!edit_selected(sel, invert, i)) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x = xyz[3 * i + k];
            v.sum[k] = v.sum[k] + (double)x;
            v.lo[k] = fminf(v.lo[k], x);
            v.hi[k] = fmaxf(v.hi[k], x);
        }
        v.n++;
    }
    const BoundsPartial total = bounds_block_reduce(v, waves);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(BOUNDS_THREADS) void edit_bounds_final_k(const BoundsPartial* __restrict__ partials, int n_partials,
                                                                      int* __restrict__ count, float* __restrict__ out) {
    __shared__ BoundsPartial waves[BOUNDS_WAVES];
    BoundsPartial v = bounds_empty();
    for (int b = threadIdx.x; b < n_partials; b += BOUNDS_THREADS) bounds_add(v, partials[b]);
    const BoundsPartial total = bounds_block_reduce(v, waves);
    if (threadIdx.x != 0) return;
    *count = (int)total.n;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out[k] = total.lo[k];
        out[3 + k] = total.hi[k];
        out[6 + k] = total.n ? (float)(total.sum[k] / (double)total.n) : 0.0f;
        out[9 + k] = total.n ? 0.5f * total.lo[k] + 0.5f * total.hi[k] : 0.0f;
    }
}

inline long long bounds_blocks(long long P) {
    const long long b = (P + BOUNDS_THREADS - 1) / BOUNDS_THREADS;
    return b < BOUNDS_MAX_BLOCKS ? b : BOUNDS_MAX_BLOCKS;
}

// ---- the transform ----------------------------------------------------------------------------------------------------------

constexpr int EDIT_WAVE = 64;

// r = R v, each component (R[i][0] v0 + R[i][1] v1) + R[i][2] v2
__device__ __forceinline__ void rotate3(const float* R, float v0, float v1, float v2, float* r) {
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = (R[3 * i] * v0 + R[3 * i + 1] * v1) + R[3 * i + 2] * v2;
}

// row <- a (x) row, the Hamilton product of (w, x, y, z) quaternions, each component summed left to right
__device__ __forceinline__ void quat_left(const float* a, float* __restrict__ row) {
    const float b0 = row[0], b1 = row[1], b2 = row[2], b3 = row[3];
    row[0] = ((a[0] * b0 - a[1] * b1) - a[2] * b2) - a[3] * b3;
    row[1] = ((a[0] * b1 + a[1] * b0) + a[2] * b3) - a[3] * b2;
    row[2] = ((a[0] * b2 - a[1] * b3) + a[2] * b0) + a[3] * b1;
    row[3] = ((a[0] * b3 + a[1] * b2) - a[2] * b1) + a[3] * b0;
}

// band of N = 2 l + 1 coefficients starting at coefficient `first` of a [.][3] row held in c: o = D c per channel, j ascending
template <int N>
__device__ __forceinline__ void rotate_band(const float* D, const float* c, float* o, int first) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            float acc = D[i * N] * c[first * 3 + ch];
#pragma unroll
            for (int j = 1; j < N; j++) acc = acc + D[i * N + j] * c[(first + j) * 3 + ch];
            o[(first + i) * 3 + ch] = acc;
        }
    }
}

// One [P][R] tensor (the parameter or its first moment): the wave's rows through LDS; only the rows in `ballot` are written.
template <int R>
__device__ __forceinline__ void edit_rest(float* __restrict__ g, long long base_row, unsigned long long ballot, bool sel,
                                          int lane, const GoiEditTransform& t, float* __restrict__ lds) {
    constexpr int STRIDE = RestRow<R>::STRIDE;
    const long long e0 = base_row * R;
    const int safe = __builtin_ctzll(ballot) * R;  // a word of a selected row: what the lanes of unselected rows read instead
    float v[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * EDIT_WAVE + lane;
        v[k] = g[e0 + (((ballot >> (e / R)) & 1ull) ? e : safe)];
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * EDIT_WAVE + lane, row = e / R;
        lds[row * STRIDE + (e - row * R)] = v[k];
    }
    __syncthreads();
    if (sel) {
        float* mine = lds + lane * STRIDE;
        float c[R], o[R];
#pragma unroll
        for (int j = 0; j < R; j++) c[j] = mine[j];
        rotate_band<3>(t.D1, c, o, 0);
        if constexpr (R > 9) rotate_band<5>(t.D2, c, o, 3);
        if constexpr (R > 24) rotate_band<7>(t.D3, c, o, 8);
#pragma unroll
        for (int j = 0; j < R; j++) mine[j] = o[j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * EDIT_WAVE + lane, row = e / R;
        v[k] = lds[row * STRIDE + (e - row * R)];
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * EDIT_WAVE + lane;
        if ((ballot >> (e / R)) & 1ull) g[e0 + e] = v[k];
    }
    __syncthreads();  // the buffer is free again
}

template <int R>
__global__ __launch_bounds__(EDIT_WAVE) void edit_transform_k(long long P, const uint8_t* __restrict__ selection, int invert,
                                                              const GoiEditTransform t, const EditPointers p) {
    __shared__ float lds[R ? EDIT_WAVE * RestRow<R>::STRIDE : 1];
    const int lane = threadIdx.x;
    const long long base = (long long)blockIdx.x * EDIT_WAVE;
    const long long i = base + lane;
    const bool sel = i < P && edit_selected(selection, invert, i);
    const unsigned long long ballot = __ballot(sel);
    if (!ballot) return;
    const bool rotate = (t.flags & GOI_EDIT_ROTATE) != 0;
    if (sel) {
        float* x = p.xyz + 3 * i;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        if (t.flags == 0) {  // a pure translation is the one add of _xyz[mask] += d
            x[0] = x0 + t.t[0];
            x[1] = x1 + t.t[1];
            x[2] = x2 + t.t[2];
        } else {
            float pv[3], r[3];
#pragma unroll
            for (int k = 0; k < 3; k++) pv[k] = p.pivot_dev ? p.pivot_dev[k] : t.pivot[k];
            rotate3(t.R, x0 - pv[0], x1 - pv[1], x2 - pv[2], r);
#pragma unroll
            for (int k = 0; k < 3; k++) x[k] = (t.s * r[k] + pv[k]) + t.t[k];
        }
        if (rotate) {
            quat_left(t.q, p.rotation + 4 * i);
            if (p.m_rotation) quat_left(t.q, p.m_rotation + 4 * i);
            if (p.m_xyz) {  // a moment gets the linear part only: no pivot, no scale, no translation
                float* m = p.m_xyz + 3 * i;
                float r[3];
                rotate3(t.R, m[0], m[1], m[2], r);
                m[0] = r[0];
                m[1] = r[1];
                m[2] = r[2];
            }
        }
        if (t.flags & GOI_EDIT_SCALE) {
            float* s = p.scaling + 3 * i;
            const float s0 = s[0], s1 = s[1], s2 = s[2];
            s[0] = s0 + t.log_s;
            s[1] = s1 + t.log_s;
            s[2] = s2 + t.log_s;
        }
    }
    if constexpr (R > 0) {  // (the launcher picks R > 0 only for a rotation)
        if (p.rest) edit_rest<R>(p.rest, base, ballot, sel, lane, t, lds);
        if (p.m_rest) edit_rest<R>(p.m_rest, base, ballot, sel, lane, t, lds);
    }
}

size_t edit_bounds_workspace_bytes(long long P) { return (size_t)(bounds_blocks(P) + 1) * sizeof(BoundsPartial); }

void launch_edit_bounds(long long P, const float* xyz, const uint8_t* selection, int invert, int* count, float* out, void* ws,
                        hipStream_t s) {
    BoundsPartial* partials = static_cast<BoundsPartial*>(ws);
    const int blocks = (int)bounds_blocks(P);
    if (blocks > 0)
        edit_bounds_partial_k<<<dim3((unsigned)blocks), dim3(BOUNDS_THREADS), 0, s>>>(P, xyz, selection, invert, partials);
    edit_bounds_final_k<<<dim3(1), dim3(BOUNDS_THREADS), 0, s>>>(partials, blocks, count, out);
}

void launch_edit_transform(long long P, int M, const uint8_t* selection, int invert, const GoiEditTransform& t,
                           const EditPointers& p, hipStream_t s) {
    if (P <= 0) return;
    const dim3 grid((unsigned)((P + EDIT_WAVE - 1) / EDIT_WAVE)), block(EDIT_WAVE);
    const int R = (t.flags & GOI_EDIT_ROTATE) && (p.rest || p.m_rest) ? 3 * (M - 1) : 0;
    if (R == 45)
        edit_transform_k<45><<<grid, block, 0, s>>>(P, selection, invert, t, p);
    else if (R == 24)
        edit_transform_k<24><<<grid, block, 0, s>>>(P, selection, invert, t, p);
    else if (R == 9)
        edit_transform_k<9><<<grid, block, 0, s>>>(P, selection, invert, t, p);
    else
        edit_transform_k<0><<<grid, block, 0, s>>>(P, selection, invert, t, p);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_edit_bounds_workspace_bytes(long long P) {
    return (P >= 0 && P < (1ll << 31)) ? edit_bounds_workspace_bytes(P) + 256 : 0;
}

int goi_edit_bounds(long long P, const float* xyz, const unsigned char* selection, int invert, int* count, float* out,
                    void* workspace, void* stream) {
    const char* fn = "goi_edit_bounds";
    if (P < 0 || P >= (1ll << 31)) return fail(std::string(fn) + ": need 0 <= P < 2^31");
    if (check_workspace(fn, workspace) < 0) return -1;
    if (!count || !out || (P > 0 && !xyz)) return fail(std::string(fn) + ": a required pointer is NULL");
    launch_edit_bounds(P, xyz, selection, invert, count, out, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_edit_transform(long long P, int M, const unsigned char* selection, int invert, const GoiEditTransform* t, float* xyz,
                       float* rotation, float* scaling, float* features_rest, float* m_xyz, float* m_rotation,
                       float* m_features_rest, const float* pivot_dev, void* stream) {
    const char* fn = "goi_edit_transform";
    if (P < 0 || P >= (1ll << 31)) return fail(std::string(fn) + ": need 0 <= P < 2^31");
    if (M != 1 && M != 4 && M != 9 && M != 16) return fail(std::string(fn) + ": M must be 1, 4, 9 or 16");
    if (!t) return fail(std::string(fn) + ": the transform is NULL");
    if (t->flags & ~(GOI_EDIT_ROTATE | GOI_EDIT_SCALE)) return fail(std::string(fn) + ": unknown flag bits");
    const bool rotate = (t->flags & GOI_EDIT_ROTATE) != 0, scale = (t->flags & GOI_EDIT_SCALE) != 0;
    if (!rotate && (m_xyz || m_rotation || m_features_rest)) return fail(std::string(fn) + ": moments are only turned by a rotation");
    if (M == 1 && m_features_rest) return fail(std::string(fn) + ": M = 1 has no features_rest moment");
    if (P > 0 && (!xyz || (rotate && !rotation) || (scale && !scaling) || (rotate && M > 1 && !features_rest)))
        return fail(std::string(fn) + ": a required pointer is NULL");
    EditPointers p;
    p.xyz = xyz;
    p.rotation = rotation;
    p.scaling = scaling;
    p.rest = M > 1 ? features_rest : nullptr;
    p.m_xyz = m_xyz;
    p.m_rotation = m_rotation;
    p.m_rest = m_features_rest;
    p.pivot_dev = pivot_dev;
    launch_edit_transform(P, M, selection, invert, *t, p, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
