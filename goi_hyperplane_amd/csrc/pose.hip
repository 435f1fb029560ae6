// Pose gradients of a selection of Gaussians from the gradients one backward left: dL/d(omega, t, sigma) of the similarity
// x' = p + t + e^sigma Exp(omega) (x - p) that edit.hip applies, as ONE deterministic reduction of the selected rows of
// dL/d_xyz, dL/d_rotation, dL/d_scaling and dL/d_features_rest.  DESIGN.md section 4.27; goi_hyperplane_amd/pose.py.
//
//   pose_partial_k   A wave owns 64 consecutive Gaussians at a time and ballots their selection bytes; with nothing selected it
//                    has read those 64 bytes and nothing else.  Position, quaternion, log-scale gradient rows (12 / 16 / 12 B)
//                    are read by the owning lane.  The _features_rest row and its gradient row are 3 (M - 1) floats, only 4-byte
//                    aligned: the wave's 64 rows are one contiguous piece of memory, loaded with coalesced dword loads into the
//                    wave's part of LDS (an unselected row's lanes all read one word of a selected row instead) and read back by
//                    the owning lane at the odd stride of RestRow<R>.  Per selected row every piece is formed in fp32, one
//                    rounding per operation in the order of tests/pose_reference.py (d = x - p first, as the transform forms it),
//                    converted to double and added to seven float64 accumulators.  The 48 non-zero generator values arrive by
//                    value; WHERE they sit is a property of the real SH basis and is compiled in (generator_entry below).
//   pose_final_k     one workgroup sums the at most 1024 per-workgroup partials.
//
// The order of every sum is fixed, as in edit_bounds_partial_k / edit_bounds_final_k: a thread adds the rows it owns in ascending
// order (which rows is a function of P alone), then the wave butterfly, then the waves in order, then the partials the same way.
// No float atomics, no inline assembly: the same bits on every run.  A gradient pointer that is NULL was not trained: its pieces
// are omitted and its parameter tensor is not read.
//
// This TU is compiled with -ffp-contract=off.  C entries at the end of the file: goi_pose_* (declared in include/goi_raster.h).
#include <utility>

#include "entry.h"
#include "rest_row.h"
#include "wave_util.h"

namespace goi {

struct PoseGenerators {
    float x[18], y[18], z[12];  // the non-zero entries of G_x, G_y, G_z over bands 1..3, row-major
};

struct PosePointers {
    const float *xyz, *rotation, *rest;                   // parameters (read only where their gradient is given)
    const float *g_xyz, *g_rotation, *g_scaling, *g_rest;  // gradients (NULL: not trained, its pieces are omitted)
    const float* pivot_dev;                                // NULL: pivot[]
    float pivot[3];
};

namespace {

constexpr int POSE_THREADS = 256;
constexpr int POSE_WAVES = POSE_THREADS / 64;
constexpr long long POSE_MAX_BLOCKS = 1024;

struct PosePartial {
    double a[7];  // omega[3], t[3], sigma
    unsigned long long n;
};

// (row, column) of the k-th non-zero entry of the generator of axis AXIS (0, 1, 2 = x, y, z; 18, 18, 12 entries), as
// coefficients of _features_rest (coefficient 0 is SH coefficient 1), row-major.  The generators are block diagonal over the
// bands, so the entries of a narrower model (M = 4, 9) are a prefix.
struct Entry {
    int i, j;
};
template <int AXIS>
__host__ __device__ constexpr Entry generator_entry(int k) {
    if constexpr (AXIS == 0) {
        constexpr Entry e[18] = {{0, 1}, {1, 0}, {3, 6}, {4, 5}, {4, 7}, {5, 4}, {6, 3}, {7, 4}, {8, 13}, {9, 12}, {9, 14}, {10, 11},
                                 {10, 13}, {11, 10}, {12, 9}, {13, 8}, {13, 10}, {14, 9}};
        return e[k];
    } else if constexpr (AXIS == 1) {
        constexpr Entry e[18] = {{1, 2}, {2, 1}, {3, 4}, {4, 3}, {5, 6}, {6, 5}, {6, 7}, {7, 6}, {8, 9}, {9, 8}, {9, 10}, {10, 9},
                                 {11, 12}, {12, 11}, {12, 13}, {13, 12}, {13, 14}, {14, 13}};
        return e[k];
    } else {
        constexpr Entry e[12] = {{0, 2}, {2, 0}, {3, 7}, {4, 6}, {6, 4}, {7, 3}, {8, 14}, {9, 13}, {10, 12}, {12, 10}, {13, 9}, {14, 8}};
        return e[k];
    }
}

// how many of a generator's entries lie within the first `coefficients` coefficients
template <int AXIS>
__host__ __device__ constexpr int entries_within(int coefficients) {
    int n = 0;
    for (int k = 0; k < (AXIS == 2 ? 12 : 18); k++)
        n += (generator_entry<AXIS>(k).i < coefficients && generator_entry<AXIS>(k).j < coefficients) ? 1 : 0;
    return n;
}

// G_K (g_i . c_j) of entry K: the dot product over the three channels in index order
template <int AXIS, int K>
__device__ __forceinline__ float colour_entry(const float* G, const float* g, const float* c) {
    constexpr Entry e = generator_entry<AXIS>(K);
    constexpr int i = 3 * e.i, j = 3 * e.j;
    return G[K] * ((g[i] * c[j] + g[i + 1] * c[j + 1]) + g[i + 2] * c[j + 2]);
}

// sum_K G_K (g_i . c_j), the entries added left to right
template <int AXIS, int... K>
__device__ __forceinline__ float colour_sum(const float* G, const float* g, const float* c, std::integer_sequence<int, K...>) {
    float acc = 0.0f;
    ((acc = K ? acc + colour_entry<AXIS, K>(G, g, c) : colour_entry<AXIS, K>(G, g, c)), ...);
    return acc;
}

template <int R, int AXIS>
__device__ __forceinline__ float colour_term(const float* G, const float* g, const float* c) {
    return colour_sum<AXIS>(G, g, c, std::make_integer_sequence<int, entries_within<AXIS>(R / 3)>());
}

// The wave's 64 rows of one [P][R] tensor through its part of LDS; a selected lane leaves with ITS row in `mine`.  Every wave of
// the workgroup calls this the same number of times (the barriers); a wave with nothing selected loads nothing.
template <int R>
__device__ __forceinline__ void pose_rest(const float* __restrict__ g, long long base_row, unsigned long long ballot, bool sel,
                                          int lane, float* __restrict__ lds, float* mine) {
    constexpr int STRIDE = RestRow<R>::STRIDE;
    if (ballot) {
        const float* __restrict__ rows = g + base_row * R;  // wave-uniform: the loads below take 32-bit offsets from it
        const unsigned safe = __builtin_ctzll(ballot) * R;  // a word of a selected row: what the lanes of unselected rows read instead
        float v[R];
#pragma unroll
        for (int k = 0; k < R; k++) {
            const unsigned e = k * 64 + lane;
            v[k] = rows[((ballot >> (e / R)) & 1ull) ? e : safe];
        }
#pragma unroll
        for (int k = 0; k < R; k++) {
            const int e = k * 64 + lane, row = e / R;
            lds[row * STRIDE + (e - row * R)] = v[k];
        }
    }
    __syncthreads();
    if (sel) {
#pragma unroll
        for (int j = 0; j < R; j++) mine[j] = lds[lane * STRIDE + j];
    }
    __syncthreads();  // the buffer is free again
}

// the workgroup's total in thread 0: butterfly inside each wave, then the waves in ascending order
__device__ __forceinline__ PosePartial pose_block_reduce(PosePartial v, PosePartial* waves) {
#pragma unroll
    for (int k = 0; k < 7; k++) v.a[k] = wave_sum(v.a[k]);
    v.n = wave_sum(v.n);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    PosePartial total = waves[0];
#pragma unroll
    for (int w = 1; w < POSE_WAVES; w++) {
#pragma unroll
        for (int k = 0; k < 7; k++) total.a[k] = total.a[k] + waves[w].a[k];
        total.n += waves[w].n;
    }
    return total;
}

template <int R>
__global__ __launch_bounds__(POSE_THREADS) void pose_partial_k(long long P, const uint8_t* __restrict__ selection, int invert,
                                                              const PoseGenerators G, const PosePointers p,
                                                              PosePartial* __restrict__ partials) {
    __shared__ float lds[R ? POSE_WAVES * 64 * RestRow<R>::STRIDE : 1];
    __shared__ PosePartial waves[POSE_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform, and the compiler knows: scalar row bases
    float pv[3] = {0.0f, 0.0f, 0.0f};
    if (p.g_xyz) {
#pragma unroll
        for (int k = 0; k < 3; k++) pv[k] = p.pivot_dev ? p.pivot_dev[k] : p.pivot[k];
    }
    PosePartial acc;
#pragma unroll
    for (int k = 0; k < 7; k++) acc.a[k] = 0.0;
    acc.n = 0;
    const long long chunks = (P + 63) / 64;
    // the same trip count for every wave of the workgroup (pose_rest holds barriers): a wave past the end has nothing selected
    for (long long c0 = (long long)blockIdx.x * POSE_WAVES; c0 < chunks; c0 += (long long)gridDim.x * POSE_WAVES) {
        const long long base = (c0 + wave) * 64;
        const long long i = base + lane;
        const bool sel = i < P && edit_selected(selection, invert, i);
        const unsigned long long ballot = __ballot(sel);
        if (sel) {
            acc.n++;
            if (p.g_xyz) {
                const float* x = p.xyz + 3 * i;
                const float* gx = p.g_xyz + 3 * i;
                const float d0 = x[0] - pv[0], d1 = x[1] - pv[1], d2 = x[2] - pv[2];
                const float g0 = gx[0], g1 = gx[1], g2 = gx[2];
                acc.a[0] = acc.a[0] + (double)(d1 * g2 - d2 * g1);  // d x g_x
                acc.a[1] = acc.a[1] + (double)(d2 * g0 - d0 * g2);
                acc.a[2] = acc.a[2] + (double)(d0 * g1 - d1 * g0);
                acc.a[3] = acc.a[3] + (double)g0;
                acc.a[4] = acc.a[4] + (double)g1;
                acc.a[5] = acc.a[5] + (double)g2;
                acc.a[6] = acc.a[6] + (double)((g0 * d0 + g1 * d1) + g2 * d2);
            }
            if (p.g_rotation) {
                const float* r = p.rotation + 4 * i;
                const float* gr = p.g_rotation + 4 * i;
                const float w = r[0], v0 = r[1], v1 = r[2], v2 = r[3];
                const float gw = gr[0], h0 = gr[1], h1 = gr[2], h2 = gr[3];
                acc.a[0] = acc.a[0] + (double)(0.5f * ((w * h0 - gw * v0) + (v1 * h2 - v2 * h1)));  // 1/2 (w g_v - g_w v + v x g_v)
                acc.a[1] = acc.a[1] + (double)(0.5f * ((w * h1 - gw * v1) + (v2 * h0 - v0 * h2)));
                acc.a[2] = acc.a[2] + (double)(0.5f * ((w * h2 - gw * v2) + (v0 * h1 - v1 * h0)));
            }
            if (p.g_scaling) {
                const float* gl = p.g_scaling + 3 * i;
                acc.a[6] = acc.a[6] + (double)((gl[0] + gl[1]) + gl[2]);
            }
        }
        if constexpr (R > 0) {  // (the launcher picks R > 0 only with g_rest)
            float c[R], gc[R];
#pragma unroll
            for (int j = 0; j < R; j++) c[j] = gc[j] = 0.0f;
            float* mine = lds + wave * 64 * RestRow<R>::STRIDE;
            pose_rest<R>(p.rest, base, ballot, sel, lane, mine, c);
            pose_rest<R>(p.g_rest, base, ballot, sel, lane, mine, gc);
            if (sel) {
                acc.a[0] = acc.a[0] + (double)colour_term<R, 0>(G.x, gc, c);
                acc.a[1] = acc.a[1] + (double)colour_term<R, 1>(G.y, gc, c);
                acc.a[2] = acc.a[2] + (double)colour_term<R, 2>(G.z, gc, c);
            }
        }
    }
    const PosePartial total = pose_block_reduce(acc, waves);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(POSE_THREADS) void pose_final_k(const PosePartial* __restrict__ partials, int n_partials,
                                                             int* __restrict__ count, double* __restrict__ out) {
    __shared__ PosePartial waves[POSE_WAVES];
    PosePartial v;
#pragma unroll
    for (int k = 0; k < 7; k++) v.a[k] = 0.0;
    v.n = 0;
    for (int b = threadIdx.x; b < n_partials; b += POSE_THREADS) {
#pragma unroll
        for (int k = 0; k < 7; k++) v.a[k] = v.a[k] + partials[b].a[k];
        v.n += partials[b].n;
    }
    const PosePartial total = pose_block_reduce(v, waves);
    if (threadIdx.x != 0) return;
    *count = (int)total.n;
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = total.a[k];
}

inline long long pose_blocks(long long P) {
    const long long b = ((P + 63) / 64 + POSE_WAVES - 1) / POSE_WAVES;
    return b < POSE_MAX_BLOCKS ? b : POSE_MAX_BLOCKS;
}

size_t pose_workspace_bytes(long long P) { return (size_t)(pose_blocks(P) + 1) * sizeof(PosePartial); }

void launch_pose_gradient(long long P, int M, const uint8_t* selection, int invert, const PoseGenerators& G, const PosePointers& p,
                          int* count, double* out, void* ws, hipStream_t s) {
    PosePartial* partials = static_cast<PosePartial*>(ws);
    const int blocks = (int)pose_blocks(P);
    if (blocks > 0) {
        const dim3 grid((unsigned)blocks), block(POSE_THREADS);
        const int R = p.g_rest ? 3 * (M - 1) : 0;
        if (R == 45)
            pose_partial_k<45><<<grid, block, 0, s>>>(P, selection, invert, G, p, partials);
        else if (R == 24)
            pose_partial_k<24><<<grid, block, 0, s>>>(P, selection, invert, G, p, partials);
        else if (R == 9)
            pose_partial_k<9><<<grid, block, 0, s>>>(P, selection, invert, G, p, partials);
        else
            pose_partial_k<0><<<grid, block, 0, s>>>(P, selection, invert, G, p, partials);
    }
    pose_final_k<<<dim3(1), dim3(POSE_THREADS), 0, s>>>(partials, blocks, count, out);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_pose_gradient_workspace_bytes(long long P) {
    return (P >= 0 && P < (1ll << 31)) ? pose_workspace_bytes(P) + 256 : 0;
}

int goi_pose_gradient(long long P, int M, const unsigned char* selection, int invert, const float* xyz, const float* rotation,
                      const float* features_rest, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                      const float* g_features_rest, const float* generators, const float* pivot_host, const float* pivot_dev,
                      int* count, double* out, void* workspace, void* stream) {
    const char* fn = "goi_pose_gradient";
    if (P < 0 || P >= (1ll << 31)) return fail(std::string(fn) + ": need 0 <= P < 2^31");
    if (M != 1 && M != 4 && M != 9 && M != 16) return fail(std::string(fn) + ": M must be 1, 4, 9 or 16");
    if (P > 0) {  // (of no rows every pointer may be NULL)
        if (!g_xyz && !g_rotation && !g_scaling && !g_features_rest) return fail(std::string(fn) + ": every gradient pointer is NULL");
        if ((g_xyz && !xyz) || (g_rotation && !rotation) || (g_features_rest && !features_rest))
            return fail(std::string(fn) + ": a gradient is given whose parameter pointer is NULL");
        if (M == 1 && g_features_rest) return fail(std::string(fn) + ": M = 1 has no features_rest gradient");
    }
    if (!out || !count || !generators) return fail(std::string(fn) + ": a required pointer is NULL");
    if (check_workspace(fn, workspace) < 0) return -1;
    PoseGenerators G;
    for (int k = 0; k < 18; k++) G.x[k] = generators[k];
    for (int k = 0; k < 18; k++) G.y[k] = generators[18 + k];
    for (int k = 0; k < 12; k++) G.z[k] = generators[36 + k];
    PosePointers p;
    p.xyz = xyz;
    p.rotation = rotation;
    p.rest = features_rest;
    p.g_xyz = g_xyz;
    p.g_rotation = g_rotation;
    p.g_scaling = g_scaling;
    p.g_rest = M > 1 ? g_features_rest : nullptr;
    p.pivot_dev = pivot_dev;
    for (int k = 0; k < 3; k++) p.pivot[k] = pivot_host ? pivot_host[k] : 0.0f;
    launch_pose_gradient(P, M, selection, invert, G, p, count, out, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
