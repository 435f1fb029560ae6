// The mask-contrast loss of a rendered feature map against one view's 2D instance masks (DESIGN.md section 4.31;
// goi_hyperplane_amd/grouping.py).  feat [S,H,W] fp32 channel-major as the rasterizer writes `semantics`, labels [H,W] int32; pixel p is
// in mask m = labels[p] iff 0 <= m < K.  With n_m the pixels of mask m, N their total, M the non-empty masks, mu_m the mean feature:
//   L_intra = sum_m a_m sum_{p in m} |f_p - mu_m|^2     a_m = 1/N (balance 0, "pixel")  or  1/(M n_m) (balance 1, "mask")
//   L_inter = 1/(M(M-1)) sum_{m != m', both non-empty} max(0, margin - |mu_m - mu_m'|)^2
//   L = w_intra L_intra + w_inter L_inter,   dL/df_p = 2 w_intra a_m (f_p - mu_m) + w_inter g_m / n_m,
//   g_m = -4/(M(M-1)) sum_{m' != m, 0 < d < margin} (margin - d)/d (mu_m - mu_m')
// (the dependence of L_intra on mu cancels).  A pair at d == 0 adds margin^2 and no gradient; M == 0: L = 0; M == 1: L_inter = 0.
//
// THE SUMS ARE INTEGERS.  v = rint(f * 2^q) in float64 with q = 40 - e, e the smallest integer with max|f| < 2^e over the WHOLE
// map (0 for an all-zero map), so |v| <= 2^40, and with H*W <= 2^22 no sum reaches 2^62: count [K] and qsum [K,S] are exact int64
// sums, free of any order.  rint is spelled as the float64 add of 1.5 * 2^52 (x + C rounds x to the nearest integer, ties to
// even, and the integer sits in the low bits of the sum's pattern): a lane adds the PATTERNS and takes n times C's pattern off
// when it hands its run over, modulo 2^64.  The maximum comes from grp_max_k (integer atomicMax on the pattern of |f| after a wave
// and a workgroup maximum), or from the caller's max_abs: then a pixel with |f| >= 2^e (a NaN included) counts as +-2^40 and raises
// bit 0 of *status.
//
// Launches, all on the caller's stream, nothing read back:
//   grp_zero_k    count, qsum, status and the workspace's three words (maximum, M, N) = 0
//   grp_max_k     (without max_abs) the maximum of |f|: one pass over feat
//   grp_sums_k    THE HOT PASS.  A wave owns a strip of 64 columns x `rows` rows and walks it downwards, lane = column: every load is
//                 256 contiguous bytes, and a lane's successive pixels are vertical neighbours, which a mask keeps together.  A lane
//                 adds into registers while its label stays (its run); when the label changes it hands the run's S + 1 sums to the
//                 workgroup's LDS table [K, S+1] of int64 by LDS atomics, and when the workgroup is done the table's non-zero
//                 words go to memory, one 64-bit integer atomic each.  A uniform map therefore costs one LDS hand-over per lane
//                 and S + 1 global atomics per WORKGROUP (some 500 per word), not per wave.  When K (S+1) int64 exceed
//                 GRP_LDS_BYTES there is no table: the lanes of a wave that hand over at the same step are peeled label by label
//                 (ballot, broadcast of the first open lane's label, a butterfly over its lanes; at most 64 rounds) and one lane
//                 adds the S + 1 sums to memory.
//   grp_means_k   mu = (double)qsum * 2^-q / n; M and N by integer atomics
//   grp_pairs_k   a workgroup per mask m: thread t takes m' = t, t + 256, ... in ascending order, the 256 threads are folded by
//                 the butterfly and the four waves in order: g_m, the mask's share of L_inter, a_m, gamma_m = w_inter g_m / n_m.
//   grp_grad_k    one read of feat and labels: d = (double)f - mu_m, grad = (float)(2 w_intra a_m d + gamma_m) -- the affine map
//                 alpha f + beta in its centred form, which loses nothing when |mu| is 1000 times the spread -- or 0 for an
//                 ignored pixel; a_m |d|^2 in float64 per lane in pixel order, then butterfly, then the four waves: one partial
//                 per workgroup.  The table (a, mu as float64; gamma as fp32) sits in LDS when it fits GRP_LDS_BYTES, else it is
//                 read from memory.  grad == NULL skips the store.
//   grp_final_k   partials and the masks' shares in a fixed order -> loss, intra, inter as fp32.
// No float atomics, every loop bounded, the same bits on every call.  C entries at the end of the file (include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace goi {

namespace {

constexpr int GRP_THREADS = 256;
constexpr int GRP_WAVES = GRP_THREADS / 64;
constexpr int GRP_S_MAX = 32;
constexpr int GRP_K_MAX = 1 << 16;
constexpr long long GRP_HW_MAX = 1ll << 22;
constexpr int GRP_QBITS = 40;                    // |v| <= 2^40
constexpr int GRP_SUM_WAVES = 2048;              // grp_sums_k: about this many strips (two workgroups of four waves per CU)
constexpr int GRP_GRAD_BLOCKS = 512;             // grp_grad_k: at most this many workgroups, hence partials
constexpr int GRP_MAX_BLOCKS = 512;              // grp_max_k: at most this many workgroups, hence atomics on the one word
constexpr size_t GRP_LDS_BYTES = 60 * 1024;      // a table larger than this stays in memory (64 KiB less the static arrays)
constexpr double GRP_MAGIC = 6755399441055744.0;  // 1.5 * 2^52
constexpr unsigned long long GRP_MAGIC_BITS = 0x4338000000000000ull;
constexpr int GRP_E_NONE = 1 << 20;              // "e comes from grp_max_k"

unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the smallest integer e with x < 2^e for the non-negative float of pattern u (0 for x == 0; 129 for inf and NaN)
__host__ __device__ inline int exp_above(uint32_t u) {
    const uint32_t E = (u >> 23) & 0xFFu, mant = u & 0x7FFFFFu;
    if (E) return (int)E - 126;
    return mant ? (32 - __builtin_clz(mant)) - 149 : 0;
}

size_t sums_table_bytes(int S, int K) { return (size_t)K * (S + 1) * sizeof(unsigned long long); }
size_t grad_table_bytes(int S, int K) { return (size_t)K * (sizeof(double) + (size_t)S * (sizeof(double) + sizeof(float))); }

__global__ __launch_bounds__(GRP_THREADS) void grp_zero_k(int K, int S, unsigned long long* __restrict__ count,
                                                          unsigned long long* __restrict__ qsum, int32_t* __restrict__ status,
                                                          unsigned long long* __restrict__ words) {
    const long long i = (long long)blockIdx.x * GRP_THREADS + threadIdx.x;
    if (i < K) count[i] = 0;
    if (i < (long long)K * S) qsum[i] = 0;
    if (i < 3) words[i] = 0;
    if (i == 0) *status = 0;
}

// words[0] = the largest pattern of |f| over feat [n]
__global__ __launch_bounds__(GRP_THREADS) void grp_max_k(long long n, const float* __restrict__ feat, unsigned long long* words) {
    __shared__ uint32_t part[GRP_WAVES];
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(feat);
    const long long stride = (long long)gridDim.x * GRP_THREADS, t = (long long)blockIdx.x * GRP_THREADS + threadIdx.x;
    uint32_t m = 0;
    if ((reinterpret_cast<uintptr_t>(feat) & 15) == 0) {
        const uint4* quads = reinterpret_cast<const uint4*>(feat);
        const long long nq = n / 4;
        for (long long i = t; i < nq; i += stride) {
            const uint4 v = quads[i];
            m = max(max(m, v.x & 0x7FFFFFFFu), max(v.y & 0x7FFFFFFFu, max(v.z & 0x7FFFFFFFu, v.w & 0x7FFFFFFFu)));
        }
        if (t < n - nq * 4) m = max(m, bits[nq * 4 + t] & 0x7FFFFFFFu);
    } else {
        for (long long i = t; i < n; i += stride) m = max(m, bits[i] & 0x7FFFFFFFu);
    }
    m = wave_butterfly(m, [](uint32_t a, uint32_t b) { return max(a, b); });
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < GRP_WAVES; w++) m = max(m, part[w]);
        if (m) atomicMax(reinterpret_cast<uint32_t*>(words), m);  // (little endian: the low half of words[0])
    }
}

// ---- stage 1: the integer sums ---------------------------------------------------------------------------------------------------------
// The lanes with `need` hand their run (label cur, n pixels, pattern sums acc) to memory, peeled label by label.  Every lane of
// the wave calls this.
template <int SP>
__device__ __forceinline__ void hand_over_wave(bool need, int cur, unsigned long long n, const unsigned long long (&acc)[SP], int S,
                                               int lane, unsigned long long* __restrict__ count, unsigned long long* __restrict__ qsum) {
    unsigned long long open = __ballot(need);
    for (int round = 0; round < 64 && open; round++) {
        const int first = __builtin_ctzll(open);
        const int lead = __shfl(cur, first);
        const bool mine = need && cur == lead;
        const unsigned long long n_all = wave_sum(mine ? n : 0ull);
        if (lane == first) atomicAdd(count + lead, n_all);
#pragma unroll
        for (int c = 0; c < SP; c++) {
            if (c < S) {
                const unsigned long long s = wave_sum(mine ? acc[c] : 0ull) - n_all * GRP_MAGIC_BITS;
                if (lane == first) atomicAdd(qsum + (size_t)lead * S + c, s);
            }
        }
        need = need && !mine;
        open = __ballot(need);
    }
}

template <int SP>
__global__ __launch_bounds__(GRP_THREADS) void grp_sums_k(int S, int H, int W, int K, int rows, int strips_y, int strips,
                                                          const float* __restrict__ feat, const int32_t* __restrict__ labels,
                                                          int e_given, const unsigned long long* __restrict__ words,
                                                          unsigned long long* __restrict__ count, unsigned long long* __restrict__ qsum,
                                                          int32_t* __restrict__ qexp, int32_t* __restrict__ status, int use_lds) {
    extern __shared__ unsigned long long tab[];  // [K, S+1]: count, then the S sums (use_lds)
    const int lane = threadIdx.x & 63, row_len = S + 1;
    const int cells = use_lds ? K * row_len : 0;
    for (int i = threadIdx.x; i < cells; i += GRP_THREADS) tab[i] = 0;
    if (use_lds) __syncthreads();
    const int e = e_given != GRP_E_NONE ? e_given : exp_above((uint32_t)words[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) *qexp = GRP_QBITS - e;
    const double scale = ldexp(1.0, GRP_QBITS - e);
    const float bound = ldexpf(1.f, e);  // (+inf from e = 128 on: then only an infinity or a NaN is "at or above")
    const size_t HW = (size_t)H * W;
    const int strip = blockIdx.x * GRP_WAVES + (threadIdx.x >> 6);  // (the same in every lane of the wave)
    int cur = -1;
    unsigned long long n = 0, acc[SP];
#pragma unroll
    for (int c = 0; c < SP; c++) acc[c] = 0;
    bool sat = false;
    if (strip < strips) {
        const int x = (strip / strips_y) * 64 + lane, y0 = (strip % strips_y) * rows, y1 = min(y0 + rows, H);
        const bool active = x < W;
        for (int y = y0; y < y1; y++) {
            const size_t p = (size_t)y * W + x;
            int lab = -1;
            float f[SP];
#pragma unroll
            for (int c = 0; c < SP; c++) f[c] = 0.f;
            if (active) {
                lab = labels[p];
                if (lab < 0 || lab >= K) lab = -1;
#pragma unroll
                for (int c = 0; c < SP; c++)
                    if (c < S) f[c] = feat[(size_t)c * HW + p];
            }
            const bool need = lab != cur && cur >= 0;
            if (use_lds) {
                if (need) {
                    unsigned long long* row = tab + cur * row_len;
                    atomicAdd(row, n);
#pragma unroll
                    for (int c = 0; c < SP; c++)
                        if (c < S) atomicAdd(row + 1 + c, acc[c] - n * GRP_MAGIC_BITS);
                }
            } else if (__any(need)) {
                hand_over_wave<SP>(need, cur, n, acc, S, lane, count, qsum);
            }
            if (lab != cur) {
                cur = lab;
                n = 0;
#pragma unroll
                for (int c = 0; c < SP; c++) acc[c] = 0;
            }
            if (lab >= 0) {
                n++;
#pragma unroll
                for (int c = 0; c < SP; c++) {
                    if (c < S) {
                        double v = (double)f[c] * scale;
                        if (!(fabsf(f[c]) < bound)) {
                            v = copysign(1099511627776.0 /* 2^40 */, (double)f[c]);
                            sat = true;
                        }
                        acc[c] += (unsigned long long)__double_as_longlong(v + GRP_MAGIC);
                    }
                }
            }
        }
    }
    // the runs that are still open
    const bool need = cur >= 0;
    if (use_lds) {
        if (need) {
            unsigned long long* row = tab + cur * row_len;
            atomicAdd(row, n);
#pragma unroll
            for (int c = 0; c < SP; c++)
                if (c < S) atomicAdd(row + 1 + c, acc[c] - n * GRP_MAGIC_BITS);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += GRP_THREADS) {
            const unsigned long long v = tab[i];
            if (v) {
                const int m = i / row_len, j = i - m * row_len;
                atomicAdd(j ? qsum + (size_t)m * S + (j - 1) : count + m, v);
            }
        }
    } else if (__any(need)) {
        hand_over_wave<SP>(need, cur, n, acc, S, lane, count, qsum);
    }
    if (__any(sat) && lane == 0) atomicOr(status, 1);
}

// ---- stage 2: the tables ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRP_THREADS) void grp_means_k(int K, int S, const unsigned long long* __restrict__ count,
                                                           const unsigned long long* __restrict__ qsum, const int32_t* __restrict__ qexp,
                                                           double* __restrict__ mu, unsigned long long* words) {
    const int m = blockIdx.x * GRP_THREADS + threadIdx.x;
    const unsigned long long n = m < K ? count[m] : 0ull;
    if (m < K) {
        const double unit = ldexp(1.0, -*qexp), dn = (double)n;
        for (int c = 0; c < S; c++) mu[(size_t)m * S + c] = n ? (double)(long long)qsum[(size_t)m * S + c] * unit / dn : 0.0;
    }
    const unsigned long long masks = wave_sum(n ? 1ull : 0ull), pixels = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && masks) {
        atomicAdd(words + 1, masks);
        atomicAdd(words + 2, pixels);
    }
}

__global__ __launch_bounds__(GRP_THREADS) void grp_pairs_k(int K, int S, const unsigned long long* __restrict__ count,
                                                           const double* __restrict__ mu, const unsigned long long* __restrict__ words,
                                                           double margin, double w_inter, int balance, double* __restrict__ a,
                                                           float* __restrict__ gamma, double* __restrict__ share) {
    __shared__ double mine[GRP_S_MAX];
    __shared__ double red[GRP_WAVES][GRP_S_MAX + 1];
    const int m = blockIdx.x, t = threadIdx.x;
    const unsigned long long n = count[m], M = words[1], N = words[2];
    if (!n) {  // (the same in every thread)
        if (t == 0) {
            a[m] = 0.0;
            share[m] = 0.0;
        }
        if (t < S) gamma[(size_t)m * S + t] = 0.f;
        return;
    }
    if (t < S) mine[t] = mu[(size_t)m * S + t];
    __syncthreads();
    double g[GRP_S_MAX], l = 0.0;
#pragma unroll
    for (int c = 0; c < GRP_S_MAX; c++) g[c] = 0.0;
    if (M > 1) {
        for (int o = t; o < K; o += GRP_THREADS) {
            if (o == m || !count[o]) continue;
            const double* other = mu + (size_t)o * S;
            double d2 = 0.0;
            for (int c = 0; c < S; c++) {
                const double e = mine[c] - other[c];
                d2 = d2 + e * e;
            }
            if (d2 == 0.0) {
                l = l + margin * margin;
                continue;
            }
            const double d = sqrt(d2);
            if (!(d < margin)) continue;
            const double r = margin - d, k = r / d;
            l = l + r * r;
#pragma unroll
            for (int c = 0; c < GRP_S_MAX; c++)
                if (c < S) g[c] = g[c] + k * (mine[c] - other[c]);
        }
    }
    const int w = t >> 6;
#pragma unroll
    for (int c = 0; c < GRP_S_MAX; c++) {
        if (c < S) {
            const double s = wave_sum(g[c]);
            if ((t & 63) == 0) red[w][c] = s;
        }
    }
    l = wave_sum(l);
    if ((t & 63) == 0) red[w][GRP_S_MAX] = l;
    __syncthreads();
    const double pairs = (double)M * (double)(M - 1);  // (> 0 where it divides)
    if (t < S) {
        const double G = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        const double gm = M > 1 ? -4.0 / pairs * G : 0.0;
        gamma[(size_t)m * S + t] = (float)(w_inter * gm / (double)n);
    }
    if (t == 0) {
        share[m] = ((red[0][GRP_S_MAX] + red[1][GRP_S_MAX]) + red[2][GRP_S_MAX]) + red[3][GRP_S_MAX];
        a[m] = balance ? 1.0 / ((double)M * (double)n) : 1.0 / (double)N;
    }
}

// ---- stage 3: the gradient and the residual --------------------------------------------------------------------------------------------
// the sum of v over the workgroup in a fixed order (butterfly, then the waves in order); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* part /*[GRP_WAVES] shared*/) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

template <bool LDS>
__global__ __launch_bounds__(GRP_THREADS) void grp_grad_k(int S, int HW, int K, int chunk, const float* __restrict__ feat,
                                                          const int32_t* __restrict__ labels, const double* __restrict__ a,
                                                          const double* __restrict__ mu, const float* __restrict__ gamma,
                                                          double w_intra, float* __restrict__ grad, double* __restrict__ partial) {
    extern __shared__ double table[];  // a [K] | mu [K,S] | gamma [K,S] fp32 (LDS)
    __shared__ double part[GRP_WAVES];
    const double *A = a, *MU = mu;
    const float* G = gamma;
    if (LDS) {
        double* sa = table;
        double* smu = table + K;
        float* sg = reinterpret_cast<float*>(table + K + (size_t)K * S);
        for (int i = threadIdx.x; i < K; i += GRP_THREADS) sa[i] = a[i];
        for (int i = threadIdx.x; i < K * S; i += GRP_THREADS) {
            smu[i] = mu[i];
            sg[i] = gamma[i];
        }
        __syncthreads();
        A = sa;
        MU = smu;
        G = sg;
    }
    const int start = blockIdx.x * chunk, end = min(start + chunk, HW);
    double r = 0.0;
    for (int p = start + threadIdx.x; p < end; p += GRP_THREADS) {
        const int lab = labels[p];
        if (lab >= 0 && lab < K) {
            const double am = A[lab], alpha = 2.0 * w_intra * am;
            const double* mrow = MU + (size_t)lab * S;
            const float* grow = G + (size_t)lab * S;
            double s = 0.0;
#pragma unroll 8
            for (int c = 0; c < S; c++) {
                const double d = (double)feat[(size_t)c * HW + p] - mrow[c];
                s = s + d * d;
                if (grad) grad[(size_t)c * HW + p] = (float)(alpha * d + (double)grow[c]);
            }
            r = r + am * s;
        } else if (grad) {
            for (int c = 0; c < S; c++) grad[(size_t)c * HW + p] = 0.f;
        }
    }
    r = block_sum(r, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(GRP_THREADS) void grp_final_k(int blocks, const double* __restrict__ partial, int K,
                                                           const double* __restrict__ share, const unsigned long long* __restrict__ words,
                                                           double w_intra, double w_inter, float* __restrict__ loss,
                                                           float* __restrict__ intra, float* __restrict__ inter) {
    __shared__ double part[GRP_WAVES], part2[GRP_WAVES];
    double r = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < blocks; i += GRP_THREADS) r = r + partial[i];
    for (int i = threadIdx.x; i < K; i += GRP_THREADS) l = l + share[i];
    r = block_sum(r, part);
    l = block_sum(l, part2);
    if (threadIdx.x == 0) {
        const unsigned long long M = words[1];
        const double L_inter = M > 1 ? l / ((double)M * (double)(M - 1)) : 0.0;
        *intra = (float)r;
        *inter = (float)L_inter;
        *loss = (float)(w_intra * r + w_inter * L_inter);
    }
}

// Workspace: the three words (maximum pattern, M, N) | a [K] | mu [K,S] | gamma [K,S] | the masks' shares of L_inter [K] | partials
struct GroupingView {
    unsigned long long* words;
    double *a, *mu, *share, *partial;
    float* gamma;
};
size_t grouping_layout(int S, int K, char* base, GroupingView* v) {
    Carver c(base);
    GroupingView t;
    t.words = c.take<unsigned long long>(3);
    t.a = c.take<double>((size_t)K);
    t.mu = c.take<double>((size_t)K * S);
    t.gamma = c.take<float>((size_t)K * S);
    t.share = c.take<double>((size_t)K);
    t.partial = c.take<double>(GRP_GRAD_BLOCKS);
    if (v) *v = t;
    return c.bytes();
}

bool sizes_ok(int S, int H, int W, int K) {
    return S >= 1 && S <= GRP_S_MAX && H >= 1 && W >= 1 && (long long)H * W <= GRP_HW_MAX && K >= 0 && K <= GRP_K_MAX;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

template <int SP>
void launch_sums(dim3 grid, size_t lds, hipStream_t s, int S, int H, int W, int K, int rows, int strips_y, int strips, const float* feat,
                 const int32_t* labels, int e_given, const unsigned long long* words, unsigned long long* count, unsigned long long* qsum,
                 int32_t* qexp, int32_t* status, int use_lds) {
    grp_sums_k<SP><<<grid, dim3(GRP_THREADS), lds, s>>>(S, H, W, K, rows, strips_y, strips, feat, labels, e_given, words, count, qsum,
                                                       qexp, status, use_lds);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_mask_contrast_workspace_bytes(int S, int H, int W, int K) {
    return sizes_ok(S, H, W, K) ? grouping_layout(S, K, nullptr, nullptr) : 0;
}

int goi_mask_contrast(int S, int H, int W, int K, const float* feat, const int32_t* labels, float margin, float w_intra, float w_inter,
                      int balance, float max_abs, float* loss, float* intra, float* inter, float* grad, int64_t* count, int64_t* qsum,
                      int32_t* qexp, int32_t* status, void* workspace, void* stream) {
    const char* fn = "goi_mask_contrast";
    if (S < 1 || S > GRP_S_MAX) return fail(std::string(fn) + ": need 1 <= S <= 32");
    if (H < 1 || W < 1) return fail(std::string(fn) + ": need H >= 1 and W >= 1");
    if ((long long)H * W > GRP_HW_MAX) return fail(std::string(fn) + ": need H * W <= 2^22");
    if (K < 0 || K > GRP_K_MAX) return fail(std::string(fn) + ": need 0 <= K <= 65536");
    if (balance != 0 && balance != 1) return fail(std::string(fn) + ": balance must be 0 (pixel) or 1 (mask)");
    if (!(margin >= 0.f) || std::isinf(margin) || std::isnan(w_intra) || std::isinf(w_intra) || std::isnan(w_inter) || std::isinf(w_inter))
        return fail(std::string(fn) + ": need a finite margin >= 0 and finite weights");
    if (std::isnan(max_abs) || std::isinf(max_abs)) return fail(std::string(fn) + ": max_abs must be finite (negative: not given)");
    if (!feat || !labels || !loss || !intra || !inter || !qexp || !status || (K > 0 && (!count || !qsum)))
        return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned(feat, 4) || misaligned(labels, 4) || misaligned(loss, 4) || misaligned(intra, 4) || misaligned(inter, 4) ||
        misaligned(grad, 4) || misaligned(qexp, 4) || misaligned(status, 4))
        return fail(std::string(fn) + ": feat, labels, loss, intra, inter, grad, qexp and status must be 4-byte aligned");
    if (misaligned(count, 8) || misaligned(qsum, 8)) return fail(std::string(fn) + ": count and qsum must be 8-byte aligned");
    if (check_workspace(fn, workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GroupingView w;
    grouping_layout(S, K, static_cast<char*>(workspace), &w);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(qsum);
    const int HW = H * W;
    const dim3 block(GRP_THREADS);

    grp_zero_k<<<dim3(blocks_for(std::max((long long)K * S, 3ll), GRP_THREADS)), block, 0, s>>>(K, S, cnt, sums, status, w.words);
    int e_given = GRP_E_NONE;
    if (max_abs >= 0.f) {
        uint32_t u;
        std::memcpy(&u, &max_abs, sizeof u);
        e_given = exp_above(u);
    } else {
        const long long n = (long long)S * HW;
        grp_max_k<<<dim3(std::min(blocks_for(n, GRP_THREADS * 8), (unsigned)GRP_MAX_BLOCKS)), block, 0, s>>>(n, feat, w.words);
    }

    // strips of 64 columns x `rows` rows, about GRP_SUM_WAVES of them
    const int strips_x = (W + 63) / 64;
    const int rows = (int)(((long long)H * strips_x + GRP_SUM_WAVES - 1) / GRP_SUM_WAVES);
    const int strips_y = (H + rows - 1) / rows, strips = strips_x * strips_y;
    const size_t sums_lds = sums_table_bytes(S, K);
    const int use_lds = sums_lds <= GRP_LDS_BYTES;
    const dim3 sums_grid(blocks_for(strips, GRP_WAVES));
    const size_t lds = use_lds ? sums_lds : 0;
    if (S <= 4)
        launch_sums<4>(sums_grid, lds, s, S, H, W, K, rows, strips_y, strips, feat, labels, e_given, w.words, cnt, sums, qexp, status, use_lds);
    else if (S <= 16)
        launch_sums<16>(sums_grid, lds, s, S, H, W, K, rows, strips_y, strips, feat, labels, e_given, w.words, cnt, sums, qexp, status, use_lds);
    else
        launch_sums<32>(sums_grid, lds, s, S, H, W, K, rows, strips_y, strips, feat, labels, e_given, w.words, cnt, sums, qexp, status, use_lds);

    if (K > 0) {
        grp_means_k<<<dim3(blocks_for(K, GRP_THREADS)), block, 0, s>>>(K, S, cnt, sums, qexp, w.mu, w.words);
        grp_pairs_k<<<dim3(K), block, 0, s>>>(K, S, cnt, w.mu, w.words, (double)margin, (double)w_inter, balance, w.a, w.gamma, w.share);
    }

    // a contiguous chunk of pixels per workgroup, a multiple of the workgroup's size
    const int want = (int)std::min(blocks_for(HW, GRP_THREADS), (unsigned)GRP_GRAD_BLOCKS);
    const int chunk = (int)blocks_for(blocks_for(HW, want), GRP_THREADS) * GRP_THREADS;
    const int grad_blocks = (int)blocks_for(HW, chunk);
    const size_t grad_lds = grad_table_bytes(S, K);
    if (grad_lds <= GRP_LDS_BYTES)
        grp_grad_k<true><<<dim3(grad_blocks), block, grad_lds, s>>>(S, HW, K, chunk, feat, labels, w.a, w.mu, w.gamma, (double)w_intra, grad,
                                                                   w.partial);
    else
        grp_grad_k<false><<<dim3(grad_blocks), block, 0, s>>>(S, HW, K, chunk, feat, labels, w.a, w.mu, w.gamma, (double)w_intra, grad,
                                                             w.partial);
    grp_final_k<<<dim3(1), block, 0, s>>>(grad_blocks, w.partial, K, w.share, w.words, (double)w_intra, (double)w_inter, loss, intra, inter);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
