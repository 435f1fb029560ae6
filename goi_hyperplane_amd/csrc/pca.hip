// A PCA picture of the semantic features on the device: fit a three-component basis on a rendered [S][H][W] map (or on
// the Gaussians' own [P][S] features), project, normalise for display.  The reference does this on the host
// (gui/main_edit.py:1841-1870 visual_latent, utils/visual_latent.py:32-40: a copy of the map to the host and sklearn's
// PCA(n_components=3).fit_transform on its HW x S rows).
//
//   pca_pivot_k       (first call only) the pivot c: the channel means of the used samples among PIVOT_SAMPLES samples
//                     in chunks spread over the whole set (of all of these when the mask uses none; 0 where that mean is not
//                     finite).  One workgroup, 32 lanes per channel, fixed summation order.
//   pca_accumulate_k  one stream of the input.  The Gram update G += D^T D of the pivoted samples d = x - c IS
//                     v_mfma_f32_16x16x4_f32 with A and B the same register: lane l holds channel l & 15 of sample l >> 4
//                     of a tile of four samples; 4 accumulator registers per 16 x 16 block, one block for S <= 16 (the
//                     channels zero-padded), three (00, 01, 11) for S <= 32.  The instruction is an exact fp32 fmaf chain.
//                     Per-channel sums of d ride along in one VALU add, the count in an integer.  A masked-out sample is
//                     SELECTED to zero, never multiplied, so what it holds (a NaN included) cannot reach the moments.
//                     A fixed grid of PCA_SLOTS workgroups of 16 waves; the waves' fp32 partials are added in wave order
//                     in fp64 and land in (first call) or are added to (later calls) the workgroup's own fp64 slot: no
//                     float atomics, bit-reproducible, and a camera set accumulates in fp64 across its views.
//   pca_reduce_k      the slots summed in slot order (fp64) into one total.
//   pca_solve_k       one wave, fp64: mean = c + sum d / n, cov = (G - n md md^T) / (n - 1) (the pivot cancels exactly:
//                     d is small, so nothing of size |x|^2 is ever subtracted), cyclic Jacobi in the round-robin ordering
//                     (S/2 disjoint rotations per step) with a FIXED maximum of sweeps, the three largest eigenpairs in
//                     descending order, the largest-magnitude entry of each component positive (sklearn's svd_flip with
//                     u_based_decision=False), negative eigenvalues clipped to zero as sklearn does.
//   pca_apply_k       q_k = (x - mean) . component_k in channel order, one fp32 rounding per operation (the file is built
//                     with -ffp-contract=off), by the same code for every normalisation, layout and path; MINMAX takes a
//                     first launch for the per-view, per-component minima and maxima (order-preserving integer keys and
//                     atomicMax, as display.hip: order-independent, NaNs skipped).  Planar maps on 16-byte boundaries with
//                     n % 4 == 0 take 16-byte loads and stores, everything else one sample per thread with the same bits.
//
// Nothing here allocates, copies or synchronises.
// C entries, with the limits they enforce, at the end of the file: goi_semantic_pca_* (declared in include/goi_raster.h).
#include <cfloat>

#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ACC_THREADS = 1024;
constexpr int ACC_WAVES = ACC_THREADS / 64;
constexpr int PCA_SLOTS = 256;      // the fixed grid of the accumulation: one fp64 slot per workgroup
constexpr int PIVOT_LANES = 32;
constexpr int PIVOT_THREADS = 32 * PIVOT_LANES;  // GOI_PCA_MAX_DIM channels
constexpr int PIVOT_SAMPLES = 2048;
constexpr int MAX_SWEEPS = 16;       // fp64 Jacobi at S <= 32 converges in 6 - 9; the bound is what ends a non-finite input
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_WAVES = APPLY_THREADS / 64;
constexpr int APPLY_MAX_BLOCKS = 2048;  // per launch, spread over the views

// fp64 words of one slot / of the total: count, SP channel sums, then the 16 x 16 blocks [row][col] (00; 01; 11)
__host__ __device__ constexpr int slot_words(int S) { return S <= 16 ? 1 + 16 + 256 : 1 + 32 + 3 * 256; }
constexpr size_t WS_PIVOT_BYTES = 128;                                   // float [32]
constexpr size_t WS_TOTAL_BYTES = 6528;                                  // double [<= 801], padded
constexpr size_t WS_SLOTS_OFFSET = WS_PIVOT_BYTES + WS_TOTAL_BYTES;      // 6656 = 26 * 256

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---------------------------------------------------------------------------------------------------------- pivot
// x at sample i, channel c is x[i * ps + c * cs] (planar: ps = 1, cs = n; rows: ps = S, cs = 1).  The pivot's samples are
// K = min(n, PIVOT_SAMPLES) samples in chunks of 32 consecutive ones, the chunks spread evenly over the WHOLE set, not
// its first K: the first rows of a rendered map are mostly empty background, which a mask on alpha excludes, and a pivot
// taken there would leave the masked fit with the raw moments.  Thread (c, j) sums sample j of every chunk of channel c:
// the 32 lanes of a channel read 128 contiguous bytes of a planar map per load, and a lane's <= 64 loads depend neither
// on each other nor on the mask (the value is loaded first and selected afterwards).  Single samples at a stride of
// n / K were measured first: 71 us at 1600 x 1056 x 16, every lane of every load in another page.
__global__ void __launch_bounds__(PIVOT_THREADS) pca_pivot_k(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                            long long n, long long ps, long long cs, int S,
                                                            float* __restrict__ pivot) {
    __shared__ float part[32][PIVOT_LANES + 1];
    __shared__ int used_total;
    const int t = threadIdx.x;
    const int c = t / PIVOT_LANES, j = t % PIVOT_LANES;
    const int K = (int)(n < PIVOT_SAMPLES ? n : PIVOT_SAMPLES);
    // sample k = 32 q + r is element r of chunk q; the chunks start n / ceil(K / 32) apart (>= 32 when n >= PIVOT_SAMPLES, so
    // the last sample is below n; a smaller set is taken whole, k = i)
    const long long cstride = n >= PIVOT_SAMPLES ? n / (PIVOT_SAMPLES / PIVOT_LANES) : PIVOT_LANES;
    if (t == 0) used_total = 0;
    __syncthreads();
    if (mask && c == 0) {
        int used = 0;
#pragma unroll 8
        for (int k = j; k < K; k += PIVOT_LANES) used += mask[(k / PIVOT_LANES) * cstride + j] != 0;
        if (used) atomicAdd(&used_total, used);
    }
    __syncthreads();
    const bool by_mask = mask != nullptr && used_total > 0;
    const int count = by_mask ? used_total : K;
    float s = 0.0f;
    if (c < S) {
        const float* xc = x + (long long)c * cs;
#pragma unroll 8
        for (int k = j; k < K; k += PIVOT_LANES) {
            const long long i = (k / PIVOT_LANES) * cstride + j;
            const float v = xc[i * ps];
            const bool use = !by_mask || mask[i];
            s += use ? v : 0.0f;  // selected, not multiplied: an unused sample may hold anything
        }
    }
    part[c][j] = s;
    __syncthreads();
    if (t < 32) {
        float r = 0.0f;
        if (t < S) {
            for (int l = 0; l < PIVOT_LANES; ++l) r += part[t][l];
            r = r / (float)count;
            if (!(fabsf(r) <= FLT_MAX)) r = 0.0f;
        }
        pivot[t] = r;
    }
}

// ----------------------------------------------------------------------------------------------------- accumulate
struct AccParams {
    const float* x;
    const uint8_t* mask;
    const float* pivot;
    double* slots;
    long long n, ps, cs;
    int S, first, vec;
};

template <int NB>
__global__ void __launch_bounds__(ACC_THREADS) pca_accumulate_k(const AccParams p) {
    constexpr int NBLK = NB == 1 ? 1 : 3;
    constexpr int SP = 16 * NB;
    constexpr int WORDS = SP + NBLK * 256;  // without the count
    constexpr int ACC_UNROLL = NB == 1 ? 4 : 2;  // groups of 16 samples a wave has in flight (register budget: 128)
    __shared__ float part[ACC_WAVES][WORDS];
    __shared__ int pcnt[ACC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const long long n = p.n;
    float piv[NB];
    bool chan[NB];
    long long coff[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int ch = c + 16 * b;
        chan[b] = ch < p.S;
        piv[b] = chan[b] ? p.pivot[ch] : 0.0f;
        coff[b] = (long long)ch * p.cs;
    }
    f32x4 acc[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) acc[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) sum[b] = 0.0f;
    int cnt = 0;

    // A group is 16 samples = 4 MFMA tiles of 4.  On the vector path tile j is samples {p0 + 4 g' + j}, on the scalar one
    // {p0 + 4 j + g'}: any partition of the group into tiles gives the same sums up to the order of the additions.
    const long long ngroups = (n + 15) >> 4;
    const long long nwaves = (long long)gridDim.x * ACC_WAVES;
    const long long w0 = (long long)wave * gridDim.x + blockIdx.x;
    for (long long g0 = w0; g0 < ngroups; g0 += ACC_UNROLL * nwaves) {
        float v[ACC_UNROLL][NB][4];
        uint32_t use[ACC_UNROLL];
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u) {
            const long long grp = g0 + u * nwaves;
            const long long p0 = grp << 4;
            use[u] = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][b][j] = 0.0f;
            if (grp >= ngroups) continue;
            if (p.vec && p0 + 16 <= n) {
                const long long i = p0 + 4 * g;
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (chan[b]) {
                        const float4 t = *reinterpret_cast<const float4*>(p.x + coff[b] + i);
                        v[u][b][0] = t.x;
                        v[u][b][1] = t.y;
                        v[u][b][2] = t.z;
                        v[u][b][3] = t.w;
                    }
                if (p.mask) {
                    const uint32_t m = *reinterpret_cast<const uint32_t*>(p.mask + i);
                    use[u] = ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 2u : 0u) | ((m & 0xff0000u) ? 4u : 0u) |
                             ((m & 0xff000000u) ? 8u : 0u);
                } else {
                    use[u] = 15u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long long i = p0 + 4 * j + g;
                    if (i < n) {
#pragma unroll
                        for (int b = 0; b < NB; ++b)
                            if (chan[b]) v[u][b][j] = p.x[i * p.ps + coff[b]];
                        if (!p.mask || p.mask[i]) use[u] |= 1u << j;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool used = (use[u] >> j) & 1u;
                float d[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    d[b] = (used && chan[b]) ? v[u][b][j] - piv[b] : 0.0f;
                    sum[b] += d[b];
                }
                cnt += used ? 1 : 0;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[0], d[0], acc[0], 0, 0, 0);
                if constexpr (NB == 2) {
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[0], d[1], acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[1], d[1], acc[2], 0, 0, 0);
                }
            }
    }

    // the four sample groups g of a channel, and of the count (every channel lane of a group counted the same samples)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float s = sum[b];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (g == 0) part[wave][16 * b + c] = s;
    }
    cnt += __shfl_xor(cnt, 16);
    cnt += __shfl_xor(cnt, 32);
    if (lane == 0) pcnt[wave] = cnt;
    // C/D map of the 16x16 MFMA: register r of lane l is row 4 (l >> 4) + r, column l & 15
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][SP + b * 256 + (4 * g + r) * 16 + c] = acc[b][r];
    __syncthreads();
    double* slot = p.slots + (size_t)blockIdx.x * (1 + WORDS);
    for (int e = threadIdx.x; e < WORDS; e += ACC_THREADS) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < ACC_WAVES; ++w) t += (double)part[w][e];
        slot[1 + e] = p.first ? t : slot[1 + e] + t;
    }
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < ACC_WAVES; ++w) t += pcnt[w];
        slot[0] = p.first ? (double)t : slot[0] + (double)t;
    }
}

// --------------------------------------------------------------------------------------------------------- reduce
// 16 words per workgroup; thread (word, part) adds 16 consecutive slots in order, then the 16 parts are added in order.
__global__ void __launch_bounds__(256) pca_reduce_k(const double* __restrict__ slots, int words, double* __restrict__ total) {
    __shared__ double part[16][17];
    const int e = threadIdx.x & 15, sg = threadIdx.x >> 4;
    const int word = blockIdx.x * 16 + e;
    double t = 0.0;
    if (word < words) {
        const double* src = slots + (size_t)(sg * (PCA_SLOTS / 16)) * words + word;
#pragma unroll
        for (int i = 0; i < PCA_SLOTS / 16; ++i) t += src[(size_t)i * words];
    }
    part[sg][e] = t;
    __syncthreads();
    if (sg == 0 && word < words) {
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += part[i][e];
        total[word] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------- solve
__device__ __forceinline__ double gram_word(const double* tot, int S, int i, int j) {
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    if (S <= 16) return tot[1 + 16 + i * 16 + j];
    const int blk = (i >> 4) + (j >> 4);  // 00 -> 0, 01 -> 1, 11 -> 2 (i <= j)
    return tot[1 + 32 + blk * 256 + (i & 15) * 16 + (j & 15)];
}

// The round-robin pairing of SE (even) indices, step r of SE - 1: index SE - 1 stays, the others rotate.
__device__ __forceinline__ void rr_pair(int SE, int r, int m, int& p, int& q) {
    const int M = SE - 1;
    int a, b;
    if (m == 0) {
        a = M;
        b = r;
    } else {
        a = (r + m) % M;
        b = (r - m + M) % M;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__global__ void __launch_bounds__(64) pca_solve_k(const float* __restrict__ pivot, const double* __restrict__ tot, int S,
                                                  float* __restrict__ basis) {
    __shared__ double A[32][33], V[32][33];
    __shared__ double md[32], rc[16], rs[16], red_off[32], red_diag[32];
    __shared__ int pick[3];
    __shared__ double pick_sign[3];
    const int t = threadIdx.x;
    const double N = tot[0];
    const int nb = 4 * S + 5;
    if (!(N >= 2.0)) {  // fewer than two samples: a mean at most, no direction
        for (int i = t; i < nb; i += 64) {
            float v = 0.0f;
            if (i < S && N == 1.0) v = (float)((double)pivot[i] + tot[1 + i]);
            if (i == nb - 1) v = (float)N;
            basis[i] = v;
        }
        return;
    }
    const int SE = (S + 1) & ~1;
    const int H = SE >> 1;
    if (t < S) md[t] = tot[1 + t] / N;
    __syncthreads();
    for (int idx = t; idx < SE * SE; idx += 64) {
        const int i = idx / SE, j = idx % SE;
        double a = 0.0;
        if (i < S && j < S) a = (gram_word(tot, S, i, j) - N * md[i] * md[j]) / (N - 1.0);
        A[i][j] = a;
        V[i][j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    double trace = 0.0;
    for (int i = 0; i < S; ++i) trace += A[i][i];

    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        if (t < SE) {
            double off = 0.0;
            for (int j = 0; j < SE; ++j)
                if (j != t) off += A[t][j] * A[t][j];
            red_off[t] = off;
            red_diag[t] = A[t][t] * A[t][t];
        }
        __syncthreads();
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < SE; ++i) {
            off += red_off[i];
            diag += red_diag[i];
        }
        __syncthreads();
        if (!(off > 1e-30 * diag)) break;  // converged, all zero, or not finite: the same for every lane
        for (int r = 0; r < SE - 1; ++r) {
            if (t < H) {
                int p, q;
                rr_pair(SE, r, t, p, q);
                const double apq = A[p][q];
                double cc = 1.0, ss = 0.0;
                if (apq != 0.0) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    cc = 1.0 / sqrt(tt * tt + 1.0);
                    ss = tt * cc;
                }
                rc[t] = cc;
                rs[t] = ss;
            }
            __syncthreads();
            for (int w = t; w < SE * H; w += 64) {  // A <- A J, V <- V J: columns p and q of every row
                const int k = w / H, m = w % H;
                int p, q;
                rr_pair(SE, r, m, p, q);
                const double cc = rc[m], ss = rs[m];
                const double ap = A[k][p], aq = A[k][q];
                A[k][p] = cc * ap - ss * aq;
                A[k][q] = ss * ap + cc * aq;
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = cc * vp - ss * vq;
                V[k][q] = ss * vp + cc * vq;
            }
            __syncthreads();
            for (int w = t; w < SE * H; w += 64) {  // A <- J^T A: rows p and q of every column
                const int k = w / H, m = w % H;
                int p, q;
                rr_pair(SE, r, m, p, q);
                const double cc = rc[m], ss = rs[m];
                const double ap = A[p][k], aq = A[q][k];
                A[p][k] = cc * ap - ss * aq;
                A[q][k] = ss * ap + cc * aq;
            }
            __syncthreads();
        }
    }

    if (t == 0) {
        uint32_t taken = 0;
        for (int k = 0; k < 3; ++k) {
            int best = -1;
            for (int i = 0; i < S; ++i)
                if (!((taken >> i) & 1u) && (best < 0 || A[i][i] > A[best][best])) best = i;
            taken |= 1u << best;
            pick[k] = best;
            int arg = 0;
            for (int i = 1; i < S; ++i)
                if (fabs(V[i][best]) > fabs(V[arg][best])) arg = i;
            pick_sign[k] = V[arg][best] < 0.0 ? -1.0 : 1.0;
        }
    }
    __syncthreads();
    if (t < S) {
        basis[t] = (float)((double)pivot[t] + md[t]);
        for (int k = 0; k < 3; ++k) basis[S + k * S + t] = (float)(pick_sign[k] * V[t][pick[k]]);
    }
    if (t < 3) {
        const double ev = A[pick[t]][pick[t]];
        basis[4 * S + t] = (float)(ev < 0.0 ? 0.0 : ev);
    }
    if (t == 0) {
        basis[4 * S + 3] = (float)trace;
        basis[4 * S + 4] = (float)N;
    }
}

// ---------------------------------------------------------------------------------------------------------- apply
// As in display.hip, the stats buffer holds the ordered key (ord_enc, wave_util.h) of the maximum and the COMPLEMENT of the key
// of the minimum, so both are atomicMax and the all-zero buffer is the identity.

struct ApplyParams {
    const float* x;      // [V][S][n] or [V][n][S]
    const float* basis;  // GOI_PCA_BASIS_FLOATS(S)
    float* out;          // [V][3][n] or [V][n][3]
    uint32_t* stats;     // [V][3][2]: ~key(min), key(max)
    long long n;
    int S, in_rows, out_rows, mode, vec;
    float two_k;
};

// q_k += (x - mean[c]) * component_k[c]: two roundings per channel and component, never contracted
__device__ __forceinline__ void project_step(const float* __restrict__ bs, int S, int c, float x, float q[3]) {
    const float d = x - bs[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = q[k] + d * bs[S + k * S + c];
}

struct Norm {
    float a[3], b[3];  // SIGMA: a = denominator; MINMAX: a = min, b = denominator
};

__device__ __forceinline__ float normalise(int mode, const Norm& nm, int k, float q) {
    if (mode == GOI_PCA_SIGMA) {
        float v = q / nm.a[k];
        v = 0.5f + v;
        return fminf(fmaxf(v, 0.0f), 1.0f);
    }
    if (mode == GOI_PCA_MINMAX) return (q - nm.a[k]) / nm.b[k];
    return q;
}

// PASS 0: the minima and maxima of q per view and component; PASS 1: write.  blockIdx.y = view.
template <int PASS>
__global__ void __launch_bounds__(APPLY_THREADS) pca_apply_k(const ApplyParams p) {
    __shared__ float bs[4 * 32 + 5];
    __shared__ float wpart[APPLY_WAVES][6];
    const int S = p.S;
    for (int i = threadIdx.x; i < 4 * S + 5; i += APPLY_THREADS) bs[i] = p.basis[i];
    __syncthreads();
    const int view = blockIdx.y;
    const long long n = p.n;
    const float* x = p.x + (size_t)view * S * n;
    float* out = p.out + (size_t)view * 3 * n;
    Norm nm;
#pragma unroll
    for (int k = 0; k < 3; ++k) nm.a[k] = nm.b[k] = 1.0f;
    if (PASS == 1 && p.mode == GOI_PCA_SIGMA) {
#pragma unroll
        for (int k = 0; k < 3; ++k) nm.a[k] = p.two_k * fmaxf(sqrtf(bs[4 * S + k]), FLT_MIN);
    }
    if (PASS == 1 && p.mode == GOI_PCA_MINMAX) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float mn = ord_dec(~p.stats[((size_t)view * 3 + k) * 2]);
            const float mx = ord_dec(p.stats[((size_t)view * 3 + k) * 2 + 1]);
            nm.a[k] = mn;
            nm.b[k] = (mx - mn) + 1e-20f;
        }
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const long long tid = (long long)blockIdx.x * APPLY_THREADS + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * APPLY_THREADS;

    if (p.vec) {  // planar in, n % 4 == 0, everything on 16-byte boundaries
        for (long long quad = tid; quad < (n >> 2); quad += nthreads) {
            float q[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j][0] = q[j][1] = q[j][2] = 0.0f;
#pragma unroll 4
            for (int c = 0; c < S; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(x + (size_t)c * n + 4 * quad);
                project_step(bs, S, c, v.x, q[0]);
                project_step(bs, S, c, v.y, q[1]);
                project_step(bs, S, c, v.z, q[2]);
                project_step(bs, S, c, v.w, q[3]);
            }
            if (PASS == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        lo[k] = fminf(lo[k], q[j][k]);
                        hi[k] = fmaxf(hi[k], q[j][k]);
                    }
            } else {
                float o[4][3];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < 3; ++k) o[j][k] = normalise(p.mode, nm, k, q[j][k]);
                if (p.out_rows) {
                    float4* dst = reinterpret_cast<float4*>(out + 12 * quad);
                    dst[0] = make_float4(o[0][0], o[0][1], o[0][2], o[1][0]);
                    dst[1] = make_float4(o[1][1], o[1][2], o[2][0], o[2][1]);
                    dst[2] = make_float4(o[2][2], o[3][0], o[3][1], o[3][2]);
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        *reinterpret_cast<float4*>(out + (size_t)k * n + 4 * quad) = make_float4(o[0][k], o[1][k], o[2][k], o[3][k]);
                }
            }
        }
    } else {
        const long long ps = p.in_rows ? S : 1, cs = p.in_rows ? 1 : n;
        for (long long i = tid; i < n; i += nthreads) {
            float q[3] = {0.0f, 0.0f, 0.0f};
            for (int c = 0; c < S; ++c) project_step(bs, S, c, x[i * ps + c * cs], q);
            if (PASS == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    lo[k] = fminf(lo[k], q[k]);
                    hi[k] = fmaxf(hi[k], q[k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float o = normalise(p.mode, nm, k, q[k]);
                    if (p.out_rows)
                        out[3 * i + k] = o;
                    else
                        out[(size_t)k * n + i] = o;
                }
            }
        }
    }

    if (PASS == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            for (int o = 32; o > 0; o >>= 1) {
                lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
                hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
            }
        }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                wpart[wave][2 * k] = lo[k];
                wpart[wave][2 * k + 1] = hi[k];
            }
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            const bool is_min = (threadIdx.x & 1) == 0;
            float v = wpart[0][threadIdx.x];
            for (int w = 1; w < APPLY_WAVES; ++w) v = is_min ? fminf(v, wpart[w][threadIdx.x]) : fmaxf(v, wpart[w][threadIdx.x]);
            // an infinity of the wrong sign means no finite-or-not value was seen at all: leave the identity
            if (is_min ? v != INFINITY : v != -INFINITY)
                atomicMax(p.stats + (size_t)view * 6 + threadIdx.x, is_min ? ~ord_enc(v) : ord_enc(v));
        }
    }
}

size_t pca_fit_workspace_bytes(int S) { return WS_SLOTS_OFFSET + sizeof(double) * (size_t)PCA_SLOTS * slot_words(S); }
size_t pca_stats_bytes(int n_views) { return sizeof(uint32_t) * 6 * (size_t)n_views; }

void launch_pca_accumulate(const float* x, int layout, int S, long long n, const uint8_t* mask, int first, void* workspace,
                           hipStream_t s) {
    char* ws = static_cast<char*>(workspace);
    float* pivot = reinterpret_cast<float*>(ws);
    const bool rows = layout == GOI_PCA_ROWS;
    const long long ps = rows ? S : 1, cs = rows ? 1 : n;
    if (first) pca_pivot_k<<<1, PIVOT_THREADS, 0, s>>>(x, mask, n, ps, cs, S, pivot);
    AccParams p;
    p.x = x;
    p.mask = mask;
    p.pivot = pivot;
    p.slots = reinterpret_cast<double*>(ws + WS_SLOTS_OFFSET);
    p.n = n;
    p.ps = ps;
    p.cs = cs;
    p.S = S;
    p.first = first;
    p.vec = (!rows && n % 4 == 0 && aligned(x, 16) && aligned(mask, 4)) ? 1 : 0;
    if (S <= 16)
        pca_accumulate_k<1><<<PCA_SLOTS, ACC_THREADS, 0, s>>>(p);
    else
        pca_accumulate_k<2><<<PCA_SLOTS, ACC_THREADS, 0, s>>>(p);
}

void launch_pca_solve(int S, void* workspace, float* basis, hipStream_t s) {
    char* ws = static_cast<char*>(workspace);
    double* total = reinterpret_cast<double*>(ws + WS_PIVOT_BYTES);
    const int words = slot_words(S);
    pca_reduce_k<<<(words + 15) / 16, 256, 0, s>>>(reinterpret_cast<const double*>(ws + WS_SLOTS_OFFSET), words, total);
    pca_solve_k<<<1, 64, 0, s>>>(reinterpret_cast<const float*>(ws), total, S, basis);
}

void launch_pca_apply(const float* x, int in_layout, int S, long long n, int n_views, const float* basis, int normalize,
                      float two_k, float* out, int out_layout, uint32_t* stats, hipStream_t s) {
    ApplyParams p;
    p.x = x;
    p.basis = basis;
    p.out = out;
    p.stats = stats;
    p.n = n;
    p.S = S;
    p.in_rows = in_layout == GOI_PCA_ROWS;
    p.out_rows = out_layout == GOI_PCA_ROWS;
    p.mode = normalize;
    p.two_k = two_k;
    p.vec = (!p.in_rows && n % 4 == 0 && aligned(x, 16) && aligned(out, 16)) ? 1 : 0;
    const long long units = p.vec ? n / 4 : n;
    const long long per_view = std::max<long long>(1, APPLY_MAX_BLOCKS / n_views);
    const long long blocks = (units + APPLY_THREADS - 1) / APPLY_THREADS;
    const dim3 grid((unsigned)std::min(std::max<long long>(blocks, 1), per_view), n_views);
    if (normalize == GOI_PCA_MINMAX) {
        (void)hipMemsetAsync(stats, 0, pca_stats_bytes(n_views), s);  // a failure surfaces in the caller's hipGetLastError
        pca_apply_k<0><<<grid, APPLY_THREADS, 0, s>>>(p);
    }
    pca_apply_k<1><<<grid, APPLY_THREADS, 0, s>>>(p);
}

int pca_dims(const char* fn, int S, long long n) {
    if (S < GOI_PCA_MIN_DIM || S > GOI_PCA_MAX_DIM) return fail(std::string(fn) + ": need 3 <= S <= 32");
    if (n < 1 || n >= (1ll << 31)) return fail(std::string(fn) + ": need 1 <= n < 2^31");
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_semantic_pca_workspace_bytes(int S, int n_views) {
    if (S < 0 || n_views < 0 || (S > 0 && (S < GOI_PCA_MIN_DIM || S > GOI_PCA_MAX_DIM)) || n_views > 65535) return 0;
    return (S > 0 ? pca_fit_workspace_bytes(S) : 0) + (n_views > 0 ? pca_stats_bytes(n_views) : 0);
}

int goi_semantic_pca_accumulate(const float* x, int layout, int S, long long n, const uint8_t* mask, int first, void* workspace,
                                void* stream) {
    const char* fn = "goi_semantic_pca_accumulate";
    if (pca_dims(fn, S, n) < 0) return -1;
    if (layout != GOI_PCA_PLANAR && layout != GOI_PCA_ROWS) return fail(std::string(fn) + ": layout must be GOI_PCA_PLANAR or GOI_PCA_ROWS");
    if (!x) return fail(std::string(fn) + ": NULL x");
    if (check_workspace(fn, workspace) < 0) return -1;
    if (reinterpret_cast<uintptr_t>(x) & 3) return fail(std::string(fn) + ": x must be 4-byte aligned");
    launch_pca_accumulate(x, layout, S, n, mask, first ? 1 : 0, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_pca_solve(int S, void* workspace, float* basis, void* stream) {
    const char* fn = "goi_semantic_pca_solve";
    if (pca_dims(fn, S, 1) < 0) return -1;
    if (!basis) return fail(std::string(fn) + ": NULL basis");
    if (check_workspace(fn, workspace) < 0) return -1;
    launch_pca_solve(S, workspace, basis, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_pca_apply(const float* x, int in_layout, int S, long long n, int n_views, const float* basis, int normalize,
                           double k_sigma, float* out, int out_layout, void* workspace, void* stream) {
    const char* fn = "goi_semantic_pca_apply";
    if (pca_dims(fn, S, n) < 0) return -1;
    if ((in_layout != GOI_PCA_PLANAR && in_layout != GOI_PCA_ROWS) || (out_layout != GOI_PCA_PLANAR && out_layout != GOI_PCA_ROWS))
        return fail(std::string(fn) + ": layouts must be GOI_PCA_PLANAR or GOI_PCA_ROWS");
    if (normalize != GOI_PCA_RAW && normalize != GOI_PCA_SIGMA && normalize != GOI_PCA_MINMAX)
        return fail(std::string(fn) + ": normalize must be GOI_PCA_RAW, GOI_PCA_SIGMA or GOI_PCA_MINMAX");
    if (n_views < 0 || n_views > 65535) return fail(std::string(fn) + ": need 0 <= n_views <= 65535");
    if (n_views == 0) return 0;
    if (!x || !basis || !out) return fail(std::string(fn) + ": NULL x, basis or out");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(basis)) & 3)
        return fail(std::string(fn) + ": x, basis and out must be 4-byte aligned");
    if (normalize == GOI_PCA_MINMAX && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3)))
        return fail(std::string(fn) + ": GOI_PCA_MINMAX needs a 4-byte aligned workspace");
    if (normalize == GOI_PCA_SIGMA && !(k_sigma > 0.0 && k_sigma <= 3.0e38)) return fail(std::string(fn) + ": need a finite k_sigma > 0");
    const float kf = (float)k_sigma;
    launch_pca_apply(x, in_layout, S, n, n_views, basis, normalize, 2.0f * kf, out, out_layout, static_cast<uint32_t*>(workspace),
                     static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
