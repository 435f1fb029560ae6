// The optimisable semantic-space hyperplane (OSH) fine-tune of the reference (gui/main.py:1673-1763,
// finetune_prompt_with_res): a LinearSVM (networks.py:12-59) trained with hinge loss and plain SGD against a binary
// mask until the IoU reaches a target or max_epochs have run.
//
// Every pixel's feature is one of n_codes normalised code-book rows, so the loss, its gradient and the IoU over HW
// pixels are exact functions of two histograms: P[c] (mask-positive pixels decoded to code c) and N[c] (negative
// ones).  osh_counts_k builds them (one pass over idx + mask, 5 B per pixel); osh_fit_k then runs the whole fit --
// every epoch, with its stop test -- inside ONE workgroup per hyperplane, with no host round trip.
//
// osh_fit_k layout (1024 threads = 16 waves):
//   * the codes present in the frame (P + N > 0) are compacted in code order; present code m belongs to wave
//     m % 16 (its i-th code is m = 16 i + wave);
//   * a lane owns the feature slice d = V lane .. V lane + V - 1 (V = ceil(D / 64));
//   * z_m = (LUT[c] / |LUT[c]|) / 0.3438 (two fp32 divisions, as the reference does per pixel).  Register path
//     (D = 256, n_codes <= 320): z lives in VGPRs, 20 codes x 4 floats per lane; generic path (D <= 1024,
//     n_codes <= 1000): z is re-formed from the LUT (L2-resident) every epoch with the same two divisions.
// One epoch is one pass over the wave's codes: margin (lane-slice partial dot, DPP + readlane wave sum), IoU counts,
// hinge loss and coefficient a_m, gradient slice += a_m z_m; then one cross-wave reduction of the gradient through
// LDS (16 x D floats, summed in wave order by the thread owning d) and the SGD step.  The margins of the NEW w are
// the next epoch's margins, so each epoch is one pass and two barriers.  Every reduction has a fixed order: runs are
// bit-reproducible, and the two paths agree bit for bit where both apply.
// C entries, with the limits they enforce, at the end of the file: goi_semantic_osh_counts / _fit (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"

namespace goi {

namespace {

constexpr int OSH_THREADS = 1024;
constexpr int OSH_WAVES = OSH_THREADS / 64;
constexpr int OSH_MAX_CODES = 1000;
constexpr int OSH_REG_D = 256;
constexpr int OSH_REG_CPW = 20;  // codes per wave on the register path: 16 x 20 = 320 codes
constexpr int OSH_GEN_DMAX = 1024;
constexpr float OSH_SCALE = 0.3438f;  // networks.py: forward(x) = linear(x / 0.3438)

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the 64 lanes, returned wave-uniform.  Each step adds a lane's value to its partner's; the two partners add
// the same two numbers (commutative), so every lane holds the same bits at every step.
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
    v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
    v += dpp<0x141>(v);  // row_half_mirror: the other quad of the 8
    v += dpp<0x140>(v);  // row_mirror: the other 8 of the row
    v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));  // bitmask swizzle: lane ^ 16
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
}

// Wave-uniform values formed from LDS reads would otherwise occupy VGPRs across the whole epoch loop.
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double uniform(double v) {
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)(x & 0xffffffffll));
    const int hi = __builtin_amdgcn_readfirstlane((int)(x >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

struct OshShared {
    int code[OSH_MAX_CODES];  // present codes, ascending
    int P[OSH_MAX_CODES];
    int N[OSH_MAX_CODES];
    float norm[OSH_MAX_CODES];  // generic path: |LUT[code[m]]|
    float loss[OSH_WAVES];
    float asum[OSH_WAVES];
    long long I[OSH_WAVES], UN[OSH_WAVES], Pall[OSH_WAVES];
    int wcount[OSH_WAVES];
    int M;
    int err;
};

// Per-wave results of one pass over the wave's codes with weights w (LDS) and bias b.  A wave's pixel counts stay
// below HW < 2^31: 32-bit sums per wave, 64-bit across waves.
struct PassAcc {
    float loss = 0.f;
    float asum = 0.f;
    int I = 0, UN = 0;
};

// The per-code part of an epoch, shared by both paths: margin o -> IoU counts, hinge loss, coefficient.
__device__ __forceinline__ float code_step(float o, int P, int N, float inv_hw, PassAcc& acc) {
    P = __builtin_amdgcn_readfirstlane(P);  // (wave-uniform: keeps the per-code scalars out of the VGPR budget)
    N = __builtin_amdgcn_readfirstlane(N);
    if (o > 0.f) {
        acc.I += P;
        acc.UN += N;
    }
    const float hp = 1.f - o;  // positive pixels: 1 - o * (+1)
    const float hn = 1.f + o;  // negative pixels: 1 - o * (-1)
    {
        // no contraction here: otherwise each instantiation may fuse a different product into an FMA, and the two paths'
        // losses would differ in the last bit
#pragma clang fp contract(off)
        acc.loss = acc.loss + ((float)P * fmaxf(hp, 0.f) + (float)N * fmaxf(hn, 0.f));
    }
    // clamp(min=0) passes the gradient where its input is >= 0 (torch's backward of clamp includes the kink); every
    // pixel of the code adds the same +-1/HW, so a = (signed pixel count) / HW
    const int cnt = (hn >= 0.f ? N : 0) - (hp >= 0.f ? P : 0);
    const float a = (float)cnt * inv_hw;
    acc.asum += a;
    return a;
}

template <bool REG>
__global__ __launch_bounds__(OSH_THREADS) void osh_fit_k(const float* __restrict__ lut, int n_codes, int D,
                                                         const int* __restrict__ counts, long long HW, float* __restrict__ w_io,
                                                         float* __restrict__ b_io, float lr, int max_epochs, double target_iou,
                                                         int* __restrict__ epochs_out, float* __restrict__ loss_out,
                                                         double* __restrict__ iou_out, double* __restrict__ init_iou_out,
                                                         double* __restrict__ trace) {
    constexpr int DMAX = REG ? OSH_REG_D : OSH_GEN_DMAX;
    constexpr int VMAX = DMAX / 64;
    __shared__ OshShared sh;
    __shared__ __attribute__((aligned(16))) float s_w[DMAX];
    __shared__ __attribute__((aligned(16))) float s_red[OSH_WAVES][DMAX];

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int k = blockIdx.x;
    const int V = REG ? 4 : (D + 63) / 64;
    const int* cP = counts + (size_t)k * 2 * n_codes;
    const int* cN = cP + n_codes;
    const float inv_hw = 1.0f / (float)HW;  // the per-pixel gradient of mean(): 1/HW in fp32

    // ---- prologue: compact the present codes (ballot + wave counts), load w
    int p = 0, n = 0;
    bool present = false;
    if (t < n_codes) {
        p = cP[t];
        n = cN[t];
        present = p + n > 0;
    }
    const unsigned long long ball = __ballot(present);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(ball >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ball, 0));
    if (lane == 0) sh.wcount[wave] = __popcll(ball);
    if (t == 0) sh.err = 0;
    for (int d = t; d < DMAX; d += OSH_THREADS) s_w[d] = d < D ? w_io[(size_t)k * D + d] : 0.f;
    __syncthreads();
    int off = 0, M = 0;
    for (int i = 0; i < OSH_WAVES; i++) {
        off += i < wave ? sh.wcount[i] : 0;
        M += sh.wcount[i];
    }
    if (present) {
        sh.code[off + rank] = t;
        sh.P[off + rank] = p;
        sh.N[off + rank] = n;
    }
    __syncthreads();
    M = __builtin_amdgcn_readfirstlane(M);
    const int n_mine = M > wave ? (M - wave + OSH_WAVES - 1) / OSH_WAVES : 0;  // codes of this wave (scalar branches)

    // ---- code norms, z (register path), the wave's share of sum_c P_c
    // |LUT[c]| of present code m (wave-uniform) from the lane slices of its row, l = the lane's slice
    auto row_norm = [&](int m, float* l) -> float {
        const float* row = lut + (size_t)sh.code[m] * D;
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < VMAX; j++) {
            const int d = lane * V + j;
            l[j] = (j < V && d < D) ? row[d] : 0.f;
            part = fmaf(l[j], l[j], part);
        }
        const float nrm = sqrtf(wave_sum(part));
        if (nrm == 0.f && lane == 0) sh.err = 1;
        return nrm;
    };
    float z[REG ? OSH_REG_CPW : 1][4];
    long long pw = 0;
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < OSH_REG_CPW; i++) {
            float l[4] = {0.f, 0.f, 0.f, 0.f};
            float nrm = 1.f;
            if (i < n_mine) {
                pw += sh.P[i * OSH_WAVES + wave];
                nrm = row_norm(i * OSH_WAVES + wave, l);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) z[i][j] = (l[j] / nrm) / OSH_SCALE;
        }
    } else {
        for (int i = 0; i < n_mine; i++) {
            const int m = i * OSH_WAVES + wave;
            float l[VMAX];
            pw += sh.P[m];
            const float nrm = row_norm(m, l);
            if (lane == 0) sh.norm[m] = nrm;
        }
    }
    if (lane == 0) sh.Pall[wave] = pw;
    __syncthreads();
    if (sh.err) {
        if (t == 0) {
            epochs_out[k] = -1;  // a present code with a zero LUT row: the reference's fit would be NaN throughout
            loss_out[k] = __int_as_float(0x7fc00000);
            iou_out[k] = __longlong_as_double(0x7ff8000000000000ll);
            init_iou_out[k] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }

    float b = uniform(b_io[k]);
    // one pass with the weights in s_w and bias b: writes the wave's gradient slice and scalars to LDS
    auto pass = [&]() {
        float wl[VMAX], g[VMAX];
#pragma unroll
        for (int j = 0; j < VMAX; j++) {
            wl[j] = (j < V) ? s_w[min(lane * V + j, DMAX - 1)] : 0.f;
            g[j] = 0.f;
        }
        PassAcc acc;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < OSH_REG_CPW; i++) {
                if (i < n_mine) {
                    const int m = i * OSH_WAVES + wave;
                    float part = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; j++) part = fmaf(wl[j], z[i][j], part);
                    const float a = code_step(wave_sum(part) + b, sh.P[m], sh.N[m], inv_hw, acc);
#pragma unroll
                    for (int j = 0; j < 4; j++) g[j] = fmaf(a, z[i][j], g[j]);
                }
            }
        } else {
            for (int i = 0; i < n_mine; i++) {
                const int m = i * OSH_WAVES + wave;
                const float* row = lut + (size_t)sh.code[m] * D;
                const float nrm = sh.norm[m];
                // z is formed twice (same bits both times) rather than held: the generic path keeps its registers for w, g
                float part = 0.f;
#pragma unroll
                for (int j = 0; j < VMAX; j++) {
                    const int d = lane * V + j;
                    part = fmaf(wl[j], (j < V && d < D) ? (row[d] / nrm) / OSH_SCALE : 0.f, part);
                }
                const float a = code_step(wave_sum(part) + b, sh.P[m], sh.N[m], inv_hw, acc);
#pragma unroll
                for (int j = 0; j < VMAX; j++) {
                    const int d = lane * V + j;
                    g[j] = fmaf(a, (j < V && d < D) ? (row[d] / nrm) / OSH_SCALE : 0.f, g[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VMAX; j++)
            if (j < V && lane * V + j < D) s_red[wave][lane * V + j] = g[j];
        if (lane == 0) {
            sh.loss[wave] = acc.loss;
            sh.asum[wave] = acc.asum;
            sh.I[wave] = acc.I;
            sh.UN[wave] = acc.UN;
        }
    };
    // the workgroup's sums of the pass scalars, in wave order (every thread computes the same values)
    auto iou_of_pass = [&]() -> double {
        long long I = 0, U = 0;
        for (int i = 0; i < OSH_WAVES; i++) {
            I += sh.I[i];
            U += sh.Pall[i] + sh.UN[i];
        }
        return uniform(U == 0 ? __longlong_as_double(0x7ff8000000000000ll) : (double)I / (double)U);
    };
    auto loss_of_pass = [&]() -> float {
        double s = 0.0;
        for (int i = 0; i < OSH_WAVES; i++) s += sh.loss[i];
        return uniform((float)(s / (double)HW));
    };

    pass();  // margins of the initial w: init IoU, epoch 0's loss and gradient
    __syncthreads();
    const double init_iou = iou_of_pass();
    float loss_cur = loss_of_pass();
    int ep = 0;
    double iou = 0.0;
    for (;;) {
        // SGD step: w -= lr * sum_m a_m z_m, b -= lr * sum_m a_m
        float asum = 0.f;
        for (int i = 0; i < OSH_WAVES; i++) asum += sh.asum[i];
        if (t < D) {
            float g = 0.f;
            for (int i = 0; i < OSH_WAVES; i++) g += s_red[i][t];
            s_w[t] = fmaf(-lr, g, s_w[t]);
        }
        b = uniform(fmaf(-lr, asum, b));
        __syncthreads();
        pass();  // margins of the new w: this epoch's IoU, the next epoch's loss and gradient
        __syncthreads();
        iou = iou_of_pass();
        if (trace && t == 0) {
            trace[((size_t)k * max_epochs + ep) * 2 + 0] = (double)loss_cur;
            trace[((size_t)k * max_epochs + ep) * 2 + 1] = iou;
        }
        ep++;
        if (ep == max_epochs || !(iou < target_iou)) break;  // (a NaN IoU stops, as in the reference's while test)
        loss_cur = loss_of_pass();
    }
    if (t < D) w_io[(size_t)k * D + t] = s_w[t];
    if (t == 0) {
        b_io[k] = b;
        epochs_out[k] = ep;
        loss_out[k] = loss_cur;
        iou_out[k] = iou;
        init_iou_out[k] = init_iou;
    }
}

constexpr int COUNTS_THREADS = 256;

// counts[0][c] += #{p : idx[p] = c, positive[p] != 0}, counts[1][c] += #{p : idx[p] = c, positive[p] == 0}.
// Workgroup-private LDS histogram, then one global atomic per non-zero bin (exact).  idx outside [0, n_codes) is skipped.
__global__ __launch_bounds__(COUNTS_THREADS) void osh_counts_k(const int* __restrict__ idx, const uint8_t* __restrict__ positive,
                                                              long long HW, int n_codes, int* __restrict__ counts) {
    __shared__ int h[2 * OSH_MAX_CODES];
    for (int i = threadIdx.x; i < 2 * n_codes; i += COUNTS_THREADS) h[i] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * COUNTS_THREADS;
    for (long long p = (long long)blockIdx.x * COUNTS_THREADS + threadIdx.x; p < HW; p += stride) {
        const int c = idx[p];
        if ((unsigned)c < (unsigned)n_codes) atomicAdd(&h[(positive[p] ? 0 : n_codes) + c], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * n_codes; i += COUNTS_THREADS)
        if (h[i]) atomicAdd(&counts[i], h[i]);
}

bool osh_register_path(int n_codes, int D) {
    return g_options.osh_path == 0 && D == OSH_REG_D && n_codes <= OSH_WAVES * OSH_REG_CPW;
}

void launch_osh_fit(const float* lut, int n_codes, int D, const int* counts, long long HW, int K, float* w, float* b,
                    float lr, int max_epochs, double target_iou, int* epochs_out, float* loss_out, double* iou_out,
                    double* init_iou_out, double* trace, hipStream_t s) {
    if (osh_register_path(n_codes, D))
        osh_fit_k<true><<<dim3(K), dim3(OSH_THREADS), 0, s>>>(lut, n_codes, D, counts, HW, w, b, lr, max_epochs, target_iou,
                                                             epochs_out, loss_out, iou_out, init_iou_out, trace);
    else
        osh_fit_k<false><<<dim3(K), dim3(OSH_THREADS), 0, s>>>(lut, n_codes, D, counts, HW, w, b, lr, max_epochs, target_iou,
                                                              epochs_out, loss_out, iou_out, init_iou_out, trace);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_semantic_osh_counts(const int* idx, const uint8_t* positive, long long HW, int n_codes, int* counts, void* stream) {
    if (HW < 0) return fail("goi_semantic_osh_counts: bad HW");
    if (n_codes < 1 || n_codes > OSH_MAX_CODES) return fail("goi_semantic_osh_counts: need 1 <= n_codes <= 1000");
    if (!counts) return fail("goi_semantic_osh_counts: counts is NULL");
    if (HW == 0) return 0;
    if (!idx || !positive) return fail("goi_semantic_osh_counts: NULL input");
    const long long per_block = (long long)COUNTS_THREADS * 8;
    const long long blocks = std::min<long long>((HW + per_block - 1) / per_block, 1024);
    osh_counts_k<<<dim3((unsigned)blocks), dim3(COUNTS_THREADS), 0, static_cast<hipStream_t>(stream)>>>(
        idx, positive, HW, n_codes, counts);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_osh_fit(const float* lut, int n_codes, int D, const int* counts, long long HW, int K, float* w, float* b,
                         float lr, int max_epochs, double target_iou, int* epochs_out, float* loss_out, double* iou_out,
                         double* init_iou_out, double* trace, void* stream) {
    refresh_options();
    if (n_codes < 1 || n_codes > OSH_MAX_CODES) return fail("goi_semantic_osh_fit: need 1 <= n_codes <= 1000");
    if (D < 1 || D > OSH_GEN_DMAX) return fail("goi_semantic_osh_fit: need 1 <= D <= 1024");
    if (HW < 1 || HW >= (1ll << 31)) return fail("goi_semantic_osh_fit: need 1 <= HW < 2^31");
    if (K < 0 || K > 65535) return fail("goi_semantic_osh_fit: need 0 <= K <= 65535");
    if (max_epochs < 1 || max_epochs > GOI_OSH_MAX_EPOCHS) return fail("goi_semantic_osh_fit: need 1 <= max_epochs <= 1000000");
    if (K == 0) return 0;
    if (!lut || !counts || !w || !b || !epochs_out || !loss_out || !iou_out || !init_iou_out)
        return fail("goi_semantic_osh_fit: a required pointer is NULL");
    launch_osh_fit(lut, n_codes, D, counts, HW, K, w, b, lr, max_epochs, target_iou, epochs_out, loss_out, iou_out,
                   init_iou_out, trace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
