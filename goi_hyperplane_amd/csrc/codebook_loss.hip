// Fused row pass of the semantic training losses for gfx950 (training half of SURVEY.md row a23 /
// 8(f) rank 2).
//
// Reference (train.py:142-163), per pixel p with rendered feature f [S], decoder (W [C,S], b [C]),
// code book LUT [C,D] and ground-truth feature g [D]:
//     P     = softmax(W f + b)                          sem_label
//     sim_c = <g/|g|, LUT_c/|LUT_c|>                    sim;  m = max_c sim_c;  label_c = (sim_c == m)
//     lab   = 50 * mean_{p,c} (P_c - label_c)^2
//     sl    = 1 - mean_p m
//     recc  = 1 - mean_p cos(LUT[argmax_c P_c], g)      (= sim at the decoder's argmax)
//     sl1   = mean_p H(softmax(t * sim)),  t = 1 (iteration < 1000) or 2
//     loss  = lab + sl + 0.3 sl1 + recc
// PyTorch runs this as two library GEMMs plus ~40 elementwise / reduction / gather / scatter kernels
// over [HW, C] tensors and keeps ~20 GB of autograd state at 1600x1056 (109 ms per iteration on
// MI355X, tools/loss_time.py).  Here the two dense contractions stay library GEMMs on the matrix
// cores (sim_raw = g^T L1^T going in, dL1 = dsim^T g coming out; hipBLASLt through torch.matmul, on
// TRANSPOSED VIEWS of the [D,H,W] map so that no permuted copy is made) and everything between them is
// this ONE kernel: it reads a row of sim once, and writes the row of dL/dsim, the pixel's dL/df and
// -- accumulated in registers across all rows a wave visits -- dL/dW, dL/db and the four loss terms.
//
// Mapping: one wave per pixel row; lane l owns codes l, l+64, ... (CPL per lane).  The decoder
// weights of a lane's codes live in its registers for the whole kernel (CPL*S VGPRs) and so do its
// dW accumulators: the [C,S] weight gradient needs no cross-lane traffic until the final write.
// The pixel's feature is wave-uniform (SGPRs, read with v_readlane from a 64-pixel register tile).
// Row statistics are DPP wave reductions whose results are wave-uniform.  All sums have a fixed
// order: the losses and gradients are bit-reproducible.
// C entries, with the limits they enforce, at the end of the file: goi_codebook_loss_* / _sim* / _dlut* / _fused* (declared in include/goi_raster.h).
#include <float.h>

#include "blend_common.h"
#include "entry.h"

namespace goi {

namespace {

constexpr int CBL_THREADS = 256;

#define GOI_DPP(v, ctrl, rmask, oldv) \
    __builtin_amdgcn_update_dpp((oldv), (v), (ctrl), (rmask), 0xF, false)

__device__ __forceinline__ float wave_sum_u(float v) {  // total in every ... lane 63; returned uniform
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0xB1, 0xF, 0));
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0x4E, 0xF, 0));
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0x141, 0xF, 0));
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0x140, 0xF, 0));
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0x142, 0xA, 0));  // row_bcast:15 into rows 1, 3
    v += __int_as_float(GOI_DPP(__float_as_int(v), 0x143, 0xC, 0));  // row_bcast:31 into rows 2, 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max_u(float v) {
    const int ninf = __float_as_int(-__builtin_inff());
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0xB1, 0xF, ninf)));
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0x4E, 0xF, ninf)));
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0x141, 0xF, ninf)));
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0x140, 0xF, ninf)));
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0x142, 0xA, ninf)));
    v = fmaxf(v, __int_as_float(GOI_DPP(__float_as_int(v), 0x143, 0xC, ninf)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_min_u(int v) {
    v = min(v, GOI_DPP(v, 0xB1, 0xF, 0x7FFFFFFF));
    v = min(v, GOI_DPP(v, 0x4E, 0xF, 0x7FFFFFFF));
    v = min(v, GOI_DPP(v, 0x141, 0xF, 0x7FFFFFFF));
    v = min(v, GOI_DPP(v, 0x140, 0xF, 0x7FFFFFFF));
    v = min(v, GOI_DPP(v, 0x142, 0xA, 0x7FFFFFFF));
    v = min(v, GOI_DPP(v, 0x143, 0xC, 0x7FFFFFFF));
    return __builtin_amdgcn_readlane(v, 63);
}

struct CblArgs {
    const float* sim;        // [HW][C]   raw <g, L1_c> (g not normalised)
    const float* inv_gnorm;  // [HW]      1 / |g_p|
    const float* sem;        // [S][HW]   rendered feature, channel-major (the rasterizer's output)
    const float* W;          // [C][S]
    const float* bias;       // [C] or NULL
    float* dsim;             // [HW][C]   dL/dsim_raw (already divided by |g_p|)
    float* dsem;             // [S][HW]
    float* partials;         // [n_waves][C*(S+1) + 4]: dW rows (S values + db), then lab, m, H, sim_a sums
    long long HW;
    int C, S;
    float t;        // anneal factor (1 or 2)
    float kappa;    // 2 * 50 / (HW * C)
    float inv_hw;   // 1 / HW
    float w_sl1;    // 0.3
};

template <int CPL, int SP>
__global__ __launch_bounds__(CBL_THREADS, (CPL <= 5 ? 2 : 1)) void codebook_rows_k(const CblArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (CBL_THREADS / 64) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (CBL_THREADS / 64);
    const int C = a.C, S = a.S;
    const long long HW = a.HW;

    // lane-stationary decoder rows and their gradient accumulators.  Only the LAST code slot of a lane can
    // fall beyond C (cpl = ceil(C / 64)); it is handled with selects, not branches: a padding code has
    // z = sim = -inf, hence P = q = 0 and no gradient.
    constexpr int KL = CPL - 1;
    const bool vlast = lane + 64 * KL < C;
    const int c_last = min(lane + 64 * KL, C - 1);  // clamped: always a readable address
    float Wr[CPL][SP], dWr[CPL][SP], br[CPL], dbr[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int c = k < KL ? lane + 64 * k : c_last;
        const bool ok = k < KL || vlast;
        br[k] = (ok && a.bias) ? a.bias[c] : 0.f;
        dbr[k] = 0.f;
#pragma unroll
        for (int s = 0; s < SP; s++) {
            Wr[k][s] = (ok && s < S) ? a.W[(size_t)c * S + s] : 0.f;
            dWr[k][s] = 0.f;
        }
    }
    float acc_lab = 0.f, acc_m = 0.f, acc_H = 0.f, acc_sa = 0.f;  // wave-uniform running loss sums
    const float NEG_INF = -__builtin_inff();
    const float g_ent = a.w_sl1 * a.t * a.inv_hw;

    const long long n_chunks = (HW + 63) / 64;
    for (long long ch = wave; ch < n_chunks; ch += n_waves) {
        const long long p0 = ch * 64;
        // 64-pixel register tile of the feature map and of 1/|g|: lane l holds pixel p0 + l
        const long long pl = min(p0 + lane, HW - 1);
        float fv[SP];
#pragma unroll
        for (int s = 0; s < SP; s++) fv[s] = a.sem[(size_t)min(s, S - 1) * HW + pl];
        const float invv = a.inv_gnorm[pl];
        const int rows = (int)min((long long)64, HW - p0);
        float x[CPL];
        const float* srow = a.sim + (size_t)p0 * C;  // wave-uniform row pointers
        float* drow = a.dsim + (size_t)p0 * C;
#pragma unroll
        for (int k = 0; k < CPL; k++) x[k] = srow[k < KL ? lane + 64 * k : c_last];
        for (int i = 0; i < rows; i++, drow += C) {
            const long long p = p0 + i;
            const float inv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invv), i));
            float xs[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) xs[k] = x[k] * inv;
            xs[KL] = vlast ? xs[KL] : NEG_INF;
            {  // prefetch the next row while this one is processed (the last row re-reads itself)
                if (p + 1 < HW) srow += C;
#pragma unroll
                for (int k = 0; k < CPL; k++) x[k] = srow[k < KL ? lane + 64 * k : c_last];
            }
            // ---- decoder logits of this lane's codes (the feature is wave-uniform)
            float fs[SP];
#pragma unroll
            for (int s = 0; s < SP; s++) fs[s] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fv[s]), i));
            float z[CPL];
            float zmax = NEG_INF, smax = NEG_INF;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                float acc = br[k];
#pragma unroll
                for (int s = 0; s < SP; s++) acc = fmaf(Wr[k][s], fs[s], acc);
                z[k] = acc;
            }
            z[KL] = vlast ? z[KL] : NEG_INF;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                zmax = fmaxf(zmax, z[k]);
                smax = fmaxf(smax, xs[k]);
            }
            const float mz = wave_max_u(zmax);
            const float ms = wave_max_u(smax);
            // ---- softmax of the logits, first arg-maxima, softmax of t * sim
            float P[CPL], q[CPL], lx[CPL];
            float sZp = 0.f, sZq = 0.f, sAq = 0.f, sNl = 0.f;
            int ia = 0x7FFFFFFF, is = 0x7FFFFFFF;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int c = lane + 64 * k;
                P[k] = __expf(z[k] - mz);  // exp(-inf) = 0 for padding
                sZp += P[k];
                lx[k] = a.t * (xs[k] - ms);  // <= 0
                q[k] = __expf(lx[k]);
                sZq += q[k];
                lx[k] = fmaxf(lx[k], -FLT_MAX);  // keep 0 * lx finite for padding
                sAq += q[k] * lx[k];
                ia = min(ia, z[k] == mz ? c : 0x7FFFFFFF);
                is = min(is, xs[k] == ms ? c : 0x7FFFFFFF);
                sNl += xs[k] == ms ? 1.f : 0.f;
            }
            const float Zp = wave_sum_u(sZp);
            const float Zq = wave_sum_u(sZq);
            const float Aq = wave_sum_u(sAq);
            const float nl = wave_sum_u(sNl);
            const int arg_a = wave_min_u(ia);  // argmax_c P_c   (first maximum)
            const int arg_s = wave_min_u(is);  // argmax_c sim_c (first maximum)
            const float rZp = 1.f / Zp, rZq = 1.f / Zq;
            const float logZq = __logf(Zq);
            const float Hq = logZq - Aq * rZq;  // entropy of softmax(t sim)
            float sP2 = 0.f, sPl = 0.f, sSa = 0.f;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int c = lane + 64 * k;
                P[k] *= rZp;
                sP2 = fmaf(P[k], P[k], sP2);
                sPl += xs[k] == ms ? P[k] : 0.f;
                sSa += c == arg_a ? xs[k] : 0.f;
            }
            const float P2 = wave_sum_u(sP2);
            const float Pl = wave_sum_u(sPl);
            const float sim_a = wave_sum_u(sSa);
            acc_lab += (P2 - 2.f * Pl) + nl;
            acc_m += ms;
            acc_H += Hq;
            acc_sa += sim_a;
            // ---- gradients of this row
            const float Dsum = a.kappa * (P2 - Pl);
            // the feature again (a second v_readlane per channel is cheaper than 16 SGPRs kept live
            // across the reductions: they spill)
            int i2 = i;
            asm volatile("" : "+s"(i2));
            float fs2[SP];
#pragma unroll
            for (int s = 0; s < SP; s++) fs2[s] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fv[s]), i2));
            float dz[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int c = lane + 64 * k;
                const float lab = xs[k] == ms ? 1.f : 0.f;
                dz[k] = P[k] * (a.kappa * (P[k] - lab) - Dsum);
                const float qk = q[k] * rZq;
                const float logq = lx[k] - logZq;
                float d = -g_ent * qk * (logq + Hq);   // d(0.3 mean H)/dsim
                d -= c == arg_s ? a.inv_hw : 0.f;      // d(1 - mean m)/dsim
                d -= c == arg_a ? a.inv_hw : 0.f;      // d(1 - mean sim_a)/dsim
                if (k < KL || vlast) drow[c] = d * inv;
                dbr[k] += dz[k];
#pragma unroll
                for (int s = 0; s < SP; s++) dWr[k][s] = fmaf(dz[k], fs2[s], dWr[k][s]);
            }
            // dL/df_s = sum_c dz_c W[c][s]: 16 lane partials, then a REDUCE-SCATTER over the wave (each exchange
            // halves the values a lane carries: 8 + 4 + 2 + 1 adds instead of 16 full reductions); lane l ends up
            // with the wave total of channel l & 15
            float part[SP];
#pragma unroll
            for (int s = 0; s < SP; s++) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < CPL; k++) acc = fmaf(dz[k], Wr[k][s], acc);
                part[s] = acc;
            }
            float dfo;
            {
                static_assert(SP == 16, "the reduce-scatter below is written for 16 channels");
                const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
                float w8[8], w4[4], w2[2];
#pragma unroll
                for (int j = 0; j < 8; j++) {  // partner lane ^ 1: keep channel 2j + b0
                    const float keep = b0 ? part[2 * j + 1] : part[2 * j], send = b0 ? part[2 * j] : part[2 * j + 1];
                    w8[j] = keep + __int_as_float(GOI_DPP(__float_as_int(send), 0xB1, 0xF, 0));
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {  // partner lane ^ 2: keep channel 4j + 2 b1 + b0
                    const float keep = b1 ? w8[2 * j + 1] : w8[2 * j], send = b1 ? w8[2 * j] : w8[2 * j + 1];
                    w4[j] = keep + __int_as_float(GOI_DPP(__float_as_int(send), 0x4E, 0xF, 0));
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {  // partner lane ^ 4 (ds_swizzle, xor mode)
                    const float keep = b2 ? w4[2 * j + 1] : w4[2 * j], send = b2 ? w4[2 * j] : w4[2 * j + 1];
                    w2[j] = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x101F));
                }
                {  // partner lane ^ 8
                    const float keep = b3 ? w2[1] : w2[0], send = b3 ? w2[0] : w2[1];
                    dfo = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x201F));
                }
                dfo += __shfl_xor(dfo, 16, 64);  // the four rows of 16 lanes
                dfo += __shfl_xor(dfo, 32, 64);
            }
            if (lane < S) a.dsem[(size_t)lane * HW + p] = dfo;
        }
    }
    // ---- this wave's partial sums
    float* out = a.partials + (size_t)wave * ((size_t)C * (S + 1) + 4);
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int c = lane + 64 * k;
        if (k < KL || vlast) {
#pragma unroll
            for (int s = 0; s < SP; s++)
                if (s < S) out[(size_t)c * (S + 1) + s] = dWr[k][s];
            out[(size_t)c * (S + 1) + S] = dbr[k];
        }
    }
    if (lane == 0) {
        float* lo = out + (size_t)C * (S + 1);
        lo[0] = acc_lab;
        lo[1] = acc_m;
        lo[2] = acc_H;
        lo[3] = acc_sa;
    }
}


// ---- dL/dL1 = dsim^T [C x HW] * g^T [HW x 256]: split-K fp32 MFMA GEMM --------------------------
// The reduction runs over the PIXEL axis (K = HW = 1.7 M) and the output is only C x 256, so the
// classic output tiling leaves the chip idle (hipBLASLt: 5.0 ms = 52 TFLOP/s).  Here every CU owns a
// contiguous pixel range and keeps a FULL 304 x 256 partial result in the accumulators of its 8
// waves (wave w: all 19 code blocks x one feature block = 76 VGPRs; two workgroups split the 256 columns): no atomics, no output traffic
// until the final 311 KB per CU, summed afterwards in a fixed order.
//   A[m = code][k = pixel]: the dsim tile of 32 pixels x 304 codes is shared by the 8 waves through
//       LDS (row stride 308 floats: the four k lanes of a fragment read land 16 banks apart);
//   B[k = pixel][n = feature]: each lane loads one float4 = 4 consecutive pixels of ITS feature row
//       straight from the channel-major map (64 B contiguous per row across the 4 k lanes) and uses
//       register r as the B operand of k-step r: the k <-> pixel assignment (16 jj + 4 kq + r) is a
//       permutation of the tile, applied to A's addressing as well.
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DL_KP = 32;       // pixels per LDS stage
constexpr int DL_THREADS = 512;  // 8 waves: a workgroup owns 128 of the 256 feature columns, wave w one block of 16

template <int NCB>
__global__ __launch_bounds__(DL_THREADS) void codebook_dlut_k(const float* __restrict__ dsim, const float* __restrict__ g,
                                                              long long HW, int C, float* __restrict__ partial) {
    constexpr int NC = NCB * 16, LDW = NC + 4;
    constexpr int PER_T = (DL_KP * NC + DL_THREADS - 1) / DL_THREADS;
    extern __shared__ __attribute__((aligned(16))) float s_tile[];  // [2][DL_KP][LDW]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const int dh = blockIdx.x & 1, nrange = gridDim.x >> 1, range = blockIdx.x >> 1;
    const long long per = ((HW + nrange - 1) / nrange + DL_KP - 1) / DL_KP * DL_KP;
    const long long pb = (long long)range * per;
    const long long pe = min(HW, pb + per);
    const int nst = pe > pb ? (int)((pe - pb + DL_KP - 1) / DL_KP) : 0;
    const int dcol = 128 * dh + 16 * w + mm;
    const float* grow = g + (size_t)dcol * HW;

    f32x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    float stage[PER_T];
    auto fetch_tile = [&](int st) {  // global -> registers (coalesced: the tile is one contiguous block of rows)
        const long long p0 = pb + (long long)st * DL_KP;
#pragma unroll
        for (int i = 0; i < PER_T; i++) {
            const int idx = tid + i * DL_THREADS;
            const int row = idx / NC, col = idx - row * NC;
            const long long p = p0 + row;
            stage[i] = (idx < DL_KP * NC && p < pe && col < C) ? dsim[(size_t)p * C + col] : 0.f;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PER_T; i++) {
            const int idx = tid + i * DL_THREADS;
            const int row = idx / NC, col = idx - row * NC;
            if (idx < DL_KP * NC) s_tile[(buf * DL_KP + row) * LDW + col] = stage[i];
        }
    };
    float4 bq[2], bn[2];
    auto fetch_b = [&](int st, float4* dst) {
        const long long p0 = pb + (long long)st * DL_KP;
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const long long p = p0 + 16 * jj + 4 * kq;  // pe and p are multiples of 4 (HW % 4 == 0, ranges of 32)
            dst[jj] = p < pe ? *reinterpret_cast<const float4*>(grow + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    if (nst > 0) {
        fetch_tile(0);
        fetch_b(0, bq);
        store_tile(0);
    }
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        const int buf = st & 1;
        if (st + 1 < nst) {  // next stage's loads fly while this stage's MFMAs run
            fetch_tile(st + 1);
            fetch_b(st + 1, bn);
        }
        const float* tile = s_tile + buf * DL_KP * LDW;
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const float bv[4] = {bq[jj].x, bq[jj].y, bq[jj].z, bq[jj].w};
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float* arow = tile + (16 * jj + 4 * kq + r) * LDW + mm;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++)
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * cb], bv[r], acc[cb], 0, 0, 0);
            }
        }
        if (st + 1 < nst) {
            store_tile(buf ^ 1);
            bq[0] = bn[0];
            bq[1] = bn[1];
        }
        __syncthreads();
    }
    // D[row = code 16 cb + 4 kq + r][col = feature 16 w + mm]
    float* out = partial + (size_t)range * NC * 256;
#pragma unroll
    for (int cb = 0; cb < NCB; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[(size_t)(16 * cb + 4 * kq + r) * 256 + dcol] = acc[cb][r];
}


// ---- sim_raw = g^T L1^T: [HW x 256] x [256 x C] on the bf16 matrix rate with SPLIT operands ----------------------------
// The library GEMM this replaces (hipBLASLt through torch.matmul) runs fp32 MFMAs at 99 TFLOP/s: 2.6 ms at 1600x1056, a
// third of the fused loss.  Here every fp32 operand is carried as two bf16 numbers (hi = rne(x), lo = rne(x - hi)) and a
// product is  hi*hi + lo*hi + hi*lo  on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- the split flush of
// render_bwd.hip.  The dropped lo*lo term is <= 2^-16 of a product; sim is a sum of 256 such products of either sign, so
// the error of sim is ~1e-6 of |g||L1_c| (the 1e-5 / 1e-3 parity of the losses and gradients is checked by the tests).
//
// Orientation: M = codes (A = L1 [c][k]: 8 consecutive k of a code row per lane), N = pixels (B = g [k][p], channel-major
// as the ground-truth map is: lane (kq, mm) loads k = 8 kq + i of pixel mm -- 64-byte segments), so D[code 4 kq + r][pixel mm]
// leaves as one float4 of 4 consecutive codes per lane into the [HW][C] result.  A workgroup of 4 waves owns 128 pixels
// (a wave: 2 pixel blocks x all 19 code blocks = 152 accumulator VGPRs) and walks K in 8 chunks of 32; the two bf16 planes
// of the code book's chunk (2 x 304 rows x 64 B) are staged through LDS once per chunk for all four waves, double-buffered
// and by LDS-DMA, so that the next chunk lands while this one is multiplied: one barrier per chunk.  The same pass over g
// also yields 1/|g_p| (the separate norm kernel is gone).
constexpr int SIM_NCB = 19, SIM_NC = SIM_NCB * 16, SIM_K = 256, SIM_KC = 32;

// L1 [C][256] fp32 -> planes[2][304][256] bf16 (hi, lo), rows >= C zero
__global__ __launch_bounds__(256) void codebook_split_k(const float* __restrict__ l1, int C, uint16_t* __restrict__ planes) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // pair index
    if (i >= SIM_NC * SIM_K / 2) return;
    const int c = (2 * i) / SIM_K;
    const float a = c < C ? l1[2 * i] : 0.f, b = c < C ? l1[2 * i + 1] : 0.f;
    uint32_t hi, lo;
    split_pair(a, b, hi, lo);
    reinterpret_cast<uint32_t*>(planes)[i] = hi;
    reinterpret_cast<uint32_t*>(planes + (size_t)SIM_NC * SIM_K)[i] = lo;
}

#ifndef GOI_SIM_PB
#define GOI_SIM_PB 2
#endif
#ifndef GOI_SIM_NW
#define GOI_SIM_NW 4
#endif
constexpr int SIM_PB = GOI_SIM_PB, SIM_NW = GOI_SIM_NW;  // pixel blocks (of 16) per wave, waves per workgroup
constexpr int SIM_WG_PIX = 16 * SIM_PB * SIM_NW;

// LDS: two buffers x two planes x [304][32] bf16, rows UNPADDED (64 B) because the staging is LDS-DMA
// (global_load_lds_dwordx4: a wave instruction lands 64 lanes x 16 B contiguously -- the destination cannot be padded, the
// per-lane SOURCE address is free).  Bank conflicts of the ds_read_b128 operand reads are avoided by a swizzle instead: the
// 16-byte piece j of row r sits in slot j ^ ((r >> 2) & 3) of its row; the 16 lanes of a read (rows r0 .. r0+15, one k
// quarter) then cover 16 different 16-byte slots of the 256-byte bank row.
constexpr int SIM_PLANE_U = SIM_NC * 64;            // bytes of one unpadded plane chunk
constexpr int SIM_BUF = 2 * SIM_PLANE_U;            // both planes: 38 KiB = 38 wave pieces of 1 KiB
constexpr int SIM_PIECES = SIM_BUF / 1024;
static_assert(SIM_BUF % 1024 == 0, "the staged chunk must be a whole number of 1 KiB wave pieces");

__global__ __launch_bounds__(64 * SIM_NW) void codebook_sim_k(const float* __restrict__ g, const uint16_t* __restrict__ planes,
                                                               long long HW, int C, float* __restrict__ sim,
                                                               float* __restrict__ inv_gnorm) {
    __shared__ __attribute__((aligned(1024))) char s_a[2][SIM_BUF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const long long p0 = (long long)blockIdx.x * SIM_WG_PIX + 16 * SIM_PB * w;  // this wave's pixel blocks p0, p0 + 16, ..
    f32x4 acc[SIM_PB][SIM_NCB];
#pragma unroll
    for (int pb = 0; pb < SIM_PB; pb++)
#pragma unroll
        for (int cb = 0; cb < SIM_NCB; cb++) acc[pb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float nrm[SIM_PB];
#pragma unroll
    for (int pb = 0; pb < SIM_PB; pb++) nrm[pb] = 0.f;
    float braw[SIM_PB][8];
    auto load_b = [&](int kc) {  // g[k = 32 kc + 8 kq + i][pixel p0 + 16 pb + mm]
#pragma unroll
        for (int pb = 0; pb < SIM_PB; pb++) {
            const long long p = p0 + 16 * pb + mm;
            const float* src = g + (size_t)(SIM_KC * kc + 8 * kq) * HW + (p < HW ? p : HW - 1);
#pragma unroll
            for (int i = 0; i < 8; i++) braw[pb][i] = p < HW ? src[(size_t)i * HW] : 0.f;
        }
    };
    // the code book's two planes of K chunk kc -> LDS buffer buf, asynchronously, no registers: wave w moves the 1 KiB
    // pieces w, w + NW, ...; lane l of piece q fills 16-byte slot 64 q + l
    auto stage = [&](int kc, int buf) {
        for (int q = w; q < SIM_PIECES; q += SIM_NW) {
            const int slot = 64 * q + lane;
            const int plane = slot / (SIM_NC * 4), rs = slot - plane * (SIM_NC * 4), r = rs >> 2, sp = rs & 3;
            const int piece = sp ^ ((r >> 2) & 3);
            const uint16_t* src = planes + ((size_t)plane * SIM_NC + r) * SIM_K + SIM_KC * kc + 8 * piece;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(s_a[buf] + 1024 * q), 16, 0, 0);
        }
    };
    const int a_off = 64 * mm + 16 * (kq ^ ((mm >> 2) & 3));  // this lane's operand in a 16-row block (rows 16 cb + mm)
    stage(0, 0);
    load_b(0);
    for (int kc = 0; kc < SIM_K / SIM_KC; kc++) {
        // chunk kc has landed for THIS wave's pieces; past the barrier it has for every wave's, and every wave is done
        // reading the other buffer (chunk kc - 1)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // ---- this chunk's B operands: split, and the running |g|^2
        bf16x8 Bh[SIM_PB], Bl[SIM_PB];
#pragma unroll
        for (int pb = 0; pb < SIM_PB; pb++) {
#pragma unroll
            for (int i = 0; i < 8; i++) nrm[pb] = fmaf(braw[pb][i], braw[pb][i], nrm[pb]);
            split_pack8(braw[pb], Bh[pb], Bl[pb]);
        }
        if (kc + 1 < SIM_K / SIM_KC) {  // the next chunk's traffic flies under this chunk's MFMAs
            stage(kc + 1, (kc + 1) & 1);
            load_b(kc + 1);
        }
        const char* buf = s_a[kc & 1] + a_off;
#pragma unroll
        for (int cb = 0; cb < SIM_NCB; cb++) {
            const bf16x8 Ah = *reinterpret_cast<const bf16x8*>(buf + 1024 * cb);
            const bf16x8 Al = *reinterpret_cast<const bf16x8*>(buf + 1024 * cb + SIM_PLANE_U);
#pragma unroll
            for (int pb = 0; pb < SIM_PB; pb++) {
                acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh[pb], acc[pb][cb], 0, 0, 0);
                acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl[pb], acc[pb][cb], 0, 0, 0);
                acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh[pb], acc[pb][cb], 0, 0, 0);
            }
        }
    }
    // ---- D[code 16 cb + 4 kq + r][pixel mm] -> sim[p][c]: one float4 of 4 consecutive codes per lane (C % 4 == 0)
#pragma unroll
    for (int pb = 0; pb < SIM_PB; pb++) {
        const long long p = p0 + 16 * pb + mm;
        // |g_p|^2: this lane summed k = 8 kq .. 8 kq + 7 of every chunk; the other three k lanes of the pixel sit 16 lanes apart
        float n2 = nrm[pb];
        n2 += __shfl_xor(n2, 16, 64);
        n2 += __shfl_xor(n2, 32, 64);
        if (p < HW) {
            if (kq == 0) inv_gnorm[p] = 1.0f / sqrtf(n2);
            float* dst = sim + (size_t)p * C;
#pragma unroll
            for (int cb = 0; cb < SIM_NCB; cb++) {
                const int c0 = 16 * cb + 4 * kq;
                if (c0 + 3 < C) *reinterpret_cast<f32x4*>(dst + c0) = acc[pb][cb];
                else
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (c0 + r < C) dst[c0 + r] = acc[pb][cb][r];
            }
        }
    }
}


// ================================================================================================================
// The whole training half with no [HW][C] fp32 matrix in memory (train.py:142-163): four kernels,
// each small enough to run at two waves per SIMD.
//
// All of them work on 16-pixel blocks in the MFMA accumulator layout with the PIXELS as rows,
// D[pixel 4 kq + r][code 16 cb + mm]: a lane holds 4 pixels of 19 codes, a reduction over the codes of a pixel is 19 values
// in the lane and then 4 DPP steps over the 16 lanes of a row (codebook_rows_k: full-wave reductions per PIXEL).
//   decoder_stats_k   z = f W^T + b (K = S <= 16: one v_mfma_f32_16x16x16_bf16 per split term, the bias is the accumulator's
//                     initial value) -> per pixel max, 1 / sum exp, sum P^2 and the first arg-maximum.
//   codebook_simgrad_k  sim = g^T L1^T on the matrix cores (codebook_sim_k with the operands swapped), its row statistics and
//                     dL/dsim, which leaves as bf16 hi/lo planes [16-pixel block][plane][304 codes][16 pixels]: a lane's 4
//                     pixels are 8 bytes, a wave store is 512 contiguous bytes, and the layout is the A operand of the last
//                     kernel.  Per pixel it records the code-book label (first arg-maximum, number of maxima; the full set
//                     of maxima as a bit mask in the rare case of a tie).
//   decoder_gd_k      z again, P from the recorded statistics, dz, and its two contractions, two code blocks at a time:
//                       dL/dW[c][s] = sum_p dz[p][c] f[p][s]  over pixels: the dz tile in the D layout IS the A operand
//                                     (M = code, k = 4 kq + r = pixel) -- persistent accumulators, one partial per wave;
//                       dL/df[p][s] = sum_c dz[p][c] W[c][s]  over codes, the lane axis of the D layout: dz goes through a
//                                     wave-private LDS tile ([16 pixels][32 codes] bf16, 80-byte rows) to become an A
//                                     operand (M = pixel).
//   codebook_dlut2_k  dL/dL1[c][d] = sum_p dsim[p][c] g[d][p]: the dsim planes stream through LDS by LDS-DMA (K = pixels, 32
//                     per chunk), g is split once by the wave that owns its 32 features, and a workgroup keeps the whole
//                     [304][256] partial in the accumulators of its 8 waves.
// HBM traffic at 1600x1056 (FETCH_SIZE / WRITE_SIZE counters): 8.6 GB -- g twice (2 x 1.73 GB), the planes once each way
// (2 x 2.05 GB), 0.8 GB in the decoder kernels -- against 14.4 GB for sim kernel + row kernel + fp32 dLUT kernel.
// (One kernel for the first three was tried first: ~400 live registers, one wave per SIMD, and the compiler spilled the
// addresses it hoisted; every load, LDS and dependent-MFMA latency was exposed: 4.7 ms against 3.6 ms for sim + row kernels.)
constexpr int FU_WG_PIX = 128;                // pixels of one codebook_simgrad_k workgroup: 8 waves x one 16-pixel block
constexpr int FU_TROW = 80;                   // transposition tile: row stride in bytes (64 + 16: conflict-free both ways)
constexpr int FU_TPLANE = 16 * FU_TROW, FU_TBUF = 2 * FU_TPLANE;
constexpr int FU_WZ_BYTES = 2 * SIM_NC * 32;  // decoder planes for z: [2][304][16] bf16
constexpr int FU_NJ = (SIM_NCB + 1) / 2;      // 32-code K steps of the df contraction (the last one half empty)
constexpr int FU_WT_BYTES = 2 * FU_NJ * 16 * 64;  // decoder planes for df: [2][10][16 s][32 codes] bf16
constexpr int FU_DCHUNK = 2 * SIM_NC * 16;    // uint16 elements of one 16-pixel block of the dsim planes
constexpr int FU_TIE_WORDS = 10;              // 304 bits
constexpr int GD_NW = 8;                      // decoder_gd_k: waves per workgroup (one workgroup per CU, persistent)
constexpr int DS_NW = 4;                      // decoder_stats_k

typedef short s16x4 __attribute__((ext_vector_type(4)));

struct FusedArgs {
    const float* g;          // [256][HW]   ground-truth feature map, channel-major
    const uint16_t* planes;  // [2][304][256] bf16: the normalised code book, hi and lo
    const uint16_t* wz;      // [2][304][16]  bf16: W[c][s] (s >= S zero, c >= C zero)
    const uint16_t* wt;      // [2][10][16][32] bf16: W[32 j + k][s]
    const float* bias;       // [C] or NULL
    const float* sem;        // [S][HW]
    uint16_t* dplanes;       // [blocks][2][304][16] bf16
    float* dsem;             // [S][HW]
    float* partials;         // [decoder_gd waves][C (S + 1) + 4]
    // per-pixel records, [16 * blocks] each
    float *r_mz, *r_rzp, *r_p2, *r_nl;
    int *r_arga, *r_args;
    uint32_t* r_tie;         // [16 * blocks][10]: the maxima of sim as a bit mask, written only where r_nl > 1
    float* sums_a;           // [simgrad waves][4]: nl, m, H, sim_a sums
    long long HW, blocks;
    int C, S, n_sums_a;
    float t, kappa, inv_hw, w_sl1;
};

// W [C][S] fp32 -> the two bf16 operand images of the decoder
__global__ __launch_bounds__(256) void decoder_split_k(const float* __restrict__ W, int C, int S, uint16_t* __restrict__ wz,
                                                       uint16_t* __restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // (c, s) over [320][16]: wt's last K step is half padding
    if (i >= FU_NJ * 32 * 16) return;
    const int c = i >> 4, s = i & 15;
    const float v = (c < C && s < S) ? W[(size_t)c * S + s] : 0.f;
    uint32_t hi, lo;
    split_pair(v, 0.f, hi, lo);
    if (c < SIM_NC) {
        wz[i] = (uint16_t)hi;
        wz[SIM_NC * 16 + i] = (uint16_t)lo;
    }
    const int j = c >> 5, k = c & 31;
    wt[(j * 16 + s) * 32 + k] = (uint16_t)hi;
    wt[FU_NJ * 16 * 32 + (j * 16 + s) * 32 + k] = (uint16_t)lo;
}

#define GOI_ROWF(v, ctrl) __int_as_float(GOI_DPP(__float_as_int(v), ctrl, 0xF, 0))
// reductions over the 16 lanes of a DPP row; every lane of the row ends up with the result
__device__ __forceinline__ float row_sum(float v) {
    v += GOI_ROWF(v, 0xB1);
    v += GOI_ROWF(v, 0x4E);
    v += GOI_ROWF(v, 0x141);
    v += GOI_ROWF(v, 0x140);
    return v;
}
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, GOI_ROWF(v, 0xB1));
    v = fmaxf(v, GOI_ROWF(v, 0x4E));
    v = fmaxf(v, GOI_ROWF(v, 0x141));
    v = fmaxf(v, GOI_ROWF(v, 0x140));
    return v;
}
__device__ __forceinline__ int row_min(int v) {
    v = min(v, GOI_DPP(v, 0xB1, 0xF, 0));
    v = min(v, GOI_DPP(v, 0x4E, 0xF, 0));
    v = min(v, GOI_DPP(v, 0x141, 0xF, 0));
    v = min(v, GOI_DPP(v, 0x140, 0xF, 0));
    return v;
}

// z tiles of one 16-pixel block: A = f [pixel mm][s = 4 kq + i] (fv: this lane's four values), B = W [code mm][s = 4 kq + i]
// from the LDS image (wz_l = image + 32 mm + 8 kq), C = bias (bias_l = s_bias + mm).  The three products of a tile are issued
// term by term over groups of four tiles: no MFMA waits for the one before it.  decoder_stats_k calls this; decoder_gd_k forms
// each tile with the same three products in the same order: the same z to the last bit.
__device__ __forceinline__ void decoder_logits(f32x4 (&z)[SIM_NCB], const float (&fv)[4], const char* wz_l, const float* bias_l,
                                               bool vlast) {
    uint32_t fh[2], fl[2];
    split_pair(fv[0], fv[1], fh[0], fl[0]);
    split_pair(fv[2], fv[3], fh[1], fl[1]);
    const s16x4 fAh = __builtin_bit_cast(s16x4, uint2{fh[0], fh[1]}), fAl = __builtin_bit_cast(s16x4, uint2{fl[0], fl[1]});
    constexpr int G = 4;
#pragma unroll
    for (int g0 = 0; g0 < SIM_NCB; g0 += G) {
        s16x4 Bh[G], Bl[G];
#pragma unroll
        for (int i = 0; i < G; i++)
            if (g0 + i < SIM_NCB) {
                const float b = bias_l[16 * (g0 + i)];
                Bh[i] = *reinterpret_cast<const s16x4*>(wz_l + 512 * (g0 + i));
                Bl[i] = *reinterpret_cast<const s16x4*>(wz_l + 512 * (g0 + i) + FU_WZ_BYTES / 2);
                z[g0 + i] = f32x4{b, b, b, b};
            }
#pragma unroll
        for (int i = 0; i < G; i++)
            if (g0 + i < SIM_NCB) z[g0 + i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAl, Bh[i], z[g0 + i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < G; i++)
            if (g0 + i < SIM_NCB) z[g0 + i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAh, Bl[i], z[g0 + i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < G; i++)
            if (g0 + i < SIM_NCB) z[g0 + i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAh, Bh[i], z[g0 + i], 0, 0, 0);
        asm volatile("" ::: "memory");  // one group's operands in flight at a time: all 19 at once cost 100 registers
    }
    const float NEG_INF = -__builtin_inff();
    if (!vlast) z[SIM_NCB - 1] = f32x4{NEG_INF, NEG_INF, NEG_INF, NEG_INF};  // padding codes: P = 0, no gradient
}

// ---- decoder statistics: one 16-pixel block per wave and iteration
__global__ __launch_bounds__(64 * DS_NW, 3) void decoder_stats_k(const FusedArgs a) {
    __shared__ __attribute__((aligned(16))) char s_wz[FU_WZ_BYTES];
    __shared__ float s_bias[SIM_NC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const long long HW = a.HW;
    for (int i = tid; i < FU_WZ_BYTES / 16; i += 64 * DS_NW)
        reinterpret_cast<uint4*>(s_wz)[i] = reinterpret_cast<const uint4*>(a.wz)[i];
    for (int i = tid; i < SIM_NC; i += 64 * DS_NW) s_bias[i] = (a.bias && i < a.C) ? a.bias[i] : 0.f;
    __syncthreads();
    const bool vlast = 16 * (SIM_NCB - 1) + mm < a.C;
    const char* const wz_l = s_wz + 32 * mm + 8 * kq;
    const float* const bias_l = s_bias + mm;
    auto fetch = [&](long long blk, float (&fv)[4]) {  // one block ahead: see decoder_gd_k
        const long long p = min(16 * min(blk, a.blocks - 1) + mm, HW - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) fv[i] = (4 * kq + i < a.S) ? a.sem[(size_t)(4 * kq + i) * HW + p] : 0.f;
    };
    const long long stride = (long long)gridDim.x * DS_NW;
    float fvn[4];
    fetch((long long)blockIdx.x * DS_NW + w, fvn);
    for (long long blk = (long long)blockIdx.x * DS_NW + w; blk < a.blocks; blk += stride) {
        const long long pbase = 16 * blk;
        const float fv[4] = {fvn[0], fvn[1], fvn[2], fvn[3]};
        fetch(blk + stride, fvn);
        f32x4 z[SIM_NCB];
        decoder_logits(z, fv, wz_l, bias_l, vlast);
        f32x4 o_mz, o_rzp, o_p2;
        int4 o_arg;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float m = -__builtin_inff();
#pragma unroll
            for (int cb = 0; cb < SIM_NCB; cb++) m = fmaxf(m, z[cb][r]);
            const float mz = row_max(m);
            float sZ = 0.f, s2 = 0.f;
            int ia = 0x7FFFFFFF;
#pragma unroll
            for (int cb = SIM_NCB - 1; cb >= 0; cb--) {  // descending: the lane's FIRST maximum wins
                ia = z[cb][r] == mz ? 16 * cb + mm : ia;
                const float e = __expf(z[cb][r] - mz);
                sZ += e;
                s2 = fmaf(e, e, s2);
            }
            const float rZ = 1.f / row_sum(sZ);
            o_mz[r] = mz;
            o_rzp[r] = rZ;
            o_p2[r] = row_sum(s2) * rZ * rZ;
            (&o_arg.x)[r] = row_min(ia);
        }
        if (mm == 0) {  // rows pbase + 4 kq .. + 3
            *reinterpret_cast<f32x4*>(a.r_mz + pbase + 4 * kq) = o_mz;
            *reinterpret_cast<f32x4*>(a.r_rzp + pbase + 4 * kq) = o_rzp;
            *reinterpret_cast<f32x4*>(a.r_p2 + pbase + 4 * kq) = o_p2;
            *reinterpret_cast<int4*>(a.r_arga + pbase + 4 * kq) = o_arg;
        }
    }
}

// ---- sim, its statistics and dL/dsim.  Pixels are MFMA rows; one 16-pixel block per wave, 8 waves per workgroup.
// BOTH operands reach LDS by LDS-DMA: the code book's chunk (shared, 3 buffers, requested two iterations ahead) and the
// wave's own g tile ([32 k][16 pixels] fp32, 2 buffers, requested two iterations ahead and re-filled right after it is read).
// An ordinary load in this loop would make hipcc drain the vector-memory counter at its use, LDS-DMA included, and the loop
// would run at the latency of one chunk's trip through L2 (that is what bounds codebook_sim_k); with nothing but LDS-DMA in
// flight the only waits are the counted ones below.  All LDS is ONE array: a second __shared__ object costs a vmcnt(0)
// before the first ds_read of every iteration.
constexpr int SG_NW = 8, SG_NBUF = 3;
constexpr int SG_A_BYTES = SIM_KC * 16 * 4;                         // one wave's g tile of one chunk
constexpr int SG_LDS = SG_NBUF * SIM_BUF + SG_NW * 2 * SG_A_BYTES;  // 146 KiB: one workgroup per CU
__global__ __launch_bounds__(64 * SG_NW, 1) void codebook_simgrad_k(const FusedArgs a) {
    __shared__ __attribute__((aligned(1024))) char smem[SG_LDS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const long long HW = a.HW;
    const int C = a.C;
    const float NEG_INF = -__builtin_inff();
    const long long pbase = (long long)blockIdx.x * FU_WG_PIX + 16 * w;  // this lane's D rows are pixels pbase + 4 kq + r
    char* const s_cb = smem;                                           // [SG_NBUF][SIM_BUF]
    char* const s_aw = smem + SG_NBUF * SIM_BUF + w * 2 * SG_A_BYTES;  // this wave's [2][32 k][16 pixels] floats
    f32x4 sx[SIM_NCB];
#pragma unroll
    for (int cb = 0; cb < SIM_NCB; cb++) sx[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float nrm = 0.f;
    constexpr int NKC = SIM_K / SIM_KC;
    // g tile of chunk kc: two wave instructions; lane l of instruction j moves 4 consecutive pixels of row k = 16 j + (l >> 2)
    // (a pixel group lies wholly inside or wholly outside the map: HW % 4 = 0; outside, the last group is read instead)
    const float* const a_src = a.g + (size_t)(lane >> 2) * HW + min(pbase + 4 * (lane & 3), HW - 4);
    auto stage_a = [&](int kc) {
#pragma unroll
        for (int j = 0; j < 2; j++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src + (size_t)(SIM_KC * kc + 16 * j) * HW),
                                             (__attribute__((address_space(3))) void*)(s_aw + SG_A_BYTES * (kc & 1) + 1024 * j), 16, 0, 0);
    };
    // code-book chunk: every wave moves the same number of 1 KiB pieces (the waits count them): 38 pieces over 8 waves are 5
    // each, the two surplus slots repeat piece 37 (the same bytes to the same place)
    const char* planes_b = reinterpret_cast<const char*>(a.planes);
    constexpr int NPIECE = (SIM_PIECES + SG_NW - 1) / SG_NW;
    auto stage = [&](int kc) {
#pragma unroll
        for (int j = 0; j < NPIECE; j++) {
            const int q = min(w + SG_NW * j, SIM_PIECES - 1);
            const int slot = 64 * q + lane;
            const int plane = slot / (SIM_NC * 4), rs = slot - plane * (SIM_NC * 4), r = rs >> 2, sp = rs & 3;
            const int piece = sp ^ ((r >> 2) & 3);
            const uint32_t so = (uint32_t)(((plane * SIM_NC + r) * SIM_K + 8 * piece + SIM_KC * kc) * 2);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(planes_b + so),
                                             (__attribute__((address_space(3))) void*)(s_cb + SIM_BUF * (kc % SG_NBUF) + 1024 * q), 16, 0, 0);
        }
    };
    static_assert(NPIECE == 5 && SG_NBUF == 3, "the s_waitcnt immediates below are written for 5 + 2 operations per chunk, two chunks ahead");
    const int b_off = 64 * mm + 16 * (kq ^ ((mm >> 2) & 3));
    const char* const a_rd = s_aw + 4 * (16 * 8 * kq + mm);  // A[k = 8 kq + i][pixel mm]: + 64 i
    stage(0);
    stage_a(0);
    stage(1);
    stage_a(1);
#pragma unroll
    for (int kc = 0; kc < NKC; kc++) {
        // issue order: chunk kc + 2's seven operations in iteration kc.  Needed now: chunk kc (issued two iterations ago); the
        // seven of chunk kc + 1 may stay in flight.  Past the barrier chunk kc has landed for every wave, and every wave is
        // done reading the buffer chunk kc + 2 goes to.
        if (kc + 1 < NKC) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        float araw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) araw[i] = *reinterpret_cast<const float*>(a_rd + SG_A_BYTES * (kc & 1) + 64 * i);
        bf16x8 Ah, Al;
#pragma unroll
        for (int i = 0; i < 8; i++) nrm = fmaf(araw[i], araw[i], nrm);
        split_pack8(araw, Ah, Al);
        if (kc + 2 < NKC) {
            stage(kc + 2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile is in registers before its buffer is re-filled
            stage_a(kc + 2);
        }
        const char* buf = s_cb + SIM_BUF * (kc % SG_NBUF) + b_off;
        // Three products per code block on one accumulator.  Issued block by block they form a chain (a dependent 16x16x32
        // issues every ~36 clocks, an independent one every 16) behind the block's own LDS reads: 19 x (LDS latency + chain)
        // per chunk.  Issued term by term over GROUPS of four blocks, with the next group's operands requested first, neither
        // latency is on the path.
        constexpr int G = 4, NG = (SIM_NCB + G - 1) / G;
        bf16x8 Bh[2][G], Bl[2][G];
        auto fetch_b = [&](int g, int slot) {
#pragma unroll
            for (int i = 0; i < G; i++)
                if (G * g + i < SIM_NCB) {
                    Bh[slot][i] = *reinterpret_cast<const bf16x8*>(buf + 1024 * (G * g + i));
                    Bl[slot][i] = *reinterpret_cast<const bf16x8*>(buf + 1024 * (G * g + i) + SIM_PLANE_U);
                }
        };
        fetch_b(0, 0);
#pragma unroll
        for (int g = 0; g < NG; g++) {
            if (g + 1 < NG) fetch_b(g + 1, (g + 1) & 1);
#pragma unroll
            for (int i = 0; i < G; i++)
                if (G * g + i < SIM_NCB) sx[G * g + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh[g & 1][i], sx[G * g + i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < G; i++)
                if (G * g + i < SIM_NCB) sx[G * g + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl[g & 1][i], sx[G * g + i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < G; i++)
                if (G * g + i < SIM_NCB) sx[G * g + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh[g & 1][i], sx[G * g + i], 0, 0, 0);
        }
    }
    const bool vlast = 16 * (SIM_NCB - 1) + mm < C;  // 288 < C <= 304: only the last code block has padding
    const float g_ent = a.w_sl1 * a.t * a.inv_hw;
    const float first = mm == 0 ? 1.f : 0.f;  // a row's scalars are replicated over its 16 lanes: count them once
    float acc_nl = 0.f, acc_m = 0.f, acc_H = 0.f, acc_sa = 0.f;
    {
        float invl;
        {  // 1 / |g|: this lane summed k = 8 kq .. + 7 of every chunk for pixel mm
            float n2 = nrm;
            n2 += __shfl_xor(n2, 16, 64);
            n2 += __shfl_xor(n2, 32, 64);
            invl = 1.0f / sqrtf(n2);
        }
        const int4 arga4 = *reinterpret_cast<const int4*>(a.r_arga + pbase + 4 * kq);
        f32x4 o_nl;
        int4 o_args;
        // The per-element work below is the kernel's VALU bill (152 elements per lane): everything that is constant over a row
        // is folded into row scalars first -- exp(t (x - ms)) as exp2(x tl + nb), the entropy sums in log2 units, the gradient
        // as (c1 q)(e2 + k2) -- and the two one-element terms of the gradient enter through a per-lane multiplicity word.
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float inv = __shfl(invl, 4 * kq + r, 64);
            const bool valid = pbase + 4 * kq + r < HW;
            const float vw = valid ? first : 0.f;
            const int arg_a = (&arga4.x)[r];
            const int cba = (arg_a & 15) == mm ? arg_a >> 4 : -1;  // the code block in which THIS lane holds code arg_a
            // sx holds the RAW products <g, L1_c>; sim = raw / |g| never exists per element: 1 / |g| > 0 goes into the row
            // constants (maxima and ties are those of the raw row)
            float m = NEG_INF;
            if (!vlast) sx[SIM_NCB - 1][r] = NEG_INF;
#pragma unroll
            for (int cb = 0; cb < SIM_NCB; cb++) m = fmaxf(m, sx[cb][r]);
            const float mraw = row_max(m), ms = mraw * inv;
            const float tl = a.t * 1.44269504088896341f * inv, nb = -mraw * tl;  // t (sim - ms) in log2 units: e2 = raw tl + nb <= 0
            float sZ = 0.f, sA = 0.f, sel = 0.f;
            int is = 0x7FFFFFFF, cnt = 0;
#pragma unroll
            for (int cb = SIM_NCB - 1; cb >= 0; cb--) {  // descending: the lane's FIRST maximum wins
                const float x = sx[cb][r];
                const bool top = x == mraw;
                is = top ? 16 * cb + mm : is;
                cnt += top ? 1 : 0;
                sel = cb == cba ? x : sel;
                float e2 = fmaf(x, tl, nb);
                const float q = __builtin_amdgcn_exp2f(e2);
                sZ += q;
                if (cb == SIM_NCB - 1) e2 = fmaxf(e2, -FLT_MAX);  // padding: keep 0 * e2 finite
                sA = fmaf(q, e2, sA);
            }
            const float Zq = row_sum(sZ), A2 = row_sum(sA), nl = row_sum((float)cnt), sim_a = row_sum(sel) * inv;
            const int arg_s = row_min(is);
            const float rZq = 1.f / Zq, k2 = -A2 * rZq;                        // k2 = (H - log Zq) / ln 2
            const float Hq = 0.69314718055994531f * (__builtin_amdgcn_logf(Zq) + k2);  // v_log_f32 is log2
            acc_nl += vw * nl;
            acc_m += vw * ms;
            acc_H += vw * Hq;
            acc_sa += vw * sim_a;
            o_nl[r] = nl;
            (&o_args.x)[r] = arg_s;
            // A tie (several codes share the maximum of sim: duplicate code-book rows) is the one case in which
            // decoder_gd_k cannot rebuild the label from (arg_s, nl): the set of maxima goes out as a bit mask, bit c of the
            // pixel's 304.  (dL/dsim itself follows the FIRST maximum, as the row kernel and torch.max do.)
            if (__builtin_expect(__any(nl > 1.f), 0)) {
                uint32_t* wd = a.r_tie + (size_t)(pbase + 4 * kq + r) * FU_TIE_WORDS;
                uint32_t word = 0;
#pragma unroll
                for (int cb = 0; cb < SIM_NCB; cb++) {
                    const unsigned long long bal = __ballot(sx[cb][r] == mraw);  // bit 16 kq + mm
                    const uint32_t bits = (uint32_t)(bal >> (16 * kq)) & 0xFFFFu;
                    word = (cb & 1) ? (word | (bits << 16)) : bits;
                    if (((cb & 1) || cb == SIM_NCB - 1) && nl > 1.f && mm == 0) wd[cb >> 1] = word;
                }
            }
            // dL/dsim_raw = inv ( -g_ent q / Zq (ln q - log Zq + H)  -  [c = arg_s] / HW  -  [c = arg_a] / HW ),  ln q = e2 ln 2
            const float invr = valid ? inv : 0.f;  // a pixel beyond the map has no gradient
            const float c1 = -g_ent * 0.69314718055994531f * rZq * invr, wone = -a.inv_hw * invr;
            // multiplicity (0, 1, 2) of the one-element terms at this lane's code of block cb: two bits per block
            const int cbs = (arg_s & 15) == mm ? arg_s >> 4 : -1;
            unsigned long long mult = (cbs >= 0 ? 1ull << (2 * cbs) : 0ull) + (cba >= 0 ? 1ull << (2 * cba) : 0ull);
            const uint32_t mult_lo = (uint32_t)mult, mult_hi = (uint32_t)(mult >> 32);
            // exp2 is evaluated a second time ON PURPOSE: kept from the statistics pass q would be 76 more live registers;
            // the opaque copy of nb stops the compiler from "saving" the work
            float nbr = nb;
            asm volatile("" : "+v"(nbr));
#pragma unroll
            for (int cb = 0; cb < SIM_NCB; cb++) {
                float e2 = fmaf(sx[cb][r], tl, nbr);
                const float q = __builtin_amdgcn_exp2f(e2);
                if (cb == SIM_NCB - 1) e2 = fmaxf(e2, -FLT_MAX);
                const uint32_t mu = cb < 16 ? (mult_lo >> (2 * cb)) & 3u : (mult_hi >> (2 * (cb - 16))) & 3u;
                sx[cb][r] = fmaf(wone, (float)mu, (c1 * q) * (e2 + k2));
            }
        }
        if (mm == 0) {
            *reinterpret_cast<f32x4*>(a.r_nl + pbase + 4 * kq) = o_nl;
            *reinterpret_cast<int4*>(a.r_args + pbase + 4 * kq) = o_args;
        }
        // ---- dsim planes of this block: [plane][code][16 pixels]
        {
            uint16_t* dst = a.dplanes + (size_t)(pbase >> 4) * FU_DCHUNK + (size_t)mm * 16 + 4 * kq;
#pragma unroll
            for (int cb = 0; cb < SIM_NCB; cb++) {
                uint32_t h0, l0, h1, l1;
                split_pair(sx[cb][0], sx[cb][1], h0, l0);
                split_pair(sx[cb][2], sx[cb][3], h1, l1);
                *reinterpret_cast<uint2*>(dst + 256 * cb) = uint2{h0, h1};
                *reinterpret_cast<uint2*>(dst + 256 * cb + SIM_NC * 16) = uint2{l0, l1};
            }
        }
    }
    const float t0 = wave_sum_u(acc_nl), t1 = wave_sum_u(acc_m), t2 = wave_sum_u(acc_H), t3 = wave_sum_u(acc_sa);
    if (lane == 0) *reinterpret_cast<f32x4*>(a.sums_a + 4 * ((size_t)blockIdx.x * SG_NW + w)) = f32x4{t0, t1, t2, t3};
}

// the recorded statistics of a 16-pixel block's rows 4 kq .. 4 kq + 3 (decoder_stats_k, codebook_simgrad_k)
struct DecIn {
    f32x4 mz, rzp, p2, nl;
    int4 args;
};
__device__ __forceinline__ void decoder_fetch(DecIn& in, const FusedArgs& a, long long pbase, int kq) {
    in.mz = *reinterpret_cast<const f32x4*>(a.r_mz + pbase + 4 * kq);
    in.rzp = *reinterpret_cast<const f32x4*>(a.r_rzp + pbase + 4 * kq);
    in.p2 = *reinterpret_cast<const f32x4*>(a.r_p2 + pbase + 4 * kq);
    in.nl = *reinterpret_cast<const f32x4*>(a.r_nl + pbase + 4 * kq);
    in.args = *reinterpret_cast<const int4*>(a.r_args + pbase + 4 * kq);
}

// ---- dL/dW, dL/db and dL/df in ONE pass over z: persistent, one 16-pixel block per wave and iteration.  dz[p][c] depends on
// every code of the pixel through ONE number: Pl = sum of P over the pixel's label codes, which enters through Dsum.  With the
// label a single code (arg_s: the only case when no two code-book rows coincide) Pl is P at that code, and its logit is a
// 16-term dot product the 16 lanes of the pixel's row form from the decoder image in LDS and the feature values the lane
// already holds -- a few instructions per pixel; for a tie the same dot product runs once per bit of the recorded mask.  With
// Pl known up front the block STREAMS: two code blocks at a time -- logits (6 matrix instructions), dz in place, dL/db sums,
// the dL/dW products, the transposition tile, the df products -- and what lives across the block is the 76 accumulator
// registers and a handful of row scalars (two waves per SIMD).  Pl is an fp32 chain over the decoder's hi + lo planes where
// the logits are the three split-bf16 products of the same planes: ~1e-6 relative on P.
//   dL/dW[c][s] += sum_p dz[p][c] f[p][s]: A = dz [code mm][k = pixel 4 kq + r] (the D layout as it is), B = f [k = pixel 4 kq + i][s = mm]
//   dL/df[p][s] = sum_c dz[p][c] W[c][s]: the contraction runs over the codes, the LANE axis of the D layout, so dz goes
//     through a wave-private LDS tile ([16 pixels][32 codes] bf16 hi and lo, 80-byte rows) to become the A operand
//     [pixel mm][k = code 8 kq + i]; the three products keep separate accumulators (no dependent MFMA chain).
__global__ __launch_bounds__(64 * GD_NW, 1) void decoder_gd_k(const FusedArgs a) {
    __shared__ __attribute__((aligned(16))) char s_wz[FU_WZ_BYTES];
    __shared__ __attribute__((aligned(16))) char s_wt[FU_WT_BYTES];
    __shared__ __attribute__((aligned(16))) char s_tr[GD_NW][2][FU_TBUF];
    __shared__ float s_bias[SIM_NC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const long long HW = a.HW;
    const int C = a.C, S = a.S;
    for (int i = tid; i < FU_WZ_BYTES / 16; i += 64 * GD_NW)
        reinterpret_cast<uint4*>(s_wz)[i] = reinterpret_cast<const uint4*>(a.wz)[i];
    for (int i = tid; i < FU_WT_BYTES / 16; i += 64 * GD_NW)
        reinterpret_cast<uint4*>(s_wt)[i] = reinterpret_cast<const uint4*>(a.wt)[i];
    for (int i = tid; i < SIM_NC; i += 64 * GD_NW) s_bias[i] = (a.bias && i < a.C) ? a.bias[i] : 0.f;
    __syncthreads();
    const bool vlast = 16 * (SIM_NCB - 1) + mm < C;
    const char* const wz_l = s_wz + 32 * mm + 8 * kq;
    const float* const bias_l = s_bias + mm;
    const char* const wt_l = s_wt + 64 * mm + 16 * kq;
    char* const tw_l = s_tr[w][0] + 2 * mm + FU_TROW * 4 * kq;     // tile writes: this lane's code column, its 4 pixel rows
    const char* const tr_l = s_tr[w][0] + FU_TROW * mm + 16 * kq;  // tile reads: pixel row mm, codes 8 kq ..
    const uint16_t* const wz16 = reinterpret_cast<const uint16_t*>(s_wz);
    f32x4 dWacc[SIM_NCB];  // D[code 16 cb + 4 kq + r][s = mm]
    float dbr[SIM_NCB];    // lane (kq, mm): sum of dz[pixel rows 4 kq + r][code 16 cb + mm]
#pragma unroll
    for (int cb = 0; cb < SIM_NCB; cb++) {
        dWacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        dbr[cb] = 0.f;
    }
    float acc_lab = 0.f;
    const long long wave = (long long)blockIdx.x * GD_NW + w, n_waves = (long long)gridDim.x * GD_NW;
    // A block's inputs are requested a block ahead: the loop is short and only two waves share a SIMD, so a load issued where
    // it is used costs its whole latency.
    float fvz[4], fvw[4];  // the decoder's two views of the feature: f[s = 4 kq + i][pixel mm], f[s = mm][pixel 4 kq + i]
    DecIn in;
    auto fetch = [&](long long blk) {
        const long long pbase = 16 * min(blk, a.blocks - 1);
        const long long pz = min(pbase + mm, HW - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            fvz[i] = (4 * kq + i < S) ? a.sem[(size_t)(4 * kq + i) * HW + pz] : 0.f;
            fvw[i] = mm < S ? a.sem[(size_t)mm * HW + min(pbase + 4 * kq + i, HW - 1)] : 0.f;
        }
        decoder_fetch(in, a, pbase, kq);
    };
    // P of pixel row r at code c (row-uniform c): the row's 16 lanes hold f[s = mm] of that pixel
    auto prob_at = [&](int c, float f_mm, float mz, float rZ) {
        const float wv = __uint_as_float((uint32_t)wz16[c * 16 + mm] << 16) + __uint_as_float((uint32_t)wz16[SIM_NC * 16 + c * 16 + mm] << 16);
        const float zc = row_sum(wv * f_mm) + s_bias[c];
        return __expf(zc - mz) * rZ;
    };
    fetch(wave);
    for (long long blk = wave; blk < a.blocks; blk += n_waves) {
        const long long pbase = 16 * blk;
        // ---- row scalars: Pl, the label bits of this lane's codes, Dsum
        float kapr[4], dsum[4], mzr[4], rzr[4];
        uint32_t labm[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool valid = pbase + 4 * kq + r < HW;
            const float mz = in.mz[r], rZ = in.rzp[r], P2 = in.p2[r], nl = in.nl[r];
            const int arg_s = (&in.args.x)[r];
            float Pl;
            uint32_t lm = 0;
            if (__builtin_expect(__any(nl > 1.f), 0)) {
                const uint32_t* wd = a.r_tie + (size_t)(pbase + 4 * kq + r) * FU_TIE_WORDS;
                if (nl > 1.f) {  // (row-uniform) every maximum of sim is a label: their P, one dot product per bit of the mask
                    Pl = 0.f;
                    for (int wi = 0; wi < FU_TIE_WORDS; wi++) {
                        uint32_t bits = wd[wi];
                        while (bits) {
                            const int b = __builtin_ctz(bits);
                            bits &= bits - 1;
                            Pl += prob_at(32 * wi + b, fvw[r], mz, rZ);
                        }
                    }
#pragma unroll
                    for (int cb = 0; cb < SIM_NCB; cb++) lm |= ((wd[cb >> 1] >> (16 * (cb & 1) + mm)) & 1u) ? (1u << cb) : 0u;
                } else {
                    Pl = prob_at(arg_s, fvw[r], mz, rZ);
                    lm = (arg_s & 15) == mm ? 1u << (arg_s >> 4) : 0u;
                }
            } else {
                Pl = prob_at(arg_s, fvw[r], mz, rZ);
                lm = (arg_s & 15) == mm ? 1u << (arg_s >> 4) : 0u;
            }
            acc_lab += (valid && mm == 0) ? (P2 - 2.f * Pl) + nl : 0.f;
            const float kap = valid ? a.kappa : 0.f;  // a pixel beyond the map has no gradient
            kapr[r] = kap;
            dsum[r] = kap * (P2 - Pl);
            mzr[r] = mz;
            rzr[r] = rZ;
            labm[r] = lm;
        }
        uint32_t fh[2], fl[2], bh[2], bl[2];
        split_pair(fvz[0], fvz[1], fh[0], fl[0]);
        split_pair(fvz[2], fvz[3], fh[1], fl[1]);
        split_pair(fvw[0], fvw[1], bh[0], bl[0]);
        split_pair(fvw[2], fvw[3], bh[1], bl[1]);
        const s16x4 fAh = __builtin_bit_cast(s16x4, uint2{fh[0], fh[1]}), fAl = __builtin_bit_cast(s16x4, uint2{fl[0], fl[1]});
        const s16x4 fBh = __builtin_bit_cast(s16x4, uint2{bh[0], bh[1]}), fBl = __builtin_bit_cast(s16x4, uint2{bl[0], bl[1]});
        fetch(blk + n_waves);  // the next block's inputs: they land under this block's products
        // one K step of the df contraction = code blocks 2 j and 2 j + 1: logits, dz, dL/db, dL/dW products, tile j & 1
        auto step = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            f32x4 z[2];
            s16x4 Bh[2], Bl[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                constexpr int dummy = 0;
                (void)dummy;
                const int cb = 2 * j + h;
                if (cb < SIM_NCB) {
                    const float b = bias_l[16 * cb];
                    Bh[h] = *reinterpret_cast<const s16x4*>(wz_l + 512 * cb);
                    Bl[h] = *reinterpret_cast<const s16x4*>(wz_l + 512 * cb + FU_WZ_BYTES / 2);
                    z[h] = f32x4{b, b, b, b};
                }
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (2 * j + h < SIM_NCB) z[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAl, Bh[h], z[h], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (2 * j + h < SIM_NCB) z[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAh, Bl[h], z[h], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (2 * j + h < SIM_NCB) z[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fAh, Bh[h], z[h], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int cb = 2 * j + h;
                char* col = tw_l + FU_TBUF * (j & 1) + 32 * h;
                uint32_t dh[2] = {0u, 0u}, dl[2] = {0u, 0u};
                if (cb < SIM_NCB) {
                    if (cb == SIM_NCB - 1 && !vlast) z[h] = f32x4{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float P = __expf(z[h][r] - mzr[r]) * rzr[r];
                        const float lab = (labm[r] >> cb) & 1u ? 1.f : 0.f;
                        z[h][r] = P * (kapr[r] * (P - lab) - dsum[r]);  // dz
                    }
                    split_pair(z[h][0], z[h][1], dh[0], dl[0]);
                    split_pair(z[h][2], z[h][3], dh[1], dl[1]);
                    dbr[cb] += (z[h][0] + z[h][1]) + (z[h][2] + z[h][3]);
                    const s16x4 Ah = __builtin_bit_cast(s16x4, uint2{dh[0], dh[1]}), Al = __builtin_bit_cast(s16x4, uint2{dl[0], dl[1]});
                    dWacc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Al, fBh, dWacc[cb], 0, 0, 0);
                    dWacc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Ah, fBl, dWacc[cb], 0, 0, 0);
                    dWacc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Ah, fBh, dWacc[cb], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    *reinterpret_cast<uint16_t*>(col + FU_TROW * r) = (uint16_t)((r & 1) ? dh[r >> 1] >> 16 : dh[r >> 1]);
                    *reinterpret_cast<uint16_t*>(col + FU_TROW * r + FU_TPLANE) = (uint16_t)((r & 1) ? dl[r >> 1] >> 16 : dl[r >> 1]);
                }
            }
            // (one step's operands and logits in flight at a time: left to itself the scheduler hoists all ten steps' loads and
            // products to the top of the block -- 80 spilled registers)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        f32x4 df0 = f32x4{0.f, 0.f, 0.f, 0.f}, df1 = df0, df2 = df0;
        auto consume = [&](int j) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const bf16x8 Ah = *reinterpret_cast<const bf16x8*>(tr_l + FU_TBUF * (j & 1));
            const bf16x8 Al = *reinterpret_cast<const bf16x8*>(tr_l + FU_TBUF * (j & 1) + FU_TPLANE);
            const bf16x8 Bh = *reinterpret_cast<const bf16x8*>(wt_l + 1024 * j);
            const bf16x8 Bl = *reinterpret_cast<const bf16x8*>(wt_l + 1024 * j + FU_WT_BYTES / 2);
            df0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, df0, 0, 0, 0);
            df1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, df1, 0, 0, 0);
            df2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, df2, 0, 0, 0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        // tile j + 1 is written before tile j is read (two tiles): the LDS round trip of a step hides behind the next step's logits
        static_assert(FU_NJ == 10, "the unrolled step sequence below is written for ten K steps");
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{}); consume(0);
        step(std::integral_constant<int, 2>{}); consume(1);
        step(std::integral_constant<int, 3>{}); consume(2);
        step(std::integral_constant<int, 4>{}); consume(3);
        step(std::integral_constant<int, 5>{}); consume(4);
        step(std::integral_constant<int, 6>{}); consume(5);
        step(std::integral_constant<int, 7>{}); consume(6);
        step(std::integral_constant<int, 8>{}); consume(7);
        step(std::integral_constant<int, 9>{}); consume(8);
        consume(9);
        // D[pixel 4 kq + r][s = mm]
        if (mm < S) {
            float* dst = a.dsem + (size_t)mm * HW + pbase + 4 * kq;
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (pbase + 4 * kq + r < HW) dst[r] = (df0[r] + df1[r]) + df2[r];
        }
    }
    // ---- this wave's partial row: dL/dW[c][s] and dL/db[c] as [C][S + 1], then the four loss sums
    float* out = a.partials + (size_t)wave * ((size_t)C * (S + 1) + 4);
#pragma unroll
    for (int cb = 0; cb < SIM_NCB; cb++) {
        if (mm < S) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int c = 16 * cb + 4 * kq + r;
                if (c < C) out[(size_t)c * (S + 1) + mm] = dWacc[cb][r];
            }
        }
        float d = dbr[cb];
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
        if (kq == 0 && 16 * cb + mm < C) out[(size_t)(16 * cb + mm) * (S + 1) + S] = d;
    }
    // the loss sums: this kernel's part (sum P^2 - 2 sum_label P + number of labels) and, folded in in a fixed order,
    // codebook_simgrad_k's per-wave sums (rows wave, wave + n_waves, ...)
    float t0 = wave_sum_u(acc_lab);
    float t1 = 0.f, t2 = 0.f, t3 = 0.f;
    for (long long i = wave + n_waves * lane; i < a.n_sums_a; i += 64 * n_waves) {  // lane partials, then the fixed DPP order
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.sums_a + 4 * i);
        t1 += v[1];
        t2 += v[2];
        t3 += v[3];
    }
    t1 = wave_sum_u(t1);
    t2 = wave_sum_u(t2);
    t3 = wave_sum_u(t3);
    if (lane == 0) {
        float* lo = out + (size_t)C * (S + 1);
        lo[0] = t0;
        lo[1] = t1;
        lo[2] = t2;
        lo[3] = t3;
    }
}

// ---- dL/dL1 from the dsim planes: partial[wg][304][256]
constexpr int DL2_NW = 8;
__global__ __launch_bounds__(64 * DL2_NW, 1) void codebook_dlut2_k(const uint16_t* __restrict__ dplanes, const float* __restrict__ g,
                                                                  long long HW, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(1024))) char s_a[2][SIM_BUF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, mm = lane & 15;
    const long long n_chunks = (HW + 31) / 32;  // 32 pixels = two blocks of the planes
    const long long per = (n_chunks + gridDim.x - 1) / gridDim.x;
    const long long c0 = (long long)blockIdx.x * per, c1 = min(c0 + per, n_chunks);
    f32x4 acc[SIM_NCB][2];
#pragma unroll
    for (int cb = 0; cb < SIM_NCB; cb++) acc[cb][0] = acc[cb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // LDS image of a chunk: [plane][code][32 pixels], 64-byte rows, 16-byte pieces swizzled as in codebook_sim_k; piece sp of
    // a row is pixels 8 sp .. 8 sp + 7 = half (sp & 1) of the row in 16-pixel block (sp >> 1)
    auto stage = [&](long long ch, int buf) {
        for (int q = w; q < SIM_PIECES; q += DL2_NW) {
            const int slot = 64 * q + lane;
            const int plane = slot / (SIM_NC * 4), rs = slot - plane * (SIM_NC * 4), r = rs >> 2, sp = rs & 3;
            const int piece = sp ^ ((r >> 2) & 3);
            const uint16_t* src = dplanes + (size_t)(2 * ch + (piece >> 1)) * FU_DCHUNK + ((size_t)plane * SIM_NC + r) * 16 + 8 * (piece & 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(s_a[buf] + 1024 * q), 16, 0, 0);
        }
    };
    f32x4 braw[2][2];
    auto load_b = [&](long long ch) {  // g[d = 32 w + 16 j + mm][pixels 32 ch + 8 kq .. + 7]   (HW % 4 == 0)
        const long long p = 32 * ch + 8 * kq;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float* row = g + (size_t)(32 * w + 16 * j + mm) * HW;
            braw[j][0] = *reinterpret_cast<const f32x4*>(row + min(p, HW - 4));
            braw[j][1] = *reinterpret_cast<const f32x4*>(row + min(p + 4, HW - 4));
        }
    };
    const int a_off = 64 * mm + 16 * (kq ^ ((mm >> 2) & 3));
    if (c0 < c1) {
        stage(c0, 0);
        load_b(c0);
    }
    for (long long ch = c0; ch < c1; ch++) {
        const int cur = (int)((ch - c0) & 1);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bf16x8 Bh[2], Bl[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float y[8] = {braw[j][0][0], braw[j][0][1], braw[j][0][2], braw[j][0][3],
                                braw[j][1][0], braw[j][1][1], braw[j][1][2], braw[j][1][3]};
            split_pack8(y, Bh[j], Bl[j]);
        }
        if (ch + 1 < c1) {
            stage(ch + 1, cur ^ 1);
            load_b(ch + 1);
        }
        const char* buf = s_a[cur] + a_off;
#pragma unroll
        for (int cb = 0; cb < SIM_NCB; cb++) {
            const bf16x8 Ah = *reinterpret_cast<const bf16x8*>(buf + 1024 * cb);
            const bf16x8 Al = *reinterpret_cast<const bf16x8*>(buf + 1024 * cb + SIM_PLANE_U);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                acc[cb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh[j], acc[cb][j], 0, 0, 0);
                acc[cb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl[j], acc[cb][j], 0, 0, 0);
                acc[cb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh[j], acc[cb][j], 0, 0, 0);
            }
        }
    }
    // D[code 16 cb + 4 kq + r][d = 32 w + 16 j + mm]
    float* out = partial + (size_t)blockIdx.x * SIM_NC * 256;
#pragma unroll
    for (int cb = 0; cb < SIM_NCB; cb++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[(size_t)(16 * cb + 4 * kq + r) * 256 + 32 * w + 16 * j + mm] = acc[cb][j][r];
}

int codebook_loss_waves() { return 256 * 8; }  // persistent: 8 waves per CU (2 per SIMD at ~230 VGPRs)

int launch_codebook_rows(const float* sim, const float* inv_gnorm, const float* sem, const float* W, const float* bias,
                         long long HW, int C, int S, float t, float* dsim, float* dsem, float* partials, hipStream_t s) {
    if (S < 1 || S > 16 || C < 1 || C > 512) return -1;
    CblArgs a;
    a.sim = sim; a.inv_gnorm = inv_gnorm; a.sem = sem; a.W = W; a.bias = bias; a.dsim = dsim; a.dsem = dsem;
    a.partials = partials; a.HW = HW; a.C = C; a.S = S; a.t = t;
    a.kappa = (float)(2.0 * 50.0 / ((double)HW * (double)C));
    a.inv_hw = (float)(1.0 / (double)HW);
    a.w_sl1 = 0.3f;
    const int blocks = codebook_loss_waves() / (CBL_THREADS / 64);
    const int cpl = (C + 63) / 64;
#define GOI_CASE(N)                                                                       \
    case N:                                                                               \
        codebook_rows_k<N, 16><<<dim3(blocks), dim3(CBL_THREADS), 0, s>>>(a);              \
        break;
    switch (cpl) {
        GOI_CASE(1) GOI_CASE(2) GOI_CASE(3) GOI_CASE(4) GOI_CASE(5) GOI_CASE(6) GOI_CASE(7) GOI_CASE(8)
        default: return -1;
    }
#undef GOI_CASE
    return 0;
}

size_t codebook_sim_workspace_bytes() { return (size_t)2 * SIM_NC * SIM_K * sizeof(uint16_t); }
// sim [HW][C] and inv_gnorm [HW] from g [256][HW] (channel-major) and l1 [C][256]; workspace: codebook_sim_workspace_bytes().
// Returns -1 when the shape is not the kernel's (D = 256, C <= 304, C % 4 = 0): the caller then uses the library GEMM.
int launch_codebook_sim(const float* g, const float* l1, long long HW, int C, int D, float* sim, float* inv_gnorm,
                        void* workspace, hipStream_t s) {
    if (D != SIM_K || C < 1 || C > SIM_NC || (C & 3) != 0 || HW < 1) return -1;
    uint16_t* planes = static_cast<uint16_t*>(workspace);
    codebook_split_k<<<dim3((SIM_NC * SIM_K / 2 + 255) / 256), dim3(256), 0, s>>>(l1, C, planes);
    codebook_sim_k<<<dim3((unsigned)((HW + SIM_WG_PIX - 1) / SIM_WG_PIX)), dim3(64 * SIM_NW), 0, s>>>(g, planes, HW, C, sim,
                                                                                                   inv_gnorm);
    return 0;
}
int codebook_dlut_blocks() { return 256; }  // pixel ranges; two workgroups (column halves) per range
// partial: [codebook_dlut_blocks()][304][256]; returns -1 when the shape is not the kernel's (C in 289..304,
// D = 256, HW % 4 = 0): the caller then uses a library GEMM
int launch_codebook_dlut(const float* dsim, const float* g, long long HW, int C, int D, float* partial, hipStream_t s) {
    constexpr int NCB = 19;
    if (D != 256 || C > NCB * 16 || C <= (NCB - 1) * 16 || (HW & 3) != 0) return -1;
    const size_t lds = (size_t)2 * DL_KP * (NCB * 16 + 4) * sizeof(float);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(codebook_dlut_k<NCB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    codebook_dlut_k<NCB><<<dim3(2 * codebook_dlut_blocks()), dim3(DL_THREADS), lds, s>>>(dsim, g, HW, C, partial);
    return 0;
}

// ---- the training half in one call.  workspace: code-book planes | decoder images | per-pixel records | simgrad wave sums |
// dsim planes (the only large part: 2 x 2 B per (pixel, code))
static long long fu_blocks(long long HW) { return (HW + FU_WG_PIX - 1) / FU_WG_PIX * (FU_WG_PIX / 16); }
static long long fu_simgrad_wgs(long long HW) { return (HW + FU_WG_PIX - 1) / FU_WG_PIX; }
// the pieces land in the kernels' argument block (the per-pixel records, the simgrad sums, both sets of planes)
static size_t fused_layout(long long HW, void* base, FusedArgs* v) {
    const size_t blocks = (size_t)fu_blocks(HW), npad = 16 * blocks;
    Carver c(base);
    FusedArgs a{};
    a.planes = c.take<uint16_t>((size_t)2 * SIM_NC * SIM_K);
    a.wz = c.take<uint16_t>(FU_WZ_BYTES / 2);
    a.wt = c.take<uint16_t>(FU_WT_BYTES / 2);
    a.r_mz = c.take<float>(npad);
    a.r_rzp = c.take<float>(npad);
    a.r_p2 = c.take<float>(npad);
    a.r_nl = c.take<float>(npad);
    a.r_arga = c.take<int>(npad);
    a.r_args = c.take<int>(npad);
    a.r_tie = c.take<uint32_t>(npad * FU_TIE_WORDS);
    a.n_sums_a = (int)(fu_simgrad_wgs(HW) * SG_NW);
    a.sums_a = c.take<float>((size_t)a.n_sums_a * 4);
    a.dplanes = c.take<uint16_t>(blocks * FU_DCHUNK);  // (the last and only large piece: 2 x 2 B per (pixel, code); not padded)
    if (v) *v = a;
    return c.end();
}
size_t codebook_fused_workspace_bytes(long long HW) { return fused_layout(HW, nullptr, nullptr); }
int codebook_fused_rows() { return 256 * GD_NW; }
// returns -1 when the shape is not the kernels' (D = 256, C in 289..304, S <= 16, HW % 4 = 0, HW < 2^25)
int launch_codebook_fused(const float* g, const float* l1, const float* sem, const float* W, const float* bias, long long HW,
                          int C, int D, int S, float t, float* dsem, float* partials, float* dl1_partial, void* workspace,
                          hipStream_t s) {
    if (D != SIM_K || C > SIM_NC || C <= SIM_NC - 16 || S < 1 || S > 16 || HW < 4 || (HW & 3) != 0 || HW >= (1ll << 25)) return -1;
    const long long blocks = fu_blocks(HW);
    FusedArgs a;
    fused_layout(HW, workspace, &a);
    // (the two split kernels write the operand images every later kernel only reads)
    codebook_split_k<<<dim3((SIM_NC * SIM_K / 2 + 255) / 256), dim3(256), 0, s>>>(l1, C, const_cast<uint16_t*>(a.planes));
    decoder_split_k<<<dim3((FU_NJ * 32 * 16 + 255) / 256), dim3(256), 0, s>>>(W, C, S, const_cast<uint16_t*>(a.wz),
                                                                             const_cast<uint16_t*>(a.wt));
    a.g = g; a.bias = bias; a.sem = sem; a.dsem = dsem;
    a.partials = partials; a.HW = HW; a.blocks = blocks; a.C = C; a.S = S; a.t = t;
    a.kappa = (float)(2.0 * 50.0 / ((double)HW * (double)C));
    a.inv_hw = (float)(1.0 / (double)HW);
    a.w_sl1 = 0.3f;
    const long long stat_wgs = (blocks + DS_NW - 1) / DS_NW;
    decoder_stats_k<<<dim3((unsigned)(stat_wgs < 2048 ? stat_wgs : 2048)), dim3(64 * DS_NW), 0, s>>>(a);
    codebook_simgrad_k<<<dim3((unsigned)fu_simgrad_wgs(HW)), dim3(64 * SG_NW), 0, s>>>(a);
    decoder_gd_k<<<dim3(codebook_fused_rows() / GD_NW), dim3(64 * GD_NW), 0, s>>>(a);
    codebook_dlut2_k<<<dim3(codebook_dlut_blocks()), dim3(64 * DL2_NW), 0, s>>>(a.dplanes, g, HW, dl1_partial);
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_codebook_loss_partial_rows(void) { return codebook_loss_waves(); }

int goi_codebook_loss_rows(const float* sim_raw, const float* inv_gnorm, const float* sem, const float* W,
                           const float* bias, long long HW, int C, int S, float t, float* dsim, float* dsem,
                           float* partials, void* stream) {
    if (HW < 0) return fail("goi_codebook_loss_rows: bad HW");
    if (!sim_raw || !inv_gnorm || !sem || !W || !dsim || !dsem || !partials)
        return fail("goi_codebook_loss_rows: a required pointer is NULL");
    if (launch_codebook_rows(sim_raw, inv_gnorm, sem, W, bias, HW, C, S, t, dsim, dsem, partials,
                             static_cast<hipStream_t>(stream)) < 0)
        return fail("goi_codebook_loss_rows: supported sizes are 1 <= S <= 16, 1 <= C <= 512");
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_codebook_sim_workspace_bytes(void) { return codebook_sim_workspace_bytes(); }

int goi_codebook_sim(const float* g, const float* lut1, long long HW, int C, int D, float* sim, float* inv_gnorm,
                     void* workspace, void* stream) {
    if (!g || !lut1 || !sim || !inv_gnorm || !workspace) return fail("goi_codebook_sim: a required pointer is NULL");
    if (launch_codebook_sim(g, lut1, HW, C, D, sim, inv_gnorm, workspace, static_cast<hipStream_t>(stream)) < 0)
        return fail("goi_codebook_sim: supported shape is D = 256, C <= 304, C % 4 = 0");
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_codebook_dlut_partial_blocks(void) { return codebook_dlut_blocks(); }

int goi_codebook_dlut(const float* dsim, const float* g, long long HW, int C, int D, float* partial, void* stream) {
    if (!dsim || !g || !partial || HW < 0) return fail("goi_codebook_dlut: bad arguments");
    if (launch_codebook_dlut(dsim, g, HW, C, D, partial, static_cast<hipStream_t>(stream)) < 0)
        return fail("goi_codebook_dlut: supported shape is D = 256, 288 < C <= 304, HW % 4 = 0");
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_codebook_fused_workspace_bytes(long long HW) { return HW < 0 ? 0 : codebook_fused_workspace_bytes(HW); }
int goi_codebook_fused_partial_rows(void) { return codebook_fused_rows(); }

int goi_codebook_fused(const float* g, const float* lut1, const float* sem, const float* W, const float* bias, long long HW,
                       int C, int D, int S, float t, float* dsem, float* partials, float* dlut_partial, void* workspace,
                       void* stream) {
    if (!g || !lut1 || !sem || !W || !dsem || !partials || !dlut_partial) return fail("goi_codebook_fused: a required pointer is NULL");
    if (check_workspace("goi_codebook_fused", workspace) < 0) return -1;  // (its layout carves from a 256-byte aligned base)
    if (launch_codebook_fused(g, lut1, sem, W, bias, HW, C, D, S, t, dsem, partials, dlut_partial, workspace,
                              static_cast<hipStream_t>(stream)) < 0)
        return fail("goi_codebook_fused: supported shape is D = 256, 288 < C <= 304, 1 <= S <= 16, HW % 4 = 0, HW < 2^25");
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
