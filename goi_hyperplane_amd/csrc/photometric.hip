// Photometric loss of 3DGS training (the reference's utils/loss_utils.py, used at train.py:137-140) and the image metrics
// of training_report / metrics.py, on the device: L1, SSIM (loss_utils._ssim restated exactly) and PSNR
// (utils/image_utils.psnr) of [N][C][H][W] fp32 batches, and the gradient of (1 - lambda) L1 + lambda (1 - SSIM).
//
// SSIM's 11x11 window is the outer product of the fp32 1-D Gaussian (sigma 1.5, normalised in fp32), applied with zero
// padding of 5 per (image, channel) plane, so every filter here is separable: a horizontal pass into LDS, then a
// vertical pass.  sigma^2 = E[x^2] - mu^2 as the reference computes it; C1 = 0.01^2, C2 = 0.03^2 (rounded to fp32).
//
//   photo_fwd_k       one workgroup per 32x32 output tile of one plane.  Stages the tile of x and y with its 5-pixel
//                     halo (zero outside the plane), filters mu1, mu2, E[x^2], E[y^2], E[xy], forms the SSIM map value
//                     S and, when a gradient is wanted, the partials of S that the backward filters:
//                       P_mu1 = dS/dmu1, P_mu2 = dS/dmu2 (only when img2 needs a gradient),
//                       P_xx = dS/dE[x^2] = dS/dE[y^2],  P_xy = dS/dE[xy].
//                     It writes the tile's sums of S, |x-y| and (x-y)^2 (fp32, fixed wave/LDS tree) as block partials.
//   photo_reduce_k    one workgroup per image: the image's block partials summed in fp64 in a fixed order; per-image
//                     SSIM, L1 and PSNR; for a batch of one, also the totals (the loss).
//   photo_total_k     one workgroup: the per-image fp64 sums in a fixed order -> the totals (batches of more than one).
//   photo_bwd_k       one workgroup per 32x32 tile: the adjoint of the zero-padded window (the same separable filter,
//                     the window being symmetric) applied to the partial maps on a 5-pixel halo, then
//                       dL/dx = g/M * [ ks * (w*P_mu1 + 2x w*P_xx + y w*P_xy) + kl * sign(x - y) ]
//                       dL/dy = g/M * [ ks * (w*P_mu2 + 2y w*P_xx + x w*P_xy) - kl * sign(x - y) ]
//                     with ks = -lambda, kl = 1 - lambda for the loss, ks = 1, kl = 0 for SSIM itself.  The upstream
//                     gradient g is read from device memory.
// No float atomics anywhere: two calls give the same bits.  Nothing synchronises the host.
// C entries, with the limits they enforce, at the end of the file: goi_raster_photometric_* (declared in include/goi_raster.h).
#include <climits>
#include <cmath>

#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int PHOTO_RADIUS = GOI_PHOTOMETRIC_WINDOW / 2;  // the only window instantiated
constexpr int PH_TW = 32, PH_TH = 32;  // output tile
constexpr int PH_THREADS = 256;
constexpr int PH_WAVES = PH_THREADS / WAVE;
constexpr int PH_ROWS_PER_THREAD = PH_TW * PH_TH / PH_THREADS;  // 4: thread = column tid % 32, rows tid / 32 + 8 j
constexpr int PH_RED_THREADS = 256;

struct PhotoWin {
    float w[2 * PHOTO_RADIUS + 1];
};

struct PhotoMaps {  // the partial maps of one call, [N][C][H][W] each; NULL when not stored
    float* mu1;
    float* mu2;
    float* xx;
    float* xy;
};

template <int R>
__global__ void __launch_bounds__(PH_THREADS) photo_fwd_k(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                          int tiles_x, int tiles_per_plane, PhotoWin win, PhotoMaps maps,
                                                          float* __restrict__ partials) {
    constexpr int K = 2 * R + 1, SW = PH_TW + 2 * R, SH = PH_TH + 2 * R;
    __shared__ float xs[SH * SW], ys[SH * SW];
    __shared__ float hq[5][SH * PH_TW];
    __shared__ float red[3][PH_WAVES];
    const int tid = threadIdx.x;
    const long long bid = blockIdx.x;
    const long long plane = bid / tiles_per_plane;
    const int t = (int)(bid - plane * tiles_per_plane);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const size_t base = (size_t)plane * (size_t)H * (size_t)W;
    const int gx0 = tx * PH_TW, gy0 = ty * PH_TH;

    for (int i = tid; i < SH * SW; i += PH_THREADS) {
        const int r = i / SW, c = i - r * SW;
        const int gy = gy0 - R + r, gx = gx0 - R + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = base + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
        xs[i] = in ? x[o] : 0.f;
        ys[i] = in ? y[o] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SH * PH_TW; i += PH_THREADS) {
        const int r = i / PH_TW, c = i - r * PH_TW;
        float m1 = 0.f, m2 = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float a = xs[r * SW + c + k], b = ys[r * SW + c + k], wk = win.w[k];
            m1 += wk * a;
            m2 += wk * b;
            sxx += wk * (a * a);
            syy += wk * (b * b);
            sxy += wk * (a * b);
        }
        hq[0][i] = m1;
        hq[1][i] = m2;
        hq[2][i] = sxx;
        hq[3][i] = syy;
        hq[4][i] = sxy;
    }
    __syncthreads();

    const double C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);  // the reference's constants, rounded to fp32
    const int c = tid % PH_TW;
    float acc_s = 0.f, acc_a = 0.f, acc_q = 0.f;
#pragma unroll
    for (int j = 0; j < PH_ROWS_PER_THREAD; ++j) {
        const int r = tid / PH_TW + j * (PH_THREADS / PH_TW);
        const int gy = gy0 + r, gx = gx0 + c;
        if (gy >= H || gx >= W) continue;
        float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) f[q] += wk * hq[q][(r + k) * PH_TW + c];
        }
        // the per-pixel algebra in fp64 from the fp32 filter outputs: the partials cancel (A2 - A1, B2 - B1) and reach
        // 1e2..1e3 on small planes, where fp32 here alone cost several ulps of the gradient
        const double mu1 = f[0], mu2 = f[1];
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const double s11 = f[2] - mu1_sq, s22 = f[3] - mu2_sq, s12 = f[4] - mu1_mu2;
        const double A1 = 2.0 * mu1_mu2 + C1, A2 = 2.0 * s12 + C2;
        const double B1 = mu1_sq + mu2_sq + C1, B2 = s11 + s22 + C2;
        const double inv = 1.0 / (B1 * B2);
        const double S = A1 * A2 * inv;
        const size_t o = base + (size_t)gy * W + gx;
        if (maps.xx) {
            const double dA = A2 - A1, dB = S * (B2 - B1);
            if (maps.mu1) maps.mu1[o] = (float)(2.0 * inv * (mu2 * dA - mu1 * dB));
            if (maps.mu2) maps.mu2[o] = (float)(2.0 * inv * (mu1 * dA - mu2 * dB));
            maps.xx[o] = (float)(-S / B2);
            maps.xy[o] = (float)(2.0 * A1 * inv);
        }
        const float d = xs[(r + R) * SW + c + R] - ys[(r + R) * SW + c + R];
        acc_s += (float)S;
        acc_a += fabsf(d);
        acc_q += d * d;
    }
    acc_s = wave_sum(acc_s);
    acc_a = wave_sum(acc_a);
    acc_q = wave_sum(acc_q);
    if (tid % WAVE == 0) {
        red[0][tid / WAVE] = acc_s;
        red[1][tid / WAVE] = acc_a;
        red[2][tid / WAVE] = acc_q;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < PH_WAVES; ++w) s += red[tid][w];
        partials[bid * 3 + tid] = s;
    }
}

// Block-wide fp64 sum in a fixed tree order; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid % WAVE == 0) lds[tid / WAVE] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < PH_RED_THREADS / WAVE; ++w) s += lds[w];
    return s;
}

__device__ __forceinline__ void write_totals(double s, double a, double n_elems, float kl, float ks, float* out) {
    const float l1 = (float)(a / n_elems), ssim = (float)(s / n_elems);
    out[0] = kl * l1 + ks * (1.f - ssim);
    out[1] = l1;
    out[2] = ssim;
}

__global__ void __launch_bounds__(PH_RED_THREADS) photo_reduce_k(const float* __restrict__ partials, int blocks_per_image,
                                                                 double elems_per_image, float kl, float ks,
                                                                 double* __restrict__ image_sums, float* __restrict__ out,
                                                                 float* __restrict__ out_images) {
    __shared__ double lds[PH_RED_THREADS / WAVE];
    const long long n = blockIdx.x;
    const float* p = partials + n * blocks_per_image * 3;
    double s = 0.0, a = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < blocks_per_image; b += PH_RED_THREADS) {
        s += (double)p[b * 3 + 0];
        a += (double)p[b * 3 + 1];
        q += (double)p[b * 3 + 2];
    }
    s = block_sum(s, lds);
    a = block_sum(a, lds);
    q = block_sum(q, lds);
    if (threadIdx.x != 0) return;
    image_sums[n * 3 + 0] = s;
    image_sums[n * 3 + 1] = a;
    image_sums[n * 3 + 2] = q;
    if (out_images) {
        const long long N = gridDim.x;
        out_images[n] = (float)(s / elems_per_image);
        out_images[N + n] = (float)(a / elems_per_image);
        out_images[2 * N + n] = (float)(20.0 * log10(1.0 / sqrt(q / elems_per_image)));  // utils/image_utils.psnr
    }
    if (gridDim.x == 1) write_totals(s, a, elems_per_image, kl, ks, out);
}

__global__ void __launch_bounds__(PH_RED_THREADS) photo_total_k(const double* __restrict__ image_sums, long long N,
                                                                double n_elems, float kl, float ks, float* __restrict__ out) {
    __shared__ double lds[PH_RED_THREADS / WAVE];
    double s = 0.0, a = 0.0;
    for (long long n = threadIdx.x; n < N; n += PH_RED_THREADS) {
        s += image_sums[n * 3 + 0];
        a += image_sums[n * 3 + 1];
    }
    s = block_sum(s, lds);
    a = block_sum(a, lds);
    if (threadIdx.x == 0) write_totals(s, a, n_elems, kl, ks, out);
}

// G1 / G2: gradient of img1 / img2 wanted.  Maps staged: P_xx, P_xy, then P_mu1 (G1) and P_mu2 (G2).
template <int R, bool G1, bool G2>
__global__ void __launch_bounds__(PH_THREADS) photo_bwd_k(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                          int tiles_x, int tiles_per_plane, int planes_per_grad, PhotoWin win,
                                                          PhotoMaps maps, const float* __restrict__ grad_out, float inv_m,
                                                          float ks, float kl, float* __restrict__ gx_out,
                                                          float* __restrict__ gy_out) {
    constexpr int K = 2 * R + 1, SW = PH_TW + 2 * R, SH = PH_TH + 2 * R;
    constexpr int NM = 2 + (G1 ? 1 : 0) + (G2 ? 1 : 0);
    __shared__ float ms[NM][SH * SW];
    __shared__ double hq[NM][SH * PH_TW];  // fp64 filter: see the comment at the combination below
    const int tid = threadIdx.x;
    const long long bid = blockIdx.x;
    const long long plane = bid / tiles_per_plane;
    const int t = (int)(bid - plane * tiles_per_plane);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const size_t base = (size_t)plane * (size_t)H * (size_t)W;
    const int gx0 = tx * PH_TW, gy0 = ty * PH_TH;
    const float* src[NM];
    src[0] = maps.xx;
    src[1] = maps.xy;
    if constexpr (G1) src[2] = maps.mu1;
    if constexpr (G2) src[NM - 1] = maps.mu2;

    for (int i = tid; i < SH * SW; i += PH_THREADS) {
        const int r = i / SW, c = i - r * SW;
        const int gy = gy0 - R + r, gx = gx0 - R + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = base + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
#pragma unroll
        for (int q = 0; q < NM; ++q) ms[q][i] = in ? src[q][o] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SH * PH_TW; i += PH_THREADS) {
        const int r = i / PH_TW, c = i - r * PH_TW;
        double f[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) f[q] = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double wk = win.w[k];
#pragma unroll
            for (int q = 0; q < NM; ++q) f[q] += wk * ms[q][r * SW + c + k];
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) hq[q][i] = f[q];
    }
    __syncthreads();

    const float g = grad_out[plane / planes_per_grad] * inv_m;
    const float gs = g * ks, gl = g * kl;
    const int c = tid % PH_TW;
#pragma unroll
    for (int j = 0; j < PH_ROWS_PER_THREAD; ++j) {
        const int r = tid / PH_TW + j * (PH_THREADS / PH_TW);
        const int gy = gy0 + r, gxx = gx0 + c;
        if (gy >= H || gxx >= W) continue;
        // The three filtered partials are ~1e2..1e3 on small planes and cancel in the sum below; filtered and combined
        // in fp32 the result was off by several ulps, so the filter and the combination run in fp64.
        double f[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) f[q] = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double wk = win.w[k];
#pragma unroll
            for (int q = 0; q < NM; ++q) f[q] += wk * hq[q][(r + k) * PH_TW + c];
        }
        const size_t o = base + (size_t)gy * W + gxx;
        const float a = x[o], b = y[o];
        const float d = a - b;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        if constexpr (G1) gx_out[o] = (float)(gs * (f[2] + 2.0 * a * f[0] + b * f[1])) + gl * sg;
        if constexpr (G2) gy_out[o] = (float)(gs * (f[NM - 1] + 2.0 * b * f[0] + a * f[1])) - gl * sg;
    }
}

struct PhotoView {
    float* partials;     // [n c tiles][3]
    double* image_sums;  // [n][3]
    PhotoMaps maps;      // xx, xy and the mean of every image whose gradient is wanted; all NULL when no gradient is
};

size_t photo_layout(long long n, int c, int h, int w, unsigned flags, void* base, PhotoView* v) {
    const long long tiles = (long long)((w + PH_TW - 1) / PH_TW) * ((h + PH_TH - 1) / PH_TH);
    const size_t numel = (size_t)n * c * h * w;
    Carver cv(base);
    PhotoView t;
    t.partials = cv.take<float>((size_t)n * c * tiles * 3);
    t.image_sums = cv.take<double>((size_t)n * 3);
    t.maps = {nullptr, nullptr, nullptr, nullptr};
    if (flags & (GOI_PHOTOMETRIC_GRAD1 | GOI_PHOTOMETRIC_GRAD2)) {
        t.maps.xx = cv.take<float>(numel);
        t.maps.xy = cv.take<float>(numel);
        if (flags & GOI_PHOTOMETRIC_GRAD1) t.maps.mu1 = cv.take<float>(numel);
        if (flags & GOI_PHOTOMETRIC_GRAD2) t.maps.mu2 = cv.take<float>(numel);
    }
    if (v) *v = t;
    return cv.bytes();
}

// loss_utils.gaussian(11, 1.5): exp() in double, rounded to fp32, divided by their fp32 sum.  The sum is the correctly
// rounded one (as torch's gives for these 11 values); a sequential fp32 sum is 1 ulp off, which moves every weight and
// the gradient of a plane smaller than the window by several ulps.
PhotoWin photo_window() {
    PhotoWin win;
    double sum = 0.0;
    for (int i = 0; i < 2 * PHOTO_RADIUS + 1; ++i) {
        const double d = i - PHOTO_RADIUS;
        win.w[i] = (float)std::exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += win.w[i];
    }
    for (int i = 0; i < 2 * PHOTO_RADIUS + 1; ++i) win.w[i] /= (float)sum;
    return win;
}

size_t photometric_workspace_bytes(long long n, int c, int h, int w, unsigned flags) {
    return photo_layout(n, c, h, w, flags, nullptr, nullptr);
}

void launch_photometric_forward(const float* x, const float* y, long long n, int c, int h, int w, float lambda, unsigned flags,
                                float* out, float* out_images, void* ws, hipStream_t s) {
    PhotoView v;
    photo_layout(n, c, h, w, flags, ws, &v);
    const int tiles_x = (w + PH_TW - 1) / PH_TW, tiles = tiles_x * ((h + PH_TH - 1) / PH_TH);
    const long long blocks = n * c * tiles;
    photo_fwd_k<PHOTO_RADIUS><<<dim3((unsigned)blocks), PH_THREADS, 0, s>>>(x, y, h, w, tiles_x, tiles, photo_window(), v.maps,
                                                                            v.partials);
    const float kl = (float)(1.0 - (double)lambda), ks = lambda;
    const double per_image = (double)c * h * w;
    photo_reduce_k<<<dim3((unsigned)n), PH_RED_THREADS, 0, s>>>(v.partials, c * tiles, per_image, kl, ks, v.image_sums, out,
                                                                 out_images);
    if (n > 1) photo_total_k<<<1, PH_RED_THREADS, 0, s>>>(v.image_sums, n, per_image * n, kl, ks, out);
}

void launch_photometric_backward(const float* x, const float* y, long long n, int c, int h, int w, float lambda, unsigned flags,
                                 const float* grad_out, const void* ws, float* gx, float* gy, hipStream_t s) {
    const unsigned fwd_flags = flags & (GOI_PHOTOMETRIC_GRAD1 | GOI_PHOTOMETRIC_GRAD2);
    PhotoView v;
    photo_layout(n, c, h, w, fwd_flags, const_cast<void*>(ws), &v);
    const PhotoMaps& maps = v.maps;
    const int tiles_x = (w + PH_TW - 1) / PH_TW, tiles = tiles_x * ((h + PH_TH - 1) / PH_TH);
    const long long blocks = n * c * tiles;
    const bool per_image = flags & GOI_PHOTOMETRIC_PER_IMAGE;
    const bool ssim_only = flags & GOI_PHOTOMETRIC_SSIM_ONLY;
    const float inv_m = (float)(1.0 / ((double)c * h * w * (per_image ? 1 : n)));
    const int planes_per_grad = per_image ? c : INT_MAX;
    const float ks = ssim_only ? 1.f : -lambda, kl = ssim_only ? 0.f : (float)(1.0 - (double)lambda);
    const PhotoWin win = photo_window();
    const dim3 grid((unsigned)blocks);
    if ((flags & GOI_PHOTOMETRIC_GRAD1) && (flags & GOI_PHOTOMETRIC_GRAD2))
        photo_bwd_k<PHOTO_RADIUS, true, true><<<grid, PH_THREADS, 0, s>>>(x, y, h, w, tiles_x, tiles, planes_per_grad, win, maps,
                                                                           grad_out, inv_m, ks, kl, gx, gy);
    else if (flags & GOI_PHOTOMETRIC_GRAD1)
        photo_bwd_k<PHOTO_RADIUS, true, false><<<grid, PH_THREADS, 0, s>>>(x, y, h, w, tiles_x, tiles, planes_per_grad, win, maps,
                                                                            grad_out, inv_m, ks, kl, gx, gy);
    else
        photo_bwd_k<PHOTO_RADIUS, false, true><<<grid, PH_THREADS, 0, s>>>(x, y, h, w, tiles_x, tiles, planes_per_grad, win, maps,
                                                                            grad_out, inv_m, ks, kl, gx, gy);
}

// the shape limits of goi_raster_photometric_*: "" when the call may go ahead
std::string photometric_check(long long n, int c, int h, int w, int window_size) {
    if (window_size != GOI_PHOTOMETRIC_WINDOW) return "window_size " + std::to_string(window_size) + " is not supported (only 11)";
    if (n < 1 || c < 1 || h < 1 || w < 1) return "need n, c, h, w >= 1";
    if ((long long)h * w >= (1ll << 31)) return "need h * w < 2^31";
    if (n * c * ((h + 31) / 32) * (long long)((w + 31) / 32) >= (1ll << 31)) return "need n * c * ceil(h/32) * ceil(w/32) < 2^31";
    return "";
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_raster_photometric_workspace_bytes(long long n, int c, int h, int w, unsigned flags) {
    if (!photometric_check(n, c, h, w, GOI_PHOTOMETRIC_WINDOW).empty()) return 0;
    return photometric_workspace_bytes(n, c, h, w, flags & (GOI_PHOTOMETRIC_GRAD1 | GOI_PHOTOMETRIC_GRAD2));
}

int goi_raster_photometric_forward(const float* img1, const float* img2, long long n, int c, int h, int w, int window_size,
                                   float lambda_dssim, unsigned flags, float* out, float* out_images, void* workspace, void* stream) {
    const std::string fn = "goi_raster_photometric_forward: ";
    const std::string bad = photometric_check(n, c, h, w, window_size);
    if (!bad.empty()) return fail(fn + bad);
    if (!img1 || !img2 || !out) return fail(fn + "a required pointer is NULL");
    if (check_workspace("goi_raster_photometric_forward", workspace) < 0) return -1;
    launch_photometric_forward(img1, img2, n, c, h, w, lambda_dssim, flags & (GOI_PHOTOMETRIC_GRAD1 | GOI_PHOTOMETRIC_GRAD2), out,
                               out_images, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_photometric_backward(const float* img1, const float* img2, long long n, int c, int h, int w, int window_size,
                                    float lambda_dssim, unsigned flags, const float* grad_out, const void* workspace, float* grad1,
                                    float* grad2, void* stream) {
    const std::string fn = "goi_raster_photometric_backward: ";
    const std::string bad = photometric_check(n, c, h, w, window_size);
    if (!bad.empty()) return fail(fn + bad);
    if (!(flags & (GOI_PHOTOMETRIC_GRAD1 | GOI_PHOTOMETRIC_GRAD2))) return fail(fn + "no gradient asked for");
    if (!img1 || !img2 || !grad_out || ((flags & GOI_PHOTOMETRIC_GRAD1) && !grad1) || ((flags & GOI_PHOTOMETRIC_GRAD2) && !grad2))
        return fail(fn + "a required pointer is NULL");
    if (check_workspace("goi_raster_photometric_backward", workspace) < 0) return -1;
    launch_photometric_backward(img1, img2, n, c, h, w, lambda_dssim, flags, grad_out, workspace, grad1, grad2,
                                static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
