// Texture bake for a triangle mesh on the device: a z-buffer triangle rasterizer, the per-pixel
// resolve of uv / normal / colour, the mip-mapped bilinear grid put, the per-view accumulation and the margin fill.
// gfx950 only; compiled with -ffp-contract=off: every float operation below is rounded once, in the order written, as the
// numpy restatement of tests/texture_reference.py is.
//
// Shared properties: no float is accumulated with atomics (the only atomics are a 64-bit integer min, an integer counter and
// integer ORs, all order-independent), so two runs give the same bits; stages are separated by kernel boundaries, nothing
// spins on another workgroup; nothing is read back.
//
//   rasterize    tex_raster_wave_k: one wave per face, a lane per pixel of its clipped bounding box (boxes over
//                TEX_WAVE_PIXELS go to a list); tex_raster_large_k: the listed faces, a slice of workgroups per face.  Both
//                atomicMin (orderable depth bits << 32 | face) into [H][W] words.  tex_raster_shade_k: one lane per pixel
//                recomputes the winner's barycentrics.
//   resolve      one lane per pixel: uv, normal, view cosine, mask, grid coordinates, colour.
//   grid put     per level: tex_splat_key_k writes (texel, tap * N + sample) for the 4 N taps, a stable radix sort leaves each
//                texel's taps adjacent in ascending (tap, sample) order -- the order of the reference's four sequential
//                scatter_adds -- tex_segment_k sums each run with one lane, tex_compose_k upsamples the level and adds it
//                where the running count is 0 (and, on the last level, folds the view into the accumulated texture and,
//                for a bake's last view, normalizes that).
//   fill         tex_fill_columns_k: per texel the nearest mask texel above / below within the radius; tex_fill_nearest_k:
//                the minimum over the 2 R + 1 columns of (dx^2 + dy^2, row, column), the L1 test carried along.
// C entries, with the limits they enforce, at the end of the file: goi_texture_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

#include <math.h>

namespace goi {
namespace {

constexpr int TEX_THREADS = 256;
constexpr long long TEX_WAVE_PIXELS = 1024;  // a larger clipped box goes to tex_raster_large_k
constexpr int TEX_LARGE_X = 64, TEX_LARGE_Y = 16;
constexpr unsigned long long TEX_EMPTY = ~0ull;
constexpr int TEX_SUB = 256;             // sub-pixel positions per pixel
constexpr float TEX_MAX_SCREEN = 1048576.f;  // |screen position| beyond this: the face is skipped (keeps every product in 64 bits)
constexpr uint8_t TEX_FAR = 255;

unsigned tblocks(long long n) { return (unsigned)((n + TEX_THREADS - 1) / TEX_THREADS); }
__device__ __forceinline__ long long tgid() { return (long long)blockIdx.x * TEX_THREADS + threadIdx.x; }
int tbits_for(uint32_t limit) { return limit == 0 ? 1 : 32 - __builtin_clz(limit); }

// ---- rasterize -------------------------------------------------------------------------------------------------------------
struct TriSetup {
    long long X[3], Y[3], area;  // 1/256-pixel positions; area = |twice the signed area|
    int sgn;
    float z[3], w[3];
    int x0, x1, y0, y1;  // the clipped box of pixel centres (empty when x1 < x0 or y1 < y0)
};

// false: the face draws nothing (an index out of range, a w <= 0, a position that is not finite or too far, no area)
__device__ __forceinline__ bool tex_setup(const float* __restrict__ vclip, const int* __restrict__ faces, long long f, uint32_t V,
                                          int H, int W, TriSetup& t, uint32_t* status) {
    for (int k = 0; k < 3; k++) {
        const uint32_t i = (uint32_t)faces[3 * f + k];
        if (i >= V) {
            if (status) atomicOr(status, (uint32_t)GOI_TEXTURE_STATUS_RANGE);
            return false;
        }
        const float x = vclip[4 * (size_t)i], y = vclip[4 * (size_t)i + 1];
        t.z[k] = vclip[4 * (size_t)i + 2];
        t.w[k] = vclip[4 * (size_t)i + 3];
        if (!(t.w[k] > 0.f)) return false;
        const float sx = ((x / t.w[k] + 1.f) * (float)W - 1.f) * 0.5f;
        const float sy = ((y / t.w[k] + 1.f) * (float)H - 1.f) * 0.5f;
        if (!(fabsf(sx) <= TEX_MAX_SCREEN) || !(fabsf(sy) <= TEX_MAX_SCREEN)) return false;
        t.X[k] = (long long)rintf(sx * (float)TEX_SUB);
        t.Y[k] = (long long)rintf(sy * (float)TEX_SUB);
    }
    const long long a2 = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    if (a2 == 0) return false;
    t.sgn = a2 < 0 ? -1 : 1;
    t.area = a2 < 0 ? -a2 : a2;
    long long lx = t.X[0], hx = t.X[0], ly = t.Y[0], hy = t.Y[0];
    for (int k = 1; k < 3; k++) {
        lx = t.X[k] < lx ? t.X[k] : lx;
        hx = t.X[k] > hx ? t.X[k] : hx;
        ly = t.Y[k] < ly ? t.Y[k] : ly;
        hy = t.Y[k] > hy ? t.Y[k] : hy;
    }
    const long long px0 = (lx + TEX_SUB - 1) >> 8, px1 = hx >> 8, py0 = (ly + TEX_SUB - 1) >> 8, py1 = hy >> 8;  // ceil, floor
    t.x0 = (int)(px0 < 0 ? 0 : px0);
    t.x1 = (int)(px1 > W - 1 ? W - 1 : px1);
    t.y0 = (int)(py0 < 0 ? 0 : py0);
    t.y1 = (int)(py1 > H - 1 ? H - 1 : py1);
    return true;
}

// the three edge functions at a pixel centre, oriented so that inside is >= 0; e[k] belongs to vertex k (the edge opposite).
// Top-left rule: a centre exactly on an edge is in when the oriented edge has dy > 0, or dy == 0 and dx < 0 -- of the two
// faces that share an edge exactly one takes it.
__device__ __forceinline__ bool tex_cover(const TriSetup& t, int px, int py, long long e[3]) {
    const long long Px = (long long)px * TEX_SUB, Py = (long long)py * TEX_SUB;
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const long long dx = (t.X[b] - t.X[a]) * t.sgn, dy = (t.Y[b] - t.Y[a]) * t.sgn;
        e[k] = dx * (Py - t.Y[a]) - dy * (Px - t.X[a]);
        if (e[k] < 0) return false;
        if (e[k] == 0 && !(dy > 0 || (dy == 0 && dx < 0))) return false;
    }
    return true;
}

// perspective-correct barycentrics (u, v) of vertices 0 and 1, and the depth z / w interpolated with them
__device__ __forceinline__ void tex_shade(const TriSetup& t, const long long e[3], float& u, float& v, float& zw) {
    const float A = (float)t.area;
    const float s0 = (float)e[0] / A, s1 = (float)e[1] / A, s2 = (float)e[2] / A;
    const float p0 = s0 / t.w[0], p1 = s1 / t.w[1], p2 = s2 / t.w[2];
    const float sum = (p0 + p1) + p2;
    u = p0 / sum;
    v = p1 / sum;
    const float r = (1.f - u) - v;
    const float zi = (u * t.z[0] + v * t.z[1]) + r * t.z[2];
    const float wi = (u * t.w[0] + v * t.w[1]) + r * t.w[2];
    zw = zi / wi;
}

__device__ __forceinline__ void tex_draw(const TriSetup& t, uint32_t f, int px, int py, int W, unsigned long long* __restrict__ zbuf) {
    long long e[3];
    if (!tex_cover(t, px, py, e)) return;
    float u, v, zw;
    tex_shade(t, e, u, v, zw);
    if (!(zw == zw)) return;  // a depth that is not a number draws nothing
    atomicMin(zbuf + (size_t)py * W + px, ((unsigned long long)ord_enc(zw) << 32) | f);
}

__global__ void __launch_bounds__(TEX_THREADS) tex_raster_wave_k(long long F, uint32_t V, const float* __restrict__ vclip,
                                                                const int* __restrict__ faces, int H, int W,
                                                                unsigned long long* __restrict__ zbuf, uint32_t* __restrict__ large,
                                                                uint32_t* __restrict__ n_large, uint32_t* __restrict__ status) {
    const long long f = (long long)blockIdx.x * (TEX_THREADS / 64) + (threadIdx.x >> 6);  // one wave per face
    if (f >= F) return;
    const int lane = threadIdx.x & 63;
    TriSetup t;
    if (!tex_setup(vclip, faces, f, V, H, W, t, lane == 0 ? status : nullptr)) return;
    if (t.x1 < t.x0 || t.y1 < t.y0) return;
    const int bw = t.x1 - t.x0 + 1;
    const long long npix = (long long)bw * (t.y1 - t.y0 + 1);
    if (npix > TEX_WAVE_PIXELS) {
        if (lane == 0) large[atomicAdd(n_large, 1u)] = (uint32_t)f;  // (the list's order does not matter: the min is order-free)
        return;
    }
    for (long long i = lane; i < npix; i += 64) tex_draw(t, (uint32_t)f, t.x0 + (int)(i % bw), t.y0 + (int)(i / bw), W, zbuf);
}

__global__ void __launch_bounds__(TEX_THREADS) tex_raster_large_k(uint32_t V, const float* __restrict__ vclip,
                                                                 const int* __restrict__ faces, int H, int W,
                                                                 unsigned long long* __restrict__ zbuf,
                                                                 const uint32_t* __restrict__ large,
                                                                 const uint32_t* __restrict__ n_large) {
    const uint32_t n = *n_large;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t f = large[i];
        TriSetup t;
        if (!tex_setup(vclip, faces, f, V, H, W, t, nullptr)) continue;
        const int bw = t.x1 - t.x0 + 1;
        const long long npix = (long long)bw * (t.y1 - t.y0 + 1);
        for (long long p = (long long)blockIdx.y * TEX_THREADS + threadIdx.x; p < npix; p += (long long)gridDim.y * TEX_THREADS)
            tex_draw(t, f, t.x0 + (int)(p % bw), t.y0 + (int)(p / bw), W, zbuf);
    }
}

__global__ void __launch_bounds__(TEX_THREADS) tex_raster_shade_k(uint32_t V, const float* __restrict__ vclip,
                                                                 const int* __restrict__ faces, int H, int W,
                                                                 const unsigned long long* __restrict__ zbuf, int* __restrict__ tri,
                                                                 float* __restrict__ bary, float* __restrict__ zw_out) {
    const long long p = tgid();
    if (p >= (long long)H * W) return;
    const unsigned long long key = zbuf[p];
    int id = 0;
    float u = 0.f, v = 0.f, zw = 0.f;
    if (key != TEX_EMPTY) {
        const uint32_t f = (uint32_t)(key & 0xFFFFFFFFull);
        TriSetup t;
        long long e[3];
        if (tex_setup(vclip, faces, f, V, H, W, t, nullptr) && tex_cover(t, (int)(p % W), (int)(p / W), e)) {
            tex_shade(t, e, u, v, zw);
            id = (int)f + 1;
        }
    }
    tri[p] = id;
    bary[2 * p] = u;
    bary[2 * p + 1] = v;
    zw_out[p] = zw;
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TEX_THREADS) tex_resolve_k(uint32_t n_vt, uint32_t n_vn, uint32_t F, long long HW,
                                                            const int* __restrict__ tri, const float* __restrict__ bary,
                                                            const float* __restrict__ vt, const int* __restrict__ ft,
                                                            const float* __restrict__ vn, const int* __restrict__ faces,
                                                            const float* __restrict__ rot, const float* __restrict__ image,
                                                            float* __restrict__ coords, float* __restrict__ values,
                                                            uint8_t* __restrict__ valid, uint32_t* __restrict__ status) {
    const long long p = tgid();
    if (p >= HW) return;
    for (int c = 0; c < 3; c++) values[3 * p + c] = image[(size_t)c * HW + p];
    float cy = 0.f, cx = 0.f;
    uint32_t ok = 0;
    const uint32_t id = (uint32_t)tri[p];
    if (id != 0) {
        const size_t f = id - 1;
        uint32_t it[3] = {0, 0, 0}, in[3] = {0, 0, 0};
        bool range = id <= F;
        if (range)
            for (int k = 0; k < 3; k++) {
                it[k] = (uint32_t)ft[3 * f + k];
                in[k] = (uint32_t)faces[3 * f + k];
                range = range && it[k] < n_vt && in[k] < n_vn;
            }
        if (!range) {
            atomicOr(status, (uint32_t)GOI_TEXTURE_STATUS_RANGE);
        } else {
            const float u = bary[2 * p], v = bary[2 * p + 1];
            const float r = (1.f - u) - v;
            float uv[2], n[3];
            for (int d = 0; d < 2; d++)
                uv[d] = (u * vt[2 * (size_t)it[0] + d] + v * vt[2 * (size_t)it[1] + d]) + r * vt[2 * (size_t)it[2] + d];
            for (int d = 0; d < 3; d++)
                n[d] = (u * vn[3 * (size_t)in[0] + d] + v * vn[3 * (size_t)in[1] + d]) + r * vn[3 * (size_t)in[2] + d];
            const float dot = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            const float len = sqrtf(fmaxf(dot, 1e-20f));  // safe_normalize
            for (int d = 0; d < 3; d++) n[d] = n[d] / len;
            const float viewcos = (n[0] * rot[2] + n[1] * rot[5]) + n[2] * rot[8];  // (n @ R)[2]
            ok = viewcos > 0.5f ? 1u : 0u;
            cy = fminf(fmaxf(uv[1], 0.f), 1.f) * 2.f - 1.f;  // uvs[..., [1, 0]] * 2 - 1
            cx = fminf(fmaxf(uv[0], 0.f), 1.f) * 2.f - 1.f;
        }
    }
    coords[2 * p] = cy;
    coords[2 * p + 1] = cx;
    valid[p] = (uint8_t)ok;
}

// ---- grid put --------------------------------------------------------------------------------------------------------------
struct Tap {
    int i0, j0;
    float h, w;
};
// linear_grid_put_2d's index arithmetic for sample n on a cH x cW level; false for a sample that is masked out or whose
// coordinates are not finite
__device__ __forceinline__ bool tex_tap(const float* __restrict__ coords, const uint8_t* __restrict__ valid, long long n, int cH,
                                        int cW, Tap& t) {
    if (valid && !valid[n]) return false;
    const float a = coords[2 * n], b = coords[2 * n + 1];
    if (!isfinite(a) || !isfinite(b)) return false;
    const float fi = (a * 0.5f + 0.5f) * (float)(cH - 1), fj = (b * 0.5f + 0.5f) * (float)(cW - 1);
    const float i0 = fminf(fmaxf(floorf(fi), 0.f), (float)(cH - 2)), j0 = fminf(fmaxf(floorf(fj), 0.f), (float)(cW - 2));
    t.i0 = (int)i0;
    t.j0 = (int)j0;
    t.h = fi - i0;
    t.w = fj - j0;
    return true;
}
__device__ __forceinline__ float tex_tap_weight(const Tap& t, int tap) {
    const float a = (tap & 2) ? t.h : 1.f - t.h, b = (tap & 1) ? t.w : 1.f - t.w;  // w_00, w_01, w_10, w_11
    return a * b;
}

__global__ void __launch_bounds__(TEX_THREADS) tex_splat_key_k(long long N, const float* __restrict__ coords,
                                                              const uint8_t* __restrict__ valid, int cH, int cW,
                                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long e = tgid();
    if (e >= 4 * N) return;
    const int tap = (int)(e / N);
    Tap t;
    uint32_t key = (uint32_t)cH * (uint32_t)cW;
    if (tex_tap(coords, valid, e % N, cH, cW, t)) key = (uint32_t)(t.i0 + (tap >> 1)) * (uint32_t)cW + (uint32_t)(t.j0 + (tap & 1));
    keys[e] = key;
    vals[e] = (uint32_t)e;
}

// one lane per run of equal texels: its taps in ascending (tap, sample) order
template <int C>
__global__ void __launch_bounds__(TEX_THREADS) tex_segment_k(long long N, const uint32_t* __restrict__ skeys,
                                                            const uint32_t* __restrict__ svals, const float* __restrict__ coords,
                                                            const float* __restrict__ values, int cH, int cW,
                                                            float* __restrict__ lvl, float* __restrict__ lvl_count) {
    const long long i = tgid();
    const long long M = 4 * N;
    if (i >= M) return;
    const uint32_t key = skeys[i];
    if (key >= (uint32_t)cH * (uint32_t)cW || (i > 0 && skeys[i - 1] == key)) return;
    float acc[C], cnt = 0.f;
    for (int c = 0; c < C; c++) acc[c] = 0.f;
    for (long long j = i; j < M && skeys[j] == key; j++) {
        const long long e = svals[j];
        const long long n = e % N;
        Tap t;
        tex_tap(coords, nullptr, n, cH, cW, t);  // (valid and finite: it got a key)
        const float wt = tex_tap_weight(t, (int)(e / N));
        for (int c = 0; c < C; c++) acc[c] = acc[c] + values[(size_t)n * C + c] * wt;
        cnt = cnt + wt;
    }
    for (int c = 0; c < C; c++) lvl[(size_t)key * C + c] = acc[c];
    lvl_count[key] = cnt;
}

// upsample_bilinear2d(align_corners = false): source index and weights of an output index
__device__ __forceinline__ void tex_lerp_index(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// result / count += the level upsampled to H x W, where the running count is exactly 0.  acc != NULL (the last level): the
// view is then folded into the accumulated texture where its count is < 0.1 (texture.accumulate), and norm_out != NULL (the
// last view of a bake): the accumulated texture is divided by its count where that is > 0 (texture.normalize).
template <int C>
__global__ void __launch_bounds__(TEX_THREADS) tex_compose_k(int H, int W, int cH, int cW, const float* __restrict__ lvl,
                                                            const float* __restrict__ lvl_count, float* __restrict__ result,
                                                            float* __restrict__ count, float* __restrict__ acc,
                                                            float* __restrict__ acc_count, float* __restrict__ norm_out,
                                                            uint8_t* __restrict__ norm_mask) {
    const long long p = tgid();
    if (p >= (long long)H * W) return;
    float cnt = count[p];
    float res[C];
    for (int c = 0; c < C; c++) res[c] = result[(size_t)p * C + c];
    if (cnt == 0.f) {
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        tex_lerp_index((int)(p / W), cH, H, y0, y1, hy0, hy1);
        tex_lerp_index((int)(p % W), cW, W, x0, x1, wx0, wx1);
        const size_t a = (size_t)y0 * cW + x0, b = (size_t)y0 * cW + x1, c2 = (size_t)y1 * cW + x0, d = (size_t)y1 * cW + x1;
        for (int c = 0; c < C; c++) {
            const float up = hy0 * (wx0 * lvl[a * C + c] + wx1 * lvl[b * C + c]) + hy1 * (wx0 * lvl[c2 * C + c] + wx1 * lvl[d * C + c]);
            res[c] = res[c] + up;
            result[(size_t)p * C + c] = res[c];
        }
        const float up = hy0 * (wx0 * lvl_count[a] + wx1 * lvl_count[b]) + hy1 * (wx0 * lvl_count[c2] + wx1 * lvl_count[d]);
        cnt = cnt + up;
        count[p] = cnt;
    }
    if (!acc) return;
    float total = acc_count[p];
    float sum[C];
    for (int c = 0; c < C; c++) sum[c] = acc[(size_t)p * C + c];
    if (total < 0.1f) {
        for (int c = 0; c < C; c++) {
            sum[c] = sum[c] + res[c];
            acc[(size_t)p * C + c] = sum[c];
        }
        total = total + cnt;
        acc_count[p] = total;
    }
    if (norm_out) {
        const uint32_t m = total > 0.f ? 1u : 0u;
        for (int c = 0; c < C; c++) norm_out[(size_t)p * C + c] = m ? sum[c] / total : sum[c];
        norm_mask[p] = (uint8_t)m;
    }
}

__global__ void __launch_bounds__(TEX_THREADS) tex_accumulate_k(long long T, int C, float* __restrict__ albedo, float* __restrict__ cnt,
                                                               const float* __restrict__ cur, const float* __restrict__ cur_cnt) {
    const long long p = tgid();
    if (p >= T || !(cnt[p] < 0.1f)) return;
    for (int c = 0; c < C; c++) albedo[(size_t)p * C + c] = albedo[(size_t)p * C + c] + cur[(size_t)p * C + c];
    cnt[p] = cnt[p] + cur_cnt[p];
}

__global__ void __launch_bounds__(TEX_THREADS) tex_normalize_k(long long T, int C, const float* __restrict__ albedo,
                                                              const float* __restrict__ cnt, float* __restrict__ out,
                                                              uint8_t* __restrict__ mask) {
    const long long p = tgid();
    if (p >= T) return;
    const float n = cnt[p];
    const uint32_t m = n > 0.f ? 1u : 0u;
    for (int c = 0; c < C; c++) out[(size_t)p * C + c] = m ? albedo[(size_t)p * C + c] / n : albedo[(size_t)p * C + c];
    mask[p] = (uint8_t)m;
}

// ---- fill ------------------------------------------------------------------------------------------------------------------
// up[p] = the smallest d in 0 .. R with mask[y - d][x], dn[p] = the smallest d in 1 .. R with mask[y + d][x]; TEX_FAR: none
__global__ void __launch_bounds__(TEX_THREADS) tex_fill_columns_k(int h, int w, int R, const uint8_t* __restrict__ mask,
                                                                 uint8_t* __restrict__ up, uint8_t* __restrict__ dn) {
    const long long p = tgid();
    if (p >= (long long)h * w) return;
    const int y = (int)(p / w), x = (int)(p % w);
    uint32_t a = TEX_FAR, b = TEX_FAR;
    for (int d = 0; d <= R && y - d >= 0; d++)
        if (mask[(size_t)(y - d) * w + x]) {
            a = (uint32_t)d;
            break;
        }
    for (int d = 1; d <= R && y + d < h; d++)
        if (mask[(size_t)(y + d) * w + x]) {
            b = (uint32_t)d;
            break;
        }
    up[p] = (uint8_t)a;
    dn[p] = (uint8_t)b;
}

// a texel outside the mask with a mask texel within L1 distance R takes the colour of its nearest mask texel: the smallest
// (dx^2 + dy^2, row, column).  nearest[p] = that texel's flat index, -1 elsewhere.
__global__ void __launch_bounds__(TEX_THREADS) tex_fill_nearest_k(int h, int w, int R, int C, const uint8_t* __restrict__ mask,
                                                                 const uint8_t* __restrict__ up, const uint8_t* __restrict__ dn,
                                                                 const float* __restrict__ albedo, float* __restrict__ out,
                                                                 int* __restrict__ nearest) {
    const long long p = tgid();
    if (p >= (long long)h * w) return;
    const int y = (int)(p / w), x = (int)(p % w);
    long long src = p;
    int near = -1;
    if (!mask[p]) {
        unsigned long long best = ~0ull;
        bool region = false;
        const int xa = x - R < 0 ? 0 : x - R, xb = x + R > w - 1 ? w - 1 : x + R;
        for (int xx = xa; xx <= xb; xx++) {
            const int adx = xx < x ? x - xx : xx - x;
            const uint32_t du = up[(size_t)y * w + xx], dd = dn[(size_t)y * w + xx];
            if (du != TEX_FAR) {
                region = region || adx + (int)du <= R;
                const unsigned long long k = ((unsigned long long)(adx * adx + (int)(du * du)) << 42) | ((unsigned long long)(y - (int)du) << 21) | (unsigned)xx;
                best = k < best ? k : best;
            }
            if (dd != TEX_FAR) {
                region = region || adx + (int)dd <= R;
                const unsigned long long k = ((unsigned long long)(adx * adx + (int)(dd * dd)) << 42) | ((unsigned long long)(y + (int)dd) << 21) | (unsigned)xx;
                best = k < best ? k : best;
            }
        }
        if (region) {
            const long long row = (long long)((best >> 21) & 0x1FFFFFull), col = (long long)(best & 0x1FFFFFull);
            src = row * w + col;
            near = (int)src;
        }
    }
    for (int c = 0; c < C; c++) out[(size_t)p * C + c] = albedo[(size_t)src * C + c];
    nearest[p] = near;
}

struct RasterView {
    unsigned long long* zbuf;
    uint32_t *large, *n_large;
};
size_t raster_layout(size_t F, size_t HW, char* base, RasterView* v) {
    Carver c(base);
    RasterView t;
    t.zbuf = c.take<unsigned long long>(HW);
    t.large = c.take<uint32_t>(at_least_one(F));  // (F = 0 is a valid mesh; its piece stays)
    t.n_large = c.take<uint32_t>(4);
    if (v) *v = t;
    return c.bytes();
}

struct PutView {
    SortBufs sb;  // [4 N] splat taps
    float *lvl, *lvl_count;
};
size_t put_layout(size_t N, size_t C, size_t HW, char* base, PutView* v) {
    Carver c(base);
    PutView t;
    carve_sort(c, 4 * N, &t.sb);
    t.lvl = c.take<float>(HW * C);
    t.lvl_count = c.take<float>(HW);
    if (v) *v = t;
    return c.bytes();
}

struct FillView {
    uint8_t *up, *dn;
};
size_t fill_layout(size_t hw, char* base, FillView* v) {
    Carver c(base);
    FillView t;
    t.up = c.take<uint8_t>(hw);
    t.dn = c.take<uint8_t>(hw);
    if (v) *v = t;
    return c.bytes();
}

template <int C>
void run_level(long long N, const float* coords, const float* values, const uint8_t* valid, int H, int W, int cH, int cW,
               const PutView& w, float* result, float* count, float* acc, float* acc_count, float* norm_out, uint8_t* norm_mask,
               uint32_t* status, hipStream_t s) {
    const size_t T = (size_t)cH * cW;
    (void)hipMemsetAsync(w.lvl, 0, T * C * sizeof(float), s);
    (void)hipMemsetAsync(w.lvl_count, 0, T * sizeof(float), s);
    if (N > 0) {
        tex_splat_key_k<<<dim3(tblocks(4 * N)), dim3(TEX_THREADS), 0, s>>>(N, coords, valid, cH, cW, w.sb.keys[0], w.sb.vals[0]);
        const int fin = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)(4 * N), 0, tbits_for((uint32_t)T), w.sb.scratch, s, false, false, nullptr, status);
        tex_segment_k<C><<<dim3(tblocks(4 * N)), dim3(TEX_THREADS), 0, s>>>(N, w.sb.keys[fin], w.sb.vals[fin], coords, values, cH, cW, w.lvl, w.lvl_count);
    }
    tex_compose_k<C><<<dim3(tblocks((long long)H * W)), dim3(TEX_THREADS), 0, s>>>(H, W, cH, cW, w.lvl, w.lvl_count, result, count, acc,
                                                                                  acc_count, norm_out, norm_mask);
}

size_t texture_rasterize_workspace_bytes(long long F, int H, int W) { return raster_layout((size_t)F, (size_t)H * W, nullptr, nullptr); }

void launch_texture_rasterize(long long V, long long F, const float* v_clip, const int* faces, int H, int W, int* tri, float* bary,
                              float* zw, int* status, void* workspace, hipStream_t s) {
    RasterView w;
    raster_layout((size_t)F, (size_t)H * W, static_cast<char*>(workspace), &w);
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    (void)hipMemsetAsync(st, 0, sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.n_large, 0, sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.zbuf, 0xFF, (size_t)H * W * sizeof(unsigned long long), s);
    if (F > 0) {
        const unsigned g = (unsigned)((F + TEX_THREADS / 64 - 1) / (TEX_THREADS / 64));
        tex_raster_wave_k<<<dim3(g), dim3(TEX_THREADS), 0, s>>>(F, (uint32_t)V, v_clip, faces, H, W, w.zbuf, w.large, w.n_large, st);
        tex_raster_large_k<<<dim3(TEX_LARGE_X, TEX_LARGE_Y), dim3(TEX_THREADS), 0, s>>>((uint32_t)V, v_clip, faces, H, W, w.zbuf, w.large,
                                                                                        w.n_large);
    }
    tex_raster_shade_k<<<dim3(tblocks((long long)H * W)), dim3(TEX_THREADS), 0, s>>>((uint32_t)V, v_clip, faces, H, W, w.zbuf, tri, bary, zw);
}

void launch_texture_resolve(long long n_vt, long long n_vn, long long F, int H, int W, const int* tri, const float* bary,
                            const float* vt, const int* ft, const float* vn, const int* faces, const float* pose_rot,
                            const float* image, float* coords, float* values, unsigned char* valid, int* status, hipStream_t s) {
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    (void)hipMemsetAsync(st, 0, sizeof(uint32_t), s);
    const long long HW = (long long)H * W;
    tex_resolve_k<<<dim3(tblocks(HW)), dim3(TEX_THREADS), 0, s>>>((uint32_t)n_vt, (uint32_t)n_vn, (uint32_t)F, HW, tri, bary, vt, ft, vn, faces,
                                                                 pose_rot, image, coords, values, valid, st);
}

size_t texture_grid_put_workspace_bytes(long long N, int C, int H, int W) {
    return put_layout((size_t)N, (size_t)C, (size_t)H * W, nullptr, nullptr);
}

void launch_texture_grid_put(long long N, int C, int H, int W, int min_resolution, const float* coords, const float* values,
                             const unsigned char* valid, float* result, float* count, float* acc, float* acc_count, float* norm_out,
                             unsigned char* norm_mask, int* status, void* workspace, hipStream_t s) {
    PutView w;
    put_layout((size_t)N, (size_t)C, (size_t)H * W, static_cast<char*>(workspace), &w);
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    const size_t T = (size_t)H * W;
    (void)hipMemsetAsync(st, 0, sizeof(uint32_t), s);
    (void)hipMemsetAsync(result, 0, T * C * sizeof(float), s);
    (void)hipMemsetAsync(count, 0, T * sizeof(float), s);
    int levels = 0;
    for (int cH = H, cW = W; (cH < cW ? cH : cW) > min_resolution; cH /= 2, cW /= 2) levels++;
    int cH = H, cW = W;
    for (int l = 0; l < levels; l++, cH /= 2, cW /= 2) {
        const bool last = l == levels - 1;
        float* a = last ? acc : nullptr;
        float* ac = last ? acc_count : nullptr;
        float* no = last ? norm_out : nullptr;
        uint8_t* nm = last ? norm_mask : nullptr;
        switch (C) {
            case 1: run_level<1>(N, coords, values, valid, H, W, cH, cW, w, result, count, a, ac, no, nm, st, s); break;
            case 2: run_level<2>(N, coords, values, valid, H, W, cH, cW, w, result, count, a, ac, no, nm, st, s); break;
            case 3: run_level<3>(N, coords, values, valid, H, W, cH, cW, w, result, count, a, ac, no, nm, st, s); break;
            default: run_level<4>(N, coords, values, valid, H, W, cH, cW, w, result, count, a, ac, no, nm, st, s); break;
        }
    }
    if (levels == 0 && acc) {  // no level: the view is all zeros, and adding it still follows the rule
        tex_accumulate_k<<<dim3(tblocks((long long)T)), dim3(TEX_THREADS), 0, s>>>((long long)T, C, acc, acc_count, result, count);
        if (norm_out) tex_normalize_k<<<dim3(tblocks((long long)T)), dim3(TEX_THREADS), 0, s>>>((long long)T, C, acc, acc_count, norm_out, norm_mask);
    }
}

size_t texture_fill_workspace_bytes(int h, int w) { return fill_layout((size_t)h * w, nullptr, nullptr); }

void launch_texture_fill(int h, int w, int C, int radius, const float* albedo, const unsigned char* mask, float* out, int* nearest,
                         void* workspace, hipStream_t s) {
    FillView v;
    fill_layout((size_t)h * w, static_cast<char*>(workspace), &v);
    const long long T = (long long)h * w;
    tex_fill_columns_k<<<dim3(tblocks(T)), dim3(TEX_THREADS), 0, s>>>(h, w, radius, mask, v.up, v.dn);
    tex_fill_nearest_k<<<dim3(tblocks(T)), dim3(TEX_THREADS), 0, s>>>(h, w, radius, C, mask, v.up, v.dn, albedo, out, nearest);
}

bool texture_size_ok(int H, int W) { return H >= 1 && W >= 1 && H <= GOI_TEXTURE_MAX_SIZE && W <= GOI_TEXTURE_MAX_SIZE; }
int texture_size(const char* fn, int H, int W) {
    if (!texture_size_ok(H, W)) return fail(std::string(fn) + ": need 1 <= H, W <= 16384");
    return 0;
}
bool texture_put_ok(long long N, int C, int H, int W) {
    return N >= 0 && 4 * N < SORT_MAX_KEYS && C >= 1 && C <= GOI_TEXTURE_MAX_CHANNELS && texture_size_ok(H, W);
}
int texture_texels(const char* fn, long long T, int C) {
    if (T < 0 || T > (long long)GOI_TEXTURE_MAX_SIZE * GOI_TEXTURE_MAX_SIZE || C < 1 || C > GOI_TEXTURE_MAX_CHANNELS)
        return fail(std::string(fn) + ": need 0 <= T <= 16384^2 and 1 <= C <= 4");
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_texture_rasterize_workspace_bytes(long long F, int H, int W) {
    return F >= 0 && 3 * F < SORT_MAX_KEYS && texture_size_ok(H, W) ? texture_rasterize_workspace_bytes(F, H, W) : 0;
}

int goi_texture_rasterize(long long V, long long F, const float* v_clip, const int* faces, int H, int W, int* tri, float* bary,
                          float* zw, int* status, void* workspace, void* stream) {
    const char* fn = "goi_texture_rasterize";
    if (mesh_sizes(fn, V, F, 0) < 0 || texture_size(fn, H, W) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (!status || !tri || !bary || !zw || (F > 0 && (!faces || !v_clip))) return fail(std::string(fn) + ": a required pointer is NULL");
    launch_texture_rasterize(V, F, v_clip, faces, H, W, tri, bary, zw, status, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_texture_resolve(long long n_vt, long long n_vn, long long F, int H, int W, const int* tri, const float* bary,
                        const float* vt, const int* ft, const float* vn, const int* faces, const float* pose_rot,
                        const float* image, float* coords, float* values, unsigned char* valid, int* status, void* stream) {
    const char* fn = "goi_texture_resolve";
    if (mesh_sizes(fn, n_vt, F, 0) < 0 || mesh_sizes(fn, n_vn, F, 0) < 0 || texture_size(fn, H, W) < 0) return -1;
    if (!status || !tri || !bary || !pose_rot || !image || !coords || !values || !valid || (F > 0 && (!vt || !ft || !vn || !faces)))
        return fail(std::string(fn) + ": a required pointer is NULL");
    launch_texture_resolve(n_vt, n_vn, F, H, W, tri, bary, vt, ft, vn, faces, pose_rot, image, coords, values, valid, status,
                           static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_texture_grid_put_workspace_bytes(long long N, int C, int H, int W) {
    return texture_put_ok(N, C, H, W) ? texture_grid_put_workspace_bytes(N, C, H, W) : 0;
}

int goi_texture_grid_put(long long N, int C, int H, int W, int min_resolution, const float* coords, const float* values,
                         const unsigned char* valid, float* result, float* count, float* acc, float* acc_count, float* norm_out,
                         unsigned char* norm_mask, int* status, void* workspace, void* stream) {
    const char* fn = "goi_texture_grid_put";
    if (!texture_put_ok(N, C, H, W)) return fail(std::string(fn) + ": need 0 <= N < 2^28, 1 <= C <= 4 and 1 <= H, W <= 16384");
    if (min_resolution < 1) return fail(std::string(fn) + ": need min_resolution >= 1");
    if (check_workspace(fn, workspace) < 0) return -1;
    if (!status || !result || !count || (N > 0 && (!coords || !values))) return fail(std::string(fn) + ": a required pointer is NULL");
    if ((acc == nullptr) != (acc_count == nullptr)) return fail(std::string(fn) + ": give both of acc and acc_count, or neither");
    if ((norm_out == nullptr) != (norm_mask == nullptr) || (norm_out && !acc))
        return fail(std::string(fn) + ": give both of norm_out and norm_mask, with acc, or neither");
    launch_texture_grid_put(N, C, H, W, min_resolution, coords, values, valid, result, count, acc, acc_count, norm_out, norm_mask,
                            status, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_texture_accumulate(long long T, int C, float* albedo, float* cnt, const float* cur, const float* cur_cnt, void* stream) {
    const char* fn = "goi_texture_accumulate";
    if (texture_texels(fn, T, C) < 0) return -1;
    if (T > 0 && (!albedo || !cnt || !cur || !cur_cnt)) return fail(std::string(fn) + ": a required pointer is NULL");
    if (T > 0)
        tex_accumulate_k<<<dim3(tblocks(T)), dim3(TEX_THREADS), 0, static_cast<hipStream_t>(stream)>>>(T, C, albedo, cnt, cur, cur_cnt);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_texture_normalize(long long T, int C, const float* albedo, const float* cnt, float* out, unsigned char* mask,
                          void* stream) {
    const char* fn = "goi_texture_normalize";
    if (texture_texels(fn, T, C) < 0) return -1;
    if (T > 0 && (!albedo || !cnt || !out || !mask)) return fail(std::string(fn) + ": a required pointer is NULL");
    if (T > 0)
        tex_normalize_k<<<dim3(tblocks(T)), dim3(TEX_THREADS), 0, static_cast<hipStream_t>(stream)>>>(T, C, albedo, cnt, out, mask);
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_texture_fill_workspace_bytes(int h, int w) { return texture_size_ok(h, w) ? texture_fill_workspace_bytes(h, w) : 0; }

int goi_texture_fill(int h, int w, int C, int radius, const float* albedo, const unsigned char* mask, float* out, int* nearest,
                     void* workspace, void* stream) {
    const char* fn = "goi_texture_fill";
    if (texture_size(fn, h, w) < 0 || texture_texels(fn, 0, C) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (radius < 0 || radius > GOI_TEXTURE_MAX_RADIUS) return fail(std::string(fn) + ": need 0 <= radius <= 127");
    if (!albedo || !mask || !out || !nearest) return fail(std::string(fn) + ": a required pointer is NULL");
    launch_texture_fill(h, w, C, radius, albedo, mask, out, nearest, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
