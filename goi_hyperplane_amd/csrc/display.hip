// The viewer's frame composed on the device: the stage between a render with its decoded similarity and the picture
// the user sees (the reference's gui/main.py:549-604 test_step, :387-398 set_clip_mask with utils/image_utils.py:129-178
// cmap / clip_color, and :1766-1801 render_video, all of which run on the host in numpy).
//
// Per view v, every operation one fp32 rounding in the order written (this file is built with -ffp-contract=off: the
// blend a*b + c*d must not become an FMA, the output is compared bit for bit):
//
//   base = image[v] [C][H][W], C in {1, 3}; C == 1 is repeated to three channels
//   normalize:  base = (base - min_v) / ((max_v - min_v) + 1e-20f)            min / max over the whole view
//   base = clamp(base, 0, 1)
//   NONE      out = base
//   BINARY    out = sim > 0 ? 1 : 0
//   WHITEN    col = 1;  a = bg ? 1 : 0;  opa = a * ratio;  om = 1 - opa
//   HEAT      rel = clamp(((sim - t) - 0.05f) / (max_v(sim) - t), 0, 1)
//             col = bg ? 1 : clamp(table[(long)(rel * (K-1))], 0, 1);  opa = ratio;  om = one_minus_ratio
//   HEAT_FT   rel = clamp(sim + 0.2f, 0.1f, 0.9f);  col as HEAT;  a = bg ? 1 : 0;  opa = a * ratio;  om = 1 - opa
//   overlay   out = clamp(col * opa + base * om, 0, 1)
//   uint8     out = (uint8)(out * 255f)                                       truncation
//
// `ratio` and `one_minus_ratio` come rounded from the host: the reference forms 1 - ratio in double (a Python float)
// before numpy rounds it to fp32, so it is not 1.0f - ratio.
//
//   frame_stats_k    per-view min / max of the base and max of sim into a [V][3] uint32 buffer of order-preserving
//                    keys (zeroed on the stream by the same call): 16-byte loads, wave64 shuffle reduction, LDS across
//                    the waves, one atomicMax per workgroup and statistic, <= 256 workgroups per view.  min and max are
//                    order-independent, so the result is exact and reproducible.  A NaN is skipped (fminf / fmaxf).
//   frame_compose_k  planar 16-byte loads of the channels, sim and four mask bytes; the colour table staged in LDS once
//                    per workgroup; interleaved stores (48 contiguous bytes per four pixels in fp32, 12 in uint8).  A
//                    scalar path takes the tail and every view whose planes are not 16-byte aligned.  The table index
//                    is clamped into [0, K-1] and a NaN rel takes index 0: no input reads outside the table.
//
// Neither allocates, copies or synchronises: both are asynchronous on the caller's stream.
// C entries, with the limits they enforce, at the end of the file: goi_semantic_frame_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_WAVES = FRAME_THREADS / 64;
constexpr int STATS_MAX_BLOCKS = 256;     // per view (one per CU): they all hit the view's three words
constexpr int COMPOSE_MAX_BLOCKS = 2048;  // per launch, spread over the views

// The stats buffer holds the ordered key (ord_enc, wave_util.h) of the maximum and the COMPLEMENT of the key of the minimum,
// so both are atomicMax and the all-zero buffer is the identity.

struct MinMax {
    float mn, mx;
    __device__ __forceinline__ void take(float x) {
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
    }
};

// min / max of p[0 .. n) over the threads `tid` of `nthreads`: a scalar head up to the first 16-byte boundary, float4
// body, scalar tail, so a span at any 4-byte alignment takes vector loads.
__device__ __forceinline__ MinMax span_minmax(const float* __restrict__ p, long long n, long long tid, long long nthreads) {
    MinMax r{INFINITY, -INFINITY};
    long long head = (long long)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > n) head = n;
    const long long quads = (n - head) >> 2;
    const long long tail0 = head + (quads << 2);
    if (tid < head) r.take(p[tid]);
    const float4* q = reinterpret_cast<const float4*>(p + head);
    for (long long i = tid; i < quads; i += nthreads) {
        const float4 v = q[i];
        r.take(v.x);
        r.take(v.y);
        r.take(v.z);
        r.take(v.w);
    }
    if (tid < n - tail0) r.take(p[tail0 + tid]);
    return r;
}

// blockIdx.y = view.  base == nullptr or sim == nullptr skips that statistic.  stats [V][3]: ~key(min base), key(max base),
// key(max sim).
__global__ void __launch_bounds__(FRAME_THREADS) frame_stats_k(const float* __restrict__ base, long long base_len,
                                                              const float* __restrict__ sim, long long HW,
                                                              uint32_t* __restrict__ stats) {
    __shared__ float part[FRAME_WAVES][3];
    const int view = blockIdx.y;
    const long long tid = (long long)blockIdx.x * FRAME_THREADS + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * FRAME_THREADS;
    MinMax b{INFINITY, -INFINITY}, s{INFINITY, -INFINITY};
    if (base) b = span_minmax(base + (size_t)view * base_len, base_len, tid, nthreads);
    if (sim) s = span_minmax(sim + (size_t)view * HW, HW, tid, nthreads);
    const float mn = wave_min(b.mn), mx = wave_max(b.mx), sx = wave_max(s.mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = mn;
        part[wave][1] = mx;
        part[wave][2] = sx;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = part[0][threadIdx.x];
        for (int w = 1; w < FRAME_WAVES; ++w) v = threadIdx.x == 0 ? fminf(v, part[w][0]) : fmaxf(v, part[w][threadIdx.x]);
        const uint32_t key = threadIdx.x == 0 ? ~ord_enc(v) : ord_enc(v);
        if ((threadIdx.x < 2) ? base != nullptr : sim != nullptr) atomicMax(stats + (size_t)view * 3 + threadIdx.x, key);
    }
}

struct FrameParams {
    const float* base;       // [V][C][HW]
    const float* sim;        // [V][HW] or nullptr
    const uint8_t* bg;       // [V][HW] or nullptr
    const float* table;      // [K][3] or nullptr
    const uint32_t* stats;   // [V][3] keys or nullptr
    void* out;               // [V][HW][3]
    long long HW;
    long long vec_quads;     // quads of each view that take the vector path (0: all scalar)
    int channels, n_colors, normalize;
    float ratio, one_minus_ratio, thresh;
};

struct ViewConsts {
    float mn, den, hden;
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

template <int STYLE>
__device__ __forceinline__ void compose_pixel(const FrameParams& p, const ViewConsts& vc, const float* __restrict__ tab, float b0,
                                              float b1, float b2, float s, uint8_t bg, float out[3]) {
    if (STYLE == GOI_FRAME_BINARY) {
        out[0] = out[1] = out[2] = s > 0.0f ? 1.0f : 0.0f;
        return;
    }
    float b[3] = {b0, b1, b2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (p.normalize) b[c] = (b[c] - vc.mn) / vc.den;
        b[c] = clamp01(b[c]);
    }
    if (STYLE == GOI_FRAME_NONE) {
        out[0] = b[0];
        out[1] = b[1];
        out[2] = b[2];
        return;
    }
    float col[3] = {1.0f, 1.0f, 1.0f};
    float opa, om;
    if (STYLE == GOI_FRAME_HEAT || STYLE == GOI_FRAME_HEAT_FT) {
        float rel;
        if (STYLE == GOI_FRAME_HEAT)
            rel = clamp01(((s - p.thresh) - 0.05f) / vc.hden);
        else
            rel = fminf(fmaxf(s + 0.2f, 0.1f), 0.9f);
        int i = (int)(rel * (float)(p.n_colors - 1));  // rel in [0, 1] (a NaN became 0 in the clamp): i in [0, K-1]
        i = min(max(i, 0), p.n_colors - 1);
        if (!bg) {
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = clamp01(tab[3 * i + c]);
        }
    }
    if (STYLE == GOI_FRAME_HEAT) {
        opa = p.ratio;
        om = p.one_minus_ratio;
    } else {
        opa = (bg ? 1.0f : 0.0f) * p.ratio;
        om = 1.0f - opa;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = clamp01(col[c] * opa + b[c] * om);
}

__device__ __forceinline__ void store_pixel(float* out, long long pix, const float v[3]) {
    out[3 * pix] = v[0];
    out[3 * pix + 1] = v[1];
    out[3 * pix + 2] = v[2];
}
__device__ __forceinline__ void store_pixel(uint8_t* out, long long pix, const float v[3]) {
    out[3 * pix] = (uint8_t)(v[0] * 255.0f);
    out[3 * pix + 1] = (uint8_t)(v[1] * 255.0f);
    out[3 * pix + 2] = (uint8_t)(v[2] * 255.0f);
}

// four pixels v[4][3] -> 48 contiguous bytes
__device__ __forceinline__ void store_quad(float* out, long long quad, const float v[4][3]) {
    float4* o = reinterpret_cast<float4*>(out + 12 * quad);
    o[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
    o[1] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
    o[2] = make_float4(v[2][2], v[3][0], v[3][1], v[3][2]);
}
// four pixels -> 12 contiguous bytes
__device__ __forceinline__ void store_quad(uint8_t* out, long long quad, const float v[4][3]) {
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w[k] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * k + j;
            w[k] |= (uint32_t)(uint8_t)(v[e / 3][e % 3] * 255.0f) << (8 * j);
        }
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(out + 12 * quad);
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
}

// blockIdx.y = view; the workgroups of a view stride over its quads (vector path), then over the remaining pixels.
template <int STYLE, typename OUT>
__global__ void __launch_bounds__(FRAME_THREADS) frame_compose_k(const FrameParams p) {
    constexpr bool HEAT = STYLE == GOI_FRAME_HEAT || STYLE == GOI_FRAME_HEAT_FT;
    constexpr bool USE_BASE = STYLE != GOI_FRAME_BINARY;
    constexpr bool USE_SIM = HEAT || STYLE == GOI_FRAME_BINARY;
    constexpr bool USE_BG = HEAT || STYLE == GOI_FRAME_WHITEN;
    __shared__ float tab[HEAT ? 3 * GOI_FRAME_MAX_COLORS : 1];
    if (HEAT) {
        for (int i = threadIdx.x; i < 3 * p.n_colors; i += FRAME_THREADS) tab[i] = p.table[i];
        __syncthreads();
    }
    const int view = blockIdx.y;
    const long long HW = p.HW;
    ViewConsts vc{0.0f, 1.0f, 1.0f};
    if (USE_BASE && p.normalize) {
        const float mn = ord_dec(~p.stats[(size_t)view * 3]), mx = ord_dec(p.stats[(size_t)view * 3 + 1]);
        vc.mn = mn;
        vc.den = (mx - mn) + 1e-20f;
    }
    if (STYLE == GOI_FRAME_HEAT) vc.hden = ord_dec(p.stats[(size_t)view * 3 + 2]) - p.thresh;
    const float* b0 = p.base + (size_t)view * p.channels * HW;
    const float* b1 = p.channels == 3 ? b0 + HW : b0;
    const float* b2 = p.channels == 3 ? b0 + 2 * HW : b0;
    const float* sim = USE_SIM ? p.sim + (size_t)view * HW : nullptr;
    const uint8_t* bg = USE_BG ? p.bg + (size_t)view * HW : nullptr;
    OUT* out = static_cast<OUT*>(p.out) + (size_t)view * HW * 3;
    const long long tid = (long long)blockIdx.x * FRAME_THREADS + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * FRAME_THREADS;

    for (long long q = tid; q < p.vec_quads; q += nthreads) {
        float4 c0 = make_float4(0, 0, 0, 0), c1 = c0, c2 = c0, s4 = c0;
        uint32_t m4 = 0;
        if (USE_BASE) {
            c0 = reinterpret_cast<const float4*>(b0)[q];
            if (p.channels == 3) {
                c1 = reinterpret_cast<const float4*>(b1)[q];
                c2 = reinterpret_cast<const float4*>(b2)[q];
            } else {
                c1 = c2 = c0;
            }
        }
        if (USE_SIM) s4 = reinterpret_cast<const float4*>(sim)[q];
        if (USE_BG) m4 = reinterpret_cast<const uint32_t*>(bg)[q];
        float v[4][3];
        compose_pixel<STYLE>(p, vc, tab, c0.x, c1.x, c2.x, s4.x, (uint8_t)(m4 & 0xff), v[0]);
        compose_pixel<STYLE>(p, vc, tab, c0.y, c1.y, c2.y, s4.y, (uint8_t)((m4 >> 8) & 0xff), v[1]);
        compose_pixel<STYLE>(p, vc, tab, c0.z, c1.z, c2.z, s4.z, (uint8_t)((m4 >> 16) & 0xff), v[2]);
        compose_pixel<STYLE>(p, vc, tab, c0.w, c1.w, c2.w, s4.w, (uint8_t)(m4 >> 24), v[3]);
        store_quad(out, q, v);
    }
    for (long long i = 4 * p.vec_quads + tid; i < HW; i += nthreads) {
        float v[3];
        compose_pixel<STYLE>(p, vc, tab, USE_BASE ? b0[i] : 0.0f, USE_BASE ? b1[i] : 0.0f, USE_BASE ? b2[i] : 0.0f,
                             USE_SIM ? sim[i] : 0.0f, USE_BG ? bg[i] : (uint8_t)0, v);
        store_pixel(out, i, v);
    }
}

template <int STYLE>
void compose_dispatch(const FrameParams& p, int out_dtype, dim3 grid, hipStream_t s) {
    if (out_dtype == GOI_FRAME_U8)
        frame_compose_k<STYLE, uint8_t><<<grid, FRAME_THREADS, 0, s>>>(p);
    else
        frame_compose_k<STYLE, float><<<grid, FRAME_THREADS, 0, s>>>(p);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

void launch_frame_compose(const float* base, int channels, const float* sim, const uint8_t* bg_mask, int n_views, long long HW,
                          int style, int normalize, float ratio, float one_minus_ratio, float heat_thresh, const float* table,
                          int n_colors, void* out, int out_dtype, uint32_t* stats, hipStream_t s) {
    const bool need_base_stats = normalize && style != GOI_FRAME_BINARY;
    const bool need_sim_stats = style == GOI_FRAME_HEAT;
    if (need_base_stats || need_sim_stats) {
        (void)hipMemsetAsync(stats, 0, sizeof(uint32_t) * 3 * (size_t)n_views, s);
        const long long items = std::max<long long>(need_base_stats ? channels * HW : 0, need_sim_stats ? HW : 0);
        const long long blocks = (items + FRAME_THREADS * 16 - 1) / (FRAME_THREADS * 16);
        const dim3 grid((unsigned)std::min<long long>(std::max<long long>(blocks, 1), STATS_MAX_BLOCKS), n_views);
        frame_stats_k<<<grid, FRAME_THREADS, 0, s>>>(need_base_stats ? base : nullptr, channels * HW,
                                                    need_sim_stats ? sim : nullptr, HW, stats);
    }
    FrameParams p;
    p.base = base;
    p.sim = sim;
    p.bg = bg_mask;
    p.table = table;
    p.stats = stats;
    p.out = out;
    p.HW = HW;
    p.channels = channels;
    p.n_colors = n_colors;
    p.normalize = need_base_stats ? 1 : 0;
    p.ratio = ratio;
    p.one_minus_ratio = one_minus_ratio;
    p.thresh = heat_thresh;
    // The vector path needs every plane of every view on a 16-byte boundary (mask bytes and uint8 output: 4 bytes): the
    // buffers themselves aligned, and H * W a multiple of 4 unless one single-channel view is all there is.
    const bool planes_ok = (HW % 4 == 0) || (n_views == 1 && channels == 1);
    const bool ptrs_ok = aligned(base, 16) && aligned(sim, 16) && aligned(bg_mask, 4) && aligned(out, 16);
    p.vec_quads = (planes_ok && ptrs_ok) ? HW / 4 : 0;
    const long long per_view = std::max<long long>(1, COMPOSE_MAX_BLOCKS / n_views);
    const long long blocks = (HW / 4 + FRAME_THREADS) / FRAME_THREADS;  // >= 1; one quad per thread up to the cap
    const dim3 grid((unsigned)std::min(blocks, per_view), n_views);
    switch (style) {
        case GOI_FRAME_NONE: compose_dispatch<GOI_FRAME_NONE>(p, out_dtype, grid, s); break;
        case GOI_FRAME_BINARY: compose_dispatch<GOI_FRAME_BINARY>(p, out_dtype, grid, s); break;
        case GOI_FRAME_WHITEN: compose_dispatch<GOI_FRAME_WHITEN>(p, out_dtype, grid, s); break;
        case GOI_FRAME_HEAT: compose_dispatch<GOI_FRAME_HEAT>(p, out_dtype, grid, s); break;
        default: compose_dispatch<GOI_FRAME_HEAT_FT>(p, out_dtype, grid, s); break;
    }
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_semantic_frame_workspace_bytes(int n_views) { return n_views < 1 ? 0 : sizeof(uint32_t) * 3 * (size_t)n_views; }

int goi_semantic_frame_compose(const float* base, int channels, const float* sim, const uint8_t* bg_mask, int n_views, int H, int W,
                               int style, int normalize, double overlay_ratio, double heat_thresh, const float* table,
                               int n_colors, void* out, int out_dtype, void* workspace, void* stream) {
    const char* fn = "goi_semantic_frame_compose";
    if (mask_dims(fn, H, W) < 0) return -1;
    if (style < GOI_FRAME_NONE || style > GOI_FRAME_HEAT_FT) return fail(std::string(fn) + ": unknown style");
    if (out_dtype != GOI_FRAME_F32 && out_dtype != GOI_FRAME_U8) return fail(std::string(fn) + ": out_dtype must be GOI_FRAME_F32 or GOI_FRAME_U8");
    if (channels != 1 && channels != 3) return fail(std::string(fn) + ": channels must be 1 or 3");
    if (n_views < 0 || n_views > 65535) return fail(std::string(fn) + ": need 0 <= n_views <= 65535");
    if (n_views == 0) return 0;
    const bool heat = style == GOI_FRAME_HEAT || style == GOI_FRAME_HEAT_FT;
    const bool need_base = style != GOI_FRAME_BINARY;
    if (!out || (need_base && !base)) return fail(std::string(fn) + ": NULL base or out");
    if ((heat || style == GOI_FRAME_BINARY) && !sim) return fail(std::string(fn) + ": this style needs sim");
    if ((heat || style == GOI_FRAME_WHITEN) && !bg_mask) return fail(std::string(fn) + ": this style needs bg_mask");
    if (heat && (!table || n_colors < 2 || n_colors > GOI_FRAME_MAX_COLORS))
        return fail(std::string(fn) + ": the heat styles need a table of 2 .. GOI_FRAME_MAX_COLORS (1024) colours");
    if (((normalize && need_base) || style == GOI_FRAME_HEAT) && !workspace) return fail(std::string(fn) + ": NULL workspace");
    if (!(overlay_ratio == overlay_ratio) || !(heat_thresh == heat_thresh)) return fail(std::string(fn) + ": NaN overlay_ratio or heat_thresh");
    launch_frame_compose(base, channels, sim, bg_mask, n_views, (long long)H * W, style, normalize, (float)overlay_ratio,
                         (float)(1.0 - overlay_ratio), (float)heat_thresh, table, n_colors, out, out_dtype,
                         static_cast<uint32_t*>(workspace), static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
