// Binary masks of a camera sweep, bit-packed on the device: the mask stage of the reference's relevant-camera
// precompute (gui/main.py:407-478: count_nonzero, cos_sim > 0, cv2.dilate(ones(3,3), iterations=5) >= 0.5) and of its
// segmentation evaluation (gui/main.py:1957-2016 with utils/image_utils.py:59-102).
//
// Layout: [V][H][Wwords] uint64, Wwords = ceil(W / 64); bit j of word w of a row is pixel x = 64 w + j.  Bits past W
// are zero (every kernel here keeps it so).  One wave64 ballot is one word.
//
//   mask_pack_k       fp32 / uint8 map -> packed bits (x > 0 for fp32, x != 0 for uint8) and two per-view int64
//                     counters: pixels with x != 0 (count_nonzero: a NaN counts) and pixels with a set bit.  Integer
//                     atomics (one per workgroup per counter, <= 64 workgroups per view), so the counts are
//                     deterministic.
//   mask_dilate_k     exact binary dilation by the (2r+1)^2 square clipped at the border, r <= 63.  A square is
//                     separable and OR distributes over it, so each output word ORs the clipped column of 2r+1 rows
//                     for its own word and its two neighbours, then ORs the 2r shifts of that 192-bit row slice.
//   mask_unpack_k     packed -> one byte (0 / 1) per pixel, optionally only the views of an index list (an index
//                     outside the buffer gives an empty mask: nothing is read out of bounds).
//   mask_confusion_k  TP / FP / FN / TN per view by popcounts; one workgroup per view, a fixed reduction order.
//
// None of them allocates, copies or synchronises: every launch is asynchronous on the caller's stream.
// C entries, with the limits they enforce, at the end of the file: goi_semantic_mask_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int MASK_THREADS = 256;
constexpr int MASK_WAVES = MASK_THREADS / 64;
constexpr int PACK_THREADS = 1024;
constexpr int PACK_WAVES = PACK_THREADS / 64;
constexpr int PACK_UNROLL = 8;

__device__ __forceinline__ uint64_t last_word_bits(int W) {
    const int rem = W & 63;
    return rem ? ((1ull << rem) - 1ull) : ~0ull;
}

// blockIdx.y = view of the batch; the workgroups of a view stride over its H * Wwords words, one wave per word, with
// PACK_UNROLL words' loads in flight per wave.  Few workgroups per view (<= 64) keep the global atomics on the view's two
// counters few: they all hit one address.
template <typename T>
__global__ void __launch_bounds__(PACK_THREADS) mask_pack_k(const T* __restrict__ src, int H, int W, int Wwords, int first_view,
                                                           uint64_t* __restrict__ packed, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long acc[2];
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int view = blockIdx.y;
    const int words = H * Wwords;  // H * W < 2^31
    const T* vsrc = src + (size_t)view * H * W;
    uint64_t* vout = packed + ((size_t)first_view + view) * (size_t)words;
    const int step = gridDim.x * PACK_WAVES;
    unsigned long long nz = 0, pos = 0;
    for (int g0 = blockIdx.x * PACK_WAVES + (threadIdx.x >> 6); g0 < words; g0 += step * PACK_UNROLL) {
        T v[PACK_UNROLL];
#pragma unroll
        for (int u = 0; u < PACK_UNROLL; ++u) {
            const int g = g0 + u * step;
            v[u] = T(0);
            if (g < words) {
                const int y = g / Wwords;
                const int x = (g - y * Wwords) * 64 + lane;
                if (x < W) v[u] = vsrc[(size_t)y * W + x];
            }
        }
#pragma unroll
        for (int u = 0; u < PACK_UNROLL; ++u) {
            const int g = g0 + u * step;
            if (g < words) {  // wave-uniform
                const uint64_t m_nz = __ballot(v[u] != T(0));
                const uint64_t m_pos = __ballot(v[u] > T(0));
                if (lane == 0) {
                    vout[g] = m_pos;
                    nz += __popcll(m_nz);
                    pos += __popcll(m_pos);
                }
            }
        }
    }
    if (lane == 0 && counts) {
        atomicAdd(&acc[0], nz);
        atomicAdd(&acc[1], pos);
    }
    __syncthreads();
    if (threadIdx.x == 0 && counts) {
        atomicAdd(counts + 2 * ((size_t)first_view + view), acc[0]);
        atomicAdd(counts + 2 * ((size_t)first_view + view) + 1, acc[1]);
    }
}

__global__ void __launch_bounds__(MASK_THREADS) mask_dilate_k(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                             long long total, int H, int W, int Wwords, int r) {
    const uint64_t tail = last_word_bits(W);
    for (long long g = (long long)blockIdx.x * MASK_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * MASK_THREADS) {
        const long long vy = g / Wwords;
        const int wd = (int)(g - vy * Wwords);
        const int y = (int)(vy % H);
        const uint64_t* base = src + (size_t)(vy - y) * Wwords + wd;  // word wd of row 0 of this view
        const int y0 = max(0, y - r), y1 = min(H - 1, y + r);
        uint64_t c = 0, lo = 0, hi = 0;  // the column OR of words wd, wd - 1, wd + 1 (outside the row: 0)
        for (int yy = y0; yy <= y1; ++yy) {
            const uint64_t* row = base + (size_t)yy * Wwords;
            c |= row[0];
            if (wd > 0) lo |= row[-1];
            if (wd + 1 < Wwords) hi |= row[1];
        }
        uint64_t out = c;
        for (int d = 1; d <= r; ++d) {  // pixel x takes x - d (from lower bits / word wd - 1) and x + d (higher / wd + 1)
            out |= (c << d) | (lo >> (64 - d));
            out |= (c >> d) | (hi << (64 - d));
        }
        if (wd == Wwords - 1) out &= tail;
        dst[g] = out;
    }
}

__global__ void __launch_bounds__(MASK_THREADS) mask_unpack_k(const uint64_t* __restrict__ packed, int n_views, const long long* __restrict__ index,
                                                             long long total, int H, int W, int Wwords, uint8_t* __restrict__ out) {
    const long long HW = (long long)H * W;
    for (long long g = (long long)blockIdx.x * MASK_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * MASK_THREADS) {
        const long long k = g / HW;
        const long long p = g - k * HW;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const long long view = index ? index[k] : k;
        if (view < 0 || view >= n_views) {  // an index naming no view of the buffer unpacks to an empty mask
            out[g] = 0;
            continue;
        }
        const uint64_t word = packed[((size_t)view * H + y) * Wwords + (x >> 6)];
        out[g] = (uint8_t)((word >> (x & 63)) & 1ull);
    }
}

__global__ void __launch_bounds__(MASK_THREADS) mask_confusion_k(const uint64_t* __restrict__ pred, const uint64_t* __restrict__ gt,
                                                                int H, int Wwords, uint64_t tail, long long* __restrict__ out) {
    __shared__ unsigned long long part[MASK_WAVES][4];
    const int view = blockIdx.x;
    const long long words = (long long)H * Wwords;
    const uint64_t* p = pred + (size_t)view * words;
    const uint64_t* q = gt + (size_t)view * words;
    unsigned long long tp = 0, fp = 0, fn = 0, tn = 0;
    for (long long g = threadIdx.x; g < words; g += MASK_THREADS) {
        const uint64_t a = p[g], b = q[g];
        const uint64_t valid = ((g % Wwords) == Wwords - 1) ? tail : ~0ull;
        tp += __popcll(a & b);
        fp += __popcll(a & ~b);
        fn += __popcll(~a & b);
        tn += __popcll(~a & ~b & valid);
    }
    tp = wave_sum(tp);
    fp = wave_sum(fp);
    fn = wave_sum(fn);
    tn = wave_sum(tn);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = tp;
        part[wave][1] = fp;
        part[wave][2] = fn;
        part[wave][3] = tn;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
        for (int w = 0; w < MASK_WAVES; ++w) s += part[w][threadIdx.x];
        out[(size_t)view * 4 + threadIdx.x] = (long long)s;
    }
}

inline int grid_for(long long items, int per_block, int cap) {
    const long long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_semantic_mask_pack(const void* src, int src_dtype, int n_views, int H, int W, int first_view, uint64_t* packed, long long* counts,
                  void* stream) {
    if (mask_dims("goi_semantic_mask_pack", H, W) < 0) return -1;
    if (src_dtype != GOI_MASK_F32 && src_dtype != GOI_MASK_U8) return fail("goi_semantic_mask_pack: src_dtype must be GOI_MASK_F32 or GOI_MASK_U8");
    if (n_views < 0 || n_views > 65535 || first_view < 0) return fail("goi_semantic_mask_pack: need 0 <= n_views <= 65535, first_view >= 0");
    if (n_views == 0) return 0;
    if (!src || !packed) return fail("goi_semantic_mask_pack: NULL src or packed");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int Wwords = (W + 63) / 64;
    const dim3 grid(grid_for((long long)H * Wwords, PACK_WAVES * PACK_UNROLL, 64), n_views);
    auto* c = reinterpret_cast<unsigned long long*>(counts);
    if (src_dtype == GOI_MASK_F32)
        mask_pack_k<float><<<grid, PACK_THREADS, 0, s>>>(static_cast<const float*>(src), H, W, Wwords, first_view, packed, c);
    else
        mask_pack_k<uint8_t><<<grid, PACK_THREADS, 0, s>>>(static_cast<const uint8_t*>(src), H, W, Wwords, first_view, packed, c);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_mask_dilate(const uint64_t* src, uint64_t* dst, int n_views, int H, int W, int radius, void* stream) {
    if (mask_dims("goi_semantic_mask_dilate", H, W) < 0) return -1;
    if (radius < 0 || radius > GOI_MASK_MAX_RADIUS) return fail("goi_semantic_mask_dilate: need 0 <= radius <= 63");
    if (n_views < 0) return fail("goi_semantic_mask_dilate: need n_views >= 0");
    if (n_views == 0) return 0;
    if (!src || !dst) return fail("goi_semantic_mask_dilate: NULL src or dst");
    if (src == dst) return fail("goi_semantic_mask_dilate: dst must not be src");
    const int Wwords = (W + 63) / 64;
    const long long total = (long long)n_views * H * Wwords;
    mask_dilate_k<<<grid_for(total, MASK_THREADS, 4096), MASK_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        src, dst, total, H, W, Wwords, radius);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_mask_unpack(const uint64_t* packed, int n_views, int H, int W, int n_out, const long long* index, uint8_t* out,
                             void* stream) {
    if (mask_dims("goi_semantic_mask_unpack", H, W) < 0) return -1;
    if (n_out < 0 || n_views < 0) return fail("goi_semantic_mask_unpack: need n_out >= 0 and n_views >= 0");
    if (n_out == 0) return 0;
    if (!packed || !out) return fail("goi_semantic_mask_unpack: NULL packed or out");
    const int Wwords = (W + 63) / 64;
    const long long total = (long long)n_out * H * W;
    mask_unpack_k<<<grid_for(total, MASK_THREADS, 8192), MASK_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        packed, n_views, index, total, H, W, Wwords, out);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_semantic_mask_confusion(const uint64_t* pred, const uint64_t* gt, int n_views, int H, int W, long long* out, void* stream) {
    if (mask_dims("goi_semantic_mask_confusion", H, W) < 0) return -1;
    if (n_views < 0) return fail("goi_semantic_mask_confusion: need n_views >= 0");
    if (n_views == 0) return 0;
    if (!pred || !gt || !out) return fail("goi_semantic_mask_confusion: NULL pred, gt or out");
    const int Wwords = (W + 63) / 64;
    const uint64_t tail = (W & 63) ? ((1ull << (W & 63)) - 1ull) : ~0ull;
    mask_confusion_k<<<n_views, MASK_THREADS, 0, static_cast<hipStream_t>(stream)>>>(pred, gt, H, Wwords, tail, out);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
