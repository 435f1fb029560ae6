// Peak blend weight per Gaussian and the dominant contributor per pixel, from what a forward left behind
// (goi_raster_contrib_frame), and blend-weight votes per (Gaussian, label) for a 2D label map on the same
// walk (goi_raster_contrib_votes, votes_k below).
//
// One replay of the frame's tile lists with the forward's own pair evaluation and no feature arithmetic: one wave per 8x8
// quadrant, one pixel per lane, the list walked exactly as render_fwd_k walks it -- candidates by ellipse_hits_quadrant, a
// pixel LIVE until a pair that passes both alpha guards fails T (1 - alpha) >= kTMin, the wave done when no lane is live.
// The recorded member masks are NOT walked: the pair that ends a pixel (its stopper) is no member, and it counts here.
//
// Per pair that passes both guards on a live pixel: w = alpha * T and test_T = T * (1 - alpha), the two fp32 operations of
// render_fwd_k's apply(), spelled with the rounding intrinsics so that nothing fuses or reassociates them.
//   peak[id]   the largest w of the Gaussian over every live pixel inside the image, contributors AND stoppers (a stopper's w
//              is what it would have added), merged by maximum with what the caller left there.  w >= 0, so the bit patterns
//              order like the values: one integer atomicMax per (quadrant, Gaussian) after a wave maximum -- order-free,
//              the same bits every run, no float atomics.  The array only grows, so a plain load that finds it at least as
//              large already skips the atomic.
//   top_id / top_w   the pixel's dominant CONTRIBUTOR (stopper excluded: it added nothing to the picture) and its weight; the
//              front-most wins a tie (strict >, in list order); -1 / 0 where nothing contributed.
// A Gaussian whose peak is 0 over a camera set never passed the guards on a live pixel of any of those frames: without it
// every pixel's sequence of live hits, and therefore every output map, is unchanged bit for bit.
#include "blend_common.h"
#include "entry.h"

namespace goi {

namespace {

// Largest of the wave's 64 unsigned values, as a scalar: a shift-and-max ladder inside the 16-lane rows (row_shr 1, 2, 4,
// 8: lane 15 of a row then holds the row's maximum), the rows joined by row_bcast 15 / 31, the result read from lane 63.
// Lanes without a source keep `old` = 0, the identity.  Six VALU instructions and one v_readlane, no LDS; all 64 lanes must
// be active (every call site is in wave-uniform control flow of a 64-thread workgroup).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define GOI_DPP_MAX(CTRL, ROWS) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false))
    GOI_DPP_MAX(0x111, 0xf);  // row_shr:1
    GOI_DPP_MAX(0x112, 0xf);  // row_shr:2
    GOI_DPP_MAX(0x114, 0xf);  // row_shr:4
    GOI_DPP_MAX(0x118, 0xf);  // row_shr:8
    GOI_DPP_MAX(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    GOI_DPP_MAX(0x143, 0xc);  // row_bcast:31 into rows 2 and 3
#undef GOI_DPP_MAX
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(64) void contrib_k(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int P,
                                                int W, int H, int gx, int n_quads, const GaussRec* __restrict__ rec,
                                                const uint32_t* __restrict__ frame_flags, uint32_t* __restrict__ peak,
                                                int* __restrict__ top_id, float* __restrict__ top_w) {
    __shared__ f32x4 s_geo[64];
    __shared__ f32x4 s_geo2[64];
    const QuadGeom t = quad_geom(W, H, gx, n_quads);
    if (t.tile < 0) return;
    const int lane = t.lane;
    const size_t pix_id = (size_t)W * t.py + t.px;
    if (frame_flags[0] != 0) {  // truncated / missorted frame: its lists are not the frame's -- nothing is merged
        if (t.inside) {
            if (top_id) top_id[pix_id] = -1;
            if (top_w) top_w[pix_id] = 0.f;
        }
        return;
    }
    const uint2 range = ranges[t.tile];
    const int len = (int)(range.y - range.x);
    const int rounds = (len + 63) / 64;
    const float QCX = t.QX0 + 3.5f, QCY = t.QY0 + 3.5f;
    const f32x2 uv = {t.pxf - QCX, t.pyf - QCY};

    float T_live = t.inside ? 1.0f : 0.0f;  // as render_fwd_k: the transmittance while the pixel is live, 0 once it is done
    unsigned long long live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);
    float best_w = 0.f;
    int best_id = -1;

    uint32_t id_n = 0;
    float4 q0_n = make_float4(0, 0, 0, 0), q1_n = make_float4(1.f, 0.f, -1.f, -1.f);
    auto prefetch = [&](int b) {
        const int k = b * 64 + lane;
        q1_n.z = -1.f;  // hx < 0: an absent lane hits nothing
        if (k < len) {
            id_n = point_list[range.x + k];
            const float4* r4 = reinterpret_cast<const float4*>(rec + id_n);
            q0_n = r4[0];
            q1_n = r4[1];
        }
    };
    if (rounds > 0) prefetch(0);

    for (int b = 0; b < rounds && live != 0; b++) {
        const uint32_t id = id_n;
        const float4 q0 = q0_n, q1 = q1_n;
        const bool hit = ellipse_hits_quadrant(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, t.QX0, t.QY0);
        if (b + 1 < rounds) prefetch(b + 1);
        unsigned long long m = __ballot(hit);
        if (m != 0 && hit) {
            const PolyCoef pc = poly_coefs(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, QCX, QCY);
            s_geo[lane] = f32x4{pc.A35.x, pc.A35.y, pc.A12.x, pc.A12.y};
            s_geo2[lane] = f32x4{pc.A0, pc.A4, pc.lim, 0.f};
        }
        __builtin_amdgcn_wave_barrier();

        uint32_t slot_max = 0;  // lane j: the wave maximum of w for the Gaussian it staged (slot = lane), as bits
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const f32x4 g = s_geo[j], g2 = s_geo2[j];
            const PairEval e = eval_poly(g.xy, g.zw, g2.x, g2.y, g2.z, uv);
            const float test_T = __fmul_rn(T_live, __fsub_rn(1.f, e.alpha));
            const bool ok = test_T >= kTMin;
            const unsigned long long hm = __builtin_amdgcn_ballot_w64(e.below) & __builtin_amdgcn_ballot_w64(e.seen);
            if ((hm & live) == 0) continue;  // no live pixel passes the guards: nothing to record, nothing ends
            const float wgt = __fmul_rn(e.alpha, T_live);  // (a finished pixel: alpha * 0 = 0)
            if (peak) {
                const uint32_t wmax = wave_max_u32(e.hit ? __float_as_uint(wgt) : 0u);
                slot_max = lane == j ? wmax : slot_max;
            }
            const int gid = __builtin_amdgcn_readlane((int)id, j);
            if (e.hit && ok) {
                if (wgt > best_w) {
                    best_w = wgt;
                    best_id = gid;
                }
                T_live = test_T;
            }
            const unsigned long long em = hm & ~__builtin_amdgcn_ballot_w64(ok);
            if ((em & live) != 0) {
                if (e.hit && !ok) T_live = 0.0f;
                live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);
                if (live == 0) m = 0;
            }
        }
        // one atomic per (quadrant, Gaussian) that reached a live pixel, all of the round's in one wave instruction
        if (peak && slot_max != 0 && id < (uint32_t)P) {
            if (peak[id] < slot_max) atomicMax(&peak[id], slot_max);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (t.inside) {
        if (top_id) top_id[pix_id] = best_id;
        if (top_w) top_w[pix_id] = best_w;
    }
}

// Sum of the wave's 64 unsigned values, as a scalar: wave_max_u32's ladder with an add.  Lanes without a source add `old` = 0.
// The caller guarantees that the sum fits (here: 64 values below 2^24).  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#define GOI_DPP_ADD(CTRL, ROWS) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false)
    GOI_DPP_ADD(0x111, 0xf);  // row_shr:1
    GOI_DPP_ADD(0x112, 0xf);  // row_shr:2
    GOI_DPP_ADD(0x114, 0xf);  // row_shr:4
    GOI_DPP_ADD(0x118, 0xf);  // row_shr:8
    GOI_DPP_ADD(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    GOI_DPP_ADD(0x143, 0xc);  // row_bcast:31 into rows 2 and 3
#undef GOI_DPP_ADD
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Blend-weight votes per (Gaussian, label) (goi_raster_contrib_votes): contrib_k's walk, and for every pair
// that CONTRIBUTES to a pixel (guards passed, test_T >= kTMin: the stopper is excluded, it added nothing to the picture)
// whose label l is in [0, K):  votes[id * K + l] += q,  q = w * 2^24 rounded half-to-even to an integer (the product is
// exact in fp32; w >= kTMin / 255 > 2^-25, so q >= 1).  Integer sums: order-free, the same bits every run.
//   uniform quadrant (one distinct valid label, the common case of a segmentation mask): a wave sum per pair, kept by the
//       lane that staged the Gaussian; the round's sums leave in ONE wave instruction of 64-bit atomics, as contrib_k's peak;
//   mixed quadrant: a prologue finds, label by label, the lanes that hold a label ALONE and the first lane of every label
//       that several lanes share.  Per pair a lone lane adds its own q, the first lane of a shared label the label's masked wave
//       sum (taken only when one of its lanes contributed): ONE wave instruction of atomics per pair, a lane per label.
// A wave sum is below 64 * 0.99 * 2^24 < 2^30.  A quadrant without a valid label leaves at once.
__global__ __launch_bounds__(64) void votes_k(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int P,
                                              int W, int H, int gx, int n_quads, const GaussRec* __restrict__ rec,
                                              const uint32_t* __restrict__ frame_flags, const int* __restrict__ labels, int K,
                                              unsigned long long* __restrict__ votes) {
    __shared__ f32x4 s_geo[64];
    __shared__ f32x4 s_geo2[64];
    const QuadGeom t = quad_geom(W, H, gx, n_quads);
    if (t.tile < 0) return;
    const int lane = t.lane;
    if (frame_flags[0] != 0) return;  // truncated / missorted frame: its lists are not the frame's -- nothing is added
    int lab = t.inside ? labels[(size_t)W * t.py + t.px] : -1;
    if ((uint32_t)lab >= (uint32_t)K) lab = -1;  // every label outside [0, K) is ignored
    const unsigned long long valid = __builtin_amdgcn_ballot_w64(lab >= 0);
    if (valid == 0) return;
    const int lab0 = __builtin_amdgcn_readlane(lab, __builtin_ctzll(valid));
    const bool mixed = __builtin_amdgcn_ballot_w64(lab >= 0 && lab != lab0) != 0;
    bool alone = false;            // mixed: no other lane of the quadrant holds this lane's label
    unsigned long long firsts = 0;  // mixed, bit f: lane f is the first lane of a label that several lanes share
    if (mixed) {
        unsigned long long rem = valid;
        do {
            const int f = __builtin_ctzll(rem);
            const int lf = __builtin_amdgcn_readlane(lab, f);
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(lab == lf);
            rem &= ~cm;
            const bool one = (cm & (cm - 1)) == 0;
            if (lab == lf) alone = one;
            if (!one) firsts |= 1ull << f;
        } while (rem);
    }
    const uint2 range = ranges[t.tile];
    const int len = (int)(range.y - range.x);
    const int rounds = (len + 63) / 64;
    const float QCX = t.QX0 + 3.5f, QCY = t.QY0 + 3.5f;
    const f32x2 uv = {t.pxf - QCX, t.pyf - QCY};

    float T_live = t.inside ? 1.0f : 0.0f;
    unsigned long long live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);

    uint32_t id_n = 0;
    float4 q0_n = make_float4(0, 0, 0, 0), q1_n = make_float4(1.f, 0.f, -1.f, -1.f);
    auto prefetch = [&](int b) {
        const int k = b * 64 + lane;
        q1_n.z = -1.f;  // hx < 0: an absent lane hits nothing
        if (k < len) {
            id_n = point_list[range.x + k];
            const float4* r4 = reinterpret_cast<const float4*>(rec + id_n);
            q0_n = r4[0];
            q1_n = r4[1];
        }
    };
    if (rounds > 0) prefetch(0);

    for (int b = 0; b < rounds && live != 0; b++) {
        const uint32_t id = id_n;
        const float4 q0 = q0_n, q1 = q1_n;
        const bool hit = ellipse_hits_quadrant(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, t.QX0, t.QY0);
        if (b + 1 < rounds) prefetch(b + 1);
        unsigned long long m = __ballot(hit);
        if (m != 0 && hit) {
            const PolyCoef pc = poly_coefs(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, QCX, QCY);
            s_geo[lane] = f32x4{pc.A35.x, pc.A35.y, pc.A12.x, pc.A12.y};
            s_geo2[lane] = f32x4{pc.A0, pc.A4, pc.lim, 0.f};
        }
        __builtin_amdgcn_wave_barrier();

        uint32_t slot_sum = 0;  // uniform quadrant, lane j: the wave sum of q for the Gaussian it staged (slot = lane)
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const f32x4 g = s_geo[j], g2 = s_geo2[j];
            const PairEval e = eval_poly(g.xy, g.zw, g2.x, g2.y, g2.z, uv);
            const float test_T = __fmul_rn(T_live, __fsub_rn(1.f, e.alpha));
            const bool ok = test_T >= kTMin;
            const unsigned long long hm = __builtin_amdgcn_ballot_w64(e.below) & __builtin_amdgcn_ballot_w64(e.seen);
            if ((hm & live) == 0) continue;  // no live pixel passes the guards: nothing to add, nothing ends
            const float wgt = __fmul_rn(e.alpha, T_live);
            // (a finished pixel has T_live = 0: test_T = 0 fails `ok`)
            const uint32_t qv = (e.hit && ok && lab >= 0) ? __float2uint_rn(__fmul_rn(wgt, 16777216.f)) : 0u;
            if (!mixed) {
                const uint32_t sum = wave_sum_u32(qv);
                slot_sum = lane == j ? sum : slot_sum;
            } else {
                if (__builtin_amdgcn_ballot_w64(qv != 0) != 0) {
                    uint32_t add = alone ? qv : 0u;  // what this lane adds to ITS label: a lone lane its q, a first lane the label's sum
                    for (unsigned long long rem = firsts; rem; rem &= rem - 1) {
                        const int f = __builtin_ctzll(rem);
                        const bool mine = lab == __builtin_amdgcn_readlane(lab, f);
                        if (__builtin_amdgcn_ballot_w64(mine && qv != 0) == 0) continue;
                        const uint32_t sum = wave_sum_u32(mine ? qv : 0u);
                        add = lane == f ? sum : add;
                    }
                    const uint32_t gid = (uint32_t)__builtin_amdgcn_readlane((int)id, j);
                    // one atomic per (quadrant, Gaussian, label) with a contribution, all of the pair's in one wave instruction
                    if (add != 0 && gid < (uint32_t)P) atomicAdd(&votes[(size_t)gid * K + lab], (unsigned long long)add);
                }
            }
            if (e.hit && ok) T_live = test_T;
            const unsigned long long em = hm & ~__builtin_amdgcn_ballot_w64(ok);
            if ((em & live) != 0) {
                if (e.hit && !ok) T_live = 0.0f;
                live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);
                if (live == 0) m = 0;
            }
        }
        // uniform: one atomic per (quadrant, Gaussian) that contributed, all of the round's in one wave instruction
        if (slot_sum != 0 && id < (uint32_t)P) atomicAdd(&votes[(size_t)id * K + lab0], (unsigned long long)slot_sum);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_raster_contrib_frame(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                             const void* image_buffer, float* peak, int* top_id, float* top_w, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P <= 0 || W <= 0 || H <= 0 || R < 0) return fail("goi_raster_contrib_frame: bad P/W/H/R");
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail("goi_raster_contrib_frame: workspace pointer is NULL");
    if (!peak && !top_id && !top_w) return fail("goi_raster_contrib_frame: peak, top_id and top_w are all NULL");
    if (R == 0) {  // nothing listed: peak stays as it is, no pixel has a contributor
        const size_t HW = (size_t)W * H;
        if (top_id) GOI_HIP(hipMemsetAsync(top_id, 0xFF, HW * sizeof(int), s));
        if (top_w) GOI_HIP(hipMemsetAsync(top_w, 0, HW * sizeof(float), s));
        return 0;
    }
    const FrameViews f = frame_views(P, W, H, R, geom_buffer, image_buffer, binning_buffer);
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int n_quads = gx * gy * 4;
    contrib_k<<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(f.im.ranges, f.plist, P, W, H, gx, n_quads, f.g.rec,
                                                            f.g.counters + COUNTER_OVF, reinterpret_cast<uint32_t*>(peak), top_id,
                                                            top_w);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_contrib_votes(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                             const void* image_buffer, const int* labels, int K, int64_t* votes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P <= 0 || W <= 0 || H <= 0 || R < 0) return fail("goi_raster_contrib_votes: bad P/W/H/R");
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail("goi_raster_contrib_votes: workspace pointer is NULL");
    if (!labels || !votes) return fail("goi_raster_contrib_votes: labels or votes is NULL");
    if (K < 1) return fail("goi_raster_contrib_votes: K must be at least 1");
    if (R == 0) return 0;  // nothing listed: nothing is added, nothing is launched
    const FrameViews f = frame_views(P, W, H, R, geom_buffer, image_buffer, binning_buffer);
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int n_quads = gx * gy * 4;
    votes_k<<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(f.im.ranges, f.plist, P, W, H, gx, n_quads, f.g.rec,
                                                          f.g.counters + COUNTER_OVF, labels, K,
                                                          reinterpret_cast<unsigned long long*>(votes));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
