// Lane utilisation of the blend kernels, MEASURED from what a forward left behind (diagnostic; goi_raster_blend_stats).
//
// Both blend kernels give one wave to an 8x8 quadrant and one loop trip to a (quadrant, Gaussian) pair
// (render_fwd.hip, render_bwd.hip; the reference's loops are CR/forward.cu:330-372 and CR/backward.cu:523-589, one thread
// per pixel of a 16x16 tile).  How many of the 64 lanes do useful work in such a trip is a property of the scene, and
// this kernel counts it exactly: it re-walks every quadrant's list over the positions the backward walks (up to the
// quadrant's last contributor, ImageView::qcost), re-evaluates every MEMBER pair (the masks the forward recorded) with the
// same two functions the blend kernels use, and counts the lanes whose pixel composited that Gaussian (position below the
// pixel's n_contrib and both alpha guards passed -- the backward's own condition, and exactly the pairs the forward
// accumulated).  The same pass counts what denser mappings would see -- a wave split into 8x4, 4x4 or 2x2 pixel blocks
// that each walk their own list: the number of (block, Gaussian) pairs with at least one live lane -- and how many
// candidates pass the forward's quadrant hit test (its evaluated pairs).
#include "blend_common.h"
#include "entry.h"

namespace goi {

namespace {

__global__ __launch_bounds__(64) void blend_stats_k(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                                                    int W, int H, int gx, int n_quads, const GaussRec* __restrict__ rec,
                                                    const uint32_t* __restrict__ n_contrib,
                                                    const uint32_t* __restrict__ qcost,
                                                    const unsigned long long* __restrict__ qmask0,
                                                    const unsigned long long* __restrict__ qmask,
                                                    unsigned long long* __restrict__ out) {
    __shared__ f32x4 s_geo[64];
    __shared__ f32x4 s_geo2[64];
    const QuadGeom t = quad_geom(W, H, gx, n_quads);
    if (t.tile < 0) return;
    const int tq = quad_slot();
    const int lane = t.lane;
    const uint2 range = ranges[t.tile];
    const int len = (int)(range.y - range.x);
    const int n_proc = min((int)qcost[tq], len);
    const size_t pix_id = (size_t)W * t.py + t.px;
    const uint32_t nc = t.inside ? n_contrib[pix_id] : 0u;
    const float QCX = t.QX0 + 3.5f, QCY = t.QY0 + 3.5f;
    const f32x2 uv = {t.pxf - QCX, t.pyf - QCY};
    unsigned long long c_rounds = 0, c_cand = 0, c_hits = 0, c_members = 0, c_live = 0, c_m84 = 0, c_m44 = 0, c_m22 = 0,
                       c_dead = 0;
    const int rounds = (n_proc + 63) / 64;
    for (int b = 0; b < rounds; b++) {
        const int pos = b * 64 + lane;
        const bool present = pos < n_proc;
        float4 q0 = make_float4(0, 0, 0, 0), q1 = make_float4(1.f, 0.f, -1.f, -1.f);
        if (present) {
            const uint32_t id = point_list[range.x + (uint32_t)pos];
            const float4* r4 = reinterpret_cast<const float4*>(rec + id);
            q0 = r4[0];
            q1 = r4[1];
        }
        const bool hit = ellipse_hits_quadrant(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, t.QX0, t.QY0);
        unsigned long long members = *member_mask_ptr(const_cast<unsigned long long*>(qmask0),
                                                      const_cast<unsigned long long*>(qmask), t.tile, t.q, range.x, b);
        members = uniform_u64(members);
        if (n_proc - b * 64 < 64) members &= (1ull << (n_proc - b * 64)) - 1ull;
        c_cand += (unsigned long long)__popcll(__ballot(present));
        c_hits += (unsigned long long)__popcll(__ballot(hit));
        if ((members >> lane) & 1ull) {
            const PolyCoef pc = poly_coefs(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, QCX, QCY);
            s_geo[lane] = f32x4{pc.A35.x, pc.A35.y, pc.A12.x, pc.A12.y};
            s_geo2[lane] = f32x4{pc.A0, pc.A4, pc.lim, 0.f};
        }
        __builtin_amdgcn_wave_barrier();
        c_rounds++;
        c_members += (unsigned long long)__popcll(members);
        unsigned long long m = members;
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const f32x4 g = s_geo[j], g2 = s_geo2[j];
            const PairEval e = eval_poly(g.xy, g.zw, g2.x, g2.y, g2.z, uv);
            const bool live = e.hit && (uint32_t)(b * 64 + j) < nc;
            const unsigned long long lv = __ballot(live);
            c_live += (unsigned long long)__popcll(lv);
            c_dead += lv == 0 ? 1ull : 0ull;
            c_m84 += ((lv & 0xFFFFFFFFull) != 0) + ((lv >> 32) != 0);
            c_m44 += ((lv & 0x000000000F0F0F0Full) != 0) + ((lv & 0x00000000F0F0F0F0ull) != 0) +
                     ((lv & 0x0F0F0F0F00000000ull) != 0) + ((lv & 0xF0F0F0F000000000ull) != 0);
            unsigned long long f = lv | (lv >> 1);
            f |= f >> 8;
            c_m22 += (unsigned long long)__popcll(f & 0x0055005500550055ull);
        }
        __builtin_amdgcn_wave_barrier();
    }
    const unsigned long long c_pix = (unsigned long long)__popcll(__ballot(t.inside));
    unsigned long long c_nc = (unsigned long long)nc;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c_nc += __shfl_xor(c_nc, d, 64);
    if (lane == 0) {
        atomicAdd(&out[0], n_proc > 0 ? 1ull : 0ull);
        atomicAdd(&out[1], c_rounds);
        atomicAdd(&out[2], c_cand);
        atomicAdd(&out[3], c_hits);
        atomicAdd(&out[4], c_members);
        atomicAdd(&out[5], c_live);
        atomicAdd(&out[6], c_m84);
        atomicAdd(&out[7], c_m44);
        atomicAdd(&out[8], c_m22);
        atomicAdd(&out[9], c_dead);
        atomicAdd(&out[10], c_pix);
        atomicAdd(&out[11], c_nc);
    }
}

// One (pixel, Gaussian) evaluation per lane, as the blend kernels do it, written out (tests only; goi_raster_debug_pair_eval).
// One wave per request (Gaussian id, quadrant index 4 tile + q): the quadrant geometry comes from quad_geom_of, the centre and the
// lane's (u, v) are formed as in render_fwd_k / render_bwd_rows_k, the coefficients by ONE call of poly_coefs (every lane forms
// the same ones: which path a Gaussian takes depends on its own S only) and the pair by eval_poly.  Lanes outside the image
// evaluate like any other: that is what the blend kernels' lanes do before `inside` masks them.  A request that names no
// Gaussian or no quadrant writes NaN and guard byte 0x80.
__global__ __launch_bounds__(64) void pair_eval_k(const uint2* __restrict__ req, long long first, long long n, int P, int W, int H,
                                                  int gx, int n_quads, const GaussRec* __restrict__ rec, float* __restrict__ E,
                                                  float* __restrict__ alpha, uint8_t* __restrict__ guards) {
    const long long r = first + (long long)blockIdx.x;
    if (r >= n) return;
    const uint2 rq = req[r];
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)r * 64 + lane;
    const QuadGeom t = quad_geom_of(rq.y < (uint32_t)n_quads ? (int)rq.y : -1, W, H, gx, n_quads);
    if (t.tile < 0 || rq.x >= (uint32_t)P) {
        E[o] = alpha[o] = __builtin_nanf("");
        guards[o] = 0x80;
        return;
    }
    const float4* r4 = reinterpret_cast<const float4*>(rec + rq.x);
    const float4 q0 = r4[0], q1 = r4[1];
    const float QCX = t.QX0 + 3.5f, QCY = t.QY0 + 3.5f;
    const f32x2 uv = {t.pxf - QCX, t.pyf - QCY};
    const PolyCoef pc = poly_coefs(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, QCX, QCY);
    const PairEval e = eval_poly(pc.A35, pc.A12, pc.A0, pc.A4, pc.lim, uv);
    E[o] = e.E;
    alpha[o] = e.alpha;
    guards[o] = (uint8_t)((e.below ? 1 : 0) | (e.seen ? 2 : 0));
}

}  // namespace

static void launch_pair_eval(int P, int W, int H, const GeomView& g, const uint32_t* requests, long long n, float* E,
                             float* alpha, uint8_t* guards, hipStream_t s) {
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    constexpr long long CHUNK = 1ll << 20;  // requests per launch: a whole frame's member pairs go through in a few launches
    for (long long first = 0; first < n; first += CHUNK) {
        const long long cnt = n - first < CHUNK ? n - first : CHUNK;
        pair_eval_k<<<dim3((unsigned)cnt), dim3(64), 0, s>>>(reinterpret_cast<const uint2*>(requests), first, n, P, W, H, gx,
                                                            gx * gy * 4, g.rec, E, alpha, guards);
    }
}

}  // namespace goi

using namespace goi;

extern "C" {

int goi_raster_debug_pair_eval(int P, int W, int H, const void* geom_buffer, const uint32_t* requests, long long n_requests,
                               float* E, float* alpha, uint8_t* guards, void* stream) {
    const std::string fn = "goi_raster_debug_pair_eval";
    if (P <= 0 || W <= 0 || H <= 0) return fail(fn + ": bad P/W/H");
    if (n_requests < 0 || n_requests > (1ll << 31)) return fail(fn + ": need 0 <= n_requests <= 2^31");
    if (n_requests == 0) return 0;
    if (!requests || !E || !alpha || !guards) return fail(fn + ": a required pointer is NULL");
    if (check_workspace(fn, geom_buffer, "geom_buffer") < 0) return -1;
    if (reinterpret_cast<uintptr_t>(requests) & 7u) return fail(fn + ": requests must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(E) & 3u) || (reinterpret_cast<uintptr_t>(alpha) & 3u))
        return fail(fn + ": E and alpha must be 4-byte aligned");
    const GeomView g = frame_views(P, W, H, 0, geom_buffer, nullptr, nullptr).g;
    launch_pair_eval(P, W, H, g, requests, n_requests, E, alpha, guards, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_blend_stats(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                           const void* image_buffer, unsigned long long* counters, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P <= 0 || W <= 0 || H <= 0 || R < 0) return fail("goi_raster_blend_stats: bad P/W/H/R");
    if (!geom_buffer || !image_buffer || !counters || (R > 0 && !binning_buffer)) return fail("workspace pointer is NULL");
    GOI_HIP(hipMemsetAsync(counters, 0, GOI_BLEND_STATS_WORDS * sizeof(unsigned long long), s));
    if (R == 0) return 0;
    const FrameViews f = frame_views(P, W, H, R, geom_buffer, image_buffer, binning_buffer);
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int n_quads = gx * gy * 4;
    blend_stats_k<<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(f.im.ranges, f.plist, W, H, gx, n_quads, f.g.rec, f.im.n_contrib,
                                                                 f.im.qcost, f.im.qmask0, f.bv.qmask, counters);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
