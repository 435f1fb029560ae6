// Per-Gaussian forward kernel: preprocess (project, EWA cov2D, conic, radius, tile rectangle, SH -> RGB, render record), with
// markVisible beside it and the goi_raster_mark_visible entry.  Its backward is preprocess_bwd.hip; what the two kernels share is
// preprocess_common.h.  Compiled with -ffp-contract=off: these stages are HBM-bound streaming, and
// keeping the reference's operation order makes radii / tile rectangles / depth keys integer-exact.
//
// Behaviour restated from the reference (paths relative to submodules/diff-gaussian-rasterization/):
//   forward : cuda_rasterizer/forward.cu:155-256 (+ :20-71 SH, :74-113 cov2D, :118-152 cov3D),
//             cuda_rasterizer/auxiliary.h:41-56,139-164
// Layout is this library's own: one 48-byte GaussRec per Gaussian instead of five arrays, depth
// keys for the per-Gaussian depth sort, 3 clamp bits in one byte.
#include "common.h"
#include "entry.h"
#include "preprocess_common.h"

namespace goi {

namespace {

__device__ __forceinline__ float ndc_to_pix(float v, int S) { return (float)(((v + 1.0) * S - 1.0) * 0.5); }

struct PreArgs {
    int P, D, M, W, H, gx, gy, prefiltered, cull;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    float scale_modifier, tan_fovx, tan_fovy, focal_x, focal_y;
    const float* view_p;    // device, [16]
    const float* proj_p;    // device, [16]
    const float* campos_p;  // device, [3]
    // speculative depth cut-off of the tile lists (api.hip, goi_raster_forward_async): zcut[t] = view depth beyond which
    // tile t's list was never walked when this camera was rendered last (NULL: no cut); zlearn[t]: what this frame learns
    // (cleared here, written by the forward blend)
    const float* zcut;
    uint32_t* zlearn;
    // per-Gaussian SELECTION (goi_raster_forward, keep; read by preprocess_fwd_k<true> only): keep[id] is one byte per Gaussian,
    // and Gaussian id is UNSELECTED when (keep[id] != 0) == (keep_invert != 0) -- keep_invert = 0 renders the Gaussians whose byte
    // is set, keep_invert = 1 the others.  NULL: no selection (preprocess_fwd_k<false>).
    const uint8_t* keep;
    int keep_invert;
};

template <typename SHK_T>
__device__ __forceinline__ V3 sh_to_rgb_sum(int D, const V3& dir, SHK_T SHK) {
    V3 res = kSH0 * SHK(0);
    if (D > 0) {
        const float x = dir.x, y = dir.y, z = dir.z;
        res = res - kSH1 * y * SHK(1) + kSH1 * z * SHK(2) - kSH1 * x * SHK(3);
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            res = res + kSH2[0] * xy * SHK(4) + kSH2[1] * yz * SHK(5) + kSH2[2] * (2.0f * zz - xx - yy) * SHK(6) +
                  kSH2[3] * xz * SHK(7) + kSH2[4] * (xx - yy) * SHK(8);
            if (D > 2) {
                res = res + kSH3[0] * y * (3.0f * xx - yy) * SHK(9) + kSH3[1] * xy * z * SHK(10) +
                      kSH3[2] * y * (4.0f * zz - xx - yy) * SHK(11) +
                      kSH3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * SHK(12) +
                      kSH3[4] * x * (4.0f * zz - xx - yy) * SHK(13) + kSH3[5] * z * (xx - yy) * SHK(14) +
                      kSH3[6] * x * (xx - 3.0f * yy) * SHK(15);
            }
        }
    }
    return res + V3{0.5f, 0.5f, 0.5f};
}

#ifndef GOI_PRE_MINBLOCKS
#define GOI_PRE_MINBLOCKS 1
#endif
// SELECT: the frame renders a SELECTION of the Gaussians (PreArgs::keep).  An unselected Gaussian leaves phase A where one behind
// the near plane does, before anything of it has been loaded -- its selection byte is all the kernel ever reads of it -- and is
// from there on what a frustum-culled Gaussian is: radius 0, no tiles, key 0xFFFFFFFF, no record, no instance.  Nothing
// downstream of this kernel knows about selections.  SELECT == false is the kernel as it was.
template <bool SELECT>
__global__ __launch_bounds__(256, GOI_PRE_MINBLOCKS) void preprocess_fwd_k(const PreArgs args, GaussRec* __restrict__ rec,
                                                        float* __restrict__ cov3D_out,
                                                        uint32_t* __restrict__ tiles_touched,
                                                        uint8_t* __restrict__ clamped, uint32_t* __restrict__ raw_key,
                                                        uint4* __restrict__ aux,
                                                        uint2* __restrict__ blk_agg,
                                                        unsigned long long* __restrict__ blk_coarse, int* __restrict__ radii,
                                                        uint32_t* __restrict__ counters, uint2* __restrict__ ranges,
                                                        int n_tiles) {
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
    // the tile ranges start from zero (emit accumulates per-tile counts into them): cleared here for free
    for (int t = gtid; t < n_tiles; t += gridDim.x * blockDim.x) ranges[t] = make_uint2(0u, 0u);
    if (args.zlearn)
        for (int t = gtid; t < n_tiles; t += gridDim.x * blockDim.x) args.zlearn[t] = 0u;
    if (gtid == 0) counters[COUNTER_CULL] = (uint32_t)args.cull;  // emit and the backward list the same rectangles
    // every lane reaches the wave reduction at the end: lanes past P redo the last Gaussian and write nothing
    const bool live = gtid < args.P;
    const int idx = live ? gtid : args.P - 1;
    const Camera cam = load_camera(args.view_p, args.proj_p, args.campos_p);
    struct : PreArgs {
        const float *view, *proj, *campos;
    } a;
    static_cast<PreArgs&>(a) = args;
    a.view = cam.view;
    a.proj = cam.proj;
    a.campos = cam.campos;
    int my_radius_i = 0;
    unsigned long long tmask_v = TMASK_FULL;
    uint32_t touched = 0, key = 0xFFFFFFFFu;
    uint8_t clamp_bits = 0;

    // (a lane past P looks at the byte of Gaussian P - 1, as it redoes that Gaussian: in bounds, and if that one is unselected
    // the lane leaves phase A with it)
    bool unselected = false;
    if constexpr (SELECT) unselected = (args.keep[idx] != 0) == (args.keep_invert != 0);
    V3 p = {0.f, 0.f, 0.f};
    if (!SELECT || !unselected) p = V3{a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]};
    const V3 p_view = xform_point_4x3(p, a.view);
    // ---- phase A: projection, covariance, conic, radius, 3-sigma rectangle: is the Gaussian rendered at all?
    bool vis = false;
    float pix = 0.f, piy = 0.f, con_a = 0.f, con_b = 0.f, con_c = 0.f, my_radius = 0.f;
    do {
        if (SELECT && unselected) break;  // (not the caller's "prefiltered" promise broken: no trap)
        if (p_view.z <= 0.2f) {
            if (a.prefiltered) atomicOr(&counters[1], 1u);  // the reference traps here
            break;
        }
        const float4 p_hom = xform_point_4x4(p, a.proj);
        const float p_w = 1.0f / (p_hom.w + 0.0000001f);
        const float projx = p_hom.x * p_w, projy = p_hom.y * p_w;

        float cov3D[6];
        if (a.cov3D_precomp) {
#pragma unroll
            for (int i = 0; i < 6; i++) cov3D[i] = a.cov3D_precomp[(size_t)6 * idx + i];
        } else {
            M3 S = make_m3(1, 0, 0, 0, 1, 0, 0, 0, 1);
            S.c[0][0] = a.scale_modifier * a.scales[3 * idx];
            S.c[1][1] = a.scale_modifier * a.scales[3 * idx + 1];
            S.c[2][2] = a.scale_modifier * a.scales[3 * idx + 2];
            const float4 q = reinterpret_cast<const float4*>(a.rotations)[idx];  // (r,x,y,z), not normalised
            M3 R = rotation_from_quat(q.x, q.y, q.z, q.w);
            M3 Mm = mul(S, R);
            M3 Sg = mul(transpose(Mm), Mm);
            cov3D[0] = Sg.c[0][0]; cov3D[1] = Sg.c[0][1]; cov3D[2] = Sg.c[0][2];
            cov3D[3] = Sg.c[1][1]; cov3D[4] = Sg.c[1][2]; cov3D[5] = Sg.c[2][2];
#pragma unroll
            for (int i = 0; i < 6; i++) cov3D_out[(size_t)6 * idx + i] = cov3D[i];
        }
        Cov2D c2;
        ewa_cov2d(p, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, cov3D, a.view, c2);
        const float cx = c2.cov.c[0][0] + 0.3f, cy = c2.cov.c[0][1], cz = c2.cov.c[1][1] + 0.3f;
        const float det = cx * cz - cy * cy;
        if (det == 0.0f) break;
        const float det_inv = 1.f / det;
        con_a = cz * det_inv;
        con_b = -cy * det_inv;
        con_c = cx * det_inv;
        const float mid = 0.5f * (cx + cz);
        const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
        const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
        my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
        pix = ndc_to_pix(projx, a.W);
        piy = ndc_to_pix(projy, a.H);
        int x0, y0, x1, y1;
        tile_rect(pix, piy, (int)my_radius, a.gx, a.gy, x0, y0, x1, y1);
        if ((x1 - x0) * (y1 - y0) == 0) break;
        vis = live;  // (a lane past P has redone the last Gaussian up to here: it must not store anything)
    } while (false);

    // ---- phase B: contribution box, listed rectangle, ellipse tile mask (nothing here needs the colour)
    float hx = -1.f, hy = -1.f, o = 0.f;
    if (vis) {
        // Box outside which alpha = min(0.99, o*exp(power)) < 1/255 is certain (see DESIGN.md,
        // "exact contribution box"): the ellipse power >= -tau of the COMPUTED conic, tau inflated.
        o = a.opacities[idx];
        if (o >= 1.0f / 255.0f) {
            // In single precision, every rounding pushed OUTWARD (the box only has to contain the region; its size
            // decides nothing but how many tiles and quadrants are looked at): the double-precision log / sqrt / divide
            // this replaces were software routines of a few hundred instructions on the critical path of every visible lane.
            //   tau = 1.01 ln(255 o) + 0.01, rounded up;  det = a c - b b by Kahan's difference of products (within
            //   1.5 ulp even when the two products cancel: a needle), rounded down;  h = sqrt(2 tau c / det), rounded up.
            const float tau = fmaf(1.01f, logf(255.0f * o), 0.01f) * 1.000002f + 1e-6f;
            const float bb = con_b * con_b;
            const float detc = (fmaf(con_a, con_c, -bb) + fmaf(-con_b, con_b, bb));
            const float det_lo = detc - 4e-7f * fabsf(detc);
            if (det_lo > 0.f && con_a > 0.f && con_c > 0.f) {
                hx = sqrtf(2.0f * tau * con_c / det_lo) * 1.000002f + 1e-3f;
                hy = sqrtf(2.0f * tau * con_a / det_lo) * 1.000002f + 1e-3f;
                if (!(hx == hx) || !(hy == hy)) hx = hy = __builtin_inff();
            } else {
                hx = hy = __builtin_inff();
            }
        }
        my_radius_i = (int)my_radius;
        int x0, y0, x1, y1;
        listed_rect(pix, piy, my_radius_i, hx, hy, a.cull != 0, a.gx, a.gy, x0, y0, x1, y1);
        touched = (uint32_t)((y1 - y0) * (x1 - x0));  // may be 0 for a visible Gaussian (radius stays > 0)
        // cull_variant 2: of that rectangle, only the tiles the contribution ELLIPSE  1/2 d^T C d <= tau  reaches (the
        // box over-covers by 1 - pi/4 for a round Gaussian, by most of its area for an elongated diagonal one: x0.80
        // instances on the headline scene).  Exact for a convex set, one tile row at a time: over the row's pixel-centre
        // band y in [16 t, 16 t + 15], clipped to the ellipse's own extent, the ellipse spans x in [L, R] with
        //     R(dy) = (-b dy + sqrt(2 a tau - det dy^2)) / a   (concave: its maximum over the band is at the band's
        // point nearest to the ellipse's rightmost point dy = -(b/c) hx), L likewise (convex, leftmost point); the row's
        // tiles are those whose pixel-centre range [16 t, 16 t + 15] meets [L, R].  tau carries the box's inflation (1 % +
        // 0.01: the blend kernels' evaluation error of `power` can never move a contributing pixel outside), every
        // rounding here is pushed outward, and a NaN keeps the whole row.  A tile that is dropped can not receive a
        // contribution; the per-pixel sequences of contributing Gaussians, hence all outputs and gradients, are untouched.
        if (a.cull >= 2 && touched > 0 && touched <= 64 && hx < 1e30f && hy < 1e30f) {
            const int w = x1 - x0;
            const float tau = (fmaf(1.01f, logf(255.0f * o), 0.01f) * 1.000002f + 1e-6f) * 1.0001f + 1e-4f;
            const float bb = con_b * con_b;
            const float det = fmaxf((fmaf(con_a, con_c, -bb) + fmaf(-con_b, con_b, bb)) * (1.f - 4e-7f), 0.f);
            const float inv_a = 1.f / con_a;
            const float dyR = -(con_b / con_c) * hx, dyL = -dyR;  // where the ellipse is rightmost / leftmost
            unsigned long long mask = 0ull;
            for (int ry = 0; ry < y1 - y0; ry++) {
                const float lo = fmaxf((float)((y0 + ry) * TILE) - piy, -hy), hi = fminf((float)((y0 + ry) * TILE + TILE - 1) - piy, hy);
                if (!(lo <= hi)) {
                    if (lo == lo && hi == hi) continue;  // the band misses the ellipse's extent
                }
                const float d1 = fminf(fmaxf(dyR, lo), hi), d2 = fminf(fmaxf(dyL, lo), hi);
                const float s1 = sqrtf(fmaxf(2.f * con_a * tau - det * d1 * d1, 0.f));
                const float s2 = sqrtf(fmaxf(2.f * con_a * tau - det * d2 * d2, 0.f));
                float R = (-con_b * d1 + s1) * inv_a, L = (-con_b * d2 - s2) * inv_a;
                R += 1e-3f + 4e-6f * fabsf(R);
                L -= 1e-3f + 4e-6f * fabsf(L);
                // columns t with 16 t <= pix + R and 16 t + 15 >= pix + L
                int c0 = (int)ceilf((pix + L - (float)(TILE - 1)) / TILE), c1 = (int)floorf((pix + R) / TILE) + 1;
                if (!(R == R) || !(L == L)) {
                    c0 = x0;
                    c1 = x1;
                }
                c0 = max(c0, x0);
                c1 = min(c1, x1);
                if (c1 > c0) mask |= ((c1 - c0 >= 64) ? ~0ull : ((1ull << (c1 - c0)) - 1ull)) << (ry * w + (c0 - x0));
            }
            // speculative depth cut-off: a tile whose list was not needed beyond depth zcut[t] the last time this camera was
            // rendered does not list a deeper Gaussian (the forward blend raises the frame's flag if a pixel of such a tile
            // turns out to want more: api.hip).  Eight tiles per trip, their cut depths requested together (one load round
            // trip for the typical 3 x 3 rectangle; tile by tile this loop cost the kernel 28 us).
            if (a.zcut) {
                unsigned long long todo = mask;
                while (todo) {
                    int bits[8];
                    float zc[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        bits[i] = todo ? __builtin_ctzll(todo) : -1;
                        if (todo) todo &= todo - 1;
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int bsafe = max(bits[i], 0);
                        zc[i] = a.zcut[(size_t)(y0 + bsafe / w) * a.gx + (x0 + bsafe % w)];
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        if (bits[i] >= 0 && zc[i] < p_view.z) mask &= ~(1ull << bits[i]);
                }
            }
            tmask_v = mask;
            touched = (uint32_t)__popcll(mask);
        }
        key = __float_as_uint(p_view.z);
    }

    // everything that does not depend on the colour leaves NOW: the values are dead while the SH rows are in registers
    if (vis) {
        float4* r4 = reinterpret_cast<float4*>(rec + idx);
        r4[0] = make_float4(pix, piy, con_a, con_b);
        r4[1] = make_float4(con_c, o, hx, hy);       // what the hit test needs beside q0: fetched for every CANDIDATE
    }
    if (live) {
        radii[idx] = my_radius_i;
        tiles_touched[idx] = touched;
        raw_key[idx] = key;  // depth bits by Gaussian id; compact_listed_k keeps the listed ones for the depth sort
        aux[idx] = make_uint4(0u, (uint32_t)my_radius_i, (uint32_t)tmask_v, (uint32_t)(tmask_v >> 32));  // (.x: emit)
    }

    // ---- phase C: the colour
    float cr = 0.f, cg = 0.f, cb = 0.f;
    V3 dir = {0.f, 0.f, 0.f};
    if (vis && !a.colors_precomp) {
        const V3 campos = {a.campos[0], a.campos[1], a.campos[2]};
        dir = p - campos;
        dir = dir / sqrtf(dot3(dir, dir));
    }
    auto finish_colour = [&](const V3& res) {
        clamp_bits = (uint8_t)((res.x < 0 ? 1 : 0) | (res.y < 0 ? 2 : 0) | (res.z < 0 ? 4 : 0));
        cr = fmaxf(res.x, 0.0f);
        cg = fmaxf(res.y, 0.0f);
        cb = fmaxf(res.z, 0.0f);
    };
    if (vis) {
        if (a.colors_precomp) {
            cr = a.colors_precomp[3 * idx];
            cg = a.colors_precomp[3 * idx + 1];
            cb = a.colors_precomp[3 * idx + 2];
        } else {
            // A degree-3 row (M = 16: 192 bytes, 16-byte aligned) is fetched as TWELVE 16-byte loads instead of sixteen 12-byte ones
            float rowf[48];
            const bool row16 = a.M == 16;
            if (row16) {
                const float4* r4 = reinterpret_cast<const float4*>(a.shs + (size_t)idx * 48);
#pragma unroll
                for (int i = 0; i < 12; i++) {
                    const float4 v = r4[i];
                    rowf[4 * i] = v.x;
                    rowf[4 * i + 1] = v.y;
                    rowf[4 * i + 2] = v.z;
                    rowf[4 * i + 3] = v.w;
                }
            }
            const V3* shg = reinterpret_cast<const V3*>(a.shs) + (size_t)idx * a.M;
            finish_colour(sh_to_rgb_sum(a.D, dir, [&](int k) { return row16 ? V3{rowf[3 * k], rowf[3 * k + 1], rowf[3 * k + 2]} : shg[k]; }));
        }
    }
    // what only a HIT needs (r, g, b, depth: the first staged feature quad as it is)
    if (vis) reinterpret_cast<float4*>(rec + idx)[2] = make_float4(cr, cg, cb, p_view.z);
    if (live) clamped[idx] = clamp_bits;
    // num_rendered = sum of tiles_touched: order-independent, so it is formed HERE (one integer atomic per wave)
    // instead of falling out of the prefix sum after the depth sort -- the host can read it while the sort runs
    __shared__ uint32_t s_wsum[4], s_wvis[4];
    uint32_t wsum = live ? touched : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wsum += (uint32_t)__shfl_xor((int)wsum, d, 64);
    const uint32_t wvis = (uint32_t)__popcll(__ballot(live && touched > 0));  // LISTED Gaussians of this wave
    if ((threadIdx.x & 63) == 0) {
        s_wsum[threadIdx.x >> 6] = wsum;
        s_wvis[threadIdx.x >> 6] = wvis;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t bsum = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        if (bsum) atomicAdd(&counters[NR_BASE + NR_STRIDE * (blockIdx.x % NR_STRIPES)], bsum);
        // the block's aggregate: compact_listed_k ranks the listed Gaussians with it
        const uint32_t bvis = s_wvis[0] + s_wvis[1] + s_wvis[2] + s_wvis[3];
        blk_agg[blockIdx.x] = make_uint2(bvis, bsum);
        // ... and the sum over COARSE_BLOCKS consecutive blocks (compact_listed_k's base rank), packed: one integer atomic
        if (bvis) atomicAdd(&blk_coarse[(size_t)(blockIdx.x / COARSE_BLOCKS) * COARSE_STRIDE], ((unsigned long long)bvis << 40) | bsum);
    }
}

__global__ __launch_bounds__(256) void mark_visible_k(int P, const float* __restrict__ means3D, const float* view,
                                                      uint8_t* __restrict__ present) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P) return;
    const V3 p = {means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]};
    float m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = view[i];
    present[idx] = xform_point_4x3(p, m).z > 0.2f ? 1 : 0;
}

}  // namespace

void launch_preprocess_fwd(const GoiRasterScene& sc, const GeomView& g, int* radii, uint2* ranges, int n_tiles,
                           hipStream_t s, const float* zcut, uint32_t* zlearn, const uint8_t* keep, int keep_invert) {
    PreArgs a;
    a.keep = keep;
    a.keep_invert = keep_invert;
    a.zcut = g_options.cull_variant >= 2 ? zcut : nullptr;  // (the cut lives in the ellipse tile masks)
    a.zlearn = zlearn;
    a.P = sc.P; a.D = sc.D; a.M = sc.M; a.W = sc.W; a.H = sc.H;
    a.gx = (sc.W + TILE - 1) / TILE;
    a.gy = (sc.H + TILE - 1) / TILE;
    a.prefiltered = sc.prefiltered;
    a.cull = g_options.cull_variant;
    a.means3D = sc.means3D; a.shs = sc.shs; a.colors_precomp = sc.colors_precomp; a.opacities = sc.opacities;
    a.scales = sc.scales; a.rotations = sc.rotations; a.cov3D_precomp = sc.cov3D_precomp;
    a.scale_modifier = sc.scale_modifier; a.tan_fovx = sc.tan_fovx; a.tan_fovy = sc.tan_fovy;
    a.focal_y = sc.H / (2.0f * sc.tan_fovy);
    a.focal_x = sc.W / (2.0f * sc.tan_fovx);
    a.view_p = sc.viewmatrix; a.proj_p = sc.projmatrix; a.campos_p = sc.campos;
    static_assert(PRE_BLOCK == 256, "preprocess_fwd_k is written for 256-thread workgroups");
    const dim3 grid((sc.P + PRE_BLOCK - 1) / PRE_BLOCK);
#define GOI_PRE(SELECT)                                                                                                          \
    preprocess_fwd_k<SELECT><<<grid, dim3(PRE_BLOCK), 0, s>>>(a, g.rec, g.cov3D, g.tiles_touched, g.clamped, g.sort_keys[1], g.aux, \
                                                              g.blk_agg, g.blk_coarse, radii, g.counters, ranges, n_tiles)
    if (keep) GOI_PRE(true);
    else GOI_PRE(false);
#undef GOI_PRE
}

}  // namespace goi

using namespace goi;

extern "C" {

int goi_raster_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                            uint8_t* present, void* stream) {
    (void)projmatrix;
    if (P < 0) return fail("bad P");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present) return fail("NULL pointer");
    mark_visible_k<<<dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(P, means3D, viewmatrix, present);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
