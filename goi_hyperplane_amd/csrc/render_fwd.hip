// Forward tile blend and trace for gfx950: front-to-back compositing of RGB + S-dim semantic feature
// + depth + alpha.
//
// Behaviour follows the reference's renderCUDA (cuda_rasterizer/forward.cu:261-386) and traceCUDA
// (forward.cu:422-551): per pixel the tile's depth-sorted list is walked front to back with the same
// guards (power > 0, alpha < 1/255, T(1-alpha) < 1e-4, 0.99 clamp) and the same outputs; tile
// membership stays 16x16 (it is part of the numerical contract).  The execution design is this
// library's own, for CDNA4:
//   * ONE WAVE = ONE WORKGROUP = one 8x8 pixel quadrant of a tile, one pixel per lane.  There are no
//     workgroup barriers and no cross-wave load imbalance: a quadrant that saturates early retires
//     its wave at once (the reference's 256-thread block waits for its slowest pixel);
//   * the wave walks the tile list in batches of 64: every lane fetches one Gaussian's position and
//     exact contribution box (GaussRec hx/hy), tests it against the quadrant, and only the lanes
//     that hit fetch the rest of the record and the S-float semantic row and park them in LDS; the
//     64-bit hit mask stays in SGPRs and is walked with a scalar bit scan, so a Gaussian that
//     provably cannot reach alpha >= 1/255 anywhere in the quadrant costs nothing in the pair loop;
//   * the pair loop issues only wave-uniform (broadcast, conflict-free) LDS reads;
//   * workgroup ids are remapped so that the four quadrants of a tile, and neighbouring tiles, run
//     on the same XCD and share its L2 (blocks are dealt round-robin to the 8 XCDs).
#include "blend_common.h"

namespace goi {

namespace {

// LEARN: the speculative depth cut-off's per-tile learning / checking (opt-in; a template parameter because the pixel's stop
// position costs the default kernel its fifth wave per SIMD: 82 -> 99 VGPRs)
template <int S4, bool TRACE, bool UNROLL2, bool MASKS, bool LEARN = false>
__global__ __launch_bounds__(64) void render_fwd_k(const uint2* __restrict__ ranges,
                                                   const uint32_t* __restrict__ point_list, int W, int H, int gx,
                                                   int n_quads, int S, const GaussRec* __restrict__ rec,
                                                   const float* __restrict__ semantics, const float* __restrict__ bg,
                                                   float* __restrict__ out_color, float* __restrict__ out_sem,
                                                   float* __restrict__ out_depth, float* __restrict__ out_alpha,
                                                   uint32_t* __restrict__ n_contrib, const float* __restrict__ img_sem,
                                                   float* __restrict__ gau_sem, int* __restrict__ num_gsem,
                                                   uint32_t* __restrict__ qcost, unsigned long long* __restrict__ qmask0,
                                                   unsigned long long* __restrict__ qmask, const float* __restrict__ zcut,
                                                   uint32_t* __restrict__ zlearn, uint32_t* __restrict__ frame_flags,
                                                   uint32_t* __restrict__ host_words, uint32_t stamp) {
    constexpr int NF4 = TRACE ? 1 : 1 + S4;  // float4 words staged per Gaussian: (r,g,b,depth) + semantics
    constexpr int NSEM = TRACE ? 0 : 4 * S4;
    // one record per staged slot: (A3, A5, A1, A2), (A0, A4, lim, -) of the quadrant-centred log2-alpha polynomial
    // (blend_common.h), then (r, g, b, depth) and the semantics: the pair loop addresses a slot with ONE base register and
    // immediate offsets.  The loop's reads are wave-uniform broadcasts; the staging writes (ds_write_b128, banked per 8 lanes
    // over 32 dwords) are conflict-free when the record's quad count REC4 is odd, i.e. for even S4 -- as with the separate
    // arrays before (feature stride NF4 quads).
    constexpr int REC4 = NF4 + 2;
    __shared__ float4 s_rec[64 * REC4];
    const f32x4* s_rec4 = reinterpret_cast<const f32x4*>(s_rec);
    __shared__ uint32_t s_id[TRACE ? 64 : 1];

    // the frame's counters for the host (speculative forward): final before this kernel starts (frame_flags - COUNTER_OVF is
    // the counters array); 32 words into pinned, device-mapped memory -- visible to the host once the kernel has completed
    if (host_words && blockIdx.x == 0 && threadIdx.x < 32) {
        host_words[threadIdx.x] = (frame_flags - COUNTER_OVF)[threadIdx.x];
        __threadfence_system();  // every lane's word is on its way to the host before ...
        if (threadIdx.x == 0 && stamp)  // ... this use's sequence number says so (api.hip: STAMP_WORD)
            __hip_atomic_store(&host_words[HOST_STAMP_WORD], stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const QuadGeom t = quad_geom(W, H, gx, n_quads);
    if (t.tile < 0) return;
    const int tq = quad_slot();
    const uint2 range = ranges[t.tile];
    const float QCX = t.QX0 + 3.5f, QCY = t.QY0 + 3.5f;  // quadrant centre
    const f32x2 uv = {t.pxf - QCX, t.pyf - QCY};         // this lane's pixel, quadrant-centred
    const int len = (int)(range.y - range.x);
    const int rounds = (len + 63) / 64;
    const size_t HW = (size_t)W * H;
    const size_t pix_id = (size_t)W * t.py + t.px;
    const int lane = t.lane;

    float T_live = t.inside ? 1.0f : 0.0f;  // the pixel's transmittance while it is live (>= 1e-4 then), 0 once it is done: a
                                            // finished pixel fails the T(1-alpha) >= 1e-4 test by itself, no separate flag to test
    float T_end = 1.0f;                     // the transmittance a finished pixel ended with (written only where a pixel ends)
    // the wave's live pixels (T_live != 0), in SGPRs: rebuilt only where a pixel ends; empty: the wave is done
    unsigned long long live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);
    auto all_done = [&]() { return live == 0; };
    uint32_t last_contributor = 0;
    // 1-based list position of the last entry that hit this pixel and failed T (1 - alpha) >= 1e-4: the entry that ended it, or
    // a later one the wave still walked; 0: still live
    uint32_t stop_pos = 0;
    // accumulators as register pairs: one v_pk_fma_f32 adds two channels (this TU is compiled with the SLP
    // vectoriser off -- it packs the alpha evaluations of two candidates at the price of six moves -- so the
    // packing is spelled out)
    f32x2 C2[2] = {{0.f, 0.f}, {0.f, 0.f}};  // (r, g), (b, depth)
    f32x2 Cs2[NSEM > 0 ? NSEM / 2 : 1];
#pragma unroll
    for (int i = 0; i < NSEM / 2; i++) Cs2[i] = f32x2{0.f, 0.f};

    // software prefetch of the next batch's id / position / box (one Gaussian per lane)
    uint32_t id_n = 0;
    // q0, q1: what the hit test reads (position, conic, opacity, box); q2 (r, g, b, depth): only a hit needs it, but fetched at
    // staging time -- a dependent 16-byte gather every round begins by waiting for -- it cost 11 of the kernel's 280 us
    float4 q0_n = make_float4(0, 0, 0, 0), q1_n = make_float4(1.f, 0.f, -1.f, -1.f), q2_n = make_float4(0, 0, 0, 0);
    auto prefetch = [&](int b) {
        const int k = b * 64 + lane;
        q1_n.z = -1.f;
        if (k < len) {
            id_n = point_list[range.x + k];
            const float4* r4 = reinterpret_cast<const float4*>(rec + id_n);
            q0_n = r4[0];
            q1_n = r4[1];
            q2_n = r4[2];
        }
    };
    if (rounds > 0) prefetch(0);

    // MEMBER mask of the round (bit j: the Gaussian at list position 64 b + j contributed to some pixel of this quadrant),
    // in SGPRs; left for the backward blend (member_mask_ptr), which then neither tests a candidate against the quadrant
    // nor evaluates a pair that cannot contribute: a (position, quadrant) pair is a member here iff some pixel has it
    // below its last contributor and passes the two alpha guards there -- exactly the backward's own condition
    // (everything the word's address is made of is wave-uniform: kept in SGPRs, or the compiler carries tile / quadrant /
    // list start and the mask itself in vector registers -- 82 -> 114 VGPRs, four waves per SIMD instead of five)
    const int tile_u = __builtin_amdgcn_readfirstlane(t.tile), q_u = __builtin_amdgcn_readfirstlane(t.q);
    const uint32_t x0_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)range.x);
    auto store_members = [&](int b, unsigned long long mm) {
        if constexpr (MASKS)
            if (lane == 0) *member_mask_ptr(qmask0, qmask, tile_u, q_u, x0_u, b) = mm;
    };
    int b_end = rounds;  // rounds of 64 list positions this wave looked at
    for (int b = 0; b < rounds; b++) {
        if (all_done()) {
            b_end = b;
            break;
        }
        unsigned long long members = 0;
        const uint32_t id = id_n;
        const float4 q0 = q0_n, q1 = q1_n, q2 = q2_n;
        const bool hit = ellipse_hits_quadrant(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, t.QX0, t.QY0);  // hx < 0 for absent lanes
        if (b + 1 < rounds) prefetch(b + 1);
        unsigned long long m = __ballot(hit);
        // (a round without a hit falls through to the store of its -- empty -- member mask: a second store site in an
        // early `continue` cost 32 VGPRs and the fifth wave per SIMD)
        // ---- stage the hits (slot = lane)
        if (m != 0 && hit) {
            const PolyCoef pc = poly_coefs(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, QCX, QCY);
            float4* slot = s_rec + lane * REC4;
            slot[0] = make_float4(pc.A35.x, pc.A35.y, pc.A12.x, pc.A12.y);
            slot[1] = make_float4(pc.A0, pc.A4, pc.lim, 0.f);
            slot[2] = q2;  // r, g, b, depth
            if constexpr (TRACE) {
                s_id[lane] = id;
            } else {
                const float* srow = semantics + (size_t)id * S;
                if ((S & 3) == 0) {
#pragma unroll
                    for (int i = 0; i < S4; i++) slot[3 + i] = reinterpret_cast<const float4*>(srow)[i];
                } else {
#pragma unroll
                    for (int i = 0; i < S4; i++) {
                        float4 v;
                        v.x = (4 * i + 0 < S) ? srow[4 * i + 0] : 0.f;
                        v.y = (4 * i + 1 < S) ? srow[4 * i + 1] : 0.f;
                        v.z = (4 * i + 2 < S) ? srow[4 * i + 2] : 0.f;
                        v.w = (4 * i + 3 < S) ? srow[4 * i + 3] : 0.f;
                        slot[3 + i] = v;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();  // single-wave workgroup: LDS is in order, only the compiler must not reorder

        // ---- pair loop over the hits, front to back
        // applies one candidate to the per-pixel state (sequential part) and accumulates its features.  Everything a pair does
        // to a pixel happens under the pixel's own condition (EXEC), nothing by select: a lane the Gaussian does not reach
        // executes no FMA -- it used to add feature * 0, which leaves an fp32 sum that started at +0 unchanged for a finite
        // feature and poisons it for a non-finite one (the reference skips such a pixel) -- and the live transmittance and the
        // last contributor are plain moves on the lanes that contribute.
        auto apply = [&](const f32x4* r, int j, const PairEval& e) {
            const float test_T = T_live * (1.f - e.alpha);
            const bool ok = test_T >= kTMin;  // CR/forward.cu:352-356: a failing contributor ends the pixel
            // (the masks are taken where the comparisons are: each ballot IS the mask the v_cmp wrote, the ANDs are scalar)
            const unsigned long long hm = __builtin_amdgcn_ballot_w64(e.below) & __builtin_amdgcn_ballot_w64(e.seen);
            const unsigned long long om = __builtin_amdgcn_ballot_w64(ok);
            if ((hm & om) != 0) {
                if constexpr (MASKS) asm("s_bitset1_b64 %0, %1" : "+s"(members) : "s"(j));  // members |= 1 << j, pinned to SGPRs
                if (e.hit && ok) {
                    const float wgt = e.alpha * T_live;
                    const f32x2 w2 = {wgt, wgt};
                    const f32x4 f0 = r[2];
                    C2[0] = __builtin_elementwise_fma(f0.xy, w2, C2[0]);
                    C2[1] = __builtin_elementwise_fma(f0.zw, w2, C2[1]);
                    if constexpr (!TRACE) {
#pragma unroll
                        for (int i = 0; i < S4; i++) {
                            const f32x4 f = r[3 + i];
                            Cs2[2 * i] = __builtin_elementwise_fma(f.xy, w2, Cs2[2 * i]);
                            Cs2[2 * i + 1] = __builtin_elementwise_fma(f.zw, w2, Cs2[2 * i + 1]);
                        }
                    } else {
                        if ((double)e.alpha > 0.005) {
                            const uint32_t gid = s_id[j];
                            for (int ch = 0; ch < S; ch++)
                                atomicAdd(&gau_sem[(size_t)gid * S + ch], img_sem[ch * HW + pix_id]);
                            atomicAdd(&num_gsem[gid], S);
                        }
                    }
                    T_live = test_T;
                    last_contributor = (uint32_t)(b * 64 + j + 1);
                }
            }
            // a pixel can only end at a pair where a LIVE lane hits and fails the transmittance test (a finished pixel fails it at
            // every later hit): the three masks are in SGPRs already, so the common pair pays two scalar ANDs for the whole
            // ending path, the wave's exit test included
            const unsigned long long em = hm & ~om;
            if constexpr (LEARN)
                if (em != 0 && e.hit && !ok) stop_pos = (uint32_t)(b * 64 + j + 1);  // (the depth cut-off must keep this entry)
            if ((em & live) != 0) {
                if (e.hit && !ok && T_live != 0.0f) {
                    T_end = T_live;
                    T_live = 0.0f;
                }
                live = __builtin_amdgcn_ballot_w64(T_live != 0.0f);
                if (live == 0) m = 0;
            }
        };
        if constexpr (UNROLL2) {
            // two candidates per trip: their alpha evaluations are independent (ILP, half the
            // branches); the state update stays strictly in list order
            while (m) {
                const int j0 = __builtin_ctzll(m);
                m &= m - 1;
                const bool has1 = m != 0;
                const int j1 = has1 ? __builtin_ctzll(m) : j0;
                if (has1) m &= m - 1;
                const f32x4 *ra = s_rec4 + j0 * REC4, *rb = s_rec4 + j1 * REC4;
                const f32x4 ga = ra[0], gb = rb[0];
                const f32x4 ha = ra[1], hb = rb[1];
                const PairEval e0 = eval_poly(ga.xy, ga.zw, ha.x, ha.y, ha.z, uv);
                const PairEval e1 = eval_poly(gb.xy, gb.zw, hb.x, hb.y, hb.z, uv);
                apply(ra, j0, e0);
                if (has1) apply(rb, j1, e1);  // (after the wave's last pixel has ended nothing passes the transmittance test)
            }
        } else {
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const f32x4* r = s_rec4 + j * REC4;
                const f32x4 g = r[0];
                const f32x4 g2 = r[1];
                const PairEval e = eval_poly(g.xy, g.zw, g2.x, g2.y, g2.z, uv);
                apply(r, j, e);
            }
        }
        store_members(b, members);
        __builtin_amdgcn_wave_barrier();
    }

    // Speculative depth cut-off (api.hip, goi_raster_forward_async).  LEARN: the view depth up to which this tile's list
    // is worth listing the next time this camera is rendered -- the depth of the entry an eighth (and 32 positions) beyond
    // the last entry that ended a pixel of the tile (max over its four quadrant waves); +inf when a pixel reached the end of its list
    // unsaturated (such a tile is never cut).  CHECK: a pixel that reaches the end of a list that WAS cut (zcut finite) without
    // saturating may have wanted what was dropped: the frame's flag is raised -- its backward writes zero gradients, the host
    // redoes or skips the view and forgets the camera's cut.
    if constexpr (LEARN) {
        {
            const bool unsat = !all_done();
            const float zc_in = zcut ? zcut[tile_u] : __builtin_inff();
            float zc = __builtin_inff();
            if (unsat) {
                if (zc_in < 3.0e38f && lane == 0) atomicOr(frame_flags, OVF_CUT_TOO_TIGHT);
            } else {
                // every pixel has stopped: what the tile needs of its list ends at the LAST stopping entry (a pixel that has
                // not met its stopping entry keeps walking: the cut must contain it); lanes outside the image never started
                int seen = min(len, wave_max_i32((int)stop_pos));
                (void)b_end;
                // A cut list is NOT a prefix of the uncut one: the cut lives in the ellipse tile masks, and a rectangle of
                // more than 64 tiles has none -- such a Gaussian stays listed at every depth.  A pixel that passes zcut
                // unsaturated and then stops on a deeper (big) entry has skipped the small Gaussians that were dropped in
                // between.  Up to zcut the list is exact, so the frame is exact iff no pixel looked beyond it: the deepest
                // entry any pixel of this wave looked at is its last stopping entry (the list is in depth order).
                if (zc_in < 3.0e38f && seen > 0) {
                    const float z_last = rec[point_list[range.x + (uint32_t)(seen - 1)]].q2.w;
                    if (z_last > zc_in && lane == 0) atomicOr(frame_flags, OVF_CUT_TOO_TIGHT);
                }
                const int pos = seen + (seen >> 3) + 32;  // margin: an eighth + 32 list positions
                if (pos < len)
                    zc = rec[point_list[range.x + (uint32_t)pos]].q2.w;  // (depth of that entry: the list is in depth order)
                else
                    zc = zc_in;  // the margin runs past the end of the list: keep the cut the list was built with (or none)
            }
            if (zlearn && lane == 0) atomicMax(&zlearn[tile_u], __float_as_uint(zc));  // (depths are positive: their bits order like uints)
        }
    }

    {   // how far the backward's wave of this quadrant has to walk: the largest last contributor of its 64 pixels
        const int qc = wave_max_i32((int)last_contributor);
        if (qcost && lane == 0) qcost[tq] = (uint32_t)qc;
    }
    if (t.inside) {
        const float T = T_live != 0.0f ? T_live : T_end;  // transmittance that is written out: frozen where the pixel ended
        n_contrib[pix_id] = last_contributor;
        out_color[0 * HW + pix_id] = C2[0].x + T * bg[0];
        out_color[1 * HW + pix_id] = C2[0].y + T * bg[1];
        out_color[2 * HW + pix_id] = C2[1].x + T * bg[2];
        if constexpr (!TRACE) {
#pragma unroll
            for (int ch = 0; ch < NSEM; ch++)
                if (ch < S) out_sem[ch * HW + pix_id] = Cs2[ch >> 1][ch & 1];
            out_alpha[pix_id] = 1.f - T;
            out_depth[pix_id] = C2[1].y;
        }
    }
}


template <int S4>
void launch_fwd_s4(const GoiRasterScene& sc, const GeomView& g, const ImageView& im, const uint32_t* point_list,
                   float* out_color, float* out_sem, float* out_depth, float* out_alpha, hipStream_t s,
                   unsigned long long* qmask, const float* zcut, uint32_t* zlearn, uint32_t* host_words, uint32_t stamp) {
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    const int n_quads = gx * gy * 4;
#define GOI_LAUNCH_FWD(U2, MK)                                                                                         \
    do {                                                                                                               \
        if (zlearn || zcut) /* a cut that is applied is always CHECKED, whether or not the frame learns a new one */    \
            render_fwd_k<S4, false, U2, MK, true><<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(                        \
                im.ranges, point_list, sc.W, sc.H, gx, n_quads, sc.S, g.rec, sc.semantics, sc.bg, out_color, out_sem,   \
                out_depth, out_alpha, im.n_contrib, nullptr, nullptr, nullptr, im.qcost, im.qmask0, qmask, zcut,        \
                zlearn, g.counters + COUNTER_OVF, host_words, stamp);                                                   \
        else                                                                                                           \
            render_fwd_k<S4, false, U2, MK><<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(                              \
                im.ranges, point_list, sc.W, sc.H, gx, n_quads, sc.S, g.rec, sc.semantics, sc.bg, out_color, out_sem,   \
                out_depth, out_alpha, im.n_contrib, nullptr, nullptr, nullptr, im.qcost, im.qmask0, qmask, zcut,        \
                zlearn, g.counters + COUNTER_OVF, host_words, stamp);                                                   \
    } while (0)
    // The member masks are recorded by EVERY forward (a backward may follow with either setting of bwd_masks, and a frame
    // without masks back-propagated through them would be garbage).  BUILD SWITCH for measuring what recording costs the
    // forward: GOI_EXTRA_FLAGS=-DGOI_FWD_NO_MASKS (such a build must run with GOI_OPTIONS=bwd_masks=0).
#ifdef GOI_FWD_NO_MASKS
    const bool masks = false;
#else
    const bool masks = qmask != nullptr;
#endif
    if (g_options.fwd_variant == 1) {
        if (masks) GOI_LAUNCH_FWD(true, true);
        else GOI_LAUNCH_FWD(true, false);
    } else {
        if (masks) GOI_LAUNCH_FWD(false, true);
        else GOI_LAUNCH_FWD(false, false);
    }
#undef GOI_LAUNCH_FWD
}

}  // namespace

void launch_render_fwd(const GoiRasterScene& sc, const GeomView& g, const ImageView& im, const uint32_t* point_list,
                       float* out_color, float* out_sem, float* out_depth, float* out_alpha, hipStream_t s,
                       unsigned long long* qmask, const float* zcut, uint32_t* zlearn, uint32_t* host_words, uint32_t stamp) {
#define GOI_CALL(N) launch_fwd_s4<N>(sc, g, im, point_list, out_color, out_sem, out_depth, out_alpha, s, qmask, zcut, zlearn, host_words, stamp)
    GOI_DISPATCH_S4(sc.S, GOI_CALL)
#undef GOI_CALL
}

void launch_trace_fwd(const GoiRasterScene& sc, const float* img_sem, const GeomView& g, const ImageView& im,
                      const uint32_t* point_list, float* out_color, float* gau_sem, int* num_gsem, hipStream_t s) {
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    const int n_quads = gx * gy * 4;
    render_fwd_k<1, true, false, false><<<dim3(quad_grid(n_quads)), dim3(64), 0, s>>>(
        im.ranges, point_list, sc.W, sc.H, gx, n_quads, sc.S, g.rec, nullptr, sc.bg, out_color, nullptr, nullptr, nullptr,
        im.n_contrib, img_sem, gau_sem, num_gsem, nullptr, nullptr, nullptr, nullptr, nullptr, g.counters + COUNTER_OVF,
        nullptr, 0u);
}

}  // namespace goi
