// Per-Gaussian backward kernel: the backward of the forward preprocess in preprocess_fwd.hip (conic -> cov3D/mean, projection,
// depth, SH, cov3D -> scale/rotation), with the factored dL/dSH kernel beside it and the two entries that drive them directly
// (goi_raster_debug_preprocess_backward, goi_raster_sh_grad_from_views).  What the two per-Gaussian kernels share is
// preprocess_common.h.  Compiled with -ffp-contract=off: these stages are HBM-bound streaming, and
// keeping the reference's operation order keeps the gradients those of the reference's statement sequence.
//
// Behaviour restated from the reference (paths relative to submodules/diff-gaussian-rasterization/):
//   backward: cuda_rasterizer/backward.cu:144-274 (cov2D), :346-412 (projection/depth),
//             :20-139 (SH), :278-341 (cov3D)
// Layout is this library's own: one 48-byte GaussRec per Gaussian instead of five arrays, 3 clamp bits in one byte.
#include <algorithm>
#include <climits>

#include "common.h"
#include "entry.h"
#include "preprocess_common.h"
#include "row_sum.h"

namespace goi {

namespace {

struct BwdArgs {
    int P, D, M;
    const float* means3D;
    const float* shs;
    const float* scales;
    const float* rotations;
    const float* cov3D;  // precomputed or the forward's
    float scale_modifier, tan_fovx, tan_fovy, focal_x, focal_y;
    const float* view_p;
    const float* proj_p;
    const float* campos_p;
    // radii of the backward that LAST WROTE these very output buffers (nothing has touched them since), or NULL: a Gaussian that
    // was invisible then and is invisible now already has zeros in every output row -- nothing is written for it (half of the
    // headline scene: 170 MB of zeros per step).  goi_raster_backward (prev_radii), csrc/torch_binding.cpp: the gradient-buffer pool.
    const int* prev_radii;
    // The same knowledge per ROW, which can also say "visible then, but the chain did not run" (an IDLE Gaussian, see RecArgs::contrib):
    // prev_mask[id] == 0 -- the backward that last wrote these buffers left zeros in the row (and nothing has touched it since);
    // it takes precedence over prev_radii.  row_mask (or NULL): this kernel writes 1 for every id whose row the chain wrote and 0
    // for every other id < P, whatever it did about that row (zeros, or nothing where they were there already).  The two may be
    // the SAME array: a thread reads the byte of an id before it writes it, and no other thread touches that byte.
    // goi_raster_backward (prev_mask, row_mask); csrc/torch_binding.cpp keeps the mask with the pooled allocation.
    const uint8_t* prev_mask;
    uint8_t* row_mask;
    // ACCUMULATE (goi_raster_backward, flags bit 0; the record path only): the outputs already hold the gradients of earlier
    // views of the same batch -- a visible Gaussian's rows are read, added to and written back, an invisible one's are left
    // alone.  The sum of K views then costs each view its visible rows once more instead of a dense [P, 75 + S] addition
    // (dist.backward_views).
    int accumulate;
};

// WITH_DSH: dL/dSH is formed ([P,M,3], staged through LDS).  Otherwise (the caller passed dL_dsh = NULL with SH
// colours: "factored" mode of goi_raster_backward) the kernel writes the clamp-masked colour gradient g back to
// dL_dcolor instead: dL/dSH[k] = basis_k(view direction) * g is then formed elsewhere (goi_raster_sh_grad_from_views).
// FROM_ROWS: the blend gradients of a Gaussian come from its RECORD in the row scratch (reduce_rows_k<.., RECORD>: the summed
// row over the Gaussian's first slot, goff[id] * 4) instead of six per-id arrays, and this kernel writes the per-id outputs
// the reduction used to write -- dL/dmean2D, dL/dcolour, dL/dopacity, dL/dsemantics -- itself: zeros for a Gaussian that is
// not listed, coalesced either way.  (dL_dconic / dL_ddepth are not written on that path: they were only ever this
// kernel's inputs.)
struct RecArgs {
    const float* rows;              // row scratch
    const uint4* aux;               // [P] .x: first emit-order instance of a listed Gaussian
    const uint32_t* tiles_touched;  // [P] 0: not listed (no record)
    int row_floats, S, nch;         // nch = padded semantic channels + 4 (see render_bwd.hip: BwdCfg)
    float* dL_dopacity;
    float* dL_dsemantic;
    // SRC == 2 (bwd_records 2): the kernel sums the rows itself
    const uint8_t* flags;           // validity bytes of the row slots
    const uint32_t* n_dev;          // the frame's counters from COUNTER_N on (instances, listed Gaussians: the BIG threshold)
    uint32_t N_cap;                 // slot capacity the scratch was laid out for
    // SRC == 1, or NULL: the CONTRIBUTION bytes of the row reduction (reduce_rows.hip), contrib[aux[id].x] == 0 -- the listed Gaussian
    // owns no valid row: its record is all +0 (and was not stored).  Such a Gaussian, and a visible one without tiles, is IDLE.
    const uint8_t* contrib;
};
// Rows of the dL/dSH staging tile = visible Gaussians a workgroup takes through the chain at a time: 224 x (3 M + 1) floats =
// 43.9 KB at M = 16, three workgroups per CU with the index lists (the kernel's 143 VGPRs allow three as well).
#ifndef GOI_PBWD_ROWS
#define GOI_PBWD_ROWS 224
#endif
#ifndef GOI_PBWD_BLOCKS
#define GOI_PBWD_BLOCKS 3
#endif
constexpr int BWD_TILE_ROWS_DEFAULT = GOI_PBWD_ROWS;
#ifndef GOI_PBWD_INFLIGHT
#define GOI_PBWD_INFLIGHT 16  // rows a quarter wave requests back to back in the in-kernel row sum (reduce_rows_k: 32)
#endif
#ifndef GOI_PBWD_ROWS_FUSED
#define GOI_PBWD_ROWS_FUSED 208
#endif
constexpr int BWD_TILE_ROWS_FUSED = GOI_PBWD_ROWS_FUSED;  // (SRC == 2: ten more floats of LDS per row; 208 rows keep three workgroups per CU)
constexpr int BWD_REC_FLOATS = 10;  // r, g, b, depth, mean2D x, y, conic a, b, c, opacity
constexpr int BWD_BLOCKS_PER_CU = GOI_PBWD_BLOCKS;

// emit(k, basis_k(x, y, z) * g) for every SH coefficient k < (D + 1)^2: dL/dSH[k] of a colour gradient g seen along the unit
// direction (x, y, z).  preprocess_bwd_k and sh_grad_from_views_k both form the products here: the factored mode is bit-identical.
template <class Emit>
__device__ __forceinline__ void sh_basis_times(int D, float x, float y, float z, const V3& g, Emit&& emit) {
    emit(0, kSH0 * g);
    if (D > 0) {
        emit(1, (-kSH1 * y) * g);
        emit(2, (kSH1 * z) * g);
        emit(3, (-kSH1 * x) * g);
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            emit(4, (kSH2[0] * xy) * g);
            emit(5, (kSH2[1] * yz) * g);
            emit(6, (kSH2[2] * (2.f * zz - xx - yy)) * g);
            emit(7, (kSH2[3] * xz) * g);
            emit(8, (kSH2[4] * (xx - yy)) * g);
            if (D > 2) {
                emit(9, (kSH3[0] * y * (3.f * xx - yy)) * g);
                emit(10, (kSH3[1] * xy * z) * g);
                emit(11, (kSH3[2] * y * (4.f * zz - xx - yy)) * g);
                emit(12, (kSH3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)) * g);
                emit(13, (kSH3[4] * x * (4.f * zz - xx - yy)) * g);
                emit(14, (kSH3[5] * z * (xx - yy)) * g);
                emit(15, (kSH3[6] * x * (xx - 3.f * yy)) * g);
            }
        }
    }
}

// What the classification reads of one id, all of it by id: the kernel requests the NEXT segment's while it works on this one
struct SegIn {
    int rad;           // radii[id]
    uint32_t tt, ax;   // (skip_idle) tiles_touched[id], aux[id].x
    uint32_t prev;     // 0: the row already holds zeros
};
__device__ __forceinline__ SegIn load_seg(const BwdArgs& args, const RecArgs& ra, const int* radii, bool skip_idle, int nseg, int sg) {
    SegIn v{0, 0u, 0u, 1u};
    const int id = sg * 256 + (int)threadIdx.x;
    if (sg < nseg && id < args.P) {
        v.rad = radii[id];
        if (skip_idle) {
            v.tt = ra.tiles_touched[id];
            v.ax = ra.aux[id].x;
        }
        if (args.prev_mask != nullptr) v.prev = args.prev_mask[id];
        else if (args.prev_radii != nullptr) v.prev = args.prev_radii[id] != 0 ? 1u : 0u;
    }
    return v;
}

// Classifies a segment's 256 ids with ballots and a scan of the wave counts, and writes row_mask: an id the chain runs for (work_t)
// goes to s_vis behind its npend entries (returns how many), any other whose rows lack zeros to s_zero as its offset from `base` (nzero).
__device__ __forceinline__ int classify_segment(const BwdArgs& args, uint32_t prev, bool work_t, int base, int npend,
                                                uint32_t* s_vis, uint16_t* s_zero, int (*s_wcnt)[4], int& nzero) {
    const int gtid = base + threadIdx.x;
    const bool in_range = gtid < args.P;
    // rows that already hold zeros (see BwdArgs::prev_radii, prev_mask) are not written again
    const bool keep_t = in_range && !work_t && prev == 0u;
    const bool zero_t = in_range && !work_t && !keep_t && !args.accumulate;
    if (args.row_mask != nullptr && in_range) args.row_mask[gtid] = work_t ? (uint8_t)1 : (uint8_t)0;
    const int wv = threadIdx.x >> 6;
    const unsigned long long bv = __ballot(work_t), bz = __ballot(zero_t);
    if ((threadIdx.x & 63) == 0) {
        s_wcnt[0][wv] = __popcll(bv);
        s_wcnt[1][wv] = __popcll(bz);
    }
    __syncthreads();
    int ov = 0, oz = 0;
    for (int i = 0; i < wv; i++) {
        ov += s_wcnt[0][i];
        oz += s_wcnt[1][i];
    }
    const int nvis = s_wcnt[0][0] + s_wcnt[0][1] + s_wcnt[0][2] + s_wcnt[0][3];
    nzero = s_wcnt[1][0] + s_wcnt[1][1] + s_wcnt[1][2] + s_wcnt[1][3];
    const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
    if (work_t) s_vis[npend + ov + __popcll(bv & lt)] = (uint32_t)gtid;
    if (zero_t) s_zero[oz + __popcll(bz & lt)] = (uint16_t)threadIdx.x;
    __syncthreads();
    return nvis;
}

// Zeros for the nzero ids of s_zero: the per-id outputs (one thread per id), then dL/dsemantics and dL/dSH by the whole block.
template <bool WITH_DSH, bool FROM_ROWS>
__device__ __forceinline__ void write_zero_rows(int nzero, int base, const uint16_t* s_zero, int w, const RecArgs& ra,
                                                float* dL_dmean2D, float* dL_dcolor, const GaussGrads& out) {
    if ((int)threadIdx.x < nzero) {
        const int idx = base + s_zero[threadIdx.x];
        if constexpr (FROM_ROWS) {
            ra.dL_dopacity[idx] = 0.f;
            dL_dmean2D[3 * idx] = dL_dmean2D[3 * idx + 1] = dL_dmean2D[3 * idx + 2] = 0.f;
            dL_dcolor[3 * idx] = dL_dcolor[3 * idx + 1] = dL_dcolor[3 * idx + 2] = 0.f;
        }
        out.dL_dmean3D[3 * idx] = out.dL_dmean3D[3 * idx + 1] = out.dL_dmean3D[3 * idx + 2] = 0.f;
#pragma unroll
        for (int i = 0; i < 6; i++) out.dL_dcov3D[(size_t)6 * idx + i] = 0.f;
        out.dL_dscale[3 * idx] = out.dL_dscale[3 * idx + 1] = out.dL_dscale[3 * idx + 2] = 0.f;
        reinterpret_cast<float4*>(out.dL_drot)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto zero_wide = [&](float* dst, int width) {  // `width` floats per row, by the whole block
        for (int i = threadIdx.x; i < nzero * width; i += 256) {
            const int r = i / width;
            dst[(size_t)(base + s_zero[r]) * width + (i - r * width)] = 0.f;
        }
    };
    if constexpr (FROM_ROWS) zero_wide(ra.dL_dsemantic, ra.S);
    if constexpr (WITH_DSH) zero_wide(out.dL_dsh, w);
}

// The SH rows of the tile's Gaussians (192 B, the widest input) into the tile the dL/dSH rows leave through, by the whole block:
// consecutive lanes take consecutive 16-byte pieces of a row.  A thread reads its coefficients there before it overwrites them.
__device__ __forceinline__ void stage_sh_rows(const float* shs, int nrows, int w, const uint32_t* s_vis, float* s_dsh) {
    if ((w & 3) == 0) {
        const int w4 = w >> 2;
        for (int i = threadIdx.x; i < nrows * w4; i += 256) {
            const int r = i / w4, q = i - r * w4;
            const float4 v = reinterpret_cast<const float4*>(shs + (size_t)s_vis[r] * w)[q];
            float* dst = s_dsh + r * (w + 1) + 4 * q;
            dst[0] = v.x;
            dst[1] = v.y;
            dst[2] = v.z;
            dst[3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < nrows * w; i += 256) {
            const int r = i / w;
            s_dsh[r * (w + 1) + (i - r * w)] = shs[(size_t)s_vis[r] * w + (i - r * w)];
        }
    }
}

// (SRC == 2) The tile's rows, summed in the kernel: quarter wave qw of the workgroup's sixteen takes tile rows qw, qw + 16, ...
// and sums one Gaussian's rows exactly as reduce_rows_k does (same function, same order of the rows: bit-identical sums; slot range
// two Gaussians ahead, validity bytes one ahead).  The 16 semantic sums leave for dL/dsemantics at once, the chain's ten go to s_rec.
__device__ __forceinline__ void sum_tile_rows(const RecArgs& ra, int nrows, const uint32_t* s_vis, float* s_rec) {
    constexpr int RF = 32;  // 128-byte rows (the launcher takes this mode for them only)
    const int qw = threadIdx.x >> 4, e = threadIdx.x & 15, quarter = (threadIdx.x & 63) >> 4;
    const uint32_t* flags32 = reinterpret_cast<const uint32_t*>(ra.flags);
    const uint32_t N = min(ra.N_cap, ra.n_dev[0]);  // (a truncated frame has no visible Gaussians: never gets here)
    const uint32_t Vl = ra.n_dev[COUNTER_V - COUNTER_N];
    const uint32_t big_inst = (N > REDUCE_DENSE_RATIO * Vl) ? REDUCE_BIG_INST : 1024u;  // (reduce_rows.hip: find_big_k)
    const int rounds = (nrows + 15) >> 4;  // (block-uniform)
    struct Meta {
        uint32_t idx, off0, cnt;
    };
    auto load_meta = [&](int k) {
        const int r = qw + 16 * k;
        Meta m{0u, 0u, 0u};
        if (k < rounds && r < nrows) {
            m.idx = s_vis[r];
            m.cnt = ra.tiles_touched[m.idx];  // instances = slots / 4 of a listed Gaussian, 0: not listed
            m.off0 = ra.aux[m.idx].x;         // its first emit-order instance
            if (m.cnt == 0u) m.off0 = 0u;
        }
        return m;
    };
    auto load_first = [&](const Meta& m) { return (m.cnt <= big_inst && (uint32_t)e < m.cnt) ? flags32[m.off0 + e] : 0u; };
    Meta m_cur = load_meta(0), m_nxt = load_meta(1);
    uint32_t f_cur = load_first(m_cur);
#pragma unroll 1
    for (int k = 0; k < rounds; k++) {
        const Meta m_far = load_meta(k + 2);
        const uint32_t f_nxt = load_first(m_nxt);
        const int r = qw + 16 * k;
        const bool big = m_cur.cnt > big_inst;
        float sum[2] = {0.f, 0.f};
        sum_instances<2, false, GOI_PBWD_INFLIGHT>(ra.rows, flags32, (size_t)m_cur.off0, big ? 0u : m_cur.cnt, f_cur, quarter, e, sum, sum);
        if (r < nrows) {
            if (big) {  // its record, left by reduce_big_k over the first slot it owns
                const float2 t = reinterpret_cast<const float2*>(ra.rows + (size_t)m_cur.off0 * 4 * RF)[e];
                sum[0] = t.x;
                sum[1] = t.y;
            }
            const int nsem = ra.nch - 4;  // lane e holds row elements 2 e, 2 e + 1
            const int el = 2 * e;
            if (el < nsem) {
                float* dst = ra.dL_dsemantic + (size_t)m_cur.idx * ra.S;
                if (el + 1 < ra.S && (ra.S & 1) == 0) *reinterpret_cast<float2*>(dst + el) = make_float2(sum[0], sum[1]);
                else {
                    if (el < ra.S) dst[el] = sum[0];
                    if (el + 1 < ra.S) dst[el + 1] = sum[1];
                }
            } else if (el < nsem + BWD_REC_FLOATS) {
                *reinterpret_cast<float2*>(&s_rec[r * BWD_REC_FLOATS + (el - nsem)]) = make_float2(sum[0], sum[1]);
            }
        }
        m_cur = m_nxt;
        m_nxt = m_far;
        f_cur = f_nxt;
    }
    __syncthreads();
}

// The small per-Gaussian inputs of the chain, to registers before anything waits.  The kernel is latency bound: its waves spent two
// thirds of their time in s_waitcnt (profiles/r04_c_pmc_summary.txt) walking ~10 dependent round trips when each input was fetched
// where the chain first needs it.
struct ChainIn {
    V3 mean, scale;
    float cov3D[6];
    float4 rot;
    uint8_t clamp;
};
__device__ __forceinline__ ChainIn load_chain_inputs(const BwdArgs& a, const uint8_t* __restrict__ clamped, int idx) {
    ChainIn in;
    in.mean = V3{a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]};
#pragma unroll
    for (int i = 0; i < 6; i++) in.cov3D[i] = a.cov3D[(size_t)6 * idx + i];
    in.rot = a.scales ? reinterpret_cast<const float4*>(a.rotations)[idx] : make_float4(1.f, 0.f, 0.f, 0.f);
    in.scale = a.scales ? V3{a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]} : V3{0.f, 0.f, 0.f};
    in.clamp = a.shs ? clamped[idx] : (uint8_t)0;
    return in;
}

// The blend gradients of tile row threadIdx.x: from the six per-id arrays (SRC 0), the Gaussian's record (1: two round trips, slot
// -> record; the slot goes to s_src for the dL/dsemantics pass) or s_rec (2).  The two row paths write the per-id outputs here.
struct BlendIn {
    float conic[3], m2d[2], depth;
    V3 col;
};
template <int SRC>
__device__ __forceinline__ BlendIn load_blend_grads(bool visible, int idx, int accumulate, const RecArgs& ra, const float* s_rec,
                                                    uint32_t* s_src, float* dL_dmean2D, const float* __restrict__ dL_dconic,
                                                    float* dL_dcolor, const float* __restrict__ dL_ddepth) {
    BlendIn b{{0.f, 0.f, 0.f}, {0.f, 0.f}, 0.f, {0.f, 0.f, 0.f}};
    auto put_outputs = [&](float opa) {
        ra.dL_dopacity[idx] = opa;
        dL_dmean2D[3 * idx] = b.m2d[0];
        dL_dmean2D[3 * idx + 1] = b.m2d[1];
        dL_dmean2D[3 * idx + 2] = 0.f;
        dL_dcolor[3 * idx] = b.col.x;  // (factored SH mode overwrites it with the clamp-masked gradient: sh_backward)
        dL_dcolor[3 * idx + 1] = b.col.y;
        dL_dcolor[3 * idx + 2] = b.col.z;
    };
    if constexpr (SRC == 2) {
        if (visible) {
            const float* rc = &s_rec[threadIdx.x * BWD_REC_FLOATS];
            b.col = V3{rc[0], rc[1], rc[2]};
            b.depth = rc[3];
            b.m2d[0] = rc[4];
            b.m2d[1] = rc[5];
            b.conic[0] = rc[6];
            b.conic[1] = rc[7];
            b.conic[2] = rc[8];
            put_outputs(rc[9]);
        }
    } else if constexpr (SRC == 1) {
        const bool listed = visible && ra.tiles_touched[idx] != 0;
        const uint32_t slot = listed ? ra.aux[idx].x : 0u;
        const float* rec = ra.rows + (size_t)slot * 4 * ra.row_floats;
        const int nsem = ra.nch - 4;
        float opa = 0.f;
        if (listed) {
            const float4 cd = *reinterpret_cast<const float4*>(rec + nsem);        // r, g, b, depth
            const float4 mc = *reinterpret_cast<const float4*>(rec + ra.nch);      // mean2D x, y, conic a, b
            const float2 co = *reinterpret_cast<const float2*>(rec + ra.nch + 4);  // conic c, opacity
            b.col = V3{cd.x, cd.y, cd.z};
            b.depth = cd.w;
            b.m2d[0] = mc.x;
            b.m2d[1] = mc.y;
            b.conic[0] = mc.z;
            b.conic[1] = mc.w;
            b.conic[2] = co.x;
            opa = co.y;
        }
        if (visible) {
            s_src[threadIdx.x] = listed ? slot : 0xFFFFFFFFu;
            if (accumulate) {
                ra.dL_dopacity[idx] += opa;
                dL_dmean2D[3 * idx] += b.m2d[0];
                dL_dmean2D[3 * idx + 1] += b.m2d[1];
                dL_dcolor[3 * idx] += b.col.x;
                dL_dcolor[3 * idx + 1] += b.col.y;
                dL_dcolor[3 * idx + 2] += b.col.z;
            } else {
                put_outputs(opa);
            }
        }
    } else if (visible) {
        b.conic[0] = dL_dconic[4 * idx];
        b.conic[1] = dL_dconic[4 * idx + 1];
        b.conic[2] = dL_dconic[4 * idx + 3];
        b.m2d[0] = dL_dmean2D[3 * idx];
        b.m2d[1] = dL_dmean2D[3 * idx + 1];
        b.depth = dL_ddepth[idx];
        b.col = V3{dL_dcolor[3 * idx], dL_dcolor[3 * idx + 1], dL_dcolor[3 * idx + 2]};
    }
    return b;
}

// The chain rule's four stages keep the reference's statement sequence (-ffp-contract=off): bit-identical gradients on any lane.
// conic -> cov2D -> cov3D (gcov, left alone where the determinant degenerates) and the covariance path of the mean gradient,
// which is returned (CR backward.cu:144-274).  c is the forward's projection (ewa_cov2d), which the KERNEL calls: called from
// in here, nested two deep, it cost <true,1> and <false,2> 24 and 8 bytes of scratch per lane (none otherwise) and <true,2> 40 for 16.
__device__ __forceinline__ V3 cov2d_backward(const BwdArgs& a, const float* view, const Cov2D& c, const float* conic, float* gcov) {
    const float dca = conic[0], dcb = conic[1], dcc = conic[2];
    const float x_grad_mul = (c.txtz < -c.limx || c.txtz > c.limx) ? 0.f : 1.f;
    const float y_grad_mul = (c.tytz < -c.limy || c.tytz > c.limy) ? 0.f : 1.f;
    const auto& T = c.T.c;
    const auto& Vrk = c.Vrk.c;
    const auto& Wm = c.W.c;
    const float ca = c.cov.c[0][0] + 0.3f, cb = c.cov.c[0][1], cc = c.cov.c[1][1] + 0.3f;
    const float denom = ca * cc - cb * cb;
    float dL_da = 0, dL_db = 0, dL_dc = 0;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    if (denom2inv != 0) {
        dL_da = denom2inv * (-cc * cc * dca + 2 * cb * cc * dcb + (denom - ca * cc) * dcc);
        dL_dc = denom2inv * (-ca * ca * dcc + 2 * ca * cb * dcb + (denom - ca * cc) * dca);
        dL_db = denom2inv * 2 * (cb * cc * dca - (denom + 2 * cb * cb) * dcb + ca * cb * dcc);
        gcov[0] = (T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc);
        gcov[3] = (T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc);
        gcov[5] = (T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc);
        gcov[1] = 2 * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db + 2 * T[1][0] * T[1][1] * dL_dc;
        gcov[2] = 2 * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db + 2 * T[1][0] * T[1][2] * dL_dc;
        gcov[4] = 2 * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db + 2 * T[1][1] * T[1][2] * dL_dc;
    }
    const float r0a = T[0][0] * Vrk[0][0] + T[0][1] * Vrk[0][1] + T[0][2] * Vrk[0][2];
    const float r0b = T[0][0] * Vrk[1][0] + T[0][1] * Vrk[1][1] + T[0][2] * Vrk[1][2];
    const float r0c = T[0][0] * Vrk[2][0] + T[0][1] * Vrk[2][1] + T[0][2] * Vrk[2][2];
    const float r1a = T[1][0] * Vrk[0][0] + T[1][1] * Vrk[0][1] + T[1][2] * Vrk[0][2];
    const float r1b = T[1][0] * Vrk[1][0] + T[1][1] * Vrk[1][1] + T[1][2] * Vrk[1][2];
    const float r1c = T[1][0] * Vrk[2][0] + T[1][1] * Vrk[2][1] + T[1][2] * Vrk[2][2];
    const float dL_dT00 = 2 * r0a * dL_da + r1a * dL_db;
    const float dL_dT01 = 2 * r0b * dL_da + r1b * dL_db;
    const float dL_dT02 = 2 * r0c * dL_da + r1c * dL_db;
    const float dL_dT10 = 2 * r1a * dL_dc + r0a * dL_db;
    const float dL_dT11 = 2 * r1b * dL_dc + r0b * dL_db;
    const float dL_dT12 = 2 * r1c * dL_dc + r0c * dL_db;
    const float dL_dJ00 = Wm[0][0] * dL_dT00 + Wm[0][1] * dL_dT01 + Wm[0][2] * dL_dT02;
    const float dL_dJ02 = Wm[2][0] * dL_dT00 + Wm[2][1] * dL_dT01 + Wm[2][2] * dL_dT02;
    const float dL_dJ11 = Wm[1][0] * dL_dT10 + Wm[1][1] * dL_dT11 + Wm[1][2] * dL_dT12;
    const float dL_dJ12 = Wm[2][0] * dL_dT10 + Wm[2][1] * dL_dT11 + Wm[2][2] * dL_dT12;
    const float tz = 1.f / c.t.z;
    const float tz2 = tz * tz;
    const float tz3 = tz2 * tz;
    const float dL_dtx = x_grad_mul * -a.focal_x * tz2 * dL_dJ02;
    const float dL_dty = y_grad_mul * -a.focal_y * tz2 * dL_dJ12;
    const float dL_dtz = -a.focal_x * tz2 * dL_dJ00 - a.focal_y * tz2 * dL_dJ11 +
                         (2 * a.focal_x * c.t.x) * tz3 * dL_dJ02 + (2 * a.focal_y * c.t.y) * tz3 * dL_dJ12;
    return xform_vec_4x3_t({dL_dtx, dL_dty, dL_dtz}, view);
}

// projection and depth paths of the mean gradient, added to gmean in that order (CR backward.cu:346-412)
__device__ __forceinline__ void projection_backward(const float* proj, const float* view, const V3& mean, const float* m2d,
                                                    float dd, V3& gmean) {
    const float4 m_hom = xform_point_4x4(mean, proj);
    const float m_w = 1.0f / (m_hom.w + 0.0000001f);
    const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
    const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
    const float d2x = m2d[0], d2y = m2d[1];
    V3 g1;
    g1.x = (proj[0] * m_w - proj[3] * mul1) * d2x + (proj[1] * m_w - proj[3] * mul2) * d2y;
    g1.y = (proj[4] * m_w - proj[7] * mul1) * d2x + (proj[5] * m_w - proj[7] * mul2) * d2y;
    g1.z = (proj[8] * m_w - proj[11] * mul1) * d2x + (proj[9] * m_w - proj[11] * mul2) * d2y;
    gmean = gmean + g1;
    const float mul3 = view[2] * mean.x + view[6] * mean.y + view[10] * mean.z + view[14];
    V3 g2;
    g2.x = (view[2] - view[3] * mul3) * dd;
    g2.y = (view[6] - view[7] * mul3) * dd;
    g2.z = (view[10] - view[11] * mul3) * dd;
    gmean = gmean + g2;
}

// SH backward (CR backward.cu:20-139): colour gradient -> SH coefficients and the view-direction path of the mean (added to gmean).
// WITH_DSH: its tile row holds the Gaussian's coefficients (stage_sh_rows) until the sh_basis_times pass at the end replaces
// them with their gradients, AFTER their last read.  Otherwise they come from memory and the clamp-masked g goes back to dL_dcolor.
template <bool WITH_DSH>
__device__ __forceinline__ void sh_backward(const BwdArgs& a, const float* campos_p, const V3& mean, int idx, uint8_t cl,
                                            const V3& col, float* s_dsh, float* dL_dcolor, V3& gmean) {
    V3* row = WITH_DSH ? reinterpret_cast<V3*>(s_dsh + (size_t)threadIdx.x * (3 * a.M + 1)) : nullptr;
    const V3 campos = {campos_p[0], campos_p[1], campos_p[2]};
    const V3 dir_orig = mean - campos;
    const V3 dir = dir_orig / sqrtf(dot3(dir_orig, dir_orig));
    const V3* sh = WITH_DSH ? row : reinterpret_cast<const V3*>(a.shs) + (size_t)idx * a.M;
    V3 g = col;
    g.x *= (cl & 1) ? 0.f : 1.f;
    g.y *= (cl & 2) ? 0.f : 1.f;
    g.z *= (cl & 4) ? 0.f : 1.f;
    if constexpr (!WITH_DSH) {
        dL_dcolor[3 * idx] = g.x;
        dL_dcolor[3 * idx + 1] = g.y;
        dL_dcolor[3 * idx + 2] = g.z;
    }
    V3 dRGBdx = {0, 0, 0}, dRGBdy = {0, 0, 0}, dRGBdz = {0, 0, 0};
    const float x = dir.x, y = dir.y, z = dir.z;
    if (a.D > 0) {
        dRGBdx = -kSH1 * sh[3];
        dRGBdy = -kSH1 * sh[1];
        dRGBdz = kSH1 * sh[2];
        if (a.D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dRGBdx = dRGBdx + (kSH2[0] * y * sh[4] + kSH2[2] * 2.f * -x * sh[6] + kSH2[3] * z * sh[7] +
                               kSH2[4] * 2.f * x * sh[8]);
            dRGBdy = dRGBdy + (kSH2[0] * x * sh[4] + kSH2[1] * z * sh[5] + kSH2[2] * 2.f * -y * sh[6] +
                               kSH2[4] * 2.f * -y * sh[8]);
            dRGBdz = dRGBdz + (kSH2[1] * y * sh[5] + kSH2[2] * 2.f * 2.f * z * sh[6] + kSH2[3] * x * sh[7]);
            if (a.D > 2) {
                dRGBdx = dRGBdx + (kSH3[0] * sh[9] * 3.f * 2.f * xy + kSH3[1] * sh[10] * yz + kSH3[2] * sh[11] * -2.f * xy +
                                   kSH3[3] * sh[12] * -3.f * 2.f * xz + kSH3[4] * sh[13] * (-3.f * xx + 4.f * zz - yy) +
                                   kSH3[5] * sh[14] * 2.f * xz + kSH3[6] * sh[15] * 3.f * (xx - yy));
                dRGBdy = dRGBdy + (kSH3[0] * sh[9] * 3.f * (xx - yy) + kSH3[1] * sh[10] * xz +
                                   kSH3[2] * sh[11] * (-3.f * yy + 4.f * zz - xx) +
                                   kSH3[3] * sh[12] * -3.f * 2.f * yz + kSH3[4] * sh[13] * -2.f * xy +
                                   kSH3[5] * sh[14] * -2.f * yz + kSH3[6] * sh[15] * -3.f * 2.f * xy);
                dRGBdz = dRGBdz + (kSH3[1] * sh[10] * xy + kSH3[2] * sh[11] * 4.f * 2.f * yz +
                                   kSH3[3] * sh[12] * 3.f * (2.f * zz - xx - yy) +
                                   kSH3[4] * sh[13] * 4.f * 2.f * xz + kSH3[5] * sh[14] * (xx - yy));
            }
        }
    }
    const V3 dL_ddir = {dot3(dRGBdx, g), dot3(dRGBdy, g), dot3(dRGBdz, g)};
    const V3 v = dir_orig;
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    V3 dm;
    dm.x = ((+sum2 - v.x * v.x) * dL_ddir.x - v.y * v.x * dL_ddir.y - v.z * v.x * dL_ddir.z) * invsum32;
    dm.y = (-v.x * v.y * dL_ddir.x + (sum2 - v.y * v.y) * dL_ddir.y - v.z * v.y * dL_ddir.z) * invsum32;
    dm.z = (-v.x * v.z * dL_ddir.x - v.y * v.z * dL_ddir.y + (sum2 - v.z * v.z) * dL_ddir.z) * invsum32;
    gmean = gmean + dm;
    if constexpr (WITH_DSH) {
        for (int k = (a.D + 1) * (a.D + 1); k < a.M; k++) row[k] = V3{0, 0, 0};
        sh_basis_times(a.D, x, y, z, g, [&](int k, const V3& t) { row[k] = t; });
    }
}

// cov3D -> scale / rotation (CR backward.cu:278-341)
__device__ __forceinline__ void cov3d_backward(float scale_modifier, const float4& q, const V3& scale, const float* gcov,
                                               V3& gscale, float4& grot) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    const M3 R = rotation_from_quat(r, x, y, z);
    M3 S = make_m3(1, 0, 0, 0, 1, 0, 0, 0, 1);
    const V3 s = scale_modifier * scale;
    S.c[0][0] = s.x;
    S.c[1][1] = s.y;
    S.c[2][2] = s.z;
    const M3 Mm = mul(S, R);
    const M3 dSig = make_m3(gcov[0], 0.5f * gcov[1], 0.5f * gcov[2], 0.5f * gcov[1], gcov[3], 0.5f * gcov[4],
                            0.5f * gcov[2], 0.5f * gcov[4], gcov[5]);
    M3 M2 = Mm;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M2.c[i][j] = Mm.c[i][j] * 2.0f;
    const M3 dL_dM = mul(M2, dSig);
    const M3 Rt = transpose(R);
    M3 dMt = transpose(dL_dM);
    gscale.x = dot3(column(Rt, 0), column(dMt, 0));
    gscale.y = dot3(column(Rt, 1), column(dMt, 1));
    gscale.z = dot3(column(Rt, 2), column(dMt, 2));
#pragma unroll
    for (int j = 0; j < 3; j++) {
        dMt.c[0][j] *= s.x;
        dMt.c[1][j] *= s.y;
        dMt.c[2][j] *= s.z;
    }
    const auto& A = dMt.c;
    grot.x = 2 * z * (A[0][1] - A[1][0]) + 2 * y * (A[2][0] - A[0][2]) + 2 * x * (A[1][2] - A[2][1]);
    grot.y = 2 * y * (A[1][0] + A[0][1]) + 2 * z * (A[2][0] + A[0][2]) + 2 * r * (A[1][2] - A[2][1]) -
             4 * x * (A[2][2] + A[1][1]);
    grot.z = 2 * x * (A[1][0] + A[0][1]) + 2 * r * (A[2][0] - A[0][2]) + 2 * z * (A[1][2] + A[2][1]) -
             4 * y * (A[2][2] + A[0][0]);
    grot.w = 2 * r * (A[0][1] - A[1][0]) + 2 * x * (A[2][0] + A[0][2]) + 2 * y * (A[1][2] + A[2][1]) -
             4 * z * (A[1][1] + A[0][0]);
}

// The five per-Gaussian gradients of id idx: written, or (accumulate) requested together, added and written back
__device__ __forceinline__ void store_gauss_grads(int accumulate, int idx, const GaussGrads& out, V3 gmean, float* gcov,
                                                  V3 gscale, float4 grot) {
    if (accumulate) {
        const float m0 = out.dL_dmean3D[3 * idx], m1 = out.dL_dmean3D[3 * idx + 1], m2 = out.dL_dmean3D[3 * idx + 2];
        float c6[6];
#pragma unroll
        for (int i = 0; i < 6; i++) c6[i] = out.dL_dcov3D[(size_t)6 * idx + i];
        const float s0 = out.dL_dscale[3 * idx], s1 = out.dL_dscale[3 * idx + 1], s2 = out.dL_dscale[3 * idx + 2];
        const float4 r4 = reinterpret_cast<const float4*>(out.dL_drot)[idx];
        gmean = gmean + V3{m0, m1, m2};
#pragma unroll
        for (int i = 0; i < 6; i++) gcov[i] += c6[i];
        gscale = gscale + V3{s0, s1, s2};
        grot = make_float4(grot.x + r4.x, grot.y + r4.y, grot.z + r4.z, grot.w + r4.w);
    }
    out.dL_dmean3D[3 * idx] = gmean.x;
    out.dL_dmean3D[3 * idx + 1] = gmean.y;
    out.dL_dmean3D[3 * idx + 2] = gmean.z;
#pragma unroll
    for (int i = 0; i < 6; i++) out.dL_dcov3D[(size_t)6 * idx + i] = gcov[i];
    out.dL_dscale[3 * idx] = gscale.x;
    out.dL_dscale[3 * idx + 1] = gscale.y;
    out.dL_dscale[3 * idx + 2] = gscale.z;
    reinterpret_cast<float4*>(out.dL_drot)[idx] = grot;
}

// (SRC == 1) dL/dsemantics of the tile's rows: S floats from the Gaussian's record (zeros for a visible Gaussian without tiles).
// Four lanes per row at S = 16 (one float4 each): an instruction moves 16 records' 64-byte pieces in and 16 rows out.
__device__ __forceinline__ void semantics_from_records(const RecArgs& ra, int accumulate, int nrows, const uint32_t* s_src,
                                                       const uint32_t* s_vis) {
    if ((ra.S & 3) == 0) {
        const int S4 = ra.S >> 2;
        for (int i = threadIdx.x; i < nrows * S4; i += 256) {
            const int r = i / S4, sub = i - r * S4;
            const uint32_t o = s_src[r];
            const float4 v = o != 0xFFFFFFFFu ? *reinterpret_cast<const float4*>(ra.rows + (size_t)o * 4 * ra.row_floats + 4 * sub)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
            float4* dst = reinterpret_cast<float4*>(ra.dL_dsemantic + (size_t)s_vis[r] * ra.S + 4 * sub);
            if (accumulate) {
                const float4 p = *dst;
                *dst = make_float4(p.x + v.x, p.y + v.y, p.z + v.z, p.w + v.w);
            } else {
                *dst = v;
            }
        }
    } else {
        for (int i = threadIdx.x; i < nrows * ra.S; i += 256) {
            const int r = i / ra.S, ch = i - r * ra.S;
            const uint32_t o = s_src[r];
            const float v = o != 0xFFFFFFFFu ? ra.rows[(size_t)o * 4 * ra.row_floats + ch] : 0.f;
            float* dst = &ra.dL_dsemantic[(size_t)s_vis[r] * ra.S + ch];
            *dst = accumulate ? *dst + v : v;
        }
    }
}

// The tile's rows -> the dL/dSH rows of their Gaussians: consecutive lanes take consecutive floats of a row (conflict-free LDS reads,
// 192 contiguous bytes per row in memory instead of 48 stores at a 192-byte lane stride); (row, column) advance without a division
__device__ __forceinline__ void stream_dsh_tile(int accumulate, int nrows, int w, const float* s_dsh, const uint32_t* s_vis,
                                                float* __restrict__ dL_dsh) {
    const int dr = 256 / w, dc = 256 - dr * w;
    int r = (int)threadIdx.x / w, col = (int)threadIdx.x - r * w;
    while (r < nrows) {
        float* dst = &dL_dsh[(size_t)s_vis[r] * w + col];
        *dst = accumulate ? *dst + s_dsh[r * (w + 1) + col] : s_dsh[r * (w + 1) + col];
        r += dr;
        col += dc;
        if (col >= w) {
            col -= w;
            r++;
        }
    }
}

// The ids that are still pending move to the front of the list (at most 255 of them: one per thread); returns how many
__device__ __forceinline__ int compact_pending(int npend, int nrows, uint32_t* s_vis) {
    __syncthreads();
    const int rest = npend - nrows;
    const uint32_t moved = (int)threadIdx.x < rest ? s_vis[nrows + threadIdx.x] : 0u;
    __syncthreads();
    if ((int)threadIdx.x < rest) s_vis[threadIdx.x] = moved;
    __syncthreads();
    return rest;
}

// The work of this kernel is per VISIBLE Gaussian (~600 instructions of chain rule, a 128-byte record, 192 bytes of SH in and
// 368 bytes of gradients out); an invisible one needs zeros in its output rows, or -- when the rows still hold the zeros of
// the backward that last wrote the buffers (BwdArgs::prev_radii) -- nothing at all.  With one thread per Gaussian id every wave
// ran the whole chain at the scene's visible fraction of its lanes (51 % on the headline view, 8 % on a close-up of a 3 M
// scene, where the kernel took 264 us for 242 k visible Gaussians), and every block walked all 256 rows of its dL/dSH tile.
// Now a PERSISTENT workgroup walks segments of 256 ids (segment = blockIdx.x, + gridDim.x, ...): it CLASSIFIES a segment's ids
// (visible / needs zeros / nothing to do), writes the zeros at once, and APPENDS the visible ids to a pending list; whenever
// BWD_TILE_ROWS of them are pending (or the input is exhausted) thread t runs the chain for the t-th pending id -- dense lanes
// whatever the visible fraction -- and the block streams out exactly the tile rows that exist.  dL/dSH (192 B per Gaussian at
// degree 3) leaves through an LDS tile (odd row stride: no bank conflicts).
// IDLE Gaussians (SRC == 1 with RecArgs::contrib): visible, but no pixel took anything from it -- it is listed and owns no valid
// row (contribution byte 0), or it has no tiles at all.  Its record is zero and so is everything the chain would form from it
// (69 % of the visible Gaussians of the headline view): the classification puts it with the INVISIBLE ids -- zeros where the
// row does not hold them already, otherwise nothing; nothing at all when accumulating; no SH row, no chain, no tile row.
// SRC: where the blend gradients of a Gaussian come from -- 0 the six per-id arrays, 1 its RECORD in the row scratch (reduce_rows_k<..,
// RECORD>), 2 the kernel SUMS THE ROWS ITSELF (bwd_records 2; 128-byte rows; sum_tile_rows): no record is written or read back,
// no second kernel walks the listed Gaussians; only the BIG ones (reduce_big_k) still pass through a record.
template <bool WITH_DSH, int SRC>
__global__ __launch_bounds__(256, GOI_PBWD_BLOCKS) void preprocess_bwd_k(
    const BwdArgs args, const int* __restrict__ radii, const uint32_t* __restrict__ counters, const uint8_t* __restrict__ clamped,
    float* dL_dmean2D, const float* __restrict__ dL_dconic, float* dL_dcolor, const float* __restrict__ dL_ddepth, const RecArgs ra,
    float* __restrict__ dL_dmean3D, float* __restrict__ dL_dcov3D, float* __restrict__ dL_dsh, float* __restrict__ dL_dscale,
    float* __restrict__ dL_drot) {
    constexpr bool FROM_ROWS = SRC != 0;
    constexpr int BWD_TILE_ROWS = SRC == 2 ? BWD_TILE_ROWS_FUSED : BWD_TILE_ROWS_DEFAULT;
    extern __shared__ float s_dsh[];  // [BWD_TILE_ROWS][3 M + 1] when dL_dsh
    __shared__ uint32_t s_vis[BWD_TILE_ROWS + 256];  // pending visible ids
    __shared__ uint16_t s_zero[256];
    __shared__ uint32_t s_src[SRC == 1 ? BWD_TILE_ROWS : 1];  // (SRC 1) the tile row's record: first slot of a listed Gaussian, ~0u: none
    __shared__ float s_rec[SRC == 2 ? BWD_TILE_ROWS * BWD_REC_FLOATS : 1];  // (SRC 2) the chain's ten inputs of every tile row
    __shared__ int s_wcnt[2][4];
    const Camera cam = load_camera(args.view_p, args.proj_p, args.campos_p);
    const GaussGrads out{dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    const int w = 3 * args.M;
    const int nseg = (args.P + 255) / 256;
    const bool truncated = counters[COUNTER_OVF] != 0;  // (a truncated frame is treated as if nothing were visible: all gradients zero)
    int npend = 0;  // (block-uniform)
    const bool skip_idle = SRC == 1 && ra.contrib != nullptr;
    SegIn cur = load_seg(args, ra, radii, skip_idle, nseg, blockIdx.x);
    for (int seg = blockIdx.x; seg < nseg || npend > 0; seg += gridDim.x) {
        const int base = seg * 256;
        // the contribution byte of a listed visible Gaussian (aux.x of any other id is not an instance), then the next segment's inputs
        const bool vis_t = cur.rad > 0 && !truncated;  // (rad == 0 beyond P and beyond the last segment)
        const bool listed_t = skip_idle && vis_t && cur.tt != 0u;
        const uint8_t contrib_t = listed_t ? ra.contrib[cur.ax] : (uint8_t)0;
        const SegIn nxt = load_seg(args, ra, radii, skip_idle, nseg, seg + (int)gridDim.x);
        int nzero = 0;
        if (seg < nseg) npend += classify_segment(args, cur.prev, skip_idle ? contrib_t != 0 : vis_t, base, npend, s_vis, s_zero, s_wcnt, nzero);
        if (nzero > 0) write_zero_rows<WITH_DSH, FROM_ROWS>(nzero, base, s_zero, w, ra, dL_dmean2D, dL_dcolor, out);
        const bool last_trip = seg + (int)gridDim.x >= nseg;  // no further segment for this block: drain the list
        while (npend >= BWD_TILE_ROWS || (last_trip && npend > 0)) {
            const int nrows = min(BWD_TILE_ROWS, npend);
            const bool visible = (int)threadIdx.x < nrows;
            const int idx = visible ? (int)s_vis[threadIdx.x] : 0;
            // Everything a Gaussian's chain reads is REQUESTED here, before anything waits (load_chain_inputs)
            if constexpr (WITH_DSH) stage_sh_rows(args.shs, nrows, w, s_vis, s_dsh);
            if constexpr (SRC == 2) sum_tile_rows(ra, nrows, s_vis, s_rec);  // (ends in a barrier: s_rec is complete)
            const ChainIn in = load_chain_inputs(args, clamped, idx);
            const BlendIn bl = load_blend_grads<SRC>(visible, idx, args.accumulate, ra, s_rec, s_src, dL_dmean2D, dL_dconic,
                                                     dL_dcolor, dL_ddepth);
            if constexpr (WITH_DSH) __syncthreads();  // the SH rows are in the tile
            if (visible) {
                float gcov[6] = {0, 0, 0, 0, 0, 0};
                V3 gscale = {0, 0, 0};
                float4 grot = make_float4(0, 0, 0, 0);
                Cov2D c;
                ewa_cov2d(in.mean, args.focal_x, args.focal_y, args.tan_fovx, args.tan_fovy, in.cov3D, cam.view, c);
                V3 gmean = cov2d_backward(args, cam.view, c, bl.conic, gcov);
                projection_backward(cam.proj, cam.view, in.mean, bl.m2d, bl.depth, gmean);
                if (args.shs) sh_backward<WITH_DSH>(args, cam.campos, in.mean, idx, in.clamp, bl.col, s_dsh, dL_dcolor, gmean);
                if (args.scales) cov3d_backward(args.scale_modifier, in.rot, in.scale, gcov, gscale, grot);
                store_gauss_grads(args.accumulate, idx, out, gmean, gcov, gscale, grot);
            }
            if constexpr (WITH_DSH || FROM_ROWS) __syncthreads();
            if constexpr (SRC == 1) semantics_from_records(ra, args.accumulate, nrows, s_src, s_vis);
            if constexpr (WITH_DSH) stream_dsh_tile(args.accumulate, nrows, w, s_dsh, s_vis, dL_dsh);
            npend = compact_pending(npend, nrows, s_vis);
        }
        cur = nxt;
    }
}

// dL/dSH of a batch of views from its factors: dL/dSH[g][k] = sum_v basis_k(dir(g, v)) * gcol[v][g], with gcol the
// clamp-masked colour gradients that preprocess_bwd_k<false> leaves in dL_dcolor and dir the normalised direction
// camera v -> Gaussian g.  The basis products are those of the SH backward above (sh_basis_times), and the views are
// added in index order starting from view 0: the result is bit-identical to summing the per-view dL/dSH arrays in
// that order.  Used by the data-parallel gradient exchange (dist.py): 12 bytes per Gaussian and view travel instead
// of 192.  One thread per Gaussian, rows staged through LDS like preprocess_bwd_k.
__global__ __launch_bounds__(256) void sh_grad_from_views_k(int P, int D, int M, int V, const float* __restrict__ means3D,
                                                            const float* __restrict__ campos,  // [V,3]
                                                            const float* __restrict__ gcol,    // [V,P,3]
                                                            float* __restrict__ dL_dsh) {      // [P,M,3]
    extern __shared__ float s_dsh[];  // [256][3 M + 1]
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
    const int idx = gtid < P ? gtid : P - 1;
    const V3 mean = {means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]};
    V3 acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = V3{0, 0, 0};
    for (int v = 0; v < V; v++) {
        const V3 cp = {campos[3 * v], campos[3 * v + 1], campos[3 * v + 2]};
        const V3 dir_orig = mean - cp;
        const V3 dir = dir_orig / sqrtf(dot3(dir_orig, dir_orig));
        const float* gp = gcol + ((size_t)v * P + idx) * 3;
        const V3 g = {gp[0], gp[1], gp[2]};
        V3 t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = V3{0, 0, 0};
        sh_basis_times(D, dir.x, dir.y, dir.z, g, [&](int k, const V3& term) { t[k] = term; });
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] = v == 0 ? t[k] : acc[k] + t[k];
    }
    float* row = s_dsh + (size_t)threadIdx.x * (3 * M + 1);
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (k < M) {
            row[3 * k] = acc[k].x;
            row[3 * k + 1] = acc[k].y;
            row[3 * k + 2] = acc[k].z;
        }
    __syncthreads();
    const int w = 3 * M;
    const int rows = min(256, P - (int)(blockIdx.x * blockDim.x));
    float* out = dL_dsh + (size_t)blockIdx.x * blockDim.x * w;
    for (int i = threadIdx.x; i < rows * w; i += 256) {
        const int r = i / w, col = i - r * w;
        out[i] = s_dsh[r * (w + 1) + col];
    }
}

}  // namespace

void launch_preprocess_bwd(const GoiRasterScene& sc, const GeomView& g, const int* radii, const PreprocessBwdArgs& args,
                           hipStream_t s) {
    const BlendGrads& bl = args.blend;
    const GaussGrads& out = args.out;
    BwdArgs a;
    a.prev_radii = args.prev_radii;
    a.prev_mask = args.prev_mask;
    a.row_mask = args.row_mask;
    a.accumulate = args.accumulate ? 1 : 0;
    a.P = sc.P; a.D = sc.D; a.M = sc.M;
    a.means3D = sc.means3D; a.shs = sc.shs; a.scales = sc.scales; a.rotations = sc.rotations;
    a.cov3D = sc.cov3D_precomp ? sc.cov3D_precomp : g.cov3D;
    a.scale_modifier = sc.scale_modifier; a.tan_fovx = sc.tan_fovx; a.tan_fovy = sc.tan_fovy;
    a.focal_y = sc.H / (2.0f * sc.tan_fovy);
    a.focal_x = sc.W / (2.0f * sc.tan_fovx);
    a.view_p = sc.viewmatrix; a.proj_p = sc.projmatrix; a.campos_p = sc.campos;
    const bool with_sh = sc.shs && sc.M > 0 && out.dL_dsh;  // dL_dsh == NULL with SH colours: factored mode
    // args.rows: the blend gradients are the records reduce_rows_k<.., RECORD> left in the row scratch -- or, with args.flags
    // (bwd_records 2), the rows themselves: the kernel sums them (128-byte rows only: the caller checks)
    const bool fused = args.rows != nullptr && args.flags != nullptr;
    const int tile_rows = fused ? BWD_TILE_ROWS_FUSED : BWD_TILE_ROWS_DEFAULT;
    const size_t lds = with_sh ? (size_t)tile_rows * (3 * sc.M + 1) * sizeof(float) : 0;  // 43.9 KB at M = 16 (40.8 fused)
    RecArgs ra;
    ra.rows = args.rows; ra.aux = g.aux; ra.tiles_touched = g.tiles_touched;
    ra.row_floats = bwd_row_floats(sc.S); ra.S = sc.S; ra.nch = 4 * ((sc.S + 3) / 4) + 4;
    ra.dL_dopacity = bl.dL_dopacity; ra.dL_dsemantic = bl.dL_dsemantic;
    ra.flags = args.flags; ra.n_dev = g.counters + COUNTER_N; ra.N_cap = (uint32_t)std::max(args.n_cap, 0);
    ra.contrib = (args.rows != nullptr && !fused) ? args.contrib : nullptr;
    // persistent workgroups: every CU gets as many as fit (registers and the staging tile: BWD_BLOCKS_PER_CU), each walks
    // segments of 256 ids
    static const int n_cu = []() {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    // max_blocks > 0 (goi_raster_debug_preprocess_backward only): fewer persistent workgroups, each walking more segments
    int blocks = std::min((sc.P + 255) / 256, n_cu * BWD_BLOCKS_PER_CU);
    if (args.max_blocks > 0) blocks = std::min(blocks, args.max_blocks);
    const dim3 grid((unsigned)blocks);
#define GOI_PBWD(DSH, SRC, LDS)                                                                                           \
    preprocess_bwd_k<DSH, SRC><<<grid, dim3(256), LDS, s>>>(a, radii, g.counters, g.clamped, bl.dL_dmean2D, bl.dL_dconic,     \
                                                            bl.dL_dcolor, bl.dL_ddepth, ra, out.dL_dmean3D, out.dL_dcov3D,   \
                                                            DSH ? out.dL_dsh : nullptr, out.dL_dscale, out.dL_drot)
    if (with_sh && fused) GOI_PBWD(true, 2, lds);
    else if (with_sh && args.rows) GOI_PBWD(true, 1, lds);
    else if (with_sh) GOI_PBWD(true, 0, lds);
    else if (fused) GOI_PBWD(false, 2, 0);
    else if (args.rows) GOI_PBWD(false, 1, 0);
    else GOI_PBWD(false, 0, 0);
#undef GOI_PBWD
}

}  // namespace goi

using namespace goi;

extern "C" {

int goi_raster_sh_grad_from_views(int P, int D, int M, int V, const float* means3D, const float* campos, const float* gcol,
                           float* dL_dsh, void* stream) {
    if (P <= 0 || V <= 0) return 0;
    if (D < 0 || D > 3 || M < (D + 1) * (D + 1) || M > 16) return fail("goi_raster_sh_grad_from_views: need 0 <= D <= 3 and (D+1)^2 <= M <= 16");
    if (!means3D || !campos || !gcol || !dL_dsh) return fail("goi_raster_sh_grad_from_views: NULL pointer");
    const size_t lds = (size_t)256 * (3 * M + 1) * sizeof(float);
    sh_grad_from_views_k<<<dim3((P + 255) / 256), dim3(256), lds, static_cast<hipStream_t>(stream)>>>(P, D, M, V, means3D, campos,
                                                                                                      gcol, dL_dsh);
    if (hipGetLastError() != hipSuccess) return fail("goi_raster_sh_grad_from_views: launch failed");
    return 0;
}

int goi_raster_debug_preprocess_backward(const GoiRasterScene* scene, int source, int flags, int max_blocks, long long n_cap,
                                         const uint32_t* frame, const int* radii, const uint8_t* clamped, const float* cov3D,
                                         const int* prev_radii, const uint32_t* aux, const uint32_t* tiles_touched,
                                         const float* rows, const uint8_t* row_flags, float* dL_dmean2D, const float* dL_dconic,
                                         float* dL_dopacity, float* dL_dcolor, float* dL_dsemantic, const float* dL_ddepth,
                                         float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                         void* workspace, void* stream) {
    const std::string fn = "goi_raster_debug_preprocess_backward";
    if (!scene) return fail(fn + ": scene is NULL");
    const GoiRasterScene& sc = *scene;
    if (sc.P < 0 || sc.W <= 0 || sc.H <= 0) return fail(fn + ": bad P/W/H");
    if (sc.S < 1 || sc.S > 32) return fail(fn + ": need 1 <= S <= 32");
    if (source < 0 || source > 2) return fail(fn + ": unknown source (0 per-id arrays, 1 records, 2 rows summed in the kernel)");
    if (flags & ~GOI_BACKWARD_ACCUMULATE) return fail(fn + ": unknown flag bits");
    if (max_blocks < 0) return fail(fn + ": max_blocks must be >= 0 (0: the product's grid)");
    if (n_cap < 0 || n_cap > INT_MAX) return fail(fn + ": need 0 <= n_cap < 2^31");
    if (source == 2 && bwd_row_floats(sc.S) != 32) return fail(fn + ": source 2 sums 128-byte rows only (S = 5 .. 20)");
    if (sc.P == 0) return 0;
    if (!(sc.tan_fovx > 0.f) || !(sc.tan_fovy > 0.f)) return fail(fn + ": tan_fovx / tan_fovy must be positive");
    if (!sc.means3D || !sc.viewmatrix || !sc.projmatrix || !sc.campos) return fail(fn + ": a required scene pointer is NULL");
    if (sc.shs && sc.colors_precomp) return fail(fn + ": shs and colors_precomp are both given");
    if (sc.shs && (sc.D < 0 || sc.D > 3 || sc.M < (sc.D + 1) * (sc.D + 1) || sc.M > 16))
        return fail(fn + ": SH degree must be 0..3 and (D+1)^2 <= M <= 16");
    if (sc.shs && (3 * sc.M) % 4 == 0 && (reinterpret_cast<uintptr_t>(sc.shs) & 15u) != 0)
        return fail(fn + ": shs must be 16-byte aligned when 3 M is a multiple of 4");
    if (!sc.shs && dL_dsh) return fail(fn + ": dL_dsh without shs");
    if ((sc.scales == nullptr) != (sc.rotations == nullptr)) return fail(fn + ": scales and rotations go together");
    if ((sc.scales != nullptr) == (sc.cov3D_precomp != nullptr))
        return fail(fn + ": exactly one of the scale/rotation pair and cov3D_precomp");
    if (sc.scales && !cov3D) return fail(fn + ": cov3D (what the forward computed from scale/rotation) is NULL");
    if (sc.rotations && (reinterpret_cast<uintptr_t>(sc.rotations) & 15u) != 0) return fail(fn + ": rotations must be 16-byte aligned");
    const bool accumulate = (flags & GOI_BACKWARD_ACCUMULATE) != 0;
    if (accumulate && source != 1) return fail(fn + ": accumulate needs source 1 (the records)");
    if (accumulate && prev_radii) return fail(fn + ": accumulate with prev_radii");
    if (accumulate && sc.shs && !dL_dsh) return fail(fn + ": accumulate with factored SH (dL_dsh NULL)");
    if (!frame || !radii || !dL_dmean2D || !dL_dcolor || !dL_dmean3D || !dL_dcov3D || !dL_dscale || !dL_drot ||
        (sc.shs && !clamped))
        return fail(fn + ": a required pointer is NULL");
    if (source == 0 && (!dL_dconic || !dL_ddepth)) return fail(fn + ": source 0 reads dL_dconic and dL_ddepth");
    if (source != 0 && (!aux || !tiles_touched || !rows || !dL_dopacity || !dL_dsemantic))
        return fail(fn + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic");
    if (source == 2 && !row_flags) return fail(fn + ": source 2 needs the validity bytes");
    if (check_workspace(fn, workspace) < 0) return -1;
    if ((reinterpret_cast<uintptr_t>(dL_drot) & 15u) || (aux && (reinterpret_cast<uintptr_t>(aux) & 15u)) ||
        (rows && (reinterpret_cast<uintptr_t>(rows) & 15u)) || (row_flags && (reinterpret_cast<uintptr_t>(row_flags) & 3u)) ||
        (dL_dsemantic && (reinterpret_cast<uintptr_t>(dL_dsemantic) & 15u)))
        return fail(fn + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    GeomView g{};
    g.counters = static_cast<uint32_t*>(workspace);  // a 256-byte counter block: the frame words where the kernel reads them
    g.cov3D = const_cast<float*>(cov3D);
    g.clamped = const_cast<uint8_t*>(clamped);
    g.aux = reinterpret_cast<uint4*>(const_cast<uint32_t*>(aux));
    g.tiles_touched = const_cast<uint32_t*>(tiles_touched);
    static_assert(COUNTER_N < 64 && COUNTER_V < 64 && COUNTER_OVF < 64, "the frame words fit the 256-byte counter block");
    GOI_HIP(hipMemcpyAsync(g.counters + COUNTER_N, frame + 0, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    GOI_HIP(hipMemcpyAsync(g.counters + COUNTER_V, frame + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    GOI_HIP(hipMemcpyAsync(g.counters + COUNTER_OVF, frame + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    PreprocessBwdArgs pa;
    pa.blend = BlendGrads{dL_dmean2D, const_cast<float*>(dL_dconic), dL_dopacity, dL_dcolor, dL_dsemantic,
                          const_cast<float*>(dL_ddepth)};  // (dL_dconic and dL_ddepth are only ever read)
    pa.out = GaussGrads{dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    pa.rows = source != 0 ? rows : nullptr;
    pa.flags = source == 2 ? row_flags : nullptr;
    pa.n_cap = (int)n_cap;
    pa.prev_radii = prev_radii;
    pa.accumulate = accumulate;
    pa.max_blocks = max_blocks;
    launch_preprocess_bwd(sc, g, radii, pa, s);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
