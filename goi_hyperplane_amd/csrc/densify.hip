// Densification and pruning of the Gaussian set (scene/gaussian_model.py:291-513): the methods that change P.
//
// The reference rebuilds all 7 parameter tensors and their 14 Adam moments four times per densify_and_prune (clone cat,
// split cat, prune of the split parents, final prune), every boolean index a host synchronisation.  Here the whole
// operation is three kernels and one scan:
//   densify_plan_k    one pass over P reads accum, denom, scaling, opacity (24 B per Gaussian) and decides for every
//                     ORIGINAL Gaussian i which of its rows survive: the original itself, its clone, its two children
//                     (they share opacity and scale, so they are kept or pruned together), and whether it was selected
//                     for a split (the normal draws Z are indexed by the rank among ALL split parents).  Four u32 streams.
//   exclusive_scan_u32 over the four streams laid end to end: the prefix of stream k at i is directly the destination
//                     row of that block in the final layout
//                         [originals kept] [clones kept] [first children kept] [second children kept]
//                     (each block in ascending original index: the order the reference's cat / repeat / boolean index
//                     sequence produces), and the counts come out at the stream boundaries.
//   densify_apply_k   one launch over a table of row groups (parameters, moments, statistics): each lane reads its
//                     source floats once, coalesced, and writes each to up to four destinations; children's xyz and
//                     scaling are formed from the parent's quaternion, scale and Z; new moments and statistics are 0.
// prune_points is the same apply with only the keep block (prune_plan_k).  No float atomics: the output is deterministic.
//
// The decisions restate the reference's fp32 torch arithmetic op for op (this TU is compiled with -ffp-contract=off):
//   grad = accum / denom, NaN -> 0;  smax = max_k exp(scaling_k) (NaN propagates, as torch.max does)
//   clone: sqrt(grad * grad) >= max_grad && smax <= thr_s     (torch.norm over the one-element last dim)
//   split: grad >= max_grad && smax > thr_s                   (padded_grad: clones see 0 and are never split)
//   prune: sigmoid(opacity) < min_opacity; with max_screen_size truthy also  max_radii2D > max_screen_size  (evaluated on
//          the ZEROED radii of densification_postfix: one flag for every row) or smax > 0.1 extent
//   child scaling = log(exp(s) * (1 / 1.6f))  (torch on the device divides by a CPU scalar as a multiply by its fp32
//          reciprocal); its prune test takes exp of that again
//   child xyz = build_rotation(q) (utils/general_utils.py:89-110) @ (Z * exp(s) + 0) + xyz
// Thresholds arrive rounded to fp32 once, as torch rounds a Python scalar for a comparison with an fp32 tensor.
// C entries, with the limits they enforce, at the end of the file: goi_raster_densify_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"

namespace goi {

// thresholds rounded to fp32 once, and the workspace of a plan
struct DensifyThresholds {
    float max_grad, thr_scale, min_opacity, big_world, split_inv;
    int screen, screen_all;  // max_screen_size truthy; 0 > max_screen_size (the zeroed radii test prunes every row)
};
struct DensifyView {
    uint8_t* flags;     // [P] plan byte per original Gaussian
    uint32_t* rank;     // [4P] keep / clone / children / split streams, scanned in place: destination rows
    uint32_t* scratch;  // scan partials
    uint32_t* total;
};

namespace {

constexpr int DENS_THREADS = 256;
constexpr int APPLY_PER_LANE = 4;
constexpr int APPLY_BLOCK_ELEMS = DENS_THREADS * APPLY_PER_LANE;
constexpr unsigned long long APPLY_GRID_X = 1ull << 20;
constexpr uint8_t F_KEEP = 1, F_CLONE = 2, F_CHILDREN = 4, F_SPLIT = 8;  // bits of the per-Gaussian plan byte

// torch.max(dim) keeps a NaN it meets
__device__ __forceinline__ float max3_nan(float a, float b, float c) {
    float m = a;
    m = ((b > m || isnan(b)) && !isnan(m)) ? b : m;
    m = ((c > m || isnan(c)) && !isnan(m)) ? c : m;
    return m;
}

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }  // torch's sigmoid kernel

__global__ __launch_bounds__(DENS_THREADS) void densify_stats_k(long long P, const float* __restrict__ grad, long long stride,
                                                                const uint8_t* __restrict__ filter, float* __restrict__ accum,
                                                                float* __restrict__ denom) {
    const long long i = (long long)blockIdx.x * DENS_THREADS + threadIdx.x;
    if (i >= P || !filter[i]) return;
    const float gx = grad[i * stride], gy = grad[i * stride + 1];
    accum[i] = accum[i] + sqrtf(gx * gx + gy * gy);
    denom[i] = denom[i] + 1.0f;
}

__global__ __launch_bounds__(DENS_THREADS) void densify_plan_k(long long P, const float* __restrict__ accum,
                                                               const float* __restrict__ denom, const float* __restrict__ scaling,
                                                               const float* __restrict__ opacity, const DensifyThresholds t,
                                                               uint8_t* __restrict__ flags, uint32_t* __restrict__ streams) {
    const long long i = (long long)blockIdx.x * DENS_THREADS + threadIdx.x;
    if (i >= P) return;
    float g = accum[i] / denom[i];
    if (isnan(g)) g = 0.0f;
    const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
    const float smax = max3_nan(e0, e1, e2);
    const bool clone = sqrtf(g * g) >= t.max_grad && smax <= t.thr_scale;
    const bool split = g >= t.max_grad && smax > t.thr_scale;
    const bool faint = sigmoid_ref(opacity[i]) < t.min_opacity;
    const bool pruned = faint || (t.screen && (t.screen_all || smax > t.big_world));
    bool children = false;
    if (split) {
        const float c0 = expf(logf(e0 * t.split_inv)), c1 = expf(logf(e1 * t.split_inv)), c2 = expf(logf(e2 * t.split_inv));
        children = !(faint || (t.screen && (t.screen_all || max3_nan(c0, c1, c2) > t.big_world)));
    }
    const bool keep = !split && !pruned, kclone = clone && !pruned;
    flags[i] = (uint8_t)((keep ? F_KEEP : 0) | (kclone ? F_CLONE : 0) | (children ? F_CHILDREN : 0) | (split ? F_SPLIT : 0));
    streams[i] = keep;
    streams[P + i] = kclone;
    streams[2 * P + i] = children;
    streams[3 * P + i] = split;
}

__global__ __launch_bounds__(DENS_THREADS) void prune_plan_k(long long P, const uint8_t* __restrict__ mask,
                                                             uint8_t* __restrict__ flags, uint32_t* __restrict__ streams) {
    const long long i = (long long)blockIdx.x * DENS_THREADS + threadIdx.x;
    if (i >= P) return;
    const bool keep = mask[i] == 0;
    flags[i] = keep ? F_KEEP : 0;
    streams[i] = keep;
}

// counts[k] = rows in stream k's block: the scanned prefix at the stream boundaries (the last one from the total)
__global__ void densify_counts_k(const uint32_t* __restrict__ rank, long long P, int n_streams, const uint32_t* __restrict__ total,
                                 uint32_t* __restrict__ counts) {
    const int k = threadIdx.x;
    if (k >= 4) return;
    if (k >= n_streams) {
        counts[k] = 0;
        return;
    }
    const uint32_t hi = k + 1 < n_streams ? rank[(k + 1) * P] : *total;
    counts[k] = hi - rank[k * P];
}

struct ApplyTable {
    GoiDensifyRows g[GOI_DENSIFY_MAX_GROUPS];
    unsigned long long block_end[GOI_DENSIFY_MAX_GROUPS];  // inclusive prefix of work blocks per group
    int n;
};

struct ApplyArgs {
    long long P;
    const uint8_t* flags;
    const uint32_t* rank;     // [4P] scanned streams: destination rows
    const float* rotation;    // [P,4] raw quaternions of the originals (children's xyz)
    const float* scaling;     // [P,3] raw log-scales of the originals
    const float* z;           // [2 n_split, 3] standard-normal draws
    long long n_split;
    long long kept_children;  // S': the second children's block starts S' rows after the first one's
    float split_inv;
};

// the parent's sample for Z row zr, component k: torch.normal = normal_(0, 1), then mul_(std), add_(mean = 0)
__device__ __forceinline__ float child_sample(const ApplyArgs& a, long long i, long long zr, int k) {
    return a.z[zr * 3 + k] * expf(a.scaling[3 * i + k]) + 0.0f;
}

// component c of build_rotation(q) @ sample + xyz_c for Z row zr
__device__ float child_xyz(const ApplyArgs& a, long long i, long long zr, int c, float xyz) {
    const float* q = a.rotation + 4 * i;
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
    float m0, m1, m2;
    if (c == 0) {
        m0 = 1.0f - 2.0f * (y * y + z * z);
        m1 = 2.0f * (x * y - r * z);
        m2 = 2.0f * (x * z + r * y);
    } else if (c == 1) {
        m0 = 2.0f * (x * y + r * z);
        m1 = 1.0f - 2.0f * (x * x + z * z);
        m2 = 2.0f * (y * z - r * x);
    } else {
        m0 = 2.0f * (x * z - r * y);
        m1 = 2.0f * (y * z + r * x);
        m2 = 1.0f - 2.0f * (x * x + y * y);
    }
    const float s0 = child_sample(a, i, zr, 0), s1 = child_sample(a, i, zr, 1), s2 = child_sample(a, i, zr, 2);
    return fmaf(m2, s2, fmaf(m1, s1, m0 * s0)) + xyz;
}

// One work block = APPLY_BLOCK_ELEMS consecutive source floats of one group, one workgroup each; the grid is 2-D (rows of
// APPLY_GRID_X workgroups) so that a launch covers any P the API accepts.  A lane first loads all of its source floats
// and plan bytes, then the ranks its plan bytes ask for, then stores: two dependent round trips per APPLY_PER_LANE
// elements, and no load waits behind a store (dst is not known not to alias the inputs, so interleaved loads and stores
// would be issued one element after the other).
__global__ __launch_bounds__(DENS_THREADS) void densify_apply_k(const ApplyTable t, const ApplyArgs a,
                                                                unsigned long long n_blocks) {
    const long long P = a.P;
    const unsigned long long wb = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;
    if (wb >= n_blocks) return;
    int gi = 0;
#pragma unroll
    for (int k = 0; k < GOI_DENSIFY_MAX_GROUPS - 1; k++)
        if (k < t.n - 1 && wb >= t.block_end[k]) gi = k + 1;
    const GoiDensifyRows grp = t.g[gi];
    const unsigned long long b0 = gi ? t.block_end[gi - 1] : 0ull;
    const long long rl = grp.row_len;
    const long long numel = grp.rows * rl;
    const long long e_blk = (long long)(wb - b0) * APPLY_BLOCK_ELEMS;
    if (grp.mode == GOI_DENSIFY_ZERO) {
#pragma unroll
        for (int j = 0; j < APPLY_PER_LANE; j++) {
            const long long e = e_blk + j * DENS_THREADS + threadIdx.x;
            if (e < numel) grp.dst[e] = 0.0f;
        }
        return;
    }
    // the block's first row once in 64 bits; each lane's row from a 32-bit quotient of its offset behind it
    const long long i_blk = e_blk / rl;
    const uint32_t c_blk = (uint32_t)(e_blk - i_blk * rl);
    float v[APPLY_PER_LANE];
    uint32_t f[APPLY_PER_LANE], r_keep[APPLY_PER_LANE], r_clone[APPLY_PER_LANE], r_child[APPLY_PER_LANE],
        r_split[APPLY_PER_LANE];
    long long row[APPLY_PER_LANE], col[APPLY_PER_LANE];
#pragma unroll
    for (int j = 0; j < APPLY_PER_LANE; j++) {  // round trip 1: source floats and plan bytes
        const long long e = e_blk + j * DENS_THREADS + threadIdx.x;
        const uint32_t off = c_blk + (uint32_t)(j * DENS_THREADS + threadIdx.x);
        const uint32_t di = off / (uint32_t)rl;
        row[j] = i_blk + di;
        col[j] = (long long)(off - di * (uint32_t)rl);
        f[j] = 0;
        v[j] = 0.0f;
        if (e < numel) {
            v[j] = grp.src[e];
            f[j] = a.flags[row[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < APPLY_PER_LANE; j++) {  // round trip 2: the destination rows the plan bytes ask for
        const long long i = row[j];
        r_keep[j] = (f[j] & F_KEEP) ? a.rank[i] : 0u;
        r_clone[j] = (f[j] & F_CLONE) ? a.rank[P + i] : 0u;
        r_child[j] = (f[j] & F_CHILDREN) ? a.rank[2 * P + i] : 0u;
        r_split[j] = (f[j] & F_CHILDREN) && grp.mode == GOI_DENSIFY_XYZ ? a.rank[3 * P + i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < APPLY_PER_LANE; j++) {  // stores
        const long long i = row[j], c = col[j];
        if (f[j] & F_KEEP) grp.dst[(long long)r_keep[j] * rl + c] = v[j];
        if (f[j] & F_CLONE) grp.dst[(long long)r_clone[j] * rl + c] = grp.mode == GOI_DENSIFY_MOMENT ? 0.0f : v[j];
        if (f[j] & F_CHILDREN) {
            const long long d1 = r_child[j], d2 = d1 + a.kept_children;
            float v1 = v[j], v2 = v[j];
            if (grp.mode == GOI_DENSIFY_MOMENT) {
                v1 = v2 = 0.0f;
            } else if (grp.mode == GOI_DENSIFY_XYZ) {
                const long long r = (long long)r_split[j] - (long long)a.rank[3 * P];
                v1 = child_xyz(a, i, r, (int)c, v[j]);
                v2 = child_xyz(a, i, a.n_split + r, (int)c, v[j]);
            } else if (grp.mode == GOI_DENSIFY_SCALING) {
                v1 = v2 = logf(expf(v[j]) * a.split_inv);
            }
            grp.dst[d1 * rl + c] = v1;
            grp.dst[d2 * rl + c] = v2;
        }
    }
}

inline size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }

// [P] plan bytes | [4P] streams, scanned in place | scan partials | total
size_t densify_layout(long long P, char* base, DensifyView* v) {
    Carver c(base);
    DensifyView d;
    d.flags = c.take<uint8_t>((size_t)P);
    d.rank = c.take<uint32_t>(4 * (size_t)P);
    d.scratch = c.take<uint32_t>(scan_scratch_words(4 * (size_t)P));
    d.total = c.take<uint32_t>(64);
    if (v) *v = d;
    return c.end();
}

void launch_densify_plan(long long P, const float* accum, const float* denom, const float* scaling, const float* opacity,
                         const DensifyThresholds& t, uint32_t* counts, const DensifyView& v, hipStream_t s) {
    if (P > 0) {
        densify_plan_k<<<dim3((unsigned)div_up((size_t)P, DENS_THREADS)), dim3(DENS_THREADS), 0, s>>>(P, accum, denom, scaling,
                                                                                                       opacity, t, v.flags, v.rank);
        exclusive_scan_u32(v.rank, nullptr, v.rank, 4 * (size_t)P, v.total, v.scratch, s);
    }
    densify_counts_k<<<dim3(1), dim3(64), 0, s>>>(v.rank, P, P > 0 ? 4 : 0, v.total, counts);
}

void launch_prune_plan(long long P, const uint8_t* mask, uint32_t* counts, const DensifyView& v, hipStream_t s) {
    if (P > 0) {
        prune_plan_k<<<dim3((unsigned)div_up((size_t)P, DENS_THREADS)), dim3(DENS_THREADS), 0, s>>>(P, mask, v.flags, v.rank);
        exclusive_scan_u32(v.rank, nullptr, v.rank, (size_t)P, v.total, v.scratch, s);
    }
    densify_counts_k<<<dim3(1), dim3(64), 0, s>>>(v.rank, P, P > 0 ? 1 : 0, v.total, counts);
}

void launch_densify_apply(long long P, const GoiDensifyRows* groups, int n_groups, const float* rotation, const float* scaling,
                          const float* z, long long n_split, long long kept_children, float split_inv, const DensifyView& v,
                          hipStream_t s) {
    ApplyTable t;
    unsigned long long blocks = 0;
    t.n = 0;
    for (int k = 0; k < n_groups; k++) {
        const long long numel = groups[k].rows * (long long)groups[k].row_len;
        if (numel <= 0) continue;
        t.g[t.n] = groups[k];
        blocks += div_up((size_t)numel, APPLY_BLOCK_ELEMS);
        t.block_end[t.n] = blocks;
        t.n++;
    }
    if (t.n == 0) return;
    for (int k = t.n; k < GOI_DENSIFY_MAX_GROUPS; k++) {
        t.g[k] = t.g[0];
        t.block_end[k] = blocks;
    }
    ApplyArgs a;
    a.P = P;
    a.flags = v.flags;
    a.rank = v.rank;
    a.rotation = rotation;
    a.scaling = scaling;
    a.z = z;
    a.n_split = n_split;
    a.kept_children = kept_children;
    a.split_inv = split_inv;
    // one workgroup per work block, in rows of APPLY_GRID_X (each grid dimension stays below 2^32 work-items)
    const unsigned gx = (unsigned)(blocks < APPLY_GRID_X ? blocks : APPLY_GRID_X);
    const unsigned gy = (unsigned)div_up((size_t)blocks, gx);
    densify_apply_k<<<dim3(gx, gy), dim3(DENS_THREADS), 0, s>>>(t, a, blocks);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_raster_densify_workspace_bytes(long long P) {
    return (P >= 0 && P < (1ll << 30)) ? densify_layout(P, nullptr, nullptr) + 256 : 0;
}

int goi_raster_densify_stats(long long P, const float* grad, long long grad_stride, const unsigned char* filter, float* accum,
                             float* denom, void* stream) {
    const std::string fn = "goi_raster_densify_stats: ";
    if (P < 0 || P >= (1ll << 31)) return fail(fn + "need 0 <= P < 2^31");
    if (grad_stride < 2) return fail(fn + "grad_stride must be >= 2");
    if (P > 0 && (!grad || !filter || !accum || !denom)) return fail(fn + "a required pointer is NULL");
    if (P > 0)
        densify_stats_k<<<dim3((unsigned)div_up((size_t)P, DENS_THREADS)), dim3(DENS_THREADS), 0, static_cast<hipStream_t>(stream)>>>(
            P, grad, grad_stride, filter, accum, denom);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_densify_plan(long long P, const float* accum, const float* denom, const float* scaling, const float* opacity,
                            double max_grad, double scale_threshold, double min_opacity, int screen_test, double max_screen_size,
                            double big_threshold, unsigned* counts, void* workspace, void* stream) {
    const std::string fn = "goi_raster_densify_plan: ";
    if (P < 0 || P >= (1ll << 30)) return fail(fn + "need 0 <= P < 2^30");
    if (!counts || (P > 0 && (!accum || !denom || !scaling || !opacity))) return fail(fn + "a required pointer is NULL");
    if (check_workspace("goi_raster_densify_plan", workspace) < 0) return -1;
    refresh_options();
    DensifyView v;
    densify_layout(P, static_cast<char*>(workspace), &v);
    DensifyThresholds t;
    t.max_grad = (float)max_grad;  // a Python scalar meets an fp32 tensor: rounded to fp32 once
    t.thr_scale = (float)scale_threshold;
    t.min_opacity = (float)min_opacity;
    t.big_world = (float)big_threshold;
    t.split_inv = 1.0f / (float)(0.8 * 2);  // torch's reciprocal of the CPU scalar 0.8 * N
    t.screen = screen_test != 0;
    t.screen_all = 0.0f > (float)max_screen_size;  // max_radii2D is all zeros when the reference tests it
    launch_densify_plan(P, accum, denom, scaling, opacity, t, counts, v, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_densify_prune_plan(long long P, const unsigned char* mask, unsigned* counts, void* workspace, void* stream) {
    const std::string fn = "goi_raster_densify_prune_plan: ";
    if (P < 0 || P >= (1ll << 30)) return fail(fn + "need 0 <= P < 2^30");
    if (!counts || (P > 0 && !mask)) return fail(fn + "a required pointer is NULL");
    if (check_workspace("goi_raster_densify_prune_plan", workspace) < 0) return -1;
    refresh_options();
    DensifyView v;
    densify_layout(P, static_cast<char*>(workspace), &v);
    launch_prune_plan(P, mask, counts, v, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_densify_apply(long long P, const GoiDensifyRows* groups, int n_groups, const float* rotation, const float* scaling,
                             const float* z, long long n_split, long long kept_children, const void* workspace, void* stream) {
    const std::string fn = "goi_raster_densify_apply: ";
    if (P < 0 || P >= (1ll << 30)) return fail(fn + "need 0 <= P < 2^30");
    if (n_groups < 0 || n_groups > GOI_DENSIFY_MAX_GROUPS) return fail(fn + "n_groups must be 0..24");
    if (n_groups && !groups) return fail(fn + "groups is NULL");
    if (n_split < 0 || n_split > P || kept_children < 0 || kept_children > n_split) return fail(fn + "bad n_split / kept_children");
    if (check_workspace("goi_raster_densify_apply", workspace) < 0) return -1;
    for (int k = 0; k < n_groups; k++) {
        const GoiDensifyRows& g = groups[k];
        if (g.row_len < 1 || g.rows < 0 || g.mode < GOI_DENSIFY_PARAM || g.mode > GOI_DENSIFY_ZERO) return fail(fn + "bad group");
        if (g.mode != GOI_DENSIFY_ZERO && g.rows != P) return fail(fn + "a copied group must have P source rows");
        if (g.rows > 0 && (!g.dst || (g.mode != GOI_DENSIFY_ZERO && !g.src))) return fail(fn + "a group pointer is NULL");
        if ((g.mode == GOI_DENSIFY_XYZ || g.mode == GOI_DENSIFY_SCALING) && g.row_len != 3) return fail(fn + "xyz / scaling rows are 3 floats");
        if (g.mode == GOI_DENSIFY_XYZ && kept_children > 0 && (!rotation || !scaling || !z))
            return fail(fn + "children's xyz need rotation, scaling and z");
    }
    DensifyView v;
    densify_layout(P, static_cast<char*>(const_cast<void*>(workspace)), &v);
    launch_densify_apply(P, groups, n_groups, rotation, scaling, z, n_split, kept_children, 1.0f / (float)(0.8 * 2), v,
                         static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
