// A mesh from the Gaussians: the density grid of DreamGaussian's extract_fields and a marching-
// tetrahedra iso-surface of it.  gfx950 only; compiled with -ffp-contract=off (the iso-surface's vertices are compared bit
// for bit with a numpy restatement, one rounding per operation; the density loop asks for its FMAs by name).
//
// Density, goi_field_density:
//   field_bounds_k   min / max of the kept centres (integer atomics on order-preserving encodings: exact and order-free)
//   field_frame_k    center = (min + max) / 2, scale = 1.8 / max extent -- or the caller's frame
//   field_prep_k     per Gaussian: normalised centre, the six coefficients of the inverse covariance by gaussian_3d_coeff's
//                    formulas (in fp64, rounded once), and the key of its home cell (cells of one block's size on a lattice that
//                    reaches `reach` cells beyond the grid; a Gaussian that is not kept gets the key behind the last cell)
//   radix_sort_pairs stable: inside a cell the Gaussians stay in ascending index
//   field_gather_k   (centre, opacity) in sorted order;  field_cells_k  first sorted position of every cell (lower bound)
//   field_density_k  one workgroup per block.  The candidates of a block are the (2 reach + 1)^2 contiguous runs of
//                    2 reach + 1 cells around it; every candidate takes the reference's strict box test against the block's
//                    widened point bounds; survivors are appended IN ORDER to an LDS list (centre, six coefficients, opacity,
//                    attributes) and, whenever the list holds FIELD_BATCH or more, every thread adds them to its points'
//                    register accumulators.  The sum at a point therefore runs over the block's members in (cell, index)
//                    order whatever the batching: no atomics, the same bits every run.
// reach = floor(relax_ratio) + 2 covers every member: a member's centre c obeys lo_b < c < hi_b with
// lo_b >= -1 + b w - relax w and hi_b <= -1 + (b + 1) w + relax w (w = 2 / num_blocks; the points of torch.linspace(-1, 1, R)
// that block b owns lie inside [-1 + b w, -1 + (b + 1) w]), so floor((c + 1) / w) is in [b - ceil(relax), b + 1 + floor(relax)];
// one more cell pays for the rounding of the fp32 cell coordinate.
//
// Iso-surface, goi_field_iso_count / goi_field_iso_emit: marching tetrahedra on the Kuhn split (six tetrahedra around the
// cube's main diagonal, one per axis permutation: v0 = origin, v1 = v0 + e_p1, v2 = v1 + e_p2, v3 = origin + (1,1,1)).  Every
// tetrahedron edge is one of the seven edges its lower endpoint owns (+x +y +z +xy +xz +yz +xyz), so a vertex is
// addressed as (owner point, slot) and neighbouring cubes agree on it.  Orientation is closed form: with s the parity of
// the permutation, a lone vertex at tetrahedron index m gives the triangle (m j, m k, m l), j < k < l, the orientation
// s (-1)^m (positive: its normal points away from m); two inside vertices a < b against c < d give the quad
// (ac, ad, bd, bc) with orientation s sign(a b c d) (positive: towards c d).
// C entries, with the limits they enforce, at the end of the file: goi_field_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

#include <math.h>

namespace goi {
namespace {

constexpr int FIELD_THREADS = 256;
constexpr int FIELD_BATCH = GOI_FIELD_BATCH;
constexpr int FIELD_CAP = FIELD_BATCH + FIELD_THREADS;  // a chunk of candidates always fits behind a list below FIELD_BATCH
constexpr uint32_t ENC_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ bool field_keep(long long i, const float* xyz, const float* opacity, const uint8_t* sel, int sel_invert,
                                           float min_opacity, float& x, float& y, float& z) {
    x = xyz[3 * i];
    y = xyz[3 * i + 1];
    z = xyz[3 * i + 2];
    bool keep = opacity[i] > min_opacity;  // (a NaN opacity is not kept)
    if (sel) keep = keep && ((sel[i] != 0) != (sel_invert != 0));
    return keep && isfinite(x) && isfinite(y) && isfinite(z);
}

__global__ void __launch_bounds__(FIELD_THREADS) field_bounds_k(long long P, const float* __restrict__ xyz,
                                                                const float* __restrict__ opacity,
                                                                const uint8_t* __restrict__ sel, int sel_invert,
                                                                float min_opacity, uint32_t* __restrict__ enc) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false;
    for (long long i = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x; i < P; i += (long long)gridDim.x * FIELD_THREADS) {
        float c[3];
        if (!field_keep(i, xyz, opacity, sel, sel_invert, min_opacity, c[0], c[1], c[2])) continue;
        any = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            mn[a] = fminf(mn[a], c[a]);
            mx[a] = fmaxf(mx[a], c[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
        for (int o = 32; o >= 1; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
        }
    const bool wave_any = __ballot(any) != 0ull;
    if ((threadIdx.x & 63) == 0 && wave_any) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(enc + a, ord_enc(mn[a]));
            atomicMax(enc + 3 + a, ord_enc(mx[a]));
        }
    }
}

// frame = (center x y z, scale).  Nothing kept: (0, 0, 0, 1).  A kept set without extent (one point): scale 1.
__global__ void field_frame_k(const uint32_t* __restrict__ enc, const float* __restrict__ bounds, float* __restrict__ frame) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (bounds) {
        for (int a = 0; a < 4; a++) frame[a] = bounds[a];
        return;
    }
    if (enc[0] == ENC_NONE) {
        frame[0] = frame[1] = frame[2] = 0.f;
        frame[3] = 1.f;
        return;
    }
    float ext = 0.f;
    for (int a = 0; a < 3; a++) {
        const float mn = ord_dec(enc[a]), mx = ord_dec(enc[3 + a]);
        frame[a] = (mn + mx) / 2.f;
        ext = fmaxf(ext, mx - mn);
    }
    frame[3] = ext > 0.f ? (float)(1.8 / (double)ext) : 1.f;  // 1.8 / (mx - mn).amax().item(): a double, rounded when it scales fp32
}

struct FieldLattice {
    int nb, reach, nc;  // blocks per axis, cells the candidate walk reaches beyond a block, cells per axis = nb + 2 reach
    uint32_t ncells;    // nc^3 = the key of a Gaussian that is not kept
};

__global__ void __launch_bounds__(FIELD_THREADS) field_prep_k(long long P, const float* __restrict__ xyz,
                                                              const float* __restrict__ opacity,
                                                              const float* __restrict__ scaling,
                                                              const float* __restrict__ rotation,
                                                              const uint8_t* __restrict__ sel, int sel_invert, float min_opacity,
                                                              const float* __restrict__ frame, FieldLattice lat,
                                                              float4* __restrict__ q0, float4* __restrict__ q1,
                                                              float4* __restrict__ q2, uint32_t* __restrict__ keys,
                                                              uint32_t* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (i >= P) return;
    float x, y, z;
    bool keep = field_keep(i, xyz, opacity, sel, sel_invert, min_opacity, x, y, z);
    const float scale = frame[3];
    const float cx = (x - frame[0]) * scale, cy = (y - frame[1]) * scale, cz = (z - frame[2]) * scale;
    keep = keep && isfinite(cx) && isfinite(cy) && isfinite(cz);
    // build_scaling_rotation of the normalised scales, strip_symmetric(L L^T) and gaussian_3d_coeff's symmetric inverse, formula
    // for formula, but in fp64 from the fp32 inputs and rounded once: with 10 : 1 anisotropy the fp32 covariance loses
    // cond(Sigma) ~ 100 ulps in its inverse, which was the whole error of the grid; once per Gaussian it costs nothing
    const double sd = (double)scale;
    const double s0 = (double)scaling[3 * i] * sd, s1 = (double)scaling[3 * i + 1] * sd, s2 = (double)scaling[3 * i + 2] * sd;
    const double r0 = rotation[4 * i], r1 = rotation[4 * i + 1], r2 = rotation[4 * i + 2], r3 = rotation[4 * i + 3];
    const double norm = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const double qr = r0 / norm, qx = r1 / norm, qy = r2 / norm, qz = r3 / norm;
    const double R00 = 1.0 - 2.0 * (qy * qy + qz * qz), R01 = 2.0 * (qx * qy - qr * qz), R02 = 2.0 * (qx * qz + qr * qy);
    const double R10 = 2.0 * (qx * qy + qr * qz), R11 = 1.0 - 2.0 * (qx * qx + qz * qz), R12 = 2.0 * (qy * qz - qr * qx);
    const double R20 = 2.0 * (qx * qz - qr * qy), R21 = 2.0 * (qy * qz + qr * qx), R22 = 1.0 - 2.0 * (qx * qx + qy * qy);
    const double L00 = R00 * s0, L01 = R01 * s1, L02 = R02 * s2;
    const double L10 = R10 * s0, L11 = R11 * s1, L12 = R12 * s2;
    const double L20 = R20 * s0, L21 = R21 * s1, L22 = R22 * s2;
    const double a = L00 * L00 + L01 * L01 + L02 * L02, b = L00 * L10 + L01 * L11 + L02 * L12, c = L00 * L20 + L01 * L21 + L02 * L22;
    const double d = L10 * L10 + L11 * L11 + L12 * L12, e = L10 * L20 + L11 * L21 + L12 * L22, f = L20 * L20 + L21 * L21 + L22 * L22;
    const double inv_det = 1.0 / (a * d * f + 2.0 * e * c * b - e * e * a - c * c * d - b * b * f + 1e-24);
    const float inv_a = (float)((d * f - e * e) * inv_det), inv_b = (float)((e * c - b * f) * inv_det);
    const float inv_c = (float)((e * b - c * d) * inv_det), inv_d = (float)((a * f - c * c) * inv_det);
    const float inv_e = (float)((b * c - e * a) * inv_det), inv_f = (float)((a * d - b * b) * inv_det);
    q0[i] = make_float4(cx, cy, cz, opacity[i]);
    q1[i] = make_float4(inv_a, inv_b, inv_c, inv_d);
    q2[i] = make_float4(inv_e, inv_f, 0.f, 0.f);
    uint32_t key = lat.ncells;
    if (keep) {
        const float half_nb = 0.5f * (float)lat.nb, top = (float)(lat.nc - 1);
        // clamped as a float BEFORE it becomes an index: a centre far outside lands in a border cell and fails the box test there
        const int kx = (int)fminf(fmaxf(floorf((cx + 1.f) * half_nb) + (float)lat.reach, 0.f), top);
        const int ky = (int)fminf(fmaxf(floorf((cy + 1.f) * half_nb) + (float)lat.reach, 0.f), top);
        const int kz = (int)fminf(fmaxf(floorf((cz + 1.f) * half_nb) + (float)lat.reach, 0.f), top);
        key = (uint32_t)((kx * lat.nc + ky) * lat.nc + kz);
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(FIELD_THREADS) field_gather_k(long long P, const uint32_t* __restrict__ order,
                                                                const float4* __restrict__ q0, float4* __restrict__ q0s) {
    const long long j = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (j >= P) return;
    const uint32_t id = min(order[j], (uint32_t)(P - 1));
    q0s[j] = q0[id];
}

// cell_start[c] = number of sorted keys below c, c = 0 .. ncells (the last one: how many Gaussians are kept)
__global__ void __launch_bounds__(FIELD_THREADS) field_cells_k(long long P, const uint32_t* __restrict__ sorted_keys,
                                                               uint32_t ncells, uint32_t* __restrict__ cell_start) {
    const uint32_t c = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (c > ncells) return;
    long long lo = 0, hi = P;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted_keys[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    cell_start[c] = (uint32_t)lo;
}

struct DensityArgs {
    int R, split;
    FieldLattice lat;
    uint32_t P;
    const float* coords;    // [R] torch.linspace(-1, 1, R)
    const float* block_lo;  // [nb] coords[b split] - w relax
    const float* block_hi;  // [nb] coords[(b + 1) split - 1] + w relax
    const uint32_t* cell_start;
    const float4* q0s;      // sorted (centre, opacity)
    const uint32_t* order;  // sorted position -> Gaussian
    const float4 *q1, *q2;  // by Gaussian: (inv_a, inv_b, inv_c, inv_d), (inv_e, inv_f, -, -)
    const float* attr;      // [P][3] or NULL
    float* occ;             // [R][R][R]
    float* attr_out;        // [3][R][R][R]
};

template <int PPT, int ATTR>
__global__ void __launch_bounds__(FIELD_THREADS) field_density_k(DensityArgs A) {
    __shared__ float4 s0[FIELD_CAP], s1[FIELD_CAP], s2[FIELD_CAP];
    __shared__ float4 s3[ATTR ? FIELD_CAP : 1];
    __shared__ uint32_t wave_hits[FIELD_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = A.lat.nb, nc = A.lat.nc, span = 2 * A.lat.reach + 1, split = A.split;
    const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);
    const float lox = A.block_lo[bx], hix = A.block_hi[bx], loy = A.block_lo[by], hiy = A.block_hi[by];
    const float loz = A.block_lo[bz], hiz = A.block_hi[bz];
    const int npts = split * split * split;
    float px[PPT], py[PPT], pz[PPT], acc[PPT], ca[ATTR ? PPT : 1][3];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int p = min(tid + k * FIELD_THREADS, npts - 1);
        px[k] = A.coords[bx * split + p / (split * split)];
        py[k] = A.coords[by * split + (p / split) % split];
        pz[k] = A.coords[bz * split + p % split];
        acc[k] = 0.f;
        if constexpr (ATTR != 0) ca[k][0] = ca[k][1] = ca[k][2] = 0.f;
    }
    auto flush = [&](int n) {  // (n is the same in every thread; the list is complete: the caller has synchronised)
        for (int m = 0; m < n; m++) {
            const float4 g = s0[m], u = s1[m], v = s2[m];
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (ATTR != 0) t = s3[m];
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const float dx = px[k] - g.x, dy = py[k] - g.y, dz = pz[k] - g.z;
                const float quad = __builtin_fmaf(dz * dz, v.y, __builtin_fmaf(dy * dy, u.w, dx * dx * u.x));
                float power = -0.5f * quad;
                power = __builtin_fmaf(-(dx * dy), u.y, power);
                power = __builtin_fmaf(-(dx * dz), u.z, power);
                power = __builtin_fmaf(-(dy * dz), v.x, power);
                const float w = power > 0.f ? 0.f : expf(power);
                const float ow = g.w * w;
                acc[k] += ow;
                if constexpr (ATTR != 0) {
                    ca[k][0] = __builtin_fmaf(ow, t.x, ca[k][0]);
                    ca[k][1] = __builtin_fmaf(ow, t.y, ca[k][1]);
                    ca[k][2] = __builtin_fmaf(ow, t.z, ca[k][2]);
                }
            }
        }
    };
    int count = 0;  // survivors in the LDS list: the same value in every thread
    for (int rx = 0; rx < span; rx++) {
        for (int ry = 0; ry < span; ry++) {
            const uint32_t k0 = (uint32_t)(((bx + rx) * nc + (by + ry)) * nc + bz);  // < ncells: bx + rx <= nb - 1 + 2 reach = nc - 1
            const uint32_t k1 = k0 + (uint32_t)span;                                 // <= ncells
            uint32_t beg = min(A.cell_start[min(k0, A.lat.ncells)], A.P), end = min(A.cell_start[min(k1, A.lat.ncells)], A.P);
            if (end < beg) end = beg;
            for (uint32_t base = beg; base < end; base += FIELD_THREADS) {
                const uint32_t j = base + tid;
                bool hit = false;
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < end) {
                    g = A.q0s[j];
                    hit = g.x > lox && g.x < hix && g.y > loy && g.y < hiy && g.z > loz && g.z < hiz;
                }
                const unsigned long long ballot = __ballot(hit);
                if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(ballot);
                __syncthreads();
                int off = count, total = 0;
#pragma unroll
                for (int w = 0; w < FIELD_THREADS / 64; w++) {
                    const int h = (int)wave_hits[w];
                    if (w < wave) off += h;
                    total += h;
                }
                if (hit) {
                    const int pos = off + __popcll(ballot & ((1ull << lane) - 1ull));  // < count + 256 <= FIELD_CAP - 1
                    const uint32_t id = min(A.order[j], A.P - 1u);
                    s0[pos] = g;
                    s1[pos] = A.q1[id];
                    s2[pos] = A.q2[id];
                    if constexpr (ATTR != 0) s3[pos] = make_float4(A.attr[3 * (size_t)id], A.attr[3 * (size_t)id + 1], A.attr[3 * (size_t)id + 2], 0.f);
                }
                count += total;
                __syncthreads();
                if (count >= FIELD_BATCH) {
                    flush(count);
                    count = 0;
                    __syncthreads();
                }
            }
        }
    }
    if (count > 0) flush(count);
    const size_t R = (size_t)A.R, vol = R * R * R;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int p = tid + k * FIELD_THREADS;
        if (p >= npts) continue;
        const size_t gx = (size_t)(bx * split + p / (split * split)), gy = (size_t)(by * split + (p / split) % split),
                     gz = (size_t)(bz * split + p % split);
        const size_t o = (gx * R + gy) * R + gz;
        A.occ[o] = acc[k];
        if constexpr (ATTR != 0) {
            A.attr_out[o] = ca[k][0];
            A.attr_out[vol + o] = ca[k][1];
            A.attr_out[2 * vol + o] = ca[k][2];
        }
    }
}

template <int ATTR>
void launch_density_ppt(int ppt, unsigned blocks, const DensityArgs& A, hipStream_t s) {
    const dim3 g(blocks), b(FIELD_THREADS);
    if (ppt <= 1) field_density_k<1, ATTR><<<g, b, 0, s>>>(A);
    else if (ppt <= 2) field_density_k<2, ATTR><<<g, b, 0, s>>>(A);
    else if (ppt <= 4) field_density_k<4, ATTR><<<g, b, 0, s>>>(A);
    else if (ppt <= 8) field_density_k<8, ATTR><<<g, b, 0, s>>>(A);
    else field_density_k<16, ATTR><<<g, b, 0, s>>>(A);
}

struct FieldView {
    uint32_t* ctl;  // [16]: 0..2 encoded minima, 3..5 encoded maxima
    SortBufs sb;    // [P] cell keys, Gaussian ids
    float4 *q0, *q1, *q2, *q0s;
    uint32_t* cell_start;  // [ncells + 1]
};

size_t field_layout(size_t P, size_t ncells, char* base, FieldView* v) {
    Carver c(base);
    FieldView t;
    t.ctl = c.take<uint32_t>(16);
    carve_sort(c, P, &t.sb);
    t.q0 = c.take<float4>(P);
    t.q1 = c.take<float4>(P);
    t.q2 = c.take<float4>(P);
    t.q0s = c.take<float4>(P);
    t.cell_start = c.take<uint32_t>(ncells + 1);
    if (v) *v = t;
    return c.bytes();
}

FieldLattice field_lattice(int num_blocks, double relax_ratio) {
    FieldLattice lat;
    lat.nb = num_blocks;
    lat.reach = (int)floor(relax_ratio) + 2;
    lat.nc = num_blocks + 2 * lat.reach;
    lat.ncells = (uint32_t)lat.nc * (uint32_t)lat.nc * (uint32_t)lat.nc;
    return lat;
}

// ---- iso-surface -------------------------------------------------------------------------------------------------------
// corner code = 4 dx + 2 dy + dz.  The seven owned edges by slot, and the slot of a difference of corner codes.
__device__ __constant__ const int ISO_SLOT_CODE[7] = {4, 2, 1, 6, 5, 3, 7};
__device__ __constant__ const int ISO_CODE_SLOT[8] = {-1, 2, 1, 5, 0, 4, 3, 6};
// the six Kuhn tetrahedra: corner codes of v0 .. v3, in the lexicographic order of the axis permutation; its parity
__device__ __constant__ const int ISO_TET[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
__device__ __constant__ const int ISO_TET_SIGN[6] = {1, -1, -1, 1, 1, -1};

struct IsoDims {
    int X, Y, Z;
    long long N;  // X Y Z
};

__device__ __forceinline__ int tet_triangles(int pc) { return (pc == 1 || pc == 3) ? 1 : (pc == 2 ? 2 : 0); }

// counts[i] = crossings on the edges point i owns, counts[N + i] = triangles of the cube whose origin is point i, emask[i] = the
// owned edges that cross (bit = slot)
__global__ void __launch_bounds__(FIELD_THREADS) iso_flag_k(const float* __restrict__ grid, IsoDims D, float thresh,
                                                            uint32_t* __restrict__ counts, uint8_t* __restrict__ emask) {
    const long long i = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (i >= D.N) return;
    const int z = (int)(i % D.Z), y = (int)((i / D.Z) % D.Y), x = (int)(i / ((long long)D.Z * D.Y));
    const bool hx = x + 1 < D.X, hy = y + 1 < D.Y, hz = z + 1 < D.Z;
    int inside = 0;  // bit = corner code
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int dx = c >> 2, dy = (c >> 1) & 1, dz = c & 1;
        if ((dx && !hx) || (dy && !hy) || (dz && !hz)) continue;
        const float v = grid[i + ((long long)dx * D.Y + dy) * D.Z + dz];
        if (v > thresh) inside |= 1 << c;
    }
    const int in0 = inside & 1;
    int mask = 0;
#pragma unroll
    for (int s = 0; s < 7; s++) {
        const int c = ISO_SLOT_CODE[s];
        const int dx = c >> 2, dy = (c >> 1) & 1, dz = c & 1;
        if ((dx && !hx) || (dy && !hy) || (dz && !hz)) continue;
        if (((inside >> c) & 1) != in0) mask |= 1 << s;
    }
    int tris = 0;
    if (hx && hy && hz) {
#pragma unroll
        for (int t = 0; t < 6; t++) {
            int pc = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) pc += (inside >> ISO_TET[t][k]) & 1;
            tris += tet_triangles(pc);
        }
    }
    counts[i] = (uint32_t)__popc(mask);
    counts[D.N + i] = (uint32_t)tris;
    emask[i] = (uint8_t)mask;
}

__global__ void iso_totals_k(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ total, long long N, int* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = (int)scan[N];             // vertices: the prefix in front of the triangle stream
    out[1] = (int)(*total - scan[N]);  // triangles
}

__device__ __forceinline__ float iso_coord(const float* table, int i) { return table ? table[i] : (float)i; }

__global__ void __launch_bounds__(FIELD_THREADS) iso_vertex_k(const float* __restrict__ grid, const float* __restrict__ attr,
                                                              IsoDims D, float thresh, const float* __restrict__ cx,
                                                              const float* __restrict__ cy, const float* __restrict__ cz,
                                                              const uint32_t* __restrict__ scan, const uint8_t* __restrict__ emask,
                                                              long long V, float* __restrict__ vertices, float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (i >= D.N) return;
    const int mask = emask[i];
    if (!mask) return;
    const int z = (int)(i % D.Z), y = (int)((i / D.Z) % D.Y), x = (int)(i / ((long long)D.Z * D.Y));
    const float va = grid[i];
    const float pax = iso_coord(cx, x), pay = iso_coord(cy, y), paz = iso_coord(cz, z);
    long long o = scan[i];
    for (int s = 0; s < 7; s++) {
        if (!((mask >> s) & 1)) continue;
        const int c = ISO_SLOT_CODE[s];
        const int dx = c >> 2, dy = (c >> 1) & 1, dz = c & 1;
        // (the flag pass set the bit only for a neighbour inside the grid; the clamp keeps a corrupt mask in bounds)
        const int nx = min(x + dx, D.X - 1), ny = min(y + dy, D.Y - 1), nz = min(z + dz, D.Z - 1);
        const long long nb = ((long long)nx * D.Y + ny) * D.Z + nz;
        const float vb = grid[nb];
        const float t = (thresh - va) / (vb - va);
        if (o < V) {
            vertices[3 * o] = pax + t * (iso_coord(cx, nx) - pax);
            vertices[3 * o + 1] = pay + t * (iso_coord(cy, ny) - pay);
            vertices[3 * o + 2] = paz + t * (iso_coord(cz, nz) - paz);
            if (colors) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const float aa = attr[ch * D.N + i], ab = attr[ch * D.N + nb];
                    colors[3 * o + ch] = (aa + t * (ab - aa)) / thresh;
                }
            }
        }
        o++;
    }
}

__global__ void __launch_bounds__(FIELD_THREADS) iso_face_k(const float* __restrict__ grid, IsoDims D, float thresh,
                                                            const uint32_t* __restrict__ scan, const uint8_t* __restrict__ emask,
                                                            long long V, long long F, int* __restrict__ faces) {
    const long long i = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (i >= D.N) return;
    const int z = (int)(i % D.Z), y = (int)((i / D.Z) % D.Y), x = (int)(i / ((long long)D.Z * D.Y));
    if (!(x + 1 < D.X && y + 1 < D.Y && z + 1 < D.Z)) return;
    long long o = (long long)scan[D.N + i] - (long long)scan[D.N];
    if (o < 0) return;
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; c++)
        if (grid[i + ((long long)(c >> 2) * D.Y + ((c >> 1) & 1)) * D.Z + (c & 1)] > thresh) inside |= 1 << c;
    if (inside == 0 || inside == 255) return;
    // the vertex on the edge between corners p and q of this cube (p the lower one: q - p is an owned direction)
    auto vertex = [&](int p, int q) -> int {
        const long long owner = i + ((long long)(p >> 2) * D.Y + ((p >> 1) & 1)) * D.Z + (p & 1);
        const int slot = ISO_CODE_SLOT[(q - p) & 7];
        const long long v = (long long)scan[owner] + __popc((int)emask[owner] & ((1 << slot) - 1));
        return (int)min(v, V > 0 ? V - 1 : 0);
    };
    auto emit = [&](int a, int b, int c, bool flip) {
        if (o < F) {
            faces[3 * o] = a;
            faces[3 * o + 1] = flip ? c : b;
            faces[3 * o + 2] = flip ? b : c;
        }
        o++;
    };
    for (int t = 0; t < 6; t++) {
        int m = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) m |= ((inside >> ISO_TET[t][k]) & 1) << k;
        const int pc = __popc(m);
        if (pc == 0 || pc == 4) continue;
        const int sgn = ISO_TET_SIGN[t];
        const int* T = ISO_TET[t];
        if (pc == 2) {
            int in[2], out[2], ni = 0, no = 0;
            for (int k = 0; k < 4; k++) {
                if ((m >> k) & 1) in[ni++] = k;
                else out[no++] = k;
            }
            const int a = in[0], b = in[1], c = out[0], d = out[1];
            const int inversions = (a > c) + (a > d) + (b > c) + (b > d);
            const bool flip = (sgn * ((inversions & 1) ? -1 : 1)) < 0;
            auto edge = [&](int p, int q) { return p < q ? vertex(T[p], T[q]) : vertex(T[q], T[p]); };
            const int ac = edge(a, c), ad = edge(a, d), bd = edge(b, d), bc = edge(b, c);
            emit(ac, ad, bd, flip);
            emit(ac, bd, bc, flip);
        } else {
            const int lone_bits = pc == 1 ? m : (~m & 15);
            const int lone = __ffs(lone_bits) - 1;
            int rest[3], n = 0;
            for (int k = 0; k < 4; k++)
                if (k != lone) rest[n++] = k;
            auto edge = [&](int p, int q) { return p < q ? vertex(T[p], T[q]) : vertex(T[q], T[p]); };
            const int orient = sgn * ((lone & 1) ? -1 : 1);
            const bool flip = (orient < 0) != (pc == 3);
            emit(edge(lone, rest[0]), edge(lone, rest[1]), edge(lone, rest[2]), flip);
        }
    }
}

struct IsoView {
    uint32_t* counts;  // [2 N] crossings per point, triangles per cube origin; scanned in place
    uint32_t* total;
    uint8_t* emask;  // [N]
    uint32_t* scan_scratch;
};

size_t iso_layout(size_t N, char* base, IsoView* v) {
    Carver c(base);
    IsoView t;
    t.counts = c.take<uint32_t>(2 * N);
    t.total = c.take<uint32_t>(16);
    t.emask = c.take<uint8_t>(N);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words(2 * N));
    if (v) *v = t;
    return c.bytes();
}

unsigned blocks_for(long long n) { return (unsigned)((n + FIELD_THREADS - 1) / FIELD_THREADS); }

size_t field_density_workspace_bytes(long long P, int num_blocks, double relax_ratio) {
    return field_layout((size_t)P, field_lattice(num_blocks, relax_ratio).ncells, nullptr, nullptr);
}

void launch_field_density(long long P, const float* xyz, const float* opacity, const float* scaling, const float* rotation,
                          const uint8_t* selection, int selection_invert, float min_opacity, const float* attributes,
                          const float* bounds, int R, int num_blocks, double relax_ratio, const float* coords,
                          const float* block_lo, const float* block_hi, float* occ, float* attr_out, float* frame, int* status,
                          void* workspace, hipStream_t s) {
    const FieldLattice lat = field_lattice(num_blocks, relax_ratio);
    FieldView v;
    field_layout((size_t)P, lat.ncells, static_cast<char*>(workspace), &v);
    (void)hipMemsetAsync(v.ctl, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(v.ctl + 3, 0x00, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(status, 0, sizeof(int), s);
    const unsigned g = blocks_for(P);
    if (!bounds)
        field_bounds_k<<<dim3(g < 1024 ? g : 1024), dim3(FIELD_THREADS), 0, s>>>(P, xyz, opacity, selection, selection_invert, min_opacity, v.ctl);
    field_frame_k<<<dim3(1), dim3(64), 0, s>>>(v.ctl, bounds, frame);
    field_prep_k<<<dim3(g), dim3(FIELD_THREADS), 0, s>>>(P, xyz, opacity, scaling, rotation, selection, selection_invert, min_opacity,
                                                         frame, lat, v.q0, v.q1, v.q2, v.sb.keys[0], v.sb.vals[0]);
    const int bits = 32 - __builtin_clz(lat.ncells);  // covers the key ncells of a Gaussian that is not kept
    const int fin = radix_sort_pairs(v.sb.keys, v.sb.vals, (size_t)P, 0, bits, v.sb.scratch, s, false, false, nullptr,
                                     reinterpret_cast<uint32_t*>(status));
    field_gather_k<<<dim3(g), dim3(FIELD_THREADS), 0, s>>>(P, v.sb.vals[fin], v.q0, v.q0s);
    field_cells_k<<<dim3(blocks_for((long long)lat.ncells + 1)), dim3(FIELD_THREADS), 0, s>>>(P, v.sb.keys[fin], lat.ncells, v.cell_start);
    DensityArgs A;
    A.R = R;
    A.split = R / num_blocks;
    A.lat = lat;
    A.P = (uint32_t)P;
    A.coords = coords;
    A.block_lo = block_lo;
    A.block_hi = block_hi;
    A.cell_start = v.cell_start;
    A.q0s = v.q0s;
    A.order = v.sb.vals[fin];
    A.q1 = v.q1;
    A.q2 = v.q2;
    A.attr = attributes;
    A.occ = occ;
    A.attr_out = attr_out;
    const int npts = A.split * A.split * A.split;
    const int ppt = (npts + FIELD_THREADS - 1) / FIELD_THREADS;
    const unsigned blocks = (unsigned)(num_blocks * num_blocks * num_blocks);
    if (attributes) launch_density_ppt<3>(ppt, blocks, A, s);
    else launch_density_ppt<0>(ppt, blocks, A, s);
}

size_t field_iso_workspace_bytes(long long N) { return iso_layout((size_t)N, nullptr, nullptr); }

void launch_field_iso_count(const float* grid, int X, int Y, int Z, float thresh, void* workspace, int* counts, hipStream_t s) {
    const IsoDims D{X, Y, Z, (long long)X * Y * Z};
    IsoView v;
    iso_layout((size_t)D.N, static_cast<char*>(workspace), &v);
    iso_flag_k<<<dim3(blocks_for(D.N)), dim3(FIELD_THREADS), 0, s>>>(grid, D, thresh, v.counts, v.emask);
    exclusive_scan_u32(v.counts, nullptr, v.counts, (size_t)(2 * D.N), v.total, v.scan_scratch, s);
    iso_totals_k<<<dim3(1), dim3(64), 0, s>>>(v.counts, v.total, D.N, counts);
}

void launch_field_iso_emit(const float* grid, const float* attr, int X, int Y, int Z, float thresh, const float* cx,
                           const float* cy, const float* cz, const void* workspace, long long V, long long F, float* vertices,
                           int* faces, float* colors, hipStream_t s) {
    const IsoDims D{X, Y, Z, (long long)X * Y * Z};
    IsoView v;
    iso_layout((size_t)D.N, static_cast<char*>(const_cast<void*>(workspace)), &v);
    if (V > 0)
        iso_vertex_k<<<dim3(blocks_for(D.N)), dim3(FIELD_THREADS), 0, s>>>(grid, attr, D, thresh, cx, cy, cz, v.counts, v.emask, V,
                                                                           vertices, attr ? colors : nullptr);
    if (F > 0) iso_face_k<<<dim3(blocks_for(D.N)), dim3(FIELD_THREADS), 0, s>>>(grid, D, thresh, v.counts, v.emask, V, F, faces);
}

int field_dims(int R, int num_blocks, double relax_ratio) {
    if (num_blocks < 1 || R < 1 || R > GOI_FIELD_MAX_RESOLUTION || R % num_blocks != 0) return -1;
    const int split = R / num_blocks;
    if (split < GOI_FIELD_MIN_SPLIT || split > GOI_FIELD_MAX_SPLIT) return -1;
    if (!(relax_ratio >= 0.0 && relax_ratio <= GOI_FIELD_MAX_RELAX)) return -1;
    return 0;
}

int iso_dims(const char* fn, int X, int Y, int Z) {
    // at most 7 crossings per point and 12 triangles per cube: 19 * 2^26 < 2^32 keeps the one scan over both streams, and each
    // count (< 2^31) an int32
    if (X < 1 || Y < 1 || Z < 1 || (long long)X * Y * Z > GOI_FIELD_MAX_GRID_POINTS)
        return fail(std::string(fn) + ": need X, Y, Z >= 1 and X Y Z <= 2^26");
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_field_density_workspace_bytes(long long P, int resolution, int num_blocks, double relax_ratio) {
    if (P < 1 || P >= SORT_MAX_KEYS || field_dims(resolution, num_blocks, relax_ratio) < 0) return 0;
    return field_density_workspace_bytes(P, num_blocks, relax_ratio);
}

int goi_field_density(long long P, const float* xyz, const float* opacity, const float* scaling, const float* rotation,
                      const uint8_t* selection, int selection_invert, double min_opacity, const float* attributes,
                      const float* bounds, int resolution, int num_blocks, double relax_ratio, const float* coords,
                      const float* block_lo, const float* block_hi, float* occ, float* attr_out, float* frame, int* status,
                      void* workspace, void* stream) {
    const char* fn = "goi_field_density";
    if (P < 0 || P >= SORT_MAX_KEYS) return fail(std::string(fn) + ": need 0 <= P < 2^30");
    if (field_dims(resolution, num_blocks, relax_ratio) < 0)
        return fail(std::string(fn) + ": need resolution <= 256, resolution % num_blocks == 0, 4 <= resolution / num_blocks <= 16 "
                                      "and 0 <= relax_ratio <= 4");
    if (!(min_opacity == min_opacity)) return fail(std::string(fn) + ": NaN min_opacity");
    if (!occ || !frame || !status || !coords || !block_lo || !block_hi) return fail(std::string(fn) + ": a required pointer is NULL");
    if (attributes && !attr_out) return fail(std::string(fn) + ": attributes need attr_out");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t vol = (size_t)resolution * resolution * resolution;
    if (P == 0) {  // an empty model: zero grids, the caller's frame or (0, 0, 0, 1)
        GOI_HIP(hipMemsetAsync(occ, 0, sizeof(float) * vol, s));
        if (attr_out) GOI_HIP(hipMemsetAsync(attr_out, 0, sizeof(float) * 3 * vol, s));
        GOI_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
        if (bounds) {
            GOI_HIP(hipMemcpyAsync(frame, bounds, 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            GOI_HIP(hipMemsetAsync(frame, 0, 3 * sizeof(float), s));
            GOI_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(frame + 3), 0x3F800000, 1, s));  // 1.0f
        }
        return 0;
    }
    if (!xyz || !opacity || !scaling || !rotation) return fail(std::string(fn) + ": a required pointer is NULL");
    if (check_workspace(fn, workspace) < 0) return -1;
    launch_field_density(P, xyz, opacity, scaling, rotation, selection, selection_invert ? 1 : 0, (float)min_opacity, attributes,
                         bounds, resolution, num_blocks, relax_ratio, coords, block_lo, block_hi, occ, attr_out, frame, status,
                         workspace, s);
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_field_iso_workspace_bytes(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1 || (long long)X * Y * Z > GOI_FIELD_MAX_GRID_POINTS) return 0;
    return field_iso_workspace_bytes((long long)X * Y * Z);
}

int goi_field_iso_count(const float* grid, int X, int Y, int Z, double thresh, void* workspace, int* counts, void* stream) {
    const char* fn = "goi_field_iso_count";
    if (iso_dims(fn, X, Y, Z) < 0) return -1;
    if (!(thresh == thresh)) return fail(std::string(fn) + ": NaN thresh");
    if (!grid || !counts) return fail(std::string(fn) + ": NULL grid or counts");
    if (check_workspace(fn, workspace) < 0) return -1;
    launch_field_iso_count(grid, X, Y, Z, (float)thresh, workspace, counts, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_field_iso_emit(const float* grid, const float* attr, int X, int Y, int Z, double thresh, const float* cx, const float* cy,
                       const float* cz, const void* workspace, long long n_vertices, long long n_faces, float* vertices, int* faces,
                       float* colors, void* stream) {
    const char* fn = "goi_field_iso_emit";
    if (iso_dims(fn, X, Y, Z) < 0) return -1;
    if (!(thresh == thresh)) return fail(std::string(fn) + ": NaN thresh");
    if (n_vertices < 0 || n_faces < 0 || n_vertices >= (1ll << 31) || n_faces >= (1ll << 31))
        return fail(std::string(fn) + ": need 0 <= n_vertices, n_faces < 2^31");
    if (!grid) return fail(std::string(fn) + ": NULL grid");
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return fail(std::string(fn) + ": NULL vertices or faces");
    if (attr && n_vertices > 0 && !colors) return fail(std::string(fn) + ": attr needs colors");
    if (check_workspace(fn, workspace) < 0) return -1;
    launch_field_iso_emit(grid, attr, X, Y, Z, (float)thresh, cx, cy, cz, workspace, n_vertices, n_faces, vertices, faces, colors,
                          static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
