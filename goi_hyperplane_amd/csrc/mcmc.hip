// Fixed-budget densification (goi_hyperplane_amd/mcmc.py): the two per-row operations of "3D Gaussian
// Splatting as Markov Chain Monte Carlo" (Kheradmand et al., 2024), in place -- P never changes, nothing is allocated, re-keyed or
// read back.
//
// goi_mcmc_relocate moves the DEAD Gaussians onto ALIVE ones drawn with probability proportional to their opacity, and corrects
// the opacity and scale of a source and its copies so that the composite is preserved.  Definitions (opacity [P] is ACTIVATED):
//   dead_i   selected and (double)opacity_i <= min_opacity          alive_i   selected and (double)opacity_i > min_opacity
//            (a NaN opacity is neither; selection == NULL selects every row; a row with selection 0 is FROZEN: never dead, never a
//            source, never written)
//   d_0 < d_1 < ...   the dead rows in ascending id
//   w_i      = (uint32)(opacity_i * 2^24) for alive rows (exact: a power-of-two scale of an fp32 value, truncated; an opacity
//            above 1 counts as 1), 0 otherwise
//   C_i      = w_0 + ... + w_i in uint64, T = C_{P-1}
//   moves    = min(n_dead, n_draws, max_moves, floor(n_alive * frac_num / frac_den)) in integers; 0 when T == 0
//   t_j      = floor(u_j * T / 2^32) = the high half of the 64 x 64-bit product (u_j << 32) * T, u_j = draws[j], j < moves
//   s_j      = min{ i : C_i > t_j }  (a binary search of at most 32 steps; w_{s_j} > 0, so a source is alive)
//   r_i      = #{ j < moves : s_j = i }  (integer atomics)            N_i = min(r_i + 1, n_max)
// For every source (r_i >= 1), in float64 with one rounding to fp32 at the store:
//   o  = min((double)opacity_i, 1 - 2^-24)
//   o' = 1 - pow(1 - o, 1 / (double)N)            (N == 1: o' = o)
//   D  = sum_{m=1..N} sum_{k=0..m-1} (-1)^k (B[m-1][k] * Q[k]) * p_k,  ONE accumulator walked in exactly this order, p_k = o'^(k+1) the
//        running product p_k = p_{k-1} * o' restarted at 1 for every m, an odd k subtracted; B[n][k] = C(n, k), exact in float64
//        (C(50, 25) < 2^53), Q[k] = 1 / sqrt((double)(k + 1)) built on the host: a 51-row table
//   c  = o / D
//   new raw opacity   = log(x / (1 - x)),  x = min(max(o', min_opacity), 1 - 2^-24)
//   new raw log-scale = (double)old + log(c)   per axis
// Written: dead row d_j gets row s_j of every GOI_MCMC_PARAM group and the new opacity / log-scale of s_j; source i gets the same
// new opacity and log-scale; every GOI_MCMC_MOMENT row of a SOURCE is zeroed (as the paper's and gsplat's relocation do), the dead
// rows' moments stay as they were.  Nothing else is touched.  counts = {moves, n_dead, n_alive, sources hit}.
//
// Launches, all on the caller's stream, no workgroup waits for another, every loop bounded, no float atomics:
//   mcmc_flags_k   one pass over opacity and selection: r_i = 0, and per block of 1024 rows the sums (w, dead, alive)
//   mcmc_totals_k  one workgroup: the exclusive scan of the block sums (64-bit; the project's scan is 32-bit), T, n_dead, n_alive,
//                  moves, counts, status = 0
//   mcmc_scan_k    the pass again: C_i (block scan + block prefix) and the dead ids compacted in ascending order
//   mcmc_sample_k  draw j < moves: t_j, s_j, r_{s_j} += 1 (the lanes of a wave that drew the same source add once); the draw that
//                  finds r == 0 is the source's FIRST draw and speaks for it
//   mcmc_values_k  first draws only: o', D, c -> the new opacity and log-scale STAGED by source row.  Sources and dead rows are
//                  disjoint, but a source and every copy of it must see the source's OLD opacity and scale: so nothing is written
//                  to the model before ...
//   mcmc_apply_k   ... this launch, which reads the staged values and the sources' untouched parameter rows: a grid row per
//                  group, a lane per (draw, float); the source's own update and its moment zeroing are the first draw's.
// goi_mcmc_noise is one launch without a workspace: a lane per row, float64 throughout (see the comment at the kernel).
// This unit is compiled with -ffp-contract=off: D and the noise are restated operation for operation in tests/mcmc_reference.py.
// C entries, with the limits they enforce, at the end of the file (include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace goi {

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr int MC_ITEMS = 4;
constexpr int MC_BLOCK = MC_THREADS * MC_ITEMS;  // rows per workgroup of the two passes over P
constexpr int MC_NMAX = 51;
constexpr unsigned MC_GRID = 4096;               // cap of the grid-stride launches (sample, values, apply)
constexpr uint32_t MC_FIRST = 0x80000000u;       // src[j]: the draw that found r == 0 (P < 2^30 leaves the bit free)
constexpr double MC_ONE_LESS = 1.0 - 1.0 / 16777216.0;  // 1 - 2^-24

struct Trip {  // what the 64-bit scan carries: weights, dead rows, alive rows
    unsigned long long w;
    uint32_t d, a;
};
struct McmcHead {
    unsigned long long T;
    uint32_t n_dead, n_alive, moves, pad;
};
struct McmcView {
    unsigned long long* csum;  // [P] C_i
    uint32_t* dead;            // [P] d_0 < d_1 < ... (n_dead of them)
    uint32_t* hits;            // [P] r_i (unless the caller gave an array of its own)
    uint32_t* src;             // [P] s_j | MC_FIRST
    float* new_opacity;        // [P] staged by source row
    float* new_scale;          // [P,3]
    Trip* part;                // [ceil(P / MC_BLOCK)] block sums, scanned in place
    McmcHead* head;
};
struct McmcTables {
    double q[MC_NMAX];  // Q[k] = 1 / sqrt(k + 1)
};
struct BinomTable {
    double b[MC_NMAX][MC_NMAX];
};
constexpr BinomTable make_binom() {
    BinomTable t{};
    for (int n = 0; n < MC_NMAX; n++) {
        t.b[n][0] = 1.0;
        for (int k = 1; k <= n; k++) t.b[n][k] = t.b[n - 1][k - 1] + (k <= n - 1 ? t.b[n - 1][k] : 0.0);
    }
    return t;
}
__constant__ BinomTable MC_BINOM = make_binom();

__device__ __forceinline__ Trip operator+(const Trip& x, const Trip& y) { return Trip{x.w + y.w, x.d + y.d, x.a + y.a}; }
__device__ __forceinline__ Trip trip_shfl_up(const Trip& v, int o) {
    return Trip{__shfl_up(v.w, o), (uint32_t)__shfl_up((int)v.d, o), (uint32_t)__shfl_up((int)v.a, o)};
}

// (w_i, dead_i, alive_i) of one row
__device__ __forceinline__ Trip classify(float op, bool selected, double min_opacity) {
    Trip t{0ull, 0u, 0u};
    if (!selected) return t;
    if ((double)op <= min_opacity) {
        t.d = 1;
    } else if ((double)op > min_opacity) {
        t.a = 1;
        const float s = fminf(op, 1.0f) * 16777216.0f;
        t.w = s > 0.0f ? (unsigned long long)(uint32_t)s : 0ull;
    }
    return t;
}

// inclusive scan over the workgroup's 256 threads; *total = the workgroup's sum.  Two barriers; `lds` is MC_WAVES entries.
__device__ __forceinline__ Trip block_scan(Trip v, Trip* lds, Trip* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Trip u = trip_shfl_up(v, o);
        if (lane >= o) v = v + u;
    }
    __syncthreads();  // the previous use of lds is over
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    Trip before{0ull, 0u, 0u}, all{0ull, 0u, 0u};
#pragma unroll
    for (int k = 0; k < MC_WAVES; k++) {
        if (k < wave) before = before + lds[k];
        all = all + lds[k];
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_flags_k(long long P, const float* __restrict__ opacity,
                                                           const uint8_t* __restrict__ selection, double min_opacity,
                                                           uint32_t* __restrict__ hits, Trip* __restrict__ part) {
    __shared__ Trip lds[MC_WAVES];
    const long long base = (long long)blockIdx.x * MC_BLOCK + (long long)threadIdx.x * MC_ITEMS;
    Trip sum{0ull, 0u, 0u};
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long i = base + k;
        if (i < P) {
            sum = sum + classify(opacity[i], selection ? selection[i] != 0 : true, min_opacity);
            hits[i] = 0;
        }
    }
    Trip total;
    block_scan(sum, lds, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_totals_k(long long n_blocks, Trip* __restrict__ part, McmcHead* __restrict__ head,
                                                            long long n_draws, long long max_moves, unsigned long long frac_num,
                                                            unsigned long long frac_den, uint32_t* __restrict__ counts,
                                                            int32_t* __restrict__ status) {
    __shared__ Trip lds[MC_WAVES];
    Trip carry{0ull, 0u, 0u};
    for (long long c0 = 0; c0 < n_blocks; c0 += MC_THREADS) {  // at most 2^20 / 256 rounds
        const long long b = c0 + threadIdx.x;
        const Trip v = b < n_blocks ? part[b] : Trip{0ull, 0u, 0u};
        Trip total;
        const Trip incl = block_scan(v, lds, &total);
        if (b < n_blocks) part[b] = Trip{carry.w + incl.w - v.w, carry.d + incl.d - v.d, carry.a + incl.a - v.a};
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        unsigned long long moves = carry.d;
        moves = min(moves, (unsigned long long)n_draws);
        moves = min(moves, (unsigned long long)max_moves);
        moves = min(moves, (unsigned long long)carry.a * frac_num / frac_den);  // < 2^30 * 2^32
        if (carry.w == 0) moves = 0;
        head->T = carry.w;
        head->n_dead = carry.d;
        head->n_alive = carry.a;
        head->moves = (uint32_t)moves;
        head->pad = 0;
        counts[0] = (uint32_t)moves;
        counts[1] = carry.d;
        counts[2] = carry.a;
        counts[3] = 0;
        *status = 0;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_scan_k(long long P, const float* __restrict__ opacity,
                                                          const uint8_t* __restrict__ selection, double min_opacity,
                                                          const Trip* __restrict__ part, unsigned long long* __restrict__ csum,
                                                          uint32_t* __restrict__ dead) {
    __shared__ Trip lds[MC_WAVES];
    const long long base = (long long)blockIdx.x * MC_BLOCK + (long long)threadIdx.x * MC_ITEMS;
    Trip item[MC_ITEMS];
    Trip sum{0ull, 0u, 0u};
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long i = base + k;
        item[k] = i < P ? classify(opacity[i], selection ? selection[i] != 0 : true, min_opacity) : Trip{0ull, 0u, 0u};
        sum = sum + item[k];
    }
    Trip total;
    const Trip incl = block_scan(sum, lds, &total);
    const Trip off = part[blockIdx.x];
    Trip run{off.w + incl.w - sum.w, off.d + incl.d - sum.d, 0u};  // everything in front of this thread's first row
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long i = base + k;
        if (i < P) {
            if (item[k].d) dead[run.d] = (uint32_t)i;  // run.d < n_dead <= P
            run.w += item[k].w;
            run.d += item[k].d;
            csum[i] = run.w;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_sample_k(long long P, const long long* __restrict__ draws,
                                                            const McmcHead* __restrict__ head,
                                                            const unsigned long long* __restrict__ csum, uint32_t* __restrict__ hits,
                                                            uint32_t* __restrict__ src, uint32_t* __restrict__ counts,
                                                            int32_t* __restrict__ status) {
    const uint32_t moves = head->moves;
    const unsigned long long T = head->T;
    const uint32_t stride = gridDim.x * MC_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * MC_THREADS; base < moves; base += stride) {  // uniform per workgroup; moves <= n_draws, <= P
        const uint32_t j = base + threadIdx.x;
        const bool active = j < moves;
        uint32_t s = 0;
        if (active) {
            const long long raw = draws[j];
            if (raw < 0 || raw >= (1ll << 32)) atomicOr(status, GOI_MCMC_STATUS_DRAW);
            const unsigned long long u = (unsigned long long)raw & 0xFFFFFFFFull;
            const unsigned long long t = __umul64hi(u << 32, T);  // floor(u T / 2^32) < T
            long long lo = 0, hi = P - 1;
            for (int it = 0; it < 32 && lo < hi; it++) {
                const long long mid = (lo + hi) >> 1;
                if (csum[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            if (lo != hi || !(csum[lo] > t)) atomicOr(status, GOI_MCMC_STATUS_SEARCH);  // cannot happen: t < T = C_{P-1}
            s = (uint32_t)lo;
        }
        // The lanes of a wave that drew the same source count once: the lowest of them adds their number (registers only, at most
        // 64 rounds), so every draw on one source costs one atomic per wave, not 64 on one word.
        bool todo = active, lead = false;
        uint32_t cnt = 0;
        for (int round = 0; round < 64; round++) {
            const unsigned long long open = __ballot(todo);
            if (!open) break;
            const int leader = __builtin_ctzll(open);
            const uint32_t key = (uint32_t)__shfl((int)s, leader);
            const bool mine = todo && s == key;
            const unsigned long long grp = __ballot(mine);
            if (lane == leader) {
                lead = true;
                cnt = (uint32_t)__popcll(grp);
            }
            todo = todo && !mine;
        }
        uint32_t before = 1;
        if (lead) {
            before = atomicAdd(hits + s, cnt);
            if (before == 0) atomicAdd(counts + 3, 1u);
        }
        if (active) src[j] = s | (before == 0 ? MC_FIRST : 0u);
    }
}

// D of one source: see the header of this file.  The same function serves the product and the test entry.
__device__ double relocation_sum(double op, int N, const McmcTables& tab) {
    double D = 0.0;
    for (int m = 1; m <= N; m++) {
        double p = 1.0;
        for (int k = 0; k < m; k++) {
            p = p * op;
            const double term = (MC_BINOM.b[m - 1][k] * tab.q[k]) * p;
            D = (k & 1) ? D - term : D + term;
        }
    }
    return D;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_values_k(const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                            const McmcHead* __restrict__ head, const uint32_t* __restrict__ hits,
                                                            const uint32_t* __restrict__ src, double min_opacity, int n_max,
                                                            const McmcTables tab, float* __restrict__ new_opacity,
                                                            float* __restrict__ new_scale) {
    const uint32_t moves = head->moves;
    const uint32_t stride = gridDim.x * MC_THREADS;
    for (uint32_t j = blockIdx.x * MC_THREADS + threadIdx.x; j < moves; j += stride) {
        const uint32_t e = src[j];
        if (!(e & MC_FIRST)) continue;
        const uint32_t s = e & ~MC_FIRST;
        const uint32_t r = hits[s];
        const int N = (int)min(r + 1u, (uint32_t)n_max);
        const double o = fmin((double)opacity[s], MC_ONE_LESS);
        const double on = N == 1 ? o : 1.0 - pow(1.0 - o, 1.0 / (double)N);
        const double D = relocation_sum(on, N, tab);
        const double c = o / D;
        const double x = fmin(fmax(on, min_opacity), MC_ONE_LESS);
        new_opacity[s] = (float)log(x / (1.0 - x));
        if (scaling) {
            const double lc = log(c);
#pragma unroll
            for (int a = 0; a < 3; a++) new_scale[3ll * s + a] = (float)((double)scaling[3ll * s + a] + lc);
        }
    }
}

struct ApplyTable {
    GoiMcmcRows g[GOI_MCMC_MAX_GROUPS];
};

// grid row = group; a lane per (draw, float of the group's row), grid-stride over moves * row_len
__global__ __launch_bounds__(MC_THREADS) void mcmc_apply_k(const ApplyTable t, const McmcHead* __restrict__ head,
                                                           const uint32_t* __restrict__ src, const uint32_t* __restrict__ dead,
                                                           const float* __restrict__ new_opacity, const float* __restrict__ new_scale) {
    const GoiMcmcRows grp = t.g[blockIdx.y];
    const unsigned long long rl = (unsigned long long)grp.row_len;
    const unsigned long long n = (unsigned long long)head->moves * rl;  // < 2^30 * 2^20
    const unsigned long long stride = (unsigned long long)gridDim.x * MC_THREADS;
    float* __restrict__ data = grp.data;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * MC_THREADS; e0 < n; e0 += stride) {
        // the workgroup's first draw once in 64 bits; each lane's draw from a 32-bit quotient of its offset behind it
        const unsigned long long j0 = e0 / rl;
        const uint32_t off = (uint32_t)(e0 - j0 * rl) + threadIdx.x;  // < 2^20 + 256
        const uint32_t dj = off / (uint32_t)rl;
        const unsigned long long e = e0 + threadIdx.x;
        if (e >= n) continue;
        const uint32_t j = (uint32_t)j0 + dj;
        const unsigned long long c = off - dj * (uint32_t)rl;
        const uint32_t sj = src[j];
        const unsigned long long s = sj & ~MC_FIRST, d = dead[j];
        const bool first = (sj & MC_FIRST) != 0;
        if (grp.mode == GOI_MCMC_PARAM) {
            data[d * rl + c] = data[s * rl + c];  // a source's plain rows are never written
        } else if (grp.mode == GOI_MCMC_MOMENT) {
            if (first) data[s * rl + c] = 0.0f;
        } else {
            const float v = grp.mode == GOI_MCMC_OPACITY ? new_opacity[s] : new_scale[s * 3 + c];
            data[d * rl + c] = v;
            if (first) data[s * rl + c] = v;
        }
    }
}

// The position noise, in place, a lane per selected row, float64 throughout and one rounding at the store:
//   n = sqrt(q0 q0 + q1 q1 + q2 q2 + q3 q3) (left to right), (r, x, y, z) = q / n, R as utils/general_utils.build_rotation writes it
//   s_b = exp(raw log-scale_b),  M_ab = R_ab * s_b,  Sigma_ac = M_a0 M_c0 + M_a1 M_c1 + M_a2 M_c2 (left to right)
//   g = 1 / (1 + exp(-k * ((1 - opacity) - x0))),  v_b = (z_b * g) * step
//   xyz_a = (float)((double)xyz_a + (Sigma_a0 v_0 + Sigma_a1 v_1 + Sigma_a2 v_2))
__global__ __launch_bounds__(MC_THREADS) void mcmc_noise_k(long long P, float* __restrict__ xyz, const float* __restrict__ rotation,
                                                           const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                           const float* __restrict__ zn, const uint8_t* __restrict__ selection,
                                                           double kk, double x0, double step) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= P || (selection && !selection[i])) return;
    const double q0 = rotation[4 * i], q1 = rotation[4 * i + 1], q2 = rotation[4 * i + 2], q3 = rotation[4 * i + 3];
    const double n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z);
    R[0][1] = 2.0 * (x * y - r * z);
    R[0][2] = 2.0 * (x * z + r * y);
    R[1][0] = 2.0 * (x * y + r * z);
    R[1][1] = 1.0 - 2.0 * (x * x + z * z);
    R[1][2] = 2.0 * (y * z - r * x);
    R[2][0] = 2.0 * (x * z - r * y);
    R[2][1] = 2.0 * (y * z + r * x);
    R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    double M[3][3], v[3];
    const double g = 1.0 / (1.0 + exp(-kk * ((1.0 - (double)opacity[i]) - x0)));
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const double s = exp((double)scaling[3 * i + b]);
#pragma unroll
        for (int a = 0; a < 3; a++) M[a][b] = R[a][b] * s;
        v[b] = ((double)zn[3 * i + b] * g) * step;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double delta = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double sig = M[a][0] * M[c][0] + M[a][1] * M[c][1] + M[a][2] * M[c][2];
            delta = c == 0 ? sig * v[0] : delta + sig * v[c];
        }
        xyz[3 * i + a] = (float)((double)xyz[3 * i + a] + delta);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_debug_sum_k(int n, const double* __restrict__ o_new, const int32_t* __restrict__ N,
                                                               const McmcTables tab, double* __restrict__ D) {
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i < n) D[i] = relocation_sum(o_new[i], min(max(N[i], 1), MC_NMAX), tab);
}

inline size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }

// C | dead ids | r | sources of the draws | staged opacity | staged log-scales | block sums | totals
size_t mcmc_layout(long long P, char* base, McmcView* v) {
    Carver c(base);
    McmcView m;
    m.csum = c.take<unsigned long long>((size_t)P);
    m.dead = c.take<uint32_t>((size_t)P);
    m.hits = c.take<uint32_t>((size_t)P);
    m.src = c.take<uint32_t>((size_t)P);
    m.new_opacity = c.take<float>((size_t)P);
    m.new_scale = c.take<float>(3 * (size_t)P);
    m.part = c.take<Trip>(div_up((size_t)P, MC_BLOCK));
    m.head = c.take<McmcHead>(1);
    if (v) *v = m;
    return c.bytes();
}

McmcTables make_tables() {
    McmcTables t;
    for (int k = 0; k < MC_NMAX; k++) t.q[k] = 1.0 / std::sqrt((double)(k + 1));
    return t;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_mcmc_relocate_workspace_bytes(long long P) { return (P >= 0 && P < (1ll << 30)) ? mcmc_layout(P, nullptr, nullptr) + 256 : 0; }

int goi_mcmc_relocate(long long P, const float* opacity, const int64_t* draws, long long n_draws, const unsigned char* selection,
                      double min_opacity, long long max_moves, long long frac_num, long long frac_den, int n_max,
                      const GoiMcmcRows* groups, int n_groups, unsigned* hits, unsigned* counts, int32_t* status, void* workspace,
                      void* stream) {
    const std::string fn = "goi_mcmc_relocate: ";
    if (P < 0 || P >= (1ll << 30)) return fail(fn + "need 0 <= P < 2^30");
    if (n_draws < 0 || n_draws >= (1ll << 30)) return fail(fn + "need 0 <= n_draws < 2^30");
    if (max_moves < 0) return fail(fn + "need max_moves >= 0");
    if (frac_num < 0 || frac_num > (1ll << 32) || frac_den < 1 || frac_den > (1ll << 32))
        return fail(fn + "need 0 <= frac_num <= 2^32 and 1 <= frac_den <= 2^32");
    if (n_max < 1 || n_max > MC_NMAX) return fail(fn + "need 1 <= n_max <= 51");
    if (!(min_opacity >= 0.0 && min_opacity < 1.0)) return fail(fn + "need 0 <= min_opacity < 1");
    if (n_groups < 0 || n_groups > GOI_MCMC_MAX_GROUPS) return fail(fn + "n_groups must be 0..24");
    if (n_groups && !groups) return fail(fn + "groups is NULL");
    const float* scaling = nullptr;
    int n_opacity = 0, n_scaling = 0, max_rl = 1;
    for (int k = 0; k < n_groups; k++) {
        const GoiMcmcRows& g = groups[k];
        if (g.row_len < 1 || g.row_len > (1 << 20) || g.mode < GOI_MCMC_PARAM || g.mode > GOI_MCMC_MOMENT) return fail(fn + "bad group");
        if (P > 0 && !g.data) return fail(fn + "a group pointer is NULL");
        if (reinterpret_cast<uintptr_t>(g.data) & 3) return fail(fn + "a group pointer is not 4-byte aligned");
        if (g.mode == GOI_MCMC_OPACITY && (g.row_len != 1 || ++n_opacity > 1)) return fail(fn + "need at most one opacity group, of row length 1");
        if (g.mode == GOI_MCMC_SCALING && (g.row_len != 3 || ++n_scaling > 1)) return fail(fn + "need at most one log-scale group, of row length 3");
        if (g.mode == GOI_MCMC_SCALING) scaling = g.data;
        max_rl = g.row_len > max_rl ? g.row_len : max_rl;
    }
    if (P == 0) return 0;
    if (!opacity || !counts || !status || (n_draws > 0 && !draws)) return fail(fn + "a required pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(opacity) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(status) |
         reinterpret_cast<uintptr_t>(hits)) & 3)
        return fail(fn + "opacity, hits, counts and status must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(draws) & 7) return fail(fn + "draws must be 8-byte aligned");
    if (check_workspace("goi_mcmc_relocate", workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    McmcView v;
    mcmc_layout(P, static_cast<char*>(workspace), &v);
    if (hits) v.hits = hits;
    const unsigned blocks = (unsigned)div_up((size_t)P, MC_BLOCK);
    mcmc_flags_k<<<dim3(blocks), dim3(MC_THREADS), 0, s>>>(P, opacity, selection, min_opacity, v.hits, v.part);
    mcmc_totals_k<<<dim3(1), dim3(MC_THREADS), 0, s>>>((long long)blocks, v.part, v.head, n_draws, max_moves,
                                                       (unsigned long long)frac_num, (unsigned long long)frac_den, counts, status);
    long long bound = n_draws < max_moves ? n_draws : max_moves;  // the host's bound on moves
    bound = bound < P ? bound : P;
    if (bound > 0) {
        mcmc_scan_k<<<dim3(blocks), dim3(MC_THREADS), 0, s>>>(P, opacity, selection, min_opacity, v.part, v.csum, v.dead);
        const unsigned g1 = (unsigned)std::min<size_t>(div_up((size_t)bound, MC_THREADS), MC_GRID);
        mcmc_sample_k<<<dim3(g1), dim3(MC_THREADS), 0, s>>>(P, reinterpret_cast<const long long*>(draws), v.head, v.csum, v.hits, v.src,
                                                            counts, status);
        const McmcTables tab = make_tables();
        mcmc_values_k<<<dim3(g1), dim3(MC_THREADS), 0, s>>>(opacity, scaling, v.head, v.hits, v.src, min_opacity, n_max, tab,
                                                            v.new_opacity, v.new_scale);
        if (n_groups > 0) {
            ApplyTable t;
            for (int k = 0; k < GOI_MCMC_MAX_GROUPS; k++) t.g[k] = groups[k < n_groups ? k : 0];
            const unsigned g2 = (unsigned)std::min<size_t>(div_up((size_t)bound * (size_t)max_rl, MC_THREADS), MC_GRID);
            mcmc_apply_k<<<dim3(g2, (unsigned)n_groups), dim3(MC_THREADS), 0, s>>>(t, v.head, v.src, v.dead, v.new_opacity, v.new_scale);
        }
    }
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_mcmc_noise(long long P, float* xyz, const float* rotation, const float* scaling, const float* opacity, const float* z,
                   const unsigned char* selection, double k, double x0, double step, void* stream) {
    const std::string fn = "goi_mcmc_noise: ";
    if (P < 0 || P >= (1ll << 30)) return fail(fn + "need 0 <= P < 2^30");
    if (!std::isfinite(k) || !std::isfinite(x0) || !std::isfinite(step)) return fail(fn + "k, x0 and step must be finite");
    if (P == 0) return 0;
    if (!xyz || !rotation || !scaling || !opacity || !z) return fail(fn + "a required pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(rotation) | reinterpret_cast<uintptr_t>(scaling) |
         reinterpret_cast<uintptr_t>(opacity) | reinterpret_cast<uintptr_t>(z)) & 3)
        return fail(fn + "xyz, rotation, scaling, opacity and z must be 4-byte aligned");
    mcmc_noise_k<<<dim3((unsigned)div_up((size_t)P, MC_THREADS)), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream)>>>(
        P, xyz, rotation, scaling, opacity, z, selection, k, x0, step);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_mcmc_debug_relocation_sum(int n, const double* o_new, const int32_t* N, double* D, void* stream) {
    const std::string fn = "goi_mcmc_debug_relocation_sum: ";
    if (n < 0 || n > (1 << 24)) return fail(fn + "need 0 <= n <= 2^24");
    if (n == 0) return 0;
    if (!o_new || !N || !D) return fail(fn + "a required pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(o_new) | reinterpret_cast<uintptr_t>(D)) & 7) return fail(fn + "o_new and D must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(N) & 3) return fail(fn + "N must be 4-byte aligned");
    mcmc_debug_sum_k<<<dim3((unsigned)div_up((size_t)n, MC_THREADS)), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream)>>>(
        n, o_new, N, make_tables(), D);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
