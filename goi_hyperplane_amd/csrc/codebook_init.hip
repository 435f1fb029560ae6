// Code-book initialisation on the device (the reference's train.py:78-86): exact row dedup of per-view APE maps
// (x.permute(1,2,0).reshape(-1, D).unique(dim=0)) and spherical k-means (train.py:36-56).
//
// Row dedup of a [D][H][W] fp32 map, one view at a time on the caller's stream:
//   uniq_insert_k   lane = pixel, so every channel read is coalesced straight from the CHW layout.  The pixel's D values
//                   become order-preserving uint32 keys (-0 folded onto +0) and a 32-bit hash; the pixel goes into an
//                   open-addressing table of 2^t >= 2 HW 64-bit slots, (hash << 32 | pixel).  A slot is claimed by CAS;
//                   a pixel whose hash matches a slot's is compared against that slot's pixel over the FULL row, never
//                   by hash alone, and joins it by atomicMin, so a slot ends up holding its class's first pixel.  The
//                   table holds at most half as many classes as slots, so a probe always ends; the loop is bounded
//                   anyway and sets GOI_CODEBOOK_FLAG_TABLE if the bound is ever hit.  A NaN or Inf sets GOI_CODEBOOK_FLAG_NONFINITE.
//   uniq_mark_k     a pixel that is its slot's minimum is its class's representative: appended to the view's list
//                   (wave-aggregated atomic) and counted.  The list's order does not matter: the sort below is total.
// After the host has read the counts (one read-back for all views):
//   N <= GOI_CODEBOOK_RANK_MAX (and D <= 8192)  uniq_keys_rows_k gathers the N rows' keys row-major; uniq_rank_k gives each row its rank by
//                       comparison with every other row; uniq_write_k gathers the rows in rank order (one thread per
//                       output float: a thread per row copying its own D floats was latency-bound, 2 ms per view).
//   larger N            an LSD sort over the channels: D stable 32-bit radix sorts (scan_sort.hip) of the row list,
//                       last channel first; then uniq_write_k gathers the rows in that order.  Correct up to N = HW.
// The rows written are the representatives' own values (the kept sign of a +-0 is the first pixel's).
//
// Spherical k-means of K independent problems over ragged concatenated rows x [sum N_p][D] (fp32 only):
//   km_normalize_k   x /= |x| in place, one wave per row (a zero row becomes NaN, as in the reference)
//   km_init_k        centres = x[perm_0[:min(N, k)]]
//   per iteration (launched back to back, no host synchronisation):
//     km_center_norm_k  cn = centres / |centres|
//     km_assign_k       argmax_j x . cn_j: 64 rows x 64 centres per workgroup through LDS, fp32 FMA in d order;
//                       NaN is the largest value, ties and NaNs go to the lowest index (torch's argmax)
//     km_mean_k         one workgroup per (problem, centre): the members' sum in ascending row order (no float
//                       atomics: bit-reproducible), divided by the count; 0 members or a NaN makes the centre dead
//     km_dead_k         dead centres in index order take x[perm_{it+1}[0 .. ndead)]; ndead > N is the reference's
//                       shape-mismatch RuntimeError and is recorded in status[p] (first iteration + 1)
// C entries, with the limits they enforce, at the end of the file: goi_codebook_unique_rows* / _kmeans* (declared in include/goi_raster.h).
#include <vector>

#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int UNIQ_THREADS = 256;
constexpr int KM_THREADS = 256;
constexpr int KM_TM = 64, KM_TN = 64, KM_BK = 16;
constexpr int KM_MAX_K = GOI_CODEBOOK_KMEANS_MAX_K;  // km_dead_k's rank array in LDS
constexpr int KM_MAX_DIM = GOI_CODEBOOK_KMEANS_MAX_DIM;  // km_mean_k's accumulators per thread: KM_MAX_DIM / KM_THREADS
constexpr uint64_t SLOT_EMPTY = ~0ull;
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr int RANK_TILE_WORDS = 8192;  // uniq_rank_k's LDS tile (32 KiB); wider rows take the radix path

inline size_t div_up_sz(size_t a, size_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ uint32_t order_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u << 1) == 0u) u = 0u;  // -0 -> +0
    return ord_enc_bits(u);
}

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ uint32_t hash_step(uint32_t h, uint32_t k) {  // MurmurHash3's block step
    k *= 0xcc9e2d51u;
    k = rotl32(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

__device__ __forceinline__ uint32_t hash_final(uint32_t h, uint32_t len) {
    h ^= len;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}

__global__ void __launch_bounds__(UNIQ_THREADS) uniq_insert_k(const float* __restrict__ map, int D, uint32_t HW,
                                                              unsigned long long* __restrict__ table, uint32_t tmask,
                                                              uint32_t* __restrict__ slot_of, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * UNIQ_THREADS + threadIdx.x;
    if (p >= HW) return;
    uint32_t h = 0x9747b28cu;
    bool finite = true;
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const float v = map[(size_t)c * HW + p];
        finite &= isfinite(v);
        h = hash_step(h, order_key(v));
    }
    if (!finite) {
        atomicOr(flag, (uint32_t)GOI_CODEBOOK_FLAG_NONFINITE);
        slot_of[p] = NO_SLOT;
        return;
    }
    h = hash_final(h, (uint32_t)D);
    const unsigned long long mine = ((unsigned long long)h << 32) | p;
    uint32_t s = h & tmask;
    for (uint32_t probe = 0; probe <= tmask; ++probe, s = (s + 1) & tmask) {
        unsigned long long cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == SLOT_EMPTY) {
            cur = atomicCAS(table + s, SLOT_EMPTY, mine);
            if (cur == SLOT_EMPTY) {
                slot_of[p] = s;
                return;
            }
        }
        if ((uint32_t)(cur >> 32) != h) continue;
        const uint32_t q = (uint32_t)cur;  // any member of the slot's class: all of them hold the same row
        // finite values: == is key equality.  Eight channels per step, so eight load pairs are in flight at a time
        bool same = true;
        for (int c0 = 0; c0 < D && same; c0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = c0 + u;
                if (c < D) same &= map[(size_t)c * HW + p] == map[(size_t)c * HW + q];
            }
        }
        if (same) {
            if ((uint32_t)cur > p) atomicMin(table + s, mine);  // a slot already at a lower pixel stays there: no atomic
            slot_of[p] = s;
            return;
        }
    }
    atomicOr(flag, (uint32_t)GOI_CODEBOOK_FLAG_TABLE);
    slot_of[p] = NO_SLOT;
}

__global__ void __launch_bounds__(UNIQ_THREADS) uniq_mark_k(const unsigned long long* __restrict__ table,
                                                            const uint32_t* __restrict__ slot_of, uint32_t HW,
                                                            uint32_t* __restrict__ reps, uint32_t* __restrict__ count) {
    const uint32_t p = blockIdx.x * UNIQ_THREADS + threadIdx.x;
    bool rep = false;
    if (p < HW) {
        const uint32_t s = slot_of[p];
        rep = s != NO_SLOT && (uint32_t)table[s] == p;
    }
    const uint64_t m = __ballot(rep);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    const int leader = __ffsll((unsigned long long)m) - 1;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (rep) reps[base + __popcll(m & ((1ull << lane) - 1ull))] = p;
}

// keys [N][D] row-major of the N representatives
__global__ void __launch_bounds__(UNIQ_THREADS) uniq_keys_rows_k(const float* __restrict__ map, int D, uint32_t HW,
                                                                 const uint32_t* __restrict__ reps, uint32_t N,
                                                                 uint32_t* __restrict__ keys) {
    const size_t total = (size_t)N * D;
    for (size_t g = (size_t)blockIdx.x * UNIQ_THREADS + threadIdx.x; g < total; g += (size_t)gridDim.x * UNIQ_THREADS) {
        const uint32_t i = (uint32_t)(g / D);
        const int c = (int)(g - (size_t)i * D);
        keys[g] = order_key(map[(size_t)c * HW + reps[i]]);
    }
}

// rank of row i = number of rows lexicographically below it (the rows are distinct): order[rank] = its pixel.  The other
// rows' keys come through LDS, RANK_TILE_WORDS at a time, loaded coalesced by the workgroup; a row's first key stays in
// a register, and the rest of its row is read only when a first key ties.
__global__ void __launch_bounds__(UNIQ_THREADS) uniq_rank_k(const uint32_t* __restrict__ reps, uint32_t N, int D,
                                                            const uint32_t* __restrict__ keys, uint32_t* __restrict__ order) {
    __shared__ uint32_t tile[RANK_TILE_WORDS];
    const uint32_t i = blockIdx.x * UNIQ_THREADS + threadIdx.x;
    const bool valid = i < N;
    const uint32_t* mine = keys + (size_t)(valid ? i : 0) * D;
    const uint32_t m0 = mine[0];
    const uint32_t tj = RANK_TILE_WORDS / D;  // rows per tile (D <= RANK_TILE_WORDS)
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < N; j0 += tj) {
        const uint32_t nj = N - j0 < tj ? N - j0 : tj;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < nj * D; e += UNIQ_THREADS) tile[e] = keys[(size_t)j0 * D + e];
        __syncthreads();
        if (!valid) continue;
        for (uint32_t jj = 0; jj < nj; ++jj) {
            if (j0 + jj == i) continue;
            const uint32_t* other = tile + jj * D;
            if (other[0] != m0) {
                rank += other[0] < m0 ? 1u : 0u;
                continue;
            }
            int c = 1;
            while (c < D && other[c] == mine[c]) ++c;
            rank += (c < D && other[c] < mine[c]) ? 1u : 0u;
        }
    }
    if (valid) order[rank] = reps[i];
}

// one LSD step: keys of channel c of the rows in the current order (perm may alias vals)
__global__ void __launch_bounds__(UNIQ_THREADS) uniq_channel_keys_k(const float* __restrict__ plane, const uint32_t* perm,
                                                                    uint32_t N, uint32_t* __restrict__ keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * UNIQ_THREADS + threadIdx.x;
    if (i >= N) return;
    const uint32_t p = perm[i];
    keys[i] = order_key(plane[p]);
    vals[i] = p;
}

__global__ void __launch_bounds__(UNIQ_THREADS) uniq_write_k(const float* __restrict__ map, int D, uint32_t HW,
                                                             const uint32_t* __restrict__ order, uint32_t N,
                                                             float* __restrict__ out) {
    const size_t total = (size_t)N * D;
    for (size_t g = (size_t)blockIdx.x * UNIQ_THREADS + threadIdx.x; g < total; g += (size_t)gridDim.x * UNIQ_THREADS) {
        const uint32_t i = (uint32_t)(g / D);
        const int c = (int)(g - (size_t)i * D);
        out[g] = map[(size_t)c * HW + order[i]];
    }
}

struct UniqLayout {
    uint32_t tbits;
    unsigned long long* table;
    uint32_t *slot_of, *reps, *counts, *rank_keys, *rank_order;
    SortBufs sb;  // [HW]; only where a view can take the radix path
    size_t bytes;
};

UniqLayout uniq_layout(char* base, int V, int D, uint32_t HW) {
    UniqLayout L{};
    uint32_t tbits = 6;
    while ((1ull << tbits) < 2ull * HW) ++tbits;
    L.tbits = tbits;
    Carver c(base);
    L.table = c.take<unsigned long long>((size_t)1 << tbits);
    L.slot_of = c.take<uint32_t>(HW);
    L.reps = c.take<uint32_t>((size_t)HW * V);
    L.counts = c.take<uint32_t>((size_t)V + 1);  // [V] counts, then the flag word
    const size_t nrank = (size_t)HW < (size_t)GOI_CODEBOOK_RANK_MAX ? HW : (size_t)GOI_CODEBOOK_RANK_MAX;
    L.rank_keys = c.take<uint32_t>(nrank * D);
    L.rank_order = c.take<uint32_t>(nrank);
    if (HW > (uint32_t)GOI_CODEBOOK_RANK_MAX || D > RANK_TILE_WORDS) carve_sort(c, HW, &L.sb);
    L.bytes = c.bytes();
    return L;
}

__device__ __forceinline__ bool km_better(float va, int ia, float vb, int ib) {  // a ranks before b
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// x [rows][D] /= its norm, one wave per row
__global__ void __launch_bounds__(KM_THREADS) km_normalize_k(float* __restrict__ x, long long rows, int D) {
    const long long r = (long long)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    float* row = x + r * D;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss = fmaf(row[d], row[d], ss);
    const float n = sqrtf(wave_sum(ss));
    for (int d = lane; d < D; d += 64) row[d] = row[d] / n;
}

__global__ void __launch_bounds__(KM_THREADS) km_init_k(const float* __restrict__ x, const long long* __restrict__ off, int D,
                                                        int k, int niter, const int* __restrict__ perms,
                                                        float* __restrict__ centers) {
    const int p = blockIdx.y;
    const long long o = off[p], n = off[p + 1] - o;
    const int* perm0 = perms + (long long)(niter + 1) * o;
    const long long kc = n < k ? n : k;
    for (long long g = (long long)blockIdx.x * KM_THREADS + threadIdx.x; g < (long long)k * D; g += (long long)gridDim.x * KM_THREADS) {
        const long long j = g / D;
        const int d = (int)(g - j * D);
        centers[((long long)p * k + j) * D + d] = j < kc ? x[(o + perm0[j]) * D + d] : 0.f;
    }
}

// cn = centres / |centres|, one wave per centre
__global__ void __launch_bounds__(KM_THREADS) km_center_norm_k(const float* __restrict__ centers, float* __restrict__ cn,
                                                               long long rows, int D) {
    const long long r = (long long)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* row = centers + r * D;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss = fmaf(row[d], row[d], ss);
    const float n = sqrtf(wave_sum(ss));
    for (int d = lane; d < D; d += 64) cn[r * D + d] = row[d] / n;
}

// blockIdx.y = problem, blockIdx.x = tile of 64 rows; the workgroup walks all centres 64 at a time.  Thread (tr, tc) =
// (t / 16, t % 16) holds rows 4 tr .. 4 tr + 3 against centres 4 tc .. 4 tc + 3 of the current centre tile.
__global__ void __launch_bounds__(KM_THREADS) km_assign_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                          const float* __restrict__ cn, int D, int k, int first,
                                                          int* __restrict__ assign) {
    __shared__ float xs[KM_BK][KM_TM + 4];
    __shared__ float cs[KM_BK][KM_TN + 4];
    const int p = blockIdx.y;
    const long long o = off[p], n = off[p + 1] - o;
    const long long r0 = (long long)blockIdx.x * KM_TM;
    if (r0 >= n) return;  // uniform over the workgroup
    const int kc = first ? (int)(n < k ? n : k) : k;
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const float* cnp = cn + (long long)p * k * D;
    float bv[4];
    int bi[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { bv[a] = -INFINITY; bi[a] = 0x7fffffff; }
    for (int j0 = 0; j0 < kc; j0 += KM_TN) {
        float acc[4][4] = {};
        for (int d0 = 0; d0 < D; d0 += KM_BK) {
#pragma unroll
            for (int q = 0; q < (KM_TM * KM_BK) / KM_THREADS; ++q) {
                const int e = t + q * KM_THREADS, row = e / KM_BK, kk = e % KM_BK;
                const long long r = r0 + row;
                const int d = d0 + kk;
                xs[kk][row] = (r < n && d < D) ? x[(o + r) * D + d] : 0.f;
                const int j = j0 + row;
                cs[kk][row] = (j < kc && d < D) ? cnp[(long long)j * D + d] : 0.f;
            }
            __syncthreads();
            const int kmax = D - d0 < KM_BK ? D - d0 : KM_BK;  // the FMA chain stays d = 0 .. D-1 with no padded terms
            for (int kk = 0; kk < kmax; ++kk) {
                float xa[4], cb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) { xa[a] = xs[kk][4 * tr + a]; cb[a] = cs[kk][4 * tc + a]; }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xa[a], cb[b], acc[a][b]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * tc + b;
            if (j < kc) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (km_better(acc[a][b], j, bv[a], bi[a])) { bv[a] = acc[a][b]; bi[a] = j; }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {  // the 16 threads of a row group are 16 consecutive lanes of one wave
            const float ov = __shfl_xor(bv[a], m);
            const int oi = __shfl_xor(bi[a], m);
            if (km_better(ov, oi, bv[a], bi[a])) { bv[a] = ov; bi[a] = oi; }
        }
        const long long r = r0 + 4 * tr + a;
        if (tc == 0 && r < n) assign[o + r] = bi[a];
    }
}

// grid (k, K): the mean of centre j of problem p over its members in ascending row order; dead[p][j] = empty or NaN
__global__ void __launch_bounds__(KM_THREADS) km_mean_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                        const int* __restrict__ assign, int D, int k,
                                                        float* __restrict__ centers, int* __restrict__ dead) {
    __shared__ int members[KM_THREADS];
    __shared__ int wave_count[KM_THREADS / 64];
    const int p = blockIdx.y, j = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long o = off[p], n = off[p + 1] - o;
    float acc[KM_MAX_DIM / KM_THREADS];
#pragma unroll
    for (int u = 0; u < KM_MAX_DIM / KM_THREADS; ++u) acc[u] = 0.f;
    long long count = 0;
    for (long long i0 = 0; i0 < n; i0 += KM_THREADS) {
        const bool in = i0 + t < n && assign[o + i0 + t] == j;
        const uint64_t m = __ballot(in);
        if (lane == 0) wave_count[w] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int v = 0; v < KM_THREADS / 64; ++v) {
            base += v < w ? wave_count[v] : 0;
            total += wave_count[v];
        }
        if (in) members[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)(i0 + t);
        __syncthreads();
        for (int q = 0; q < total; ++q) {
            const float* row = x + (o + members[q]) * D;
#pragma unroll
            for (int u = 0; u < KM_MAX_DIM / KM_THREADS; ++u) {
                const int d = t + u * KM_THREADS;
                if (d < D) acc[u] += row[d];
            }
        }
        count += total;
        __syncthreads();
    }
    const float cnt = (float)count;
    bool nan = false;
    float* dst = centers + ((long long)p * k + j) * D;
#pragma unroll
    for (int u = 0; u < KM_MAX_DIM / KM_THREADS; ++u) {
        const int d = t + u * KM_THREADS;
        if (d < D) {
            const float v = acc[u] / cnt;  // no members: 0 / 0 = NaN, the mean of an empty selection
            nan |= v != v;
            dst[d] = v;
        }
    }
    const int any_nan = __syncthreads_or(nan ? 1 : 0);
    if (t == 0) dead[(long long)p * k + j] = any_nan ? 1 : 0;
}

// grid K: dead centres of problem p, in index order, take rows perm_{it+1}[0 .. ndead) of x
__global__ void __launch_bounds__(KM_THREADS) km_dead_k(const float* __restrict__ x, const long long* __restrict__ off, int D,
                                                        int k, int niter, int it, const int* __restrict__ perms,
                                                        const int* __restrict__ dead, float* __restrict__ centers,
                                                        int* __restrict__ status) {
    __shared__ int rank[KM_MAX_K];
    __shared__ int ndead_s;
    const int p = blockIdx.x, t = threadIdx.x;
    const long long o = off[p], n = off[p + 1] - o;
    for (int j = t; j < k; j += KM_THREADS) rank[j] = dead[(long long)p * k + j];
    __syncthreads();
    if (t == 0) {
        int c = 0;
        for (int j = 0; j < k; ++j) {
            const int dj = rank[j];
            rank[j] = dj ? c : -1;
            c += dj;
        }
        ndead_s = c;
    }
    __syncthreads();
    const int ndead = ndead_s;
    if (ndead > n) {  // x[randperm(N)[:ndead]] has N < ndead rows: the reference raises here
        if (t == 0 && status[p] == 0) status[p] = it + 1;
        return;
    }
    const int* perm = perms + (long long)(niter + 1) * o + (long long)(it + 1) * n;
    for (int j = 0; j < k; ++j) {
        const int r = rank[j];
        if (r < 0) continue;  // uniform
        const float* src = x + (o + perm[r]) * D;
        float* dst = centers + ((long long)p * k + j) * D;
        for (int d = t; d < D; d += KM_THREADS) dst[d] = src[d];
    }
}

size_t uniq_workspace_bytes(int V, int D, uint32_t HW) { return uniq_layout(nullptr, V, D, HW).bytes; }

uint32_t* uniq_counts(void* ws, int V, int D, uint32_t HW) {
    return uniq_layout(static_cast<char*>(ws), V, D, HW).counts;
}

void launch_uniq_dedup(const float* const* maps, int V, int D, uint32_t HW, void* ws, hipStream_t s) {
    const UniqLayout L = uniq_layout(static_cast<char*>(ws), V, D, HW);
    (void)hipMemsetAsync(L.counts, 0, 4ull * (V + 1), s);
    const uint32_t grid = (uint32_t)div_up_sz(HW, UNIQ_THREADS);
    for (int v = 0; v < V; ++v) {
        (void)hipMemsetAsync(L.table, 0xFF, sizeof(uint64_t) << L.tbits, s);
        uniq_insert_k<<<grid, UNIQ_THREADS, 0, s>>>(maps[v], D, HW, L.table, (1u << L.tbits) - 1u, L.slot_of, L.counts + V);
        uniq_mark_k<<<grid, UNIQ_THREADS, 0, s>>>(L.table, L.slot_of, HW, L.reps + (size_t)v * HW, L.counts + v);
    }
}

bool launch_uniq_sort(const float* map, int v, int V, int D, uint32_t HW, uint32_t N, float* out, void* ws, hipStream_t s) {
    if (N == 0) return false;
    const UniqLayout L = uniq_layout(static_cast<char*>(ws), V, D, HW);
    const uint32_t* reps = L.reps + (size_t)v * HW;
    const size_t total = (size_t)N * D;
    const uint32_t gw = (uint32_t)(div_up_sz(total, UNIQ_THREADS) < 65536 ? div_up_sz(total, UNIQ_THREADS) : 65536);
    if (N <= (uint32_t)GOI_CODEBOOK_RANK_MAX && D <= RANK_TILE_WORDS) {
        uniq_keys_rows_k<<<gw, UNIQ_THREADS, 0, s>>>(map, D, HW, reps, N, L.rank_keys);
        uniq_rank_k<<<(uint32_t)div_up_sz(N, UNIQ_THREADS), UNIQ_THREADS, 0, s>>>(reps, N, D, L.rank_keys, L.rank_order);
        uniq_write_k<<<gw, UNIQ_THREADS, 0, s>>>(map, D, HW, L.rank_order, N, out);
        return false;
    }
    const uint32_t* perm = reps;
    const uint32_t grid = (uint32_t)div_up_sz(N, UNIQ_THREADS);
    for (int c = D - 1; c >= 0; --c) {
        uniq_channel_keys_k<<<grid, UNIQ_THREADS, 0, s>>>(map + (size_t)c * HW, perm, N, L.sb.keys[0], L.sb.vals[0]);
        const int fin = radix_sort_pairs(L.sb.keys, L.sb.vals, N, 0, 32, L.sb.scratch, s, false, false, nullptr, L.counts + V);
        perm = L.sb.vals[fin];
    }
    uniq_write_k<<<gw, UNIQ_THREADS, 0, s>>>(map, D, HW, perm, N, out);
    return true;
}

struct KmeansView {
    float* cn;    // [K k D] normalised centres
    int* assign;  // [rows]
    int* dead;    // [K k]
};
size_t kmeans_layout(long long rows, int K, int k, int D, void* base, KmeansView* v) {
    Carver c(base);
    KmeansView t;
    t.cn = c.take<float>((size_t)K * k * D);
    t.assign = c.take<int>((size_t)rows);
    t.dead = c.take<int>((size_t)K * k);
    if (v) *v = t;
    return c.bytes();
}

size_t kmeans_workspace_bytes(long long rows, int K, int k, int D) { return kmeans_layout(rows, K, k, D, nullptr, nullptr); }

void launch_kmeans(float* x, const long long* off, int K, long long max_rows, long long total_rows, int D, int k, int niter,
                   const int* perms, float* centers, int* status, void* ws, hipStream_t s) {
    KmeansView w;
    kmeans_layout(total_rows, K, k, D, ws, &w);
    (void)hipMemsetAsync(status, 0, sizeof(int) * K, s);
    const int rows_per_block = KM_THREADS / 64;
    if (total_rows > 0)
        km_normalize_k<<<(uint32_t)div_up_sz(total_rows, rows_per_block), KM_THREADS, 0, s>>>(x, total_rows, D);
    const size_t init_elems = (size_t)k * D;
    km_init_k<<<dim3((uint32_t)div_up_sz(init_elems, KM_THREADS), K), KM_THREADS, 0, s>>>(x, off, D, k, niter, perms, centers);
    const long long crow = (long long)K * k;
    const dim3 agrid((uint32_t)div_up_sz(max_rows, KM_TM), K);
    for (int it = 0; it < niter; ++it) {
        km_center_norm_k<<<(uint32_t)div_up_sz(crow, rows_per_block), KM_THREADS, 0, s>>>(centers, w.cn, crow, D);
        km_assign_k<<<agrid, KM_THREADS, 0, s>>>(x, off, w.cn, D, k, it == 0, w.assign);
        km_mean_k<<<dim3(k, K), KM_THREADS, 0, s>>>(x, off, w.assign, D, k, centers, w.dead);
        km_dead_k<<<K, KM_THREADS, 0, s>>>(x, off, D, k, niter, it, perms, w.dead, centers, status);
    }
}

int uniq_dims(const char* fn, int n_views, int D, int H, int W) {
    if (n_views < 0 || D < 1 || H < 1 || W < 1) return fail(std::string(fn) + ": need n_views >= 0 and D, H, W >= 1");
    if ((long long)H * W >= SORT_MAX_KEYS) return fail(std::string(fn) + ": need H * W < 2^30");
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_codebook_unique_rows_workspace_bytes(int n_views, int D, int H, int W) {
    if (n_views < 1 || D < 1 || H < 1 || W < 1 || (long long)H * W >= SORT_MAX_KEYS) return 0;
    return uniq_workspace_bytes(n_views, D, (uint32_t)((long long)H * W));
}

int goi_codebook_unique_rows(const float* const* maps, int n_views, int D, int H, int W, long long* counts, unsigned* flags,
                             goi_alloc_fn alloc, void* alloc_user, void* workspace, void* stream) {
    refresh_options();
    const char* fn = "goi_codebook_unique_rows";
    if (uniq_dims(fn, n_views, D, H, W) < 0) return -1;
    if (!flags || (n_views > 0 && (!maps || !counts || !alloc))) return fail(std::string(fn) + ": a required pointer is NULL");
    *flags = 0;
    if (n_views == 0) return 0;
    for (int v = 0; v < n_views; ++v)
        if (!maps[v]) return fail(std::string(fn) + ": maps[" + std::to_string(v) + "] is NULL");
    if (check_workspace(fn, workspace) < 0) return -1;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t HW = (uint32_t)((long long)H * W);
    launch_uniq_dedup(maps, n_views, D, HW, workspace, s);
    GOI_HIP(hipGetLastError());
    std::vector<uint32_t> host(n_views + 1);
    uint32_t* dev_counts = uniq_counts(workspace, n_views, D, HW);
    GOI_HIP(hipMemcpyAsync(host.data(), dev_counts, sizeof(uint32_t) * (n_views + 1), hipMemcpyDeviceToHost, s));
    GOI_HIP(hipStreamSynchronize(s));  // the one read-back: counts and flag word of every view
    *flags = host[n_views];
    long long total = 0;
    for (int v = 0; v < n_views; ++v) total += (counts[v] = host[v]);
    if (*flags) return 0;
    float* out = static_cast<float*>(alloc(alloc_user, (size_t)total * D * sizeof(float) + 1));
    if (!out) return fail(std::string(fn) + ": output allocation failed");
    bool sorted = false;
    for (int v = 0; v < n_views; ++v) {
        sorted |= launch_uniq_sort(maps[v], v, n_views, D, HW, host[v], out, workspace, s);
        GOI_HIP(hipGetLastError());
        out += (size_t)host[v] * D;
    }
    if (sorted) {  // the radix sorts OR their look-back error into the flag word
        uint32_t f = 0;
        GOI_HIP(hipMemcpyAsync(&f, dev_counts + n_views, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GOI_HIP(hipStreamSynchronize(s));
        *flags = f;
    }
    return 0;
}

size_t goi_codebook_kmeans_workspace_bytes(long long n_rows, int n_problems, int ncluster, int D) {
    if (n_rows < 0 || n_problems < 1 || ncluster < 1 || D < 1) return 0;
    return kmeans_workspace_bytes(n_rows, n_problems, ncluster, D);
}

int goi_codebook_kmeans(float* x, const long long* row_offsets, int n_problems, long long max_rows, long long n_rows, int D,
                        int ncluster, int niter, const int* perms, float* centers, int* status, void* workspace, void* stream) {
    const char* fn = "goi_codebook_kmeans";
    if (n_problems < 0 || n_problems > 65535) return fail(std::string(fn) + ": need 0 <= n_problems <= 65535");
    if (ncluster < 1 || ncluster > GOI_CODEBOOK_KMEANS_MAX_K) return fail(std::string(fn) + ": need 1 <= ncluster <= 4096");
    if (D < 1 || D > GOI_CODEBOOK_KMEANS_MAX_DIM) return fail(std::string(fn) + ": need 1 <= D <= 1024");
    if (niter < 0) return fail(std::string(fn) + ": need niter >= 0");
    if (n_rows < 0 || n_rows >= (1ll << 31) || max_rows < 1 || max_rows > n_rows)
        return fail(std::string(fn) + ": need 1 <= max_rows <= n_rows < 2^31");
    if (n_problems == 0) return 0;
    if (!x || !row_offsets || !perms || !centers || !status) return fail(std::string(fn) + ": a required pointer is NULL");
    if (check_workspace(fn, workspace) < 0) return -1;
    launch_kmeans(x, row_offsets, n_problems, max_rows, n_rows, D, ncluster, niter, perms, centers, status, workspace,
                  static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
