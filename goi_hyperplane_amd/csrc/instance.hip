// Per-instance statistics over a partition of the Gaussians (goi_hyperplane_amd/instance.py): the
// partition as member lists, and one segmented reduction that gives every statistic of every instance.
//
// goi_instance_members -- label [P] -> member_ptr [K+1], member [P].  A row is in instance label[i] iff 0 <= label[i] < K.
//   inst_count_k    key[i] = label[i] of a row in an instance, K of any other; val[i] = i; cnt[key]++ by integer atomics.  A wave
//                   walks INST_ROWS consecutive batches of 64 rows; a label that holds more than half of a batch (ballot +
//                   popcount) is counted in a register across batches, so ONE giant instance costs an atomic per 1024 rows,
//                   not per row, whatever rows of other instances lie between its own.
//   exclusive_scan_u32 over cnt [K+1] (cnt[K] stays 0) is member_ptr, and member_ptr[K] the number of rows in an instance.
//   radix_sort_pairs, stable, over just the key bits K + 1 needs: rows in ascending (label, row) order, the others behind them.
//   inst_members_k  member[r] = the r-th sorted row, -1 from member_ptr[K] on.
//   (goi_knn_transpose's method with the same helpers: smooth.hip.)
//
// goi_instance_stats -- THE SUMMATION ORDER of an instance is a fixed function of its own member sequence m_0 .. m_{n-1} and of
// nothing else (not of the grid, of K, of the other instances, of how its chunks were spread over the machine):
//   pivot   p = xyz[m_0] (fp32; 0 for an empty instance; without xyz every position is the origin)
//   member  w = (double)weight[m] (1 without weights), d_a = (double)xyz[m,a] - (double)p_a, t_a = w * d_a, and the terms
//               W: w     Sd_a: t_a     Sdd_ab: t_a * d_b  (ab = xx xy xz yy yz zz)     Sf_c: w * (double)f[m,c]
//   chunk   the members are cut into chunks of 256 consecutive members.  Inside a chunk every quantity has four accumulators
//           a_0 .. a_3, each +0.0 at the start; the member at position r goes to a_(r mod 4): a = a + term, in ascending r.  The
//           chunk's partial is (a_0 + a_2) + (a_1 + a_3).
//   total   T = +0.0, then T = T + partial in ascending chunk order.
//   result  m_a = Sd_a / W;  centroid_a = (float)(p_a + m_a);  cov_ab = (float)(Sdd_ab / W - m_a * m_b);  feature_c =
//           (float)(Sf_c / W);  wsum = (float)W.  W == 0 (an empty instance included): centroid, cov and feature are 0, nothing
//           is divided.
//   Everything in float64, one rounding per operation (this TU is compiled with -ffp-contract=off), one rounding to fp32 at
//   the end.  lo / hi go through the order-preserving integer key of wave_util.h (-0 < +0), a NaN coordinate is skipped, so
//   they are exact and independent of any order; an instance without a number on an axis keeps +inf / -inf.  n and hits are
//   integers.
//
// MAPPING.  A QUARTER WAVE (16 lanes) walks one chunk.  Lane l fetches member l of a batch of 16 (its id, weight, position, hit
// byte), the batch is then broadcast member by member, four members in flight -- the four accumulators are the four slots of
// that unrolled loop.  Lane l holds channels l and l + 16 of Sf (a member's feature row is one coalesced read of at most 128
// bytes, as in smooth_loss_k), lanes 0 .. 9 one of W, Sd, Sdd each (a lane's term is (w * dA) * dB with dA, dB picked from 1, dx,
// dy, dz: a product by 1.0 is exact, so the ten lanes run ONE instruction stream), lanes 0 .. 7 one hit bit, lanes 0 .. 2 one axis.
//   inst_small_k    a quarter wave per instance of at most 256 members: its one chunk, then the results.  No search.
//   inst_slots_k + exclusive_scan_u32   an instance of more than 256 members takes one workspace slot per chunk.
//   inst_chunks_k   a quarter wave per slot (at most 2 * floor(P / 256) of them): finds its instance in the scanned slot counts
//                   by bisection, walks the chunk, stores the partial.  A giant instance is spread over the whole machine.
//   inst_final_k    a quarter wave per instance with slots: adds the partials in ascending order, then the results.
// Stages are separated by kernel boundaries, no workgroup waits for another, no float atomics, nothing is read back, every
// store is an ordinary vector store, every loop is bounded.  What a caller hands in as member_ptr / member is clamped before it
// is used: wrong lists give wrong statistics, never an access outside the arrays.
// C entries at the end of the file: goi_instance_members, goi_instance_stats (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int INST_THREADS = 256;
constexpr int INST_GROUP = 16;                          // lanes per chunk: a quarter wave
constexpr int INST_GROUPS = INST_THREADS / INST_GROUP;  // chunks a workgroup walks at a time
constexpr int INST_CHUNK = 256;                         // members per chunk
constexpr int INST_ROWS = 16;                           // batches of 64 rows a wave of inst_count_k walks
constexpr int INST_LEADS = 4;                           // labels of a batch that inst_count_k combines before the lanes add one by one
constexpr int INST_AHEAD = 16;                          // partials inst_final_k has in flight
constexpr long long INST_MAX = 1ll << 30;               // P and K below this: the sort's limit
constexpr int INST_MOMENTS = 10;                        // W, Sd[3], Sdd[6]
constexpr int INST_SLOT_DOUBLES = 50;  // a slot: 10 moments, 32 channels (doubles 0 .. 41), then 6 lo / hi keys and 8 hit counts (words)

unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
size_t slot_capacity(int P) { return 2 * ((size_t)P / INST_CHUNK); }  // (n > 256: ceil(n / 256) <= 2 * floor(n / 256))

// ---- the partition as lists ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(INST_THREADS) void inst_count_k(int P, int K, const int32_t* __restrict__ label,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                             uint32_t* cnt) {
    const int lane = threadIdx.x & 63;
    const long long wave_base = ((long long)blockIdx.x * (INST_THREADS / 64) + (threadIdx.x >> 6)) * (64 * INST_ROWS);
    uint32_t run_label = 0, run_n = 0;  // (the same in every lane of the wave)
    for (int r = 0; r < INST_ROWS; r++) {
        const long long i = wave_base + (long long)r * 64 + lane;
        bool in = false;
        uint32_t key = (uint32_t)K;
        if (i < P) {
            const int32_t l = label[i];
            in = l >= 0 && l < K;
            if (in) key = (uint32_t)l;
            keys[i] = key;
            vals[i] = (uint32_t)i;
        }
        // Up to INST_LEADS times: the first open lane's label is broadcast and its lanes are counted.  A label that holds more than
        // half of the batch goes to the run register (flushed when the label changes), any other costs one atomic; the lanes
        // that are still open after that add 1 each.
        bool todo = in;
        for (int round = 0; round < INST_LEADS; round++) {
            const unsigned long long open = __ballot(todo);
            if (!open) break;
            const int first = __builtin_ctzll(open);
            const uint32_t lead = (uint32_t)__shfl((int)key, first);
            const uint32_t same = (uint32_t)__popcll(__ballot(todo && key == lead));
            if (same > 32) {
                if (run_n && lead != run_label) {
                    if (lane == 0) atomicAdd(cnt + run_label, run_n);
                    run_n = 0;
                }
                run_label = lead;
                run_n += same;
            } else if (lane == first) {
                atomicAdd(cnt + lead, same);
            }
            if (key == lead) todo = false;
        }
        if (todo) atomicAdd(cnt + key, 1u);
    }
    if (run_n && lane == 0) atomicAdd(cnt + run_label, run_n);
}

__global__ __launch_bounds__(INST_THREADS) void inst_members_k(int P, int K, const uint32_t* __restrict__ sorted_vals,
                                                               const int32_t* __restrict__ member_ptr,
                                                               int32_t* __restrict__ member) {
    const uint32_t r = blockIdx.x * INST_THREADS + threadIdx.x;
    if (r >= (uint32_t)P) return;
    member[r] = r < (uint32_t)member_ptr[K] ? (int32_t)sorted_vals[r] : -1;
}

// Workspace: counts [K + 1] | the scan's scratch | the sort's buffers over the P rows
struct MembersView {
    uint32_t* cnt;
    uint32_t* scan_scratch;
    SortBufs sb;
};
size_t members_layout(int P, int K, char* base, MembersView* v) {
    Carver c(base);
    MembersView t;
    t.cnt = c.take<uint32_t>((size_t)K + 1);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words((size_t)K + 1));
    carve_sort(c, (size_t)P, &t.sb);
    if (v) *v = t;
    return c.bytes();
}

// ---- the statistics ------------------------------------------------------------------------------------------------------------------
// what a lane holds of a chunk's partial, or of an instance's total
struct Part {
    double m, f0, f1;   // this lane's moment (lanes 0 .. 9), channels l and l + 16
    uint32_t klo, khi;  // this lane's axis (lanes 0 .. 2): ord_enc keys of the smallest / largest coordinate
    int32_t hits;       // this lane's hit bit (lanes 0 .. 7)
};
__device__ __forceinline__ Part empty_part() {
    return Part{0.0, 0.0, 0.0, 0xFF800000u /* ord_enc(+inf) */, 0x007FFFFFu /* ord_enc(-inf) */, 0};
}

// member_ptr[k], member_ptr[k + 1] as a range inside member [P]
__device__ __forceinline__ void member_range(int P, const int32_t* __restrict__ member_ptr, int k, int* lo, int* hi) {
    *lo = min(max(member_ptr[k], 0), P);
    *hi = min(max(member_ptr[k + 1], *lo), P);
}

// the pivot of the instance whose members start at `lo` (0 where there is no valid first member)
__device__ __forceinline__ void load_pivot(int P, int lo, int hi, const int32_t* __restrict__ member, const float* __restrict__ xyz,
                                           float p[3]) {
    p[0] = p[1] = p[2] = 0.f;
    if (xyz && lo < hi) {
        const int32_t id = member[lo];
        if (id >= 0 && id < P) {
            p[0] = xyz[(size_t)id * 3];
            p[1] = xyz[(size_t)id * 3 + 1];
            p[2] = xyz[(size_t)id * 3 + 2];
        }
    }
}

// 1, dx, dy or dz
__device__ __forceinline__ double pick(int which, double dx, double dy, double dz) {
    return which == 0 ? 1.0 : which == 1 ? dx : which == 2 ? dy : dz;
}

// The partial of the chunk member[start .. start + count), count <= 256 and the same in the 16 lanes (header: chunk, MAPPING).
__device__ __forceinline__ Part walk_chunk(int P, int S, int l16, int start, int count, const int32_t* __restrict__ member,
                                           const float* __restrict__ xyz, const float* __restrict__ f,
                                           const float* __restrict__ weight, const uint8_t* __restrict__ hit, const float p[3]) {
    const bool has0 = f && l16 < S, has1 = f && l16 + INST_GROUP < S;
    // this lane's moment as (w * dA) * dB: W | Sd x y z | Sdd xx xy xz yy yz zz; lanes 10 .. 15 repeat W and are not read
    const int ia = l16 == 0 || l16 >= INST_MOMENTS ? 0 : l16 <= 3 ? l16 : l16 <= 6 ? 1 : l16 <= 8 ? 2 : 3;
    const int ib = l16 < 4 || l16 >= INST_MOMENTS ? 0 : l16 <= 6 ? l16 - 3 : l16 <= 8 ? l16 - 5 : 3;
    const int axis = min(l16, 2), bit = l16 & 7;
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    double am[4] = {0.0, 0.0, 0.0, 0.0}, a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
    Part out = empty_part();
    for (int base = 0; base < count; base += INST_GROUP) {
        // lane l fetches member base + l
        int32_t id = -1;
        float w = 1.f, x = 0.f, y = 0.f, z = 0.f;
        int h = 0;
        if (base + l16 < count) {
            id = member[start + base + l16];
            if (id >= 0 && id < P) {
                if (weight) w = weight[id];
                if (xyz) {
                    x = xyz[(size_t)id * 3];
                    y = xyz[(size_t)id * 3 + 1];
                    z = xyz[(size_t)id * 3 + 2];
                }
                if (hit) h = hit[id];
            } else {
                id = -1;
            }
        }
        const int nb = min(INST_GROUP, count - base);
        for (int b = 0; b < nb; b += 4) {  // (b + 3 <= 15: inside the batch; position base + b + u is u mod 4)
            int mid[4], mh[4];
            float mw[4], mx[4], my[4], mz[4], g0[4], g1[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                mid[u] = __shfl(id, b + u, INST_GROUP);
                mw[u] = __shfl(w, b + u, INST_GROUP);
                mx[u] = __shfl(x, b + u, INST_GROUP);
                my[u] = __shfl(y, b + u, INST_GROUP);
                mz[u] = __shfl(z, b + u, INST_GROUP);
                mh[u] = __shfl(h, b + u, INST_GROUP);
                const float* row = f + (size_t)max(mid[u], 0) * (size_t)S;
                g0[u] = has0 && mid[u] >= 0 ? row[l16] : 0.f;
                g1[u] = has1 && mid[u] >= 0 ? row[l16 + INST_GROUP] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (mid[u] < 0) continue;  // past the chunk's end, or an id outside the arrays
                const double wd = (double)mw[u];
                const double dx = (double)mx[u] - px, dy = (double)my[u] - py, dz = (double)mz[u] - pz;
                const double t = wd * pick(ia, dx, dy, dz);
                am[u] = am[u] + t * pick(ib, dx, dy, dz);
                a0[u] = a0[u] + wd * (double)g0[u];
                a1[u] = a1[u] + wd * (double)g1[u];
                out.hits += (mh[u] >> bit) & 1;
                const float c = axis == 0 ? mx[u] : axis == 1 ? my[u] : mz[u];
                if (c == c) {
                    const uint32_t key = ord_enc(c);
                    out.klo = min(out.klo, key);
                    out.khi = max(out.khi, key);
                }
            }
        }
    }
    out.m = (am[0] + am[2]) + (am[1] + am[3]);
    out.f0 = (a0[0] + a0[2]) + (a0[1] + a0[3]);
    out.f1 = (a1[0] + a1[2]) + (a1[1] + a1[3]);
    return out;
}

// total = total + partial (the floats), and the exact pieces
__device__ __forceinline__ void add_part(Part& total, const Part& part) {
    total.m = total.m + part.m;
    total.f0 = total.f0 + part.f0;
    total.f1 = total.f1 + part.f1;
    total.klo = min(total.klo, part.klo);
    total.khi = max(total.khi, part.khi);
    total.hits += part.hits;
}

struct StatsOut {
    int32_t *n, *hits;
    float *wsum, *centroid, *lo, *hi, *cov, *feature;
};

// the results of instance k from its totals (header: result); the 16 lanes together
__device__ __forceinline__ void write_results(int k, int S, int l16, int n, const Part& t, const float p[3], const StatsOut& o) {
    const double W = __shfl(t.m, 0, INST_GROUP);
    const bool live = W != 0.0;
    double mean[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double s = __shfl(t.m, 1 + a, INST_GROUP);
        mean[a] = live ? s / W : 0.0;
    }
    if (l16 == 0) {
        o.n[k] = n;
        o.wsum[k] = (float)W;
    }
    if (l16 >= 1 && l16 <= 3) o.centroid[(size_t)k * 3 + (l16 - 1)] = live ? (float)((double)p[l16 - 1] + mean[l16 - 1]) : 0.f;
    if (l16 >= 4 && l16 < INST_MOMENTS) {
        const int a = l16 <= 6 ? 0 : l16 <= 8 ? 1 : 2, b = l16 <= 6 ? l16 - 4 : l16 <= 8 ? l16 - 6 : 2;
        o.cov[(size_t)k * 6 + (l16 - 4)] = live ? (float)(t.m / W - mean[a] * mean[b]) : 0.f;
    }
    if (l16 < 3) {
        o.lo[(size_t)k * 3 + l16] = ord_dec(t.klo);
        o.hi[(size_t)k * 3 + l16] = ord_dec(t.khi);
    }
    if (l16 < 8) o.hits[(size_t)k * 8 + l16] = t.hits;
    if (o.feature) {
        if (l16 < S) o.feature[(size_t)k * S + l16] = live ? (float)(t.f0 / W) : 0.f;
        if (l16 + INST_GROUP < S) o.feature[(size_t)k * S + l16 + INST_GROUP] = live ? (float)(t.f1 / W) : 0.f;
    }
}

__global__ __launch_bounds__(INST_THREADS) void inst_small_k(int P, int K, int S, const int32_t* __restrict__ member_ptr,
                                                             const int32_t* __restrict__ member, const float* __restrict__ xyz,
                                                             const float* __restrict__ f, const float* __restrict__ weight,
                                                             const uint8_t* __restrict__ hit, StatsOut o) {
    const int l16 = threadIdx.x & (INST_GROUP - 1);
    const long long k64 = (long long)blockIdx.x * INST_GROUPS + threadIdx.x / INST_GROUP;
    if (k64 >= K) return;
    const int k = (int)k64;
    int lo, hi;
    member_range(P, member_ptr, k, &lo, &hi);
    if (hi - lo > INST_CHUNK) return;  // inst_chunks_k and inst_final_k
    float p[3];
    load_pivot(P, lo, hi, member, xyz, p);
    Part total = empty_part();
    add_part(total, walk_chunk(P, S, l16, lo, hi - lo, member, xyz, f, weight, hit, p));
    write_results(k, S, l16, hi - lo, total, p, o);
}

// slots[k] = the chunks of an instance of more than 256 members, 0 of any other; slots[K] = 0
__global__ __launch_bounds__(INST_THREADS) void inst_slots_k(int P, int K, const int32_t* __restrict__ member_ptr,
                                                             uint32_t* __restrict__ slots) {
    const long long k = (long long)blockIdx.x * INST_THREADS + threadIdx.x;
    if (k > K) return;
    uint32_t s = 0;
    if (k < K) {
        int lo, hi;
        member_range(P, member_ptr, (int)k, &lo, &hi);
        if (hi - lo > INST_CHUNK) s = (uint32_t)((hi - lo + INST_CHUNK - 1) / INST_CHUNK);
    }
    slots[k] = s;
}

// the slots of instance k inside the `cap` there are (wrong lists can ask for more: they get what there is)
__device__ __forceinline__ void slot_range(uint32_t cap, const uint32_t* __restrict__ slot_ptr, int k, uint32_t* lo, uint32_t* hi) {
    *lo = min(slot_ptr[k], cap);
    *hi = min(max(slot_ptr[k + 1], *lo), cap);
}

__global__ __launch_bounds__(INST_THREADS) void inst_chunks_k(int P, int K, int S, uint32_t cap, const int32_t* __restrict__ member_ptr,
                                                              const int32_t* __restrict__ member, const float* __restrict__ xyz,
                                                              const float* __restrict__ f, const float* __restrict__ weight,
                                                              const uint8_t* __restrict__ hit, const uint32_t* __restrict__ slot_ptr,
                                                              double* __restrict__ slot) {
    const int l16 = threadIdx.x & (INST_GROUP - 1);
    const uint32_t t = blockIdx.x * INST_GROUPS + threadIdx.x / INST_GROUP;
    if (t >= min(slot_ptr[K], cap)) return;
    // the last k with slot_ptr[k] <= t (slot_ptr[0] = 0): an instance with slots, because an instance without has the next one's start
    int a = 0, b = K;  // slot_ptr[a] <= t < slot_ptr[b]
    for (int it = 0; it < 32 && b - a > 1; it++) {
        const int mid = a + (b - a) / 2;
        if (slot_ptr[mid] <= t) a = mid;
        else b = mid;
    }
    const int k = a;
    int lo, hi;
    member_range(P, member_ptr, k, &lo, &hi);
    const long long start = (long long)lo + (long long)(t - slot_ptr[k]) * INST_CHUNK;
    const int count = start < hi ? (int)min((long long)INST_CHUNK, (long long)hi - start) : 0;
    float p[3];
    load_pivot(P, lo, hi, member, xyz, p);
    const Part part = walk_chunk(P, S, l16, count ? (int)start : lo, count, member, xyz, f, weight, hit, p);
    double* d = slot + (size_t)t * INST_SLOT_DOUBLES;
    uint32_t* words = reinterpret_cast<uint32_t*>(d + INST_MOMENTS + 32);
    if (l16 < INST_MOMENTS) d[l16] = part.m;
    d[INST_MOMENTS + l16] = part.f0;
    d[INST_MOMENTS + INST_GROUP + l16] = part.f1;
    if (l16 < 3) {
        words[l16] = part.klo;
        words[3 + l16] = part.khi;
    }
    if (l16 < 8) words[6 + l16] = (uint32_t)part.hits;
}

__global__ __launch_bounds__(INST_THREADS) void inst_final_k(int P, int K, int S, uint32_t cap, const int32_t* __restrict__ member_ptr,
                                                             const int32_t* __restrict__ member, const float* __restrict__ xyz,
                                                             const uint32_t* __restrict__ slot_ptr, const double* __restrict__ slot,
                                                             StatsOut o) {
    const int l16 = threadIdx.x & (INST_GROUP - 1);
    const long long k64 = (long long)blockIdx.x * INST_GROUPS + threadIdx.x / INST_GROUP;
    if (k64 >= K) return;
    const int k = (int)k64;
    int lo, hi;
    member_range(P, member_ptr, k, &lo, &hi);
    if (hi - lo <= INST_CHUNK) return;  // inst_small_k wrote it
    uint32_t s_lo, s_hi;
    slot_range(cap, slot_ptr, k, &s_lo, &s_hi);
    float p[3];
    load_pivot(P, lo, hi, member, xyz, p);
    Part total = empty_part();
    // ascending order, INST_AHEAD partials in flight: the loads of a batch are issued before the first of them is added
    for (uint32_t j0 = s_lo; j0 < s_hi; j0 += INST_AHEAD) {
        Part part[INST_AHEAD];
#pragma unroll
        for (int u = 0; u < INST_AHEAD; u++) {
            part[u] = empty_part();
            if (j0 + u < s_hi) {
                const double* d = slot + (size_t)(j0 + u) * INST_SLOT_DOUBLES;
                const uint32_t* words = reinterpret_cast<const uint32_t*>(d + INST_MOMENTS + 32);
                if (l16 < INST_MOMENTS) part[u].m = d[l16];
                part[u].f0 = d[INST_MOMENTS + l16];
                part[u].f1 = d[INST_MOMENTS + INST_GROUP + l16];
                if (l16 < 3) {
                    part[u].klo = words[l16];
                    part[u].khi = words[3 + l16];
                }
                if (l16 < 8) part[u].hits = (int32_t)words[6 + l16];
            }
        }
#pragma unroll
        for (int u = 0; u < INST_AHEAD; u++)
            if (j0 + u < s_hi) add_part(total, part[u]);
    }
    write_results(k, S, l16, hi - lo, total, p, o);
}

// Workspace: slot counts, then their scan [K + 1] | the scan's scratch | the slots
struct StatsView {
    uint32_t* slot_ptr;
    uint32_t* scan_scratch;
    double* slot;
};
size_t stats_layout(int P, int K, char* base, StatsView* v) {
    Carver c(base);
    StatsView t;
    t.slot_ptr = c.take<uint32_t>((size_t)K + 1);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words((size_t)K + 1));
    t.slot = c.take<double>(at_least_one(slot_capacity(P) * INST_SLOT_DOUBLES));
    if (v) *v = t;
    return c.bytes();
}

// P, K of both entries
int check_sizes(const char* fn, int P, int K) {
    if (P < 0) return fail(std::string(fn) + ": bad P");
    if (K < 0) return fail(std::string(fn) + ": bad K");
    if (P >= INST_MAX || K >= INST_MAX) return fail(std::string(fn) + ": need P < 2^30 and K < 2^30");
    return 0;
}
bool sizes_ok(int P, int K) { return P >= 0 && K >= 0 && P < INST_MAX && K < INST_MAX; }

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_instance_members_workspace_bytes(int P, int K) { return sizes_ok(P, K) ? members_layout(P, K, nullptr, nullptr) : 0; }

int goi_instance_members(int P, int K, const int32_t* label, int32_t* member_ptr, int32_t* member, void* workspace, void* stream) {
    const char* fn = "goi_instance_members";
    if (check_sizes(fn, P, K) < 0) return -1;
    if (!member_ptr || (P > 0 && (!label || !member))) return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned(label, 4) || misaligned(member_ptr, 4) || misaligned(member, 4))
        return fail(std::string(fn) + ": label, member_ptr and member must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {  // member_ptr [K + 1] = 0: every instance is empty
        GOI_HIP(hipMemsetAsync(member_ptr, 0, ((size_t)K + 1) * sizeof(int32_t), s));
        return 0;
    }
    if (check_workspace(fn, workspace) < 0) return -1;
    MembersView w;
    members_layout(P, K, static_cast<char*>(workspace), &w);
    GOI_HIP(hipMemsetAsync(w.cnt, 0, ((size_t)K + 1) * sizeof(uint32_t), s));
    inst_count_k<<<dim3(blocks_for(P, INST_THREADS * INST_ROWS)), dim3(INST_THREADS), 0, s>>>(P, K, label, w.sb.keys[0], w.sb.vals[0],
                                                                                             w.cnt);
    exclusive_scan_u32(w.cnt, nullptr, reinterpret_cast<uint32_t*>(member_ptr), (size_t)K + 1, nullptr, w.scan_scratch, s);
    // keys are 0 .. K: the bits that cover every id below K + 1
    const int fin = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)P, 0, tile_key_bits((uint32_t)K + 1u), w.sb.scratch, s);
    inst_members_k<<<dim3(blocks_for(P, INST_THREADS)), dim3(INST_THREADS), 0, s>>>(P, K, w.sb.vals[fin], member_ptr, member);
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_instance_stats_workspace_bytes(int P, int K) { return sizes_ok(P, K) ? stats_layout(P, K, nullptr, nullptr) : 0; }

int goi_instance_stats(int P, int K, int S, const int32_t* member_ptr, const int32_t* member, const float* xyz, const float* features,
                       const float* weight, const uint8_t* hit, int32_t* n, int32_t* hits, float* wsum, float* centroid, float* lo,
                       float* hi, float* cov, float* feature, void* workspace, void* stream) {
    const char* fn = "goi_instance_stats";
    if (check_sizes(fn, P, K) < 0) return -1;
    if (features && (S < 1 || S > 32)) return fail(std::string(fn) + ": need 1 <= S <= 32");
    if (K == 0) return 0;
    if (!member_ptr || !n || !hits || !wsum || !centroid || !lo || !hi || !cov || (features && !feature) || (P > 0 && !member))
        return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned(member_ptr, 4) || misaligned(member, 4) || misaligned(xyz, 4) || misaligned(features, 4) || misaligned(weight, 4) ||
        misaligned(n, 4) || misaligned(hits, 4) || misaligned(wsum, 4) || misaligned(centroid, 4) || misaligned(lo, 4) ||
        misaligned(hi, 4) || misaligned(cov, 4) || misaligned(feature, 4))
        return fail(std::string(fn) + ": every pointer but hit must be 4-byte aligned");
    if (check_workspace(fn, workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    StatsView w;
    stats_layout(P, K, static_cast<char*>(workspace), &w);
    const StatsOut o{n, hits, wsum, centroid, lo, hi, cov, features ? feature : nullptr};
    const dim3 per_instance(blocks_for(K, INST_GROUPS)), block(INST_THREADS);
    inst_small_k<<<per_instance, block, 0, s>>>(P, K, S, member_ptr, member, xyz, features, weight, hit, o);
    if (P > INST_CHUNK) {  // an instance of more than 256 members can exist
        const uint32_t cap = (uint32_t)slot_capacity(P);
        inst_slots_k<<<dim3(blocks_for((long long)K + 1, INST_THREADS)), block, 0, s>>>(P, K, member_ptr, w.slot_ptr);
        exclusive_scan_u32(w.slot_ptr, nullptr, w.slot_ptr, (size_t)K + 1, nullptr, w.scan_scratch, s);
        inst_chunks_k<<<dim3(blocks_for(cap, INST_GROUPS)), block, 0, s>>>(P, K, S, cap, member_ptr, member, xyz, features, weight, hit,
                                                                          w.slot_ptr, w.slot);
        inst_final_k<<<per_instance, block, 0, s>>>(P, K, S, cap, member_ptr, member, xyz, w.slot_ptr, w.slot, o);
    }
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
