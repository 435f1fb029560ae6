// Neighbour consistency of per-Gaussian features on a k-NN graph (goi_hyperplane_amd/smooth.py):
//
//     L = (1 / N_E) sum over counting edges (i, m) of w[i,m] sum_c (f[i,c] - f[idx[i,m],c])^2
//
// its gradient with respect to f, and one Jacobi step of feature diffusion over the same graph.  idx [P,k] is what goi_knn_graph
// returns; entry (i, m) is an EDGE iff 0 <= idx[i,m] < P (goi_knn_majority's rule), and an edge COUNTS iff rows[i] != 0.
//
//   knn_in_degree_k, knn_in_edges_k   The transpose of the graph: integer atomics count the edges that point at every row, an
//                    exclusive scan of the counts is in_ptr, and a stable radix sort of (key = target, value = flat edge number)
//                    over just the key bits P needs puts the edge numbers in ascending (target, edge) order.  A skipped entry
//                    gets key P, above every target, so it lands behind all edges and disturbs none of them.
//   smooth_count_k   N_E, by integer atomics (one per workgroup), so that the scale 2 / N_E is known before the gradient is
//                    written.
//   smooth_loss_k    A QUARTER WAVE (16 lanes) owns a row; lane l holds channels l and l + 16, so a neighbour's row of S <= 32
//                    floats is read as one coalesced segment of at most 128 bytes.  The lists of a row -- its k out-slots, then
//                    its in-list in stored order -- go through the same loop, 16 entries at a time: lane l fetches entry l
//                    (other row, weight, counts or not), the entries are then broadcast in order.  An in-list of any length is
//                    just more batches.  Per gradient element: acc = 0; for each counting edge in that order t = f[a,c] -
//                    f[other,c], acc = acc + w * t; then acc * scale -- every operation rounded once (this TU is compiled with
//                    -ffp-contract=off).  The row's loss is summed in fp32 in slot order, rows and workgroups in float64 in a
//                    fixed order (a group's rows ascending, the groups of a workgroup in order, smooth_final_k the workgroups).
//   knn_diffuse_k    the same mapping over the out-lists only: a pure gather.
//
// No float atomics, no read-back, every store an ordinary vector store.  What a caller hands in as in_ptr / in_edge is clamped to
// the arrays before it is used: a wrong transpose gives a wrong gradient, never an access outside idx, weight, rows or f.
// C entries at the end of the file: goi_knn_transpose, goi_knn_smooth_loss, goi_knn_diffuse (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_GROUP = 16;                        // lanes per row: a quarter wave
constexpr int SM_GROUPS = SM_THREADS / SM_GROUP;    // rows a workgroup works on at a time
constexpr int SM_MAX_BLOCKS = 2048;                 // the grid of the persistent row loops = the partials smooth_final_k sums
constexpr int SM_COUNT_BLOCKS = 1024;               // the grid of smooth_count_k = its atomics on the one N_E word
constexpr long long SM_MAX_ENTRIES = 1ll << 30;     // P * k below this: the sort's limit, and flat edge numbers fit an int32

// ---- the transpose ---------------------------------------------------------------------------------------------------------------
// keys[e] = target of entry e (P for a skipped one), vals[e] = e, deg[target]++ (deg [P + 1], zeroed; deg[P] stays 0)
__global__ __launch_bounds__(SM_THREADS) void knn_in_degree_k(int P, uint32_t n, const int32_t* __restrict__ idx,
                                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                              uint32_t* __restrict__ deg) {
    const uint32_t e = blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= n) return;
    const int32_t j = idx[e];
    const bool edge = j >= 0 && j < P;
    keys[e] = edge ? (uint32_t)j : (uint32_t)P;
    vals[e] = e;
    if (edge) atomicAdd(&deg[j], 1u);
}

// in_edge[r] = the r-th sorted edge number, -1 from in_ptr[P] (the number of edges) on
__global__ __launch_bounds__(SM_THREADS) void knn_in_edges_k(int P, uint32_t n, const uint32_t* __restrict__ sorted_vals,
                                                             const int32_t* __restrict__ in_ptr, int32_t* __restrict__ in_edge) {
    const uint32_t r = blockIdx.x * SM_THREADS + threadIdx.x;
    if (r >= n) return;
    in_edge[r] = r < (uint32_t)in_ptr[P] ? (int32_t)sorted_vals[r] : -1;
}

// Workspace: in-degrees [P + 1] | the scan's scratch | the sort's buffers over the P * k entries
struct TransposeView {
    uint32_t* deg;
    uint32_t* scan_scratch;
    SortBufs sb;
};
size_t transpose_layout(int P, int k, char* base, TransposeView* v) {
    Carver c(base);
    TransposeView t;
    t.deg = c.take<uint32_t>((size_t)P + 1);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words((size_t)P + 1));
    carve_sort(c, (size_t)P * (size_t)k, &t.sb);
    if (v) *v = t;
    return c.bytes();
}

void launch_transpose(int P, int k, const int32_t* idx, int32_t* in_ptr, int32_t* in_edge, void* workspace, hipStream_t s) {
    TransposeView w;
    transpose_layout(P, k, static_cast<char*>(workspace), &w);
    const uint32_t n = (uint32_t)P * (uint32_t)k;
    const dim3 grid((n + SM_THREADS - 1) / SM_THREADS), block(SM_THREADS);
    (void)hipMemsetAsync(w.deg, 0, ((size_t)P + 1) * sizeof(uint32_t), s);
    knn_in_degree_k<<<grid, block, 0, s>>>(P, n, idx, w.sb.keys[0], w.sb.vals[0], w.deg);
    exclusive_scan_u32(w.deg, nullptr, reinterpret_cast<uint32_t*>(in_ptr), (size_t)P + 1, nullptr, w.scan_scratch, s);
    // keys are 0 .. P: the bits that cover every id below P + 1
    const int fin = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)n, 0, tile_key_bits((uint32_t)P + 1u), w.sb.scratch, s);
    knn_in_edges_k<<<grid, block, 0, s>>>(P, n, w.sb.vals[fin], in_ptr, in_edge);
}

// ---- what the row loops share ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float group_sum(float v) {  // over the 16 lanes of a quarter wave, offsets 8, 4, 2, 1: every lane gets it
#pragma unroll
    for (int o = SM_GROUP / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, SM_GROUP);
    return v;
}

// One entry of a row's list as the lane that fetched it holds it: the other row (the own row where `use` is false, so that its
// load is always inside f), the weight, and whether the entry takes part.
struct Entry {
    int other;
    float w;
    bool use;
};

// entry `m` of row a's out-list
__device__ __forceinline__ Entry out_entry(int P, int k, int a, int m, const int32_t* __restrict__ idx,
                                           const float* __restrict__ weight) {
    Entry en{a, 0.f, false};
    if (m < k) {
        const size_t e = (size_t)a * (size_t)k + (size_t)m;
        const int32_t j = idx[e];
        if (j >= 0 && j < P) {
            en.other = j;
            en.w = weight ? weight[e] : 1.0f;
            en.use = true;
        }
    }
    return en;
}

// Walks `count` entries, 16 at a time: lane `l16` fetches entry base + l16 with fetch(position), then every entry is handed to
// visit(w, o0, o1) in order with the other row's two channels of this lane.  count is the same for the 16 lanes, and fetch
// answers a position at or past count with an entry that takes no part.  Four rows are in flight at a time: the loads of four
// entries are issued before the first of them is used (a load that is not used reads the own row).
template <class Fetch, class Visit>
__device__ __forceinline__ void walk_list(int count, int l16, int S, const float* __restrict__ f, Fetch fetch, Visit visit) {
    const bool has0 = l16 < S, has1 = l16 + SM_GROUP < S;
    for (int base = 0; base < count; base += SM_GROUP) {
        const Entry mine = fetch(base + l16);
        const int nb = min(SM_GROUP, count - base);
        for (int b = 0; b < nb; b += 4) {  // (b + 3 <= 15: inside the batch)
            float w[4], o0[4], o1[4];
            int use[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int other = __shfl(mine.other, b + u, SM_GROUP);
                w[u] = __shfl(mine.w, b + u, SM_GROUP);
                use[u] = __shfl((int)mine.use, b + u, SM_GROUP);
                const float* row = f + (size_t)other * (size_t)S;
                o0[u] = has0 ? row[l16] : 0.f;
                o1[u] = has1 ? row[l16 + SM_GROUP] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (use[u]) visit(w[u], o0[u], o1[u]);
        }
    }
}

__global__ __launch_bounds__(SM_THREADS) void smooth_count_k(int P, int k, uint32_t n, const int32_t* __restrict__ idx,
                                                             const uint8_t* __restrict__ rows,
                                                             unsigned long long* __restrict__ n_edges) {
    __shared__ uint32_t s_wave[SM_THREADS / 64];
    uint32_t mine = 0;  // (a workgroup sees fewer than 2^30 entries)
    for (uint32_t e = blockIdx.x * SM_THREADS + threadIdx.x; e < n; e += gridDim.x * SM_THREADS) {
        const int32_t j = idx[e];
        mine += (j >= 0 && j < P && (!rows || rows[e / (uint32_t)k])) ? 1u : 0u;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    // ONE atomic per workgroup: thousands of waves adding to the one word serialise (measured: 8192 adds, 0.1 ms)
    if (threadIdx.x == 0) {
        const uint32_t all = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (all) atomicAdd(n_edges, (unsigned long long)all);
    }
}

// partial[blockIdx.x] = the float64 sum of the row losses of this workgroup's rows; grad (may be NULL) [P,S]
__global__ __launch_bounds__(SM_THREADS) void smooth_loss_k(int P, int S, int k, const float* __restrict__ f,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                            const uint8_t* __restrict__ rows, const int32_t* __restrict__ in_ptr,
                                                            const int32_t* __restrict__ in_edge,
                                                            const unsigned long long* __restrict__ n_edges,
                                                            float* __restrict__ grad, double* __restrict__ partial) {
    __shared__ double s_part[SM_GROUPS];
    const int l16 = threadIdx.x & (SM_GROUP - 1), grp = threadIdx.x / SM_GROUP;
    const bool has0 = l16 < S, has1 = l16 + SM_GROUP < S;
    const unsigned long long ne = *n_edges;
    const float scale = ne ? (float)(2.0 / (double)ne) : 0.f;  // formed in float64, rounded once
    const int n = P * k;  // (below 2^30: the entry checks)
    double total = 0.0;
    for (long long a64 = (long long)blockIdx.x * SM_GROUPS + grp; a64 < P; a64 += (long long)gridDim.x * SM_GROUPS) {
        const int a = (int)a64;
        const float* self = f + (size_t)a * (size_t)S;
        const float f0 = has0 ? self[l16] : 0.f, f1 = has1 ? self[l16 + SM_GROUP] : 0.f;
        float acc0 = 0.f, acc1 = 0.f, row_loss = 0.f;
        if (!rows || rows[a]) {  // the out-list counts with the row itself
            walk_list(k, l16, S, f, [&](int m) { return out_entry(P, k, a, m, idx, weight); },
                      [&](float w, float o0, float o1) {
                          const float t0 = f0 - o0, t1 = f1 - o1;
                          acc0 = acc0 + w * t0;
                          acc1 = acc1 + w * t1;
                          float q = t0 * t0;
                          if (S > SM_GROUP) q = q + t1 * t1;
                          row_loss = row_loss + w * group_sum(q);
                      });
            total += (double)row_loss;
        }
        if (grad) {
            const int lo = min(max(in_ptr[a], 0), n), hi = min(max(in_ptr[a + 1], lo), n);
            walk_list(hi - lo, l16, S, f,
                      [&](int r) {
                          Entry en{a, 0.f, false};
                          if (r < hi - lo) {
                              const int32_t e = in_edge[lo + r];
                              if (e >= 0 && e < n) {
                                  const int i = e / k;
                                  if (!rows || rows[i]) {
                                      en.other = i;
                                      en.w = weight ? weight[e] : 1.0f;
                                      en.use = true;
                                  }
                              }
                          }
                          return en;
                      },
                      [&](float w, float o0, float o1) {
                          const float t0 = f0 - o0, t1 = f1 - o1;
                          acc0 = acc0 + w * t0;
                          acc1 = acc1 + w * t1;
                      });
            float* g = grad + (size_t)a * (size_t)S;
            if (has0) g[l16] = acc0 * scale;
            if (has1) g[l16 + SM_GROUP] = acc1 * scale;
        }
    }
    if (l16 == 0) s_part[grp] = total;  // (every lane of a group holds the same sums)
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < SM_GROUPS; i++) sum += s_part[i];
        partial[blockIdx.x] = sum;
    }
}

// *loss = float(sum of the partials / N_E), 0 when N_E = 0: thread t adds partials t, t + 256, ... in order, then the wave
// butterfly, then the four waves in order
__global__ __launch_bounds__(SM_THREADS) void smooth_final_k(int nblk, const double* __restrict__ partial,
                                                             const unsigned long long* __restrict__ n_edges,
                                                             float* __restrict__ loss) {
    __shared__ double s_wave[SM_THREADS / 64];
    double sum = 0.0;
    for (int i = threadIdx.x; i < nblk; i += SM_THREADS) sum += partial[i];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long ne = *n_edges;
        const double all = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        *loss = ne ? (float)(all / (double)ne) : 0.f;
    }
}

int row_blocks(int P) { return min((P + SM_GROUPS - 1) / SM_GROUPS, SM_MAX_BLOCKS); }

// Workspace of the loss: the per-workgroup partial sums
size_t smooth_layout(char* base, double** partial) {
    Carver c(base);
    double* p = c.take<double>(SM_MAX_BLOCKS);
    if (partial) *partial = p;
    return c.bytes();
}

// ---- one Jacobi step of diffusion over the out-lists ---------------------------------------------------------------------------
// W = sum w (slot order), m[c] = (sum w * f[j,c]) / W, out = f + lam * (m - f); a fixed row, a row without an edge and a row with
// W == 0 are copied
__global__ __launch_bounds__(SM_THREADS) void knn_diffuse_k(int P, int S, int k, const float* __restrict__ f,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                            const uint8_t* __restrict__ fixed, float lam, float* __restrict__ out) {
    const int l16 = threadIdx.x & (SM_GROUP - 1), grp = threadIdx.x / SM_GROUP;
    const bool has0 = l16 < S, has1 = l16 + SM_GROUP < S;
    for (long long a64 = (long long)blockIdx.x * SM_GROUPS + grp; a64 < P; a64 += (long long)gridDim.x * SM_GROUPS) {
        const int a = (int)a64;
        const float* self = f + (size_t)a * (size_t)S;
        const float f0 = has0 ? self[l16] : 0.f, f1 = has1 ? self[l16 + SM_GROUP] : 0.f;
        float r0 = f0, r1 = f1;
        if (!fixed || !fixed[a]) {
            float wsum = 0.f, acc0 = 0.f, acc1 = 0.f;
            int edges = 0;
            walk_list(k, l16, S, f, [&](int m) { return out_entry(P, k, a, m, idx, weight); },
                      [&](float w, float o0, float o1) {
                          wsum = wsum + w;
                          acc0 = acc0 + w * o0;
                          acc1 = acc1 + w * o1;
                          edges++;
                      });
            if (edges > 0 && wsum != 0.f) {
                const float m0 = acc0 / wsum, m1 = acc1 / wsum;
                r0 = f0 + lam * (m0 - f0);
                r1 = f1 + lam * (m1 - f1);
            }
        }
        float* o = out + (size_t)a * (size_t)S;
        if (has0) o[l16] = r0;
        if (has1) o[l16 + SM_GROUP] = r1;
    }
}

// P, S, k of every entry; `entries`: P * k has to stay below 2^30
int check_shape(const char* fn, int P, int S, int k) {
    if (P < 0) return fail(std::string(fn) + ": bad P");
    if (S < 1 || S > 32) return fail(std::string(fn) + ": need 1 <= S <= 32");
    if (k < 1) return fail(std::string(fn) + ": need k >= 1");
    if ((long long)P * k >= SM_MAX_ENTRIES) return fail(std::string(fn) + ": need P * k < 2^30");
    return 0;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_knn_transpose_workspace_bytes(int P, int k) {
    return P >= 0 && k >= 1 && (long long)P * k < SM_MAX_ENTRIES ? transpose_layout(P, k, nullptr, nullptr) : 0;
}

int goi_knn_transpose(int P, int k, const int32_t* idx, int32_t* in_ptr, int32_t* in_edge, void* workspace, void* stream) {
    if (check_shape("goi_knn_transpose", P, 1, k) < 0) return -1;
    if (!in_ptr || (P > 0 && (!idx || !in_edge))) return fail("goi_knn_transpose: a required pointer is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {  // in_ptr [1] = 0: no edges
        GOI_HIP(hipMemsetAsync(in_ptr, 0, sizeof(int32_t), s));
        return 0;
    }
    if (check_workspace("goi_knn_transpose", workspace) < 0) return -1;
    launch_transpose(P, k, idx, in_ptr, in_edge, workspace, s);
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_knn_smooth_loss_workspace_bytes(int P) { return P >= 0 ? smooth_layout(nullptr, nullptr) : 0; }

int goi_knn_smooth_loss(int P, int S, int k, const float* f, const int32_t* idx, const float* weight, const uint8_t* rows,
                        const int32_t* in_ptr, const int32_t* in_edge, float* loss, long long* n_edges, float* grad,
                        void* workspace, void* stream) {
    if (check_shape("goi_knn_smooth_loss", P, S, k) < 0) return -1;
    if (!loss || !n_edges || (P > 0 && (!f || !idx || (grad && (!in_ptr || !in_edge)))))
        return fail("goi_knn_smooth_loss: a required pointer is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {  // L = 0, N_E = 0, no gradient row
        GOI_HIP(hipMemsetAsync(n_edges, 0, sizeof(long long), s));
        GOI_HIP(hipMemsetAsync(loss, 0, sizeof(float), s));
        return 0;
    }
    if (check_workspace("goi_knn_smooth_loss", workspace) < 0) return -1;
    GOI_HIP(hipMemsetAsync(n_edges, 0, sizeof(long long), s));
    double* partial;
    smooth_layout(static_cast<char*>(workspace), &partial);
    unsigned long long* ne = reinterpret_cast<unsigned long long*>(n_edges);
    const uint32_t n = (uint32_t)P * (uint32_t)k;
    const int nblk = row_blocks(P);
    smooth_count_k<<<dim3(min((n + SM_THREADS - 1) / SM_THREADS, (uint32_t)SM_COUNT_BLOCKS)), dim3(SM_THREADS), 0, s>>>(P, k, n, idx, rows,
                                                                                                                        ne);
    smooth_loss_k<<<dim3(nblk), dim3(SM_THREADS), 0, s>>>(P, S, k, f, idx, weight, rows, in_ptr, in_edge, ne, grad, partial);
    smooth_final_k<<<dim3(1), dim3(SM_THREADS), 0, s>>>(nblk, partial, ne, loss);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_knn_diffuse(int P, int S, int k, const float* f, const int32_t* idx, const float* weight, const uint8_t* fixed, float lam,
                    float* out, void* stream) {
    if (check_shape("goi_knn_diffuse", P, S, k) < 0) return -1;
    if (lam != lam) return fail("goi_knn_diffuse: lam is NaN");
    if (P == 0) return 0;
    if (!f || !idx || !out) return fail("goi_knn_diffuse: a required pointer is NULL");
    if (f == out) return fail("goi_knn_diffuse: out must not be f (a Jacobi step reads the old values of every row)");
    knn_diffuse_k<<<dim3(row_blocks(P)), dim3(SM_THREADS), 0, static_cast<hipStream_t>(stream)>>>(P, S, k, f, idx, weight, fixed, lam,
                                                                                                 out);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
