// Instance segmentation of the Gaussians on their k-NN graph (goi_hyperplane_amd/segment.py): which edges
// of the graph JOIN their two rows, and the connected components of the joined graph.  idx [P,k] is what goi_knn_graph returns.
//
//   segment_edges_k   A LANE PER EDGE e = i * k + m, j = idx[e].  The cheap gates first (range and self, rows, labels, dist2,
//                     mutual: one pass over row j's k slots), then -- only for an edge that still stands -- the feature gate
//                         d = 0;  for c = 0 .. S-1 in order:  e_c = f[i,c] - f[j,c];  d = fmaf(e_c, e_c, d);     join iff d <= tau
//                     The two rows come in as 16-byte words where S is a multiple of 4 (and f is 16-byte aligned), as single
//                     floats otherwise: the SAME chain in both forms, one lane owns it from start to end, so the value does not
//                     depend on the launch geometry, and it is symmetric in (i, j) bit for bit ((-e)^2 = e^2).  The k edges of a
//                     row sit in neighbouring lanes, so row i is fetched from memory once.  This TU is compiled with
//                     -ffp-contract=off: the only fused operation is the fmaf that is written out.
//   segment_union_k   A lane per edge: a joining edge between two kept rows unites them, whichever endpoint lists it.  Union-find
//                     as in mesh.hip / dbscan.hip -- the larger root is hooked under the smaller with atomicCAS, so parents only
//                     decrease and the root of a finished tree is its component's smallest id, whatever the schedule -- plus PATH
//                     HALVING, because one component can hold every row: a walk writes the grandparent over the parent with
//                     atomicMin, which keeps the row in its tree and the parents decreasing.  Every walk and every retry loop
//                     is bounded; an overrun raises GOI_SEGMENT_STATUS_UNION instead of spinning.
//   segment_roots_k   root[i] = find_root (wave_util.h) of a kept row after a few rounds of pointer jumping (a tree can still be a
//                     chain of n), -1 of any other row, and the component sizes by integer atomics:
//                     the lanes of a wave that hold the same root are combined first (ballot + popcount), so ONE giant component
//                     costs an atomic per wave, not per row.
//   segment_sizes_k   size[i], and flag[i] = i is a root whose component is kept (size >= min_size)
//   exclusive_scan_u32 over the flags: the dense rank of every kept root in ascending root order, and C
//   segment_labels_k  label[i] = rank[root[i]] of a kept component, -1 otherwise
//
// Stages are separated by kernel boundaries, no workgroup waits for another, no float atomics, nothing is read back, every store
// is an ordinary vector store.  C entries at the end of the file: goi_knn_segment_edges, goi_knn_segment_components.
#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int SG_THREADS = 256;
constexpr long long SG_MAX_ENTRIES = 1ll << 30;  // P * k below this: flat edge numbers fit a uint32 with room to spare
constexpr uint32_t SG_UNION = GOI_SEGMENT_STATUS_UNION;

unsigned blocks_for(long long n) { return (unsigned)((n + SG_THREADS - 1) / SG_THREADS); }

// ---- the edge gate -----------------------------------------------------------------------------------------------------------------
// d of the header over two rows; VEC: the rows are read as S / 4 float4 words
template <bool VEC>
__device__ __forceinline__ float row_dist2(const float* __restrict__ a, const float* __restrict__ b, int S) {
    float d = 0.f;
    if (VEC) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll 4
        for (int q = 0; q < (S >> 2); q++) {
            const float4 x = a4[q], y = b4[q];
            const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z, e3 = x.w - y.w;
            d = fmaf(e0, e0, d);
            d = fmaf(e1, e1, d);
            d = fmaf(e2, e2, d);
            d = fmaf(e3, e3, d);
        }
    } else {
#pragma unroll 4
        for (int c = 0; c < S; c++) {
            const float e = a[c] - b[c];
            d = fmaf(e, e, d);
        }
    }
    return d;
}

template <bool VEC>
__global__ __launch_bounds__(SG_THREADS) void segment_edges_k(int P, int S, int k, uint32_t n, const int32_t* __restrict__ idx,
                                                              const float* __restrict__ f, float tau,
                                                              const float* __restrict__ dist2, float max_dist2,
                                                              const int64_t* __restrict__ labels, const uint8_t* __restrict__ rows,
                                                              int mutual, uint8_t* __restrict__ join) {
    const uint32_t e = blockIdx.x * SG_THREADS + threadIdx.x;
    if (e >= n) return;
    const int i = (int)(e / (uint32_t)k);
    const int32_t j = idx[e];
    bool ok = j >= 0 && j < P && j != i;
    if (ok && rows) ok = rows[i] != 0 && rows[j] != 0;
    if (ok && labels) {
        const int64_t li = labels[i];
        ok = li >= 0 && li == labels[j];
    }
    if (ok && dist2) ok = dist2[e] <= max_dist2;
    if (ok && mutual) {
        const int32_t* back = idx + (size_t)j * (size_t)k;
        bool found = false;
        for (int m = 0; m < k; m++) found = found || back[m] == i;
        ok = found;
    }
    if (ok && f) ok = row_dist2<VEC>(f + (size_t)i * (size_t)S, f + (size_t)j * (size_t)S, S) <= tau;  // (a NaN d never joins)
    join[e] = ok ? 1 : 0;
}

// ---- union-find ----------------------------------------------------------------------------------------------------------------------
// The root of x, shortening the path on the way: x's parent becomes its grandparent (atomicMin: another lane may have moved it
// further down already, and a parent never goes up).  Only a row that is NOT a root is written, and such a row never becomes a
// root again, so the atomicCAS of unite -- which only ever replaces a root's self-link -- is not disturbed.  The walk ends within
// n steps (a guard that is never reached: parents only decrease); overrunning it raises SG_UNION.
__device__ __forceinline__ uint32_t find_root_halving(uint32_t* parent, uint32_t x, uint32_t n, uint32_t* status) {
    for (uint32_t it = 0; it <= n; it++) {
        const uint32_t p = load_parent(parent, x);
        if (p == x) return x;
        const uint32_t g = load_parent(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = g;
    }
    atomicOr(status, SG_UNION);
    return x;
}

__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t n, uint32_t* status) {
    for (uint32_t it = 0;; it++) {
        uint32_t ra = find_root_halving(parent, a, n, status), rb = find_root_halving(parent, b, n, status);
        if (ra == rb) return;
        if (ra > rb) {
            const uint32_t t = ra;
            ra = rb;
            rb = t;
        }
        if (atomicCAS(parent + rb, rb, ra) == rb) return;  // a failed CAS: that root was hooked meanwhile (at most n unions)
        a = ra;  // both are ancestors still: start the next walk from them
        b = rb;
        if (it >= n) {
            atomicOr(status, SG_UNION);
            return;
        }
    }
}

__global__ __launch_bounds__(SG_THREADS) void segment_init_k(uint32_t P, uint32_t* __restrict__ parent, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= P) return;
    parent[i] = i;
    cnt[i] = 0;
}

__global__ __launch_bounds__(SG_THREADS) void segment_union_k(int P, int k, uint32_t n, const int32_t* __restrict__ idx,
                                                              const uint8_t* __restrict__ join, const uint8_t* __restrict__ rows,
                                                              uint32_t* parent, uint32_t* __restrict__ status) {
    const uint32_t e = blockIdx.x * SG_THREADS + threadIdx.x;
    if (e >= n) return;
    if (join && !join[e]) return;
    const int i = (int)(e / (uint32_t)k);
    const int32_t j = idx[e];
    if (j < 0 || j >= P || j == i) return;
    if (rows && (!rows[i] || !rows[j])) return;
    unite(parent, (uint32_t)i, (uint32_t)j, (uint32_t)P, status);
}

// After the unions (a kernel boundary earlier) a tree can still be one long chain -- a path listed from its far end hooks row
// after row without a walk ever crossing it -- and a plain walk from every row of a chain of n is n^2 / 2 steps.  So every row
// first JUMPS: its own parent becomes its grandparent, again and again, which halves its depth per round when the rows of the
// chain jump together (log2 n rounds).  The rounds are an optimisation with a small fixed bound; the walk that follows
// (find_root, bounded by n, with the status bit) is what the result rests on.
__device__ __forceinline__ void shorten(uint32_t* parent, uint32_t x) {
    for (int round = 0; round < 64; round++) {
        const uint32_t p = load_parent(parent, x);
        const uint32_t g = load_parent(parent, p);
        if (g == p) return;
        atomicMin(parent + x, g);
    }
}

// root[i], and cnt[root] += the number of this wave's lanes that hold the same root: one atomic per distinct root of a wave
__global__ __launch_bounds__(SG_THREADS) void segment_roots_k(uint32_t P, const uint8_t* __restrict__ rows, uint32_t* parent,
                                                              int32_t* __restrict__ root, uint32_t* cnt,
                                                              uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
    const bool kept = i < P && (!rows || rows[i]);
    uint32_t r = 0;
    if (kept) {
        shorten(parent, i);
        r = find_root(parent, i, P, status, SG_UNION);
    }
    if (i < P) root[i] = kept ? (int32_t)r : -1;
    bool todo = kept;
    for (int round = 0; round < 64; round++) {  // (a wave holds at most 64 distinct roots)
        const unsigned long long open = __ballot(todo);
        if (!open) break;
        const int first = __builtin_ctzll(open);
        const uint32_t lead = (uint32_t)__shfl((int)r, first);
        const unsigned long long same = __ballot(todo && r == lead);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(cnt + lead, (uint32_t)__popcll(same));
        if (r == lead) todo = false;
    }
}

__global__ __launch_bounds__(SG_THREADS) void segment_sizes_k(uint32_t P, uint32_t min_size, const int32_t* __restrict__ root,
                                                              const uint32_t* __restrict__ cnt, int32_t* __restrict__ size,
                                                              uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= P) return;
    const int32_t r = root[i];
    const uint32_t c = r >= 0 ? cnt[r] : 0u;
    size[i] = (int32_t)c;
    flag[i] = (r == (int32_t)i && c >= min_size) ? 1u : 0u;
}

__global__ __launch_bounds__(SG_THREADS) void segment_labels_k(uint32_t P, uint32_t min_size, const int32_t* __restrict__ root,
                                                               const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ rank,
                                                               int32_t* __restrict__ label) {
    const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= P) return;
    const int32_t r = root[i];
    label[i] = (r >= 0 && cnt[r] >= min_size) ? (int32_t)rank[r] : -1;
}

// Workspace: parents [P] | component sizes by root [P] | kept-root flags, then their ranks [P] | the scan's scratch
struct ComponentsView {
    uint32_t *parent, *cnt, *rank, *scan_scratch;
};
size_t components_layout(int P, char* base, ComponentsView* v) {
    Carver c(base);
    ComponentsView t;
    t.parent = c.take<uint32_t>(at_least_one((size_t)P));
    t.cnt = c.take<uint32_t>(at_least_one((size_t)P));
    t.rank = c.take<uint32_t>(at_least_one((size_t)P));
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words(at_least_one((size_t)P)));
    if (v) *v = t;
    return c.bytes();
}

// P, k of both entries: P * k has to stay below 2^30
int check_graph(const char* fn, int P, int k) {
    if (P < 0) return fail(std::string(fn) + ": bad P");
    if (k < 1) return fail(std::string(fn) + ": need k >= 1");
    if ((long long)P * k >= SG_MAX_ENTRIES) return fail(std::string(fn) + ": need P * k < 2^30");
    return 0;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_knn_segment_edges(int P, int S, int k, const int32_t* idx, const float* features, float tau, const float* dist2,
                          float max_dist2, int flags, const int64_t* labels, const uint8_t* rows, uint8_t* join, void* stream) {
    const char* fn = "goi_knn_segment_edges";
    if (check_graph(fn, P, k) < 0) return -1;
    if (features && (S < 1 || S > 32)) return fail(std::string(fn) + ": need 1 <= S <= 32");
    if (tau != tau) return fail(std::string(fn) + ": tau is NaN");
    if (flags & ~(GOI_SEGMENT_MUTUAL | GOI_SEGMENT_MAX_DIST2)) return fail(std::string(fn) + ": unknown flags");
    const bool cut = (flags & GOI_SEGMENT_MAX_DIST2) != 0;
    if (cut && !dist2) return fail(std::string(fn) + ": max_dist2 needs dist2");
    if (cut && max_dist2 != max_dist2) return fail(std::string(fn) + ": max_dist2 is NaN");
    if (P == 0) return 0;
    if (!idx || !join) return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned(idx, 4) || misaligned(features, 4) || misaligned(dist2, 4) || misaligned(labels, 8))
        return fail(std::string(fn) + ": idx, features and dist2 must be 4-byte aligned, labels 8-byte aligned");
    const uint32_t n = (uint32_t)P * (uint32_t)k;
    const dim3 grid(blocks_for(n)), block(SG_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* d2 = cut ? dist2 : nullptr;
    const int mutual = (flags & GOI_SEGMENT_MUTUAL) ? 1 : 0;
    if (features && (S & 3) == 0 && !misaligned(features, 16))
        segment_edges_k<true><<<grid, block, 0, s>>>(P, S, k, n, idx, features, tau, d2, max_dist2, labels, rows, mutual, join);
    else
        segment_edges_k<false><<<grid, block, 0, s>>>(P, S, k, n, idx, features, tau, d2, max_dist2, labels, rows, mutual, join);
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_knn_segment_components_workspace_bytes(int P, int k) {
    return P >= 0 && k >= 1 && (long long)P * k < SG_MAX_ENTRIES ? components_layout(P, nullptr, nullptr) : 0;
}

int goi_knn_segment_components(int P, int k, const int32_t* idx, const uint8_t* join, const uint8_t* rows, int min_size,
                               int32_t* root, int32_t* size, int32_t* label, int32_t* count, int32_t* status, void* workspace,
                               void* stream) {
    const char* fn = "goi_knn_segment_components";
    if (check_graph(fn, P, k) < 0) return -1;
    if (min_size < 1) return fail(std::string(fn) + ": need min_size >= 1");
    if (P == 0) return 0;
    if (!idx || !root || !size || !label || !count || !status) return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned(idx, 4) || misaligned(root, 4) || misaligned(size, 4) || misaligned(label, 4) || misaligned(count, 4) ||
        misaligned(status, 4))
        return fail(std::string(fn) + ": idx, root, size, label, count and status must be 4-byte aligned");
    if (check_workspace(fn, workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ComponentsView w;
    components_layout(P, static_cast<char*>(workspace), &w);
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    const uint32_t n = (uint32_t)P * (uint32_t)k;
    const dim3 rows_grid(blocks_for(P)), block(SG_THREADS);
    GOI_HIP(hipMemsetAsync(st, 0, sizeof(uint32_t), s));
    segment_init_k<<<rows_grid, block, 0, s>>>((uint32_t)P, w.parent, w.cnt);
    segment_union_k<<<dim3(blocks_for(n)), block, 0, s>>>(P, k, n, idx, join, rows, w.parent, st);
    segment_roots_k<<<rows_grid, block, 0, s>>>((uint32_t)P, rows, w.parent, root, w.cnt, st);
    segment_sizes_k<<<rows_grid, block, 0, s>>>((uint32_t)P, (uint32_t)min_size, root, w.cnt, size, w.rank);
    exclusive_scan_u32(w.rank, nullptr, w.rank, (size_t)P, reinterpret_cast<uint32_t*>(count), w.scan_scratch, s);
    segment_labels_k<<<rows_grid, block, 0, s>>>((uint32_t)P, (uint32_t)min_size, root, w.cnt, w.rank, label);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
