// Exact DBSCAN on the device: sklearn.cluster.DBSCAN(eps, min_samples).fit(X) with the Euclidean metric, the step
// gui/main.py:1595-1665 (group_points) runs on the host.  The definition this file computes:
//   * j is a neighbour of i when d2(i, j) <= eps32 * eps32 (i is its own neighbour), where ALWAYS
//         dx = xi - xj; dy = yi - yj; dz = zi - zj;  d2 = fma(dz, dz, fma(dy, dy, dx * dx))
//     in fp32 (this TU is compiled with -ffp-contract=off so that the spelling is the arithmetic; tests/dbscan_reference.py
//     mirrors the form);
//   * core: at least min_samples neighbours; clusters: connected components of the core points under the neighbour
//     relation, numbered 0, 1, ... by their smallest core-point index in the input order;
//   * border: a non-core point with a core neighbour takes the smallest label among its core neighbours' clusters
//     (sklearn's depth-first expansion finishes one cluster before it starts the next); every other point is noise (-1).
//
// Grid.  Cubic cells of side h = eps / sqrt(3) * (1 - 2^-12), cell coordinates c = floor((x - lo) / h) in fp64 (x, lo fp32,
// lo the device-reduced minimum), at most 2^21 cells per axis; the 63-bit key cx | cy << 21 | cz << 42 is sorted by two
// stable 32-bit onesweep radix sorts (low word, then high word), so points sit cell by cell and, inside a cell, in input
// order.  Two facts carry the whole algorithm:
//   (W) every neighbour of a point lies within +-2 cells on each axis.  fma and the products are monotone in their
//       non-negative arguments, so d2 <= eps32^2 implies fl(dx*dx) <= fl(eps32*eps32), i.e. |dx| <= eps (1 + 2^-22) and
//       the real |xi - xj| <= eps (1 + 2^-21) = h sqrt(3) (1 + 2^-11) < 1.74 h; the fp64 quotients add < 2^-30 cells, so
//       the cell coordinates differ by at most 2.  (Valid while eps32^2 is a normal fp32 number well inside the range: the
//       C entry reports eps outside [2^-40, 2^40] as DBSCAN_FLAG_RANGE; inside it eps^2 and every relevant square stay normal.)
//   (C) a cell whose members' bounding box has a diagonal with d2(lo, hi) <= eps32^2 (SAME fp32 form) holds only mutual
//       neighbours: for members p, q, |xp - xq| <= hi.x - lo.x in the reals, rounding is monotone and fl(a - b) = -fl(b - a),
//       so |fl(xp - xq)| <= fl(hi.x - lo.x) on each axis, and then each product and fma is <= its counterpart.  This is
//       CHECKED for every cell (cell_info_k) rather than assumed; by the choice of h (real diagonal < eps (1 - 2^-11), the
//       fp32 form adds < 2^-21 relative) it never fails, and if it did the call reports DBSCAN_FLAG_GRID instead of labels.
//   The same monotonicity gives exact pruning: the fp32 form of the gap between a point (or box) and a cell's member box is
//   <= the fp32 d2 of every pair it bounds, so a cell whose gap exceeds eps32^2 holds no neighbour.
// Core flags.  A clique cell with >= min_samples members makes all its members core without counting.  Every other point
// counts its own clique cell wholesale and then the members of the window's cells one by one, stopping at min_samples.
// Clusters.  All core points of a clique cell are one clique, so union-find runs over cells that hold a core point: one wave
// per cell c tests each later core cell d of its window (skipped when already joined or when the box gap exceeds eps) for
// ANY core pair within eps and stops at the first one; the union hooks the larger root under the smaller with atomicCAS.
// Roots only decrease, so find() ends within n_cells steps and a failed CAS means another union succeeded: the retry loop
// ends within n_cells rounds.  No workgroup ever waits for another.  The final root of a component is its smallest cell.
// Labels.  atomicMin of the core indices per root gives each component's smallest core index; a flag at that index and an
// exclusive scan over the n input positions give sklearn's numbering; border points then take the smallest label over the
// core cells of their window that hold a core neighbour.
// Every count is an integer and every choice a minimum, so the labels do not depend on scheduling or launch shape.
// Device flag word (result[1]): DBSCAN_FLAG_NONFINITE (NaN / inf input), DBSCAN_FLAG_SORT (a radix-sort look-back ran out of
// its budget), DBSCAN_FLAG_RANGE (more than 2^21 cells on an axis), DBSCAN_FLAG_GRID (see C), DBSCAN_FLAG_UNION (a union-find
// loop met its bound: cannot happen, see above).  Whenever it is non-zero the labels are not to be used.
// C entries, with the limits they enforce, at the end of the file: goi_semantic_dbscan* (declared in include/goi_raster.h).
#include <float.h>

#include <cmath>

#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int DB_THREADS = 256;
constexpr int DB_AXIS_BITS = 21;
constexpr int DB_AXIS_CELLS = 1 << DB_AXIS_BITS;
constexpr uint32_t CELL_CLIQUE = 1u, CELL_DENSE = 2u, CELL_CORE = 4u;  // cell_info bits
// once one of these is raised the labels are void: the searches stop (clamped or NaN cells could be huge and quadratic)
constexpr uint32_t DB_UNION = DBSCAN_FLAG_UNION;  // find_root (wave_util.h) raises it when its walk overruns: never reached
constexpr uint32_t DB_ABORT = DBSCAN_FLAG_NONFINITE | DBSCAN_FLAG_RANGE | DBSCAN_FLAG_GRID;

__device__ __forceinline__ float d2_form(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
// fp32 form of the gap between a value and an interval (0 inside); monotone bound of |fl(v - m)| for every member m
__device__ __forceinline__ float gap1(float v, float lo, float hi) {
    return v < lo ? lo - v : (v > hi ? v - hi : 0.f);
}
__device__ __forceinline__ float gap_box(float alo, float ahi, float blo, float bhi) {
    return blo > ahi ? blo - ahi : (alo > bhi ? alo - bhi : 0.f);
}

struct Box {
    float lx, ly, lz, hx, hy, hz;
};
// cbox: 8 words per cell, ordered encodings of (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z), 2 spare
__device__ __forceinline__ Box load_box(const uint32_t* cbox, uint32_t c) {
    const uint4 a = reinterpret_cast<const uint4*>(cbox)[2 * (size_t)c];
    const uint4 b = reinterpret_cast<const uint4*>(cbox)[2 * (size_t)c + 1];
    return Box{ord_dec(a.x), ord_dec(a.y), ord_dec(a.z), ord_dec(a.w), ord_dec(b.x), ord_dec(b.y)};
}
__device__ __forceinline__ float point_box_d2(const float4& p, const Box& b) {
    const float gx = gap1(p.x, b.lx, b.hx), gy = gap1(p.y, b.ly, b.hy), gz = gap1(p.z, b.lz, b.hz);
    return fmaf(gz, gz, fmaf(gy, gy, gx * gx));
}
__device__ __forceinline__ float box_box_d2(const Box& a, const Box& b) {
    const float gx = gap_box(a.lx, a.hx, b.lx, b.hx), gy = gap_box(a.ly, a.hy, b.ly, b.hy), gz = gap_box(a.lz, a.hz, b.lz, b.hz);
    return fmaf(gz, gz, fmaf(gy, gy, gx * gx));
}

__device__ __forceinline__ uint32_t axis_cell(float v, float lo, double h) {
    const double q = ((double)v - (double)lo) / h;
    if (!(q >= 0.0)) return 0u;  // (NaN: the call is flagged, the clamp only keeps indices in range)
    return q >= (double)(DB_AXIS_CELLS - 1) ? (uint32_t)(DB_AXIS_CELLS - 1) : (uint32_t)q;
}
__device__ __forceinline__ uint64_t pack_key(uint32_t cx, uint32_t cy, uint32_t cz) {
    return (uint64_t)cx | ((uint64_t)cy << DB_AXIS_BITS) | ((uint64_t)cz << (2 * DB_AXIS_BITS));
}
__device__ __forceinline__ uint64_t cell_key(const float* __restrict__ pts, uint32_t id, const uint32_t* __restrict__ enc,
                                             double h) {
    return pack_key(axis_cell(pts[3 * (size_t)id], ord_dec(enc[0]), h), axis_cell(pts[3 * (size_t)id + 1], ord_dec(enc[1]), h),
                    axis_cell(pts[3 * (size_t)id + 2], ord_dec(enc[2]), h));
}

__device__ __forceinline__ uint32_t lower_bound(const uint64_t* __restrict__ ckey, uint32_t nc, uint64_t k) {
    uint32_t lo = 0, hi = nc;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ckey[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// f(d) for every occupied cell d of the +-2 window around key k, in key order; f returns true to stop
template <class F>
__device__ __forceinline__ void for_window(uint64_t k, const uint64_t* __restrict__ ckey, uint32_t nc, F&& f) {
    const int cx = (int)(k & (DB_AXIS_CELLS - 1)), cy = (int)((k >> DB_AXIS_BITS) & (DB_AXIS_CELLS - 1)),
              cz = (int)(k >> (2 * DB_AXIS_BITS));
    const uint32_t x0 = (uint32_t)max(cx - 2, 0), x1 = (uint32_t)min(cx + 2, DB_AXIS_CELLS - 1);
    for (int z = max(cz - 2, 0); z <= min(cz + 2, DB_AXIS_CELLS - 1); z++)
        for (int y = max(cy - 2, 0); y <= min(cy + 2, DB_AXIS_CELLS - 1); y++) {
            const uint64_t k1 = pack_key(x1, (uint32_t)y, (uint32_t)z);
            for (uint32_t d = lower_bound(ckey, nc, pack_key(x0, (uint32_t)y, (uint32_t)z)); d < nc && ckey[d] <= k1; d++)
                if (f(d)) return;
        }
}

// enc[0..2] = min, enc[3..5] = max over the finite coordinates (ordered encodings; initialised to ~0 / 0 by the launcher)
__global__ __launch_bounds__(DB_THREADS) void db_bounds_k(int n, const float* __restrict__ pts, uint32_t* __restrict__ enc,
                                                          uint32_t* __restrict__ flags) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool bad = false;
    for (int i = blockIdx.x * DB_THREADS + threadIdx.x; i < n; i += gridDim.x * DB_THREADS)
        for (int c = 0; c < 3; c++) {
            const float v = pts[3 * (size_t)i + c];
            if (!isfinite(v)) {
                bad = true;
                continue;
            }
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, (uint32_t)DBSCAN_FLAG_NONFINITE);
    __shared__ float s[DB_THREADS / 64][6];
    for (int c = 0; c < 3; c++) {
        lo[c] = wave_min(lo[c]);
        hi[c] = wave_max(hi[c]);
    }
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; c++) {
            s[threadIdx.x >> 6][c] = lo[c];
            s[threadIdx.x >> 6][3 + c] = hi[c];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = s[0][c];
        for (int w = 1; w < DB_THREADS / 64; w++) v = c < 3 ? fminf(v, s[w][c]) : fmaxf(v, s[w][c]);
        if (c < 3) atomicMin(&enc[c], ord_enc(v));
        else atomicMax(&enc[c], ord_enc(v));
    }
}

// low key words + identity values; one thread also checks the extent against the 2^21-cell axis limit
__global__ __launch_bounds__(DB_THREADS) void db_key_lo_k(int n, const float* __restrict__ pts, const uint32_t* __restrict__ enc,
                                                          double h, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          uint32_t* __restrict__ flags) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i == 0)
        for (int c = 0; c < 3; c++) {
            const float lo = ord_dec(enc[c]), hi = ord_dec(enc[3 + c]);
            if (lo <= hi && ((double)hi - (double)lo) / h >= (double)(DB_AXIS_CELLS - 1))
                atomicOr(flags, (uint32_t)DBSCAN_FLAG_RANGE);
        }
    if (i >= n) return;
    keys[i] = (uint32_t)cell_key(pts, (uint32_t)i, enc, h);
    vals[i] = (uint32_t)i;
}

// second pass input: the high key words of the points in low-word order
__global__ __launch_bounds__(DB_THREADS) void db_key_hi_k(int n, const float* __restrict__ pts, const uint32_t* __restrict__ enc,
                                                          double h, const uint32_t* __restrict__ order,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = order[i];
    keys[i] = (uint32_t)(cell_key(pts, id, enc, h) >> 32);
    vals[i] = id;
}

// sorted points (x, y, z, bits(input index)), their keys, and a 1 at the first point of every cell
__global__ __launch_bounds__(DB_THREADS) void db_sorted_k(int n, const float* __restrict__ pts, const uint32_t* __restrict__ enc,
                                                          double h, const uint32_t* __restrict__ order, float4* __restrict__ spt,
                                                          uint64_t* __restrict__ skey, uint32_t* __restrict__ head) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = order[i];
    const uint64_t k = cell_key(pts, id, enc, h);
    spt[i] = make_float4(pts[3 * (size_t)id], pts[3 * (size_t)id + 1], pts[3 * (size_t)id + 2], __uint_as_float(id));
    skey[i] = k;
    head[i] = (i == 0 || cell_key(pts, order[i - 1], enc, h) != k) ? 1u : 0u;
}

// scell: exclusive scan of head -> cell of every sorted point; cell starts, keys, empty boxes
__global__ __launch_bounds__(DB_THREADS) void db_cells_k(int n, const uint32_t* __restrict__ ncell, const uint32_t* __restrict__ head,
                                                         uint32_t* __restrict__ scell, const uint64_t* __restrict__ skey,
                                                         uint32_t* __restrict__ cstart, uint64_t* __restrict__ ckey,
                                                         uint32_t* __restrict__ cbox) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t hd = head[i];
    const uint32_t c = scell[i] + hd - 1u;
    scell[i] = c;
    if (hd) {
        cstart[c] = (uint32_t)i;
        ckey[c] = skey[i];
        uint4* b = reinterpret_cast<uint4*>(cbox) + 2 * (size_t)c;
        b[0] = make_uint4(~0u, ~0u, ~0u, 0u);
        b[1] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (i == 0) cstart[*ncell] = (uint32_t)n;
}

// member bounding box of every cell: one set of atomics per wave when the wave lies in one cell (dense cells), else per lane
__global__ __launch_bounds__(DB_THREADS) void db_bbox_k(int n, const float4* __restrict__ spt, const uint32_t* __restrict__ scell,
                                                        uint32_t* __restrict__ cbox) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    const bool active = i < n;
    const float4 p = active ? spt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t c = active ? scell[i] : 0u;
    const float v[3] = {p.x, p.y, p.z};
    uint32_t* b = cbox + 8 * (size_t)c;
    if (wave_same(active, c)) {
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            lo[a] = wave_min(active ? v[a] : FLT_MAX);
            hi[a] = wave_max(active ? v[a] : -FLT_MAX);
        }
        if ((threadIdx.x & 63) == 0)
            for (int a = 0; a < 3; a++) {
                atomicMin(b + a, ord_enc(lo[a]));
                atomicMax(b + 3 + a, ord_enc(hi[a]));
            }
    } else if (active) {
        for (int a = 0; a < 3; a++) {
            atomicMin(b + a, ord_enc(v[a]));
            atomicMax(b + 3 + a, ord_enc(v[a]));
        }
    }
}

// per cell: the clique check (C), dense = clique and >= min_samples members (all core), union-find and minimum initialisation
__global__ __launch_bounds__(DB_THREADS) void db_cell_info_k(int n, const uint32_t* __restrict__ ncell,
                                                             const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ cbox,
                                                             float eps2, int min_samples, uint32_t* __restrict__ info,
                                                             uint32_t* __restrict__ parent, uint32_t* __restrict__ cmin,
                                                             uint32_t* __restrict__ flags) {
    const uint32_t c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= *ncell) return;
    const Box b = load_box(cbox, c);
    const bool clique = d2_form(b.hx, b.hy, b.hz, b.lx, b.ly, b.lz) <= eps2;
    if (!clique) atomicOr(flags, (uint32_t)DBSCAN_FLAG_GRID);
    const bool dense = clique && cstart[c + 1] - cstart[c] >= (uint32_t)min_samples;
    info[c] = (clique ? CELL_CLIQUE : 0u) | (dense ? CELL_DENSE | CELL_CORE : 0u);
    parent[c] = c;
    cmin[c] = ~0u;
}

// core flag of every sorted point
__global__ __launch_bounds__(DB_THREADS) void db_core_k(int n, const uint32_t* __restrict__ ncell, const float4* __restrict__ spt,
                                                        const uint32_t* __restrict__ scell, const uint32_t* __restrict__ cstart,
                                                        const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cbox,
                                                        uint32_t* __restrict__ info, float eps2, int min_samples,
                                                        uint8_t* __restrict__ score, const uint32_t* __restrict__ flags) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n || (*flags & DB_ABORT)) return;
    const uint32_t c = scell[i];
    const uint32_t ci = info[c];
    bool core = (ci & CELL_DENSE) != 0;
    if (!core) {
        const float4 p = spt[i];
        const uint32_t need = (uint32_t)min_samples;
        const bool own_clique = (ci & CELL_CLIQUE) != 0;
        uint32_t cnt = own_clique ? cstart[c + 1] - cstart[c] : 0u;
        if (cnt < need)
            for_window(ckey[c], ckey, *ncell, [&](uint32_t d) {
                if (d == c && own_clique) return false;
                if (d != c && point_box_d2(p, load_box(cbox, d)) > eps2) return false;
                const uint32_t e = cstart[d + 1];
                for (uint32_t j = cstart[d]; j < e; j++) {
                    const float4 q = spt[j];
                    if (d2_form(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2 && ++cnt >= need) return true;
                }
                return false;
            });
        core = cnt >= need;
        if (core && !(ci & CELL_CORE)) atomicOr(&info[c], CELL_CORE);
    }
    score[i] = core ? 1 : 0;
}

// one wave per core cell c: join c with every later core cell of its window that holds a core pair within eps
__global__ __launch_bounds__(DB_THREADS) void db_union_k(int n, const uint32_t* __restrict__ ncell, const float4* __restrict__ spt,
                                                         const uint32_t* __restrict__ cstart, const uint64_t* __restrict__ ckey,
                                                         const uint32_t* __restrict__ cbox, const uint32_t* __restrict__ info,
                                                         const uint8_t* __restrict__ score, float eps2, uint32_t* parent,
                                                         uint32_t* __restrict__ flags) {
    const uint32_t c = (blockIdx.x * DB_THREADS + threadIdx.x) >> 6;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const uint32_t nc = *ncell;
    if (c >= nc || !(info[c] & CELL_CORE) || (*flags & DB_ABORT)) return;
    const Box bc = load_box(cbox, c);
    const uint32_t c0 = cstart[c], c1 = cstart[c + 1];
    for_window(ckey[c], ckey, nc, [&](uint32_t d) {
        if (d <= c || !(info[d] & CELL_CORE)) return false;
        if (box_box_d2(bc, load_box(cbox, d)) > eps2) return false;
        if (find_root(parent, c, nc, flags, DB_UNION) == find_root(parent, d, nc, flags, DB_UNION)) return false;
        const uint32_t d0 = cstart[d], d1 = cstart[d + 1];
        bool hit = false;
        for (uint32_t a0 = c0; a0 < c1 && !hit; a0 += 64) {
            const uint32_t a = a0 + lane;
            const bool mine = a < c1 && score[a];
            const float4 p = mine ? spt[a] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (!__any(mine)) continue;
            for (uint32_t j = d0; j < d1; j++) {
                if (!score[j]) continue;  // (uniform)
                const float4 q = spt[j];
                if (__any(mine && d2_form(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2)) {
                    hit = true;
                    break;
                }
            }
        }
        if (hit && lane == 0) {
            // hook the larger root under the smaller; a failed CAS means that root was hooked meanwhile (bounded: <= nc unions)
            for (uint32_t it = 0;; it++) {
                uint32_t ra = find_root(parent, c, nc, flags, DB_UNION), rb = find_root(parent, d, nc, flags, DB_UNION);
                if (ra == rb) break;
                if (ra > rb) {
                    const uint32_t t = ra;
                    ra = rb;
                    rb = t;
                }
                if (atomicCAS(parent + rb, rb, ra) == rb) break;
                if (it >= nc) {
                    atomicOr(flags, DB_UNION);
                    break;
                }
            }
        }
        return false;
    });
}

// parent[c] = root of c for every core cell (other threads only ever see an ancestor)
__global__ __launch_bounds__(DB_THREADS) void db_flatten_k(int n, const uint32_t* __restrict__ ncell,
                                                           const uint32_t* __restrict__ info, uint32_t* parent,
                                                           uint32_t* __restrict__ flags) {
    const uint32_t c = blockIdx.x * DB_THREADS + threadIdx.x;
    const uint32_t nc = *ncell;
    if (c >= nc || !(info[c] & CELL_CORE)) return;
    parent[c] = find_root(parent, c, nc, flags, DB_UNION);
}

// cmin[root] = smallest input index of a core point in the component
__global__ __launch_bounds__(DB_THREADS) void db_cmin_k(int n, const float4* __restrict__ spt, const uint32_t* __restrict__ scell,
                                                        const uint8_t* __restrict__ score, const uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ cmin, const uint32_t* __restrict__ flags) {
    if (*flags & DB_ABORT) return;  // (uniform: the core flags were not computed)
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    const bool active = i < n && score[i];
    const uint32_t r = active ? parent[scell[i]] : 0u;
    const uint32_t id = active ? __float_as_uint(spt[i].w) : ~0u;
    if (wave_same(active, r)) {
        const uint32_t m = wave_min(id);
        const unsigned long long act = __ballot(active);
        if ((threadIdx.x & 63) == __builtin_ctzll(act)) atomicMin(&cmin[r], m);
    } else if (active) {
        atomicMin(&cmin[r], id);
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_rep_k(int n, const uint32_t* __restrict__ ncell, const uint32_t* __restrict__ info,
                                                       const uint32_t* __restrict__ parent, const uint32_t* __restrict__ cmin,
                                                       uint32_t* __restrict__ rep, const uint32_t* __restrict__ flags) {
    const uint32_t c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= *ncell || !(info[c] & CELL_CORE) || parent[c] != c || (*flags & DB_ABORT)) return;
    const uint32_t m = cmin[c];
    if (m < (uint32_t)n) rep[m] = 1u;  // (always: a core cell holds a core point)
}

__global__ __launch_bounds__(DB_THREADS) void db_label_k(int n, const uint32_t* __restrict__ ncell, const float4* __restrict__ spt,
                                                         const uint32_t* __restrict__ scell, const uint32_t* __restrict__ cstart,
                                                         const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cbox,
                                                         const uint32_t* __restrict__ info, const uint8_t* __restrict__ score,
                                                         const uint32_t* __restrict__ parent, const uint32_t* __restrict__ cmin,
                                                         const uint32_t* __restrict__ rank, float eps2, int* __restrict__ labels,
                                                         uint8_t* __restrict__ core_out, const uint32_t* __restrict__ flags) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n || (*flags & DB_ABORT)) return;
    const float4 p = spt[i];
    const uint32_t id = __float_as_uint(p.w);
    const uint32_t c = scell[i];
    const bool core = score[i] != 0;
    auto label_of = [&](uint32_t cell) {  // component label of a core cell (cmin < n always holds; the test keeps loads in range)
        const uint32_t m = cmin[parent[cell]];
        return m < (uint32_t)n ? rank[m] : ~0u;
    };
    int label;
    if (core) {
        label = (int)label_of(c);
    } else {
        uint32_t best = ~0u;
        const uint32_t ci = info[c];
        if ((ci & CELL_CORE) && (ci & CELL_CLIQUE)) best = label_of(c);  // a core point of its own clique cell
        for_window(ckey[c], ckey, *ncell, [&](uint32_t d) {
            if (!(info[d] & CELL_CORE)) return false;
            const uint32_t l = label_of(d);
            if (l >= best || point_box_d2(p, load_box(cbox, d)) > eps2) return false;
            const uint32_t e = cstart[d + 1];
            for (uint32_t j = cstart[d]; j < e; j++) {
                if (!score[j]) continue;
                const float4 q = spt[j];
                if (d2_form(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2) {
                    best = l;
                    break;
                }
            }
            return false;
        });
        label = best == ~0u ? -1 : (int)best;
    }
    labels[id] = label;
    if (core_out) core_out[id] = core ? 1 : 0;
}

inline unsigned grid_for(size_t n) { return (unsigned)((n + DB_THREADS - 1) / DB_THREADS); }

// Workspace, 256-byte aligned pieces: control words (bounds, cell count) | keys[2] | vals[2] | sort scratch | sorted points |
// point keys | head / representative flags | point cells | cell starts | cell keys | cell boxes | cell info | parents | minima |
// ranks | core flags | scan scratch  (~ 90 bytes per point plus the sort's scratch)
struct DbscanView {
    uint32_t* ctl;  // [16]: 0..5 encoded bounds, 8 the cell count
    SortBufs sb;
    float4* spt;
    uint64_t *skey, *ckey;
    uint32_t *head, *scell, *cstart, *cbox, *info, *parent, *cmin, *rank, *scan_scratch;
    uint8_t* score;
};
size_t dbscan_workspace_layout(size_t n, char* base, DbscanView* v) {
    Carver c(base);
    DbscanView t;
    t.ctl = c.take<uint32_t>(16);
    carve_sort(c, n, &t.sb);
    t.spt = c.take<float4>(n);
    t.skey = c.take<uint64_t>(n);
    t.head = c.take<uint32_t>(n);
    t.scell = c.take<uint32_t>(n);
    t.cstart = c.take<uint32_t>(n + 1);
    t.ckey = c.take<uint64_t>(n);
    t.cbox = c.take<uint32_t>(8 * n);
    t.info = c.take<uint32_t>(n);
    t.parent = c.take<uint32_t>(n);
    t.cmin = c.take<uint32_t>(n);
    t.rank = c.take<uint32_t>(n);
    t.score = c.take<uint8_t>(n);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words(n));
    if (v) *v = t;
    return c.bytes();
}

size_t dbscan_workspace_bytes(size_t n) { return dbscan_workspace_layout(n, nullptr, nullptr); }

void launch_dbscan(int n, const float* pts, float eps2, double h, int min_samples, int* labels, uint8_t* core, int* result,
                   void* workspace, hipStream_t s) {
    DbscanView w;
    dbscan_workspace_layout((size_t)n, static_cast<char*>(workspace), &w);
    uint32_t* flags = reinterpret_cast<uint32_t*>(result) + 1;
    uint32_t* enc = w.ctl;         // [6]
    uint32_t* ncell = w.ctl + 8;   // [1]
    const unsigned g = grid_for((size_t)n);
    (void)hipMemsetAsync(enc, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(enc + 3, 0x00, 3 * sizeof(uint32_t), s);
    db_bounds_k<<<dim3(g < 1024 ? g : 1024), dim3(DB_THREADS), 0, s>>>(n, pts, enc, flags);
    db_key_lo_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, pts, enc, h, w.sb.keys[0], w.sb.vals[0], flags);
    const int f1 = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)n, 0, 32, w.sb.scratch, s, false, false, nullptr, flags);
    uint32_t* k2[2] = {w.sb.keys[f1 ^ 1], w.sb.keys[f1]};
    uint32_t* v2[2] = {w.sb.vals[f1 ^ 1], w.sb.vals[f1]};
    db_key_hi_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, pts, enc, h, w.sb.vals[f1], k2[0], v2[0]);
    const int f2 = radix_sort_pairs(k2, v2, (size_t)n, 0, 63 - 32, w.sb.scratch, s, false, false, nullptr, flags);
    const uint32_t* order = v2[f2];
    db_sorted_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, pts, enc, h, order, w.spt, w.skey, w.head);
    exclusive_scan_u32(w.head, nullptr, w.scell, (size_t)n, ncell, w.scan_scratch, s);
    db_cells_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.head, w.scell, w.skey, w.cstart, w.ckey, w.cbox);
    db_bbox_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, w.spt, w.scell, w.cbox);
    db_cell_info_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.cstart, w.cbox, eps2, min_samples, w.info, w.parent, w.cmin, flags);
    db_core_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.spt, w.scell, w.cstart, w.ckey, w.cbox, w.info, eps2, min_samples, w.score,
                                                        flags);
    const size_t union_groups = ((size_t)n * 64 + DB_THREADS - 1) / DB_THREADS;  // one wave per (possible) cell
    db_union_k<<<dim3((unsigned)union_groups), dim3(DB_THREADS), 0, s>>>(n, ncell, w.spt, w.cstart, w.ckey, w.cbox, w.info, w.score, eps2,
                                                                         w.parent, flags);
    db_flatten_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.info, w.parent, flags);
    db_cmin_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, w.spt, w.scell, w.score, w.parent, w.cmin, flags);
    (void)hipMemsetAsync(w.head, 0, sizeof(uint32_t) * (size_t)n, s);  // head -> representative flags (input order)
    db_rep_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.info, w.parent, w.cmin, w.head, flags);
    exclusive_scan_u32(w.head, nullptr, w.rank, (size_t)n, reinterpret_cast<uint32_t*>(result), w.scan_scratch, s);
    db_label_k<<<dim3(g), dim3(DB_THREADS), 0, s>>>(n, ncell, w.spt, w.scell, w.cstart, w.ckey, w.cbox, w.info, w.score, w.parent, w.cmin, w.rank,
                                                    eps2, labels, core, flags);
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_semantic_dbscan_workspace_bytes(long long n) {
    return (n > 0 && n < SORT_MAX_KEYS) ? dbscan_workspace_bytes((size_t)n) : 0;
}

int goi_semantic_dbscan(long long n, const float* points, float eps, int min_samples, int* labels, uint8_t* core, int* result,
                        void* workspace, void* stream) {
    // (the cell keys go through radix_sort_pairs, exact below 2^30 keys: common.h)
    if (n < 0 || n >= SORT_MAX_KEYS) return fail("goi_semantic_dbscan: need 0 <= n < 2^30");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail("goi_semantic_dbscan: eps must be a finite number > 0");
    if (min_samples < 1) return fail("goi_semantic_dbscan: min_samples must be >= 1");
    if (!result) return fail("goi_semantic_dbscan: result is NULL");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    GOI_HIP(hipMemsetAsync(result, 0, 2 * sizeof(int), s));
    if (n == 0) return 0;
    if (!points || !labels) return fail("goi_semantic_dbscan: a required pointer is NULL");
    if (check_workspace("goi_semantic_dbscan", workspace) < 0) return -1;
    if (!(eps >= 0x1p-40f && eps <= 0x1p40f)) {  // outside the range of the grid's exactness argument (top of this file)
        GOI_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(result + 1), DBSCAN_FLAG_RANGE, 1, s));
        return 0;
    }
    const float eps2 = eps * eps;
    const double h = (double)eps / std::sqrt(3.0) * (1.0 - 1.0 / 4096.0);  // cell side: eps / sqrt(3) less a margin
    launch_dbscan((int)n, points, eps2, h, min_samples, labels, core, result, workspace, s);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
