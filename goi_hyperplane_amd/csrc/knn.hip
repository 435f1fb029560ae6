// distCUDA2 for gfx950: mean squared distance of every point to its 3 nearest neighbours
// (reference: submodules/simple-knn/simple_knn.cu:170-221 behind simple_knn._C.distCUDA2,
// spatial.cu:15-26; called once per scene by scene/gaussian_model.py:147 to size the initial
// Gaussians).
//
// The reference prunes an exhaustive search with 1024-point Morton boxes, one thread per point
// walking every box.  The result does not depend on the space partition (a box is skipped only
// when it cannot hold a nearer neighbour), so this build keeps the definition -- the 3 smallest
// fp32 squared distances to all OTHER sorted positions, (b0 + b1 + b2) / 3 -- and maps the search
// onto the CU instead:
//   * everything stays on the device: bounds by block reduction + 6 ordered-integer atomics per
//     block (no host read-back of min / max), Morton sort with the onesweep radix sort of
//     scan_sort.hip (30 key bits = 4 passes);
//   * a box is 256 consecutive sorted points = one workgroup of 4 waves.  Queries live in
//     registers, candidates are staged one box at a time through LDS (4 KB, read as same-address
//     broadcasts: no bank conflicts, one ds_read_b128 per 64 distance evaluations);
//   * pruning is two-level: 256 candidate boxes are tested per trip against the QUERY BOX inflated
//     by the workgroup's worst third-best distance (one box-box test per thread + a ballot), so
//     whole boxes are rejected without touching their points and the surviving ones are visited
//     uniformly by all 4 waves; inside, a lane whose own point is farther from the box than its
//     third best sits the box out.
// Distances are evaluated as fma(dz,dz, fma(dx,dx, dy*dy)) (this TU is compiled with
// -ffp-contract=off so that the spelling is the arithmetic), the form oracle/knn_oracle.cpp mirrors.
// The k-NN graph (knn_graph_k, further down) is a second search beside that one over the same preparation: the k
// smallest (distance, id) pairs of every query with their ids, through per-point masks, plus the majority label of a row.
// C entries, with the limits they enforce, at the end of the file: goi_knn_* (declared in include/goi_raster.h).
#include <float.h>

#include "common.h"
#include "entry.h"
#include "wave_util.h"

namespace goi {

namespace {

constexpr int KNN_BOX = 256;
// box bounds and point distances round differently; shrink the bound so rounding can never prune a
// box that holds a (by <= 1 ulp) nearer neighbour
constexpr float SLACK = 0.999999f;

// enc[0..2] = min, enc[3..5] = max (ordered-integer encoding; initialised to ~0 / 0 by the launcher)
// keep (may be NULL: everything): one byte per point, only points with a non-zero byte count
__global__ __launch_bounds__(256) void knn_bounds_k(int P, const float* __restrict__ pts, uint32_t* __restrict__ enc,
                                                    const uint8_t* __restrict__ keep = nullptr) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        if (keep && !keep[i]) continue;
        for (int c = 0; c < 3; c++) {
            const float v = pts[3 * (size_t)i + c];
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
    __shared__ float s[4][6];
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
    if (threadIdx.x < 3)
        atomicMin(&enc[threadIdx.x], ord_enc(fminf(fminf(s[0][threadIdx.x], s[1][threadIdx.x]),
                                                   fminf(s[2][threadIdx.x], s[3][threadIdx.x]))));
    else if (threadIdx.x < 6)
        atomicMax(&enc[threadIdx.x], ord_enc(fmaxf(fmaxf(s[0][threadIdx.x], s[1][threadIdx.x]),
                                                   fmaxf(s[2][threadIdx.x], s[3][threadIdx.x]))));
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {  // 10 bits -> every third bit
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// keep (may be NULL): a point that is out gets KNN_KEY_OUT, above every kept key, so the sort (then over 31 bits) moves it behind
// all kept points; n_keep (may be NULL; zeroed by the launcher) receives the number of kept points, one atomic per wave.
constexpr uint32_t KNN_KEY_OUT = 1u << 30;
__global__ __launch_bounds__(256) void knn_morton_k(int P, const float* __restrict__ pts, const uint32_t* __restrict__ enc,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                    const uint8_t* __restrict__ keep = nullptr, uint32_t* __restrict__ n_keep = nullptr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (n_keep) {
        const bool in = !keep || keep[i];
        const unsigned long long m = __ballot(in);
        if (m && (threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(n_keep, (uint32_t)__builtin_popcountll(m));
        if (!in) {
            keys[i] = KNN_KEY_OUT;
            vals[i] = (uint32_t)i;
            return;
        }
    }
    uint32_t q[3];
    for (int c = 0; c < 3; c++) {
        const float lo = ord_dec(enc[c]), hi = ord_dec(enc[3 + c]);
        const float ext = hi - lo;
        float t = ext > 0.f ? (pts[3 * (size_t)i + c] - lo) / ext * 1023.f : 0.f;
        t = fminf(fmaxf(t, 0.f), 1023.f);  // also maps NaN to 0
        q[c] = (uint32_t)t;
    }
    keys[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
    vals[i] = (uint32_t)i;
}

// sorted[i] = (x, y, z, bits(original index)) in Morton order, padded to whole boxes with +inf points;
// box b = (min corner, max corner) of sorted[256 b .. 256 b + 255].
// n_dev (may be NULL: P): the first *n_dev sorted positions are points; the ones from there to P keep their id beside +inf
// coordinates and enter no box, so a box without points has the inverted bounds (FLT_MAX, -FLT_MAX).
__global__ __launch_bounds__(KNN_BOX) void knn_boxes_k(int P, const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                       float4* __restrict__ sorted, float4* __restrict__ boxes,
                                                       const uint32_t* __restrict__ n_dev = nullptr) {
    const int i = blockIdx.x * KNN_BOX + threadIdx.x;
    float4 p = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __uint_as_float(0xFFFFFFFFu));
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (n_dev && i < P && i >= (int)*n_dev) {
        p.w = __uint_as_float(order[i]);
    } else if (i < P) {
        const uint32_t id = order[i];
        p = make_float4(pts[3 * (size_t)id], pts[3 * (size_t)id + 1], pts[3 * (size_t)id + 2], __uint_as_float(id));
        lo[0] = hi[0] = p.x;
        lo[1] = hi[1] = p.y;
        lo[2] = hi[2] = p.z;
    }
    sorted[i] = p;
    __shared__ float s[4][6];
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
    if (threadIdx.x == 0) {
        float4 a, b;
        a.x = fminf(fminf(s[0][0], s[1][0]), fminf(s[2][0], s[3][0]));
        a.y = fminf(fminf(s[0][1], s[1][1]), fminf(s[2][1], s[3][1]));
        a.z = fminf(fminf(s[0][2], s[1][2]), fminf(s[2][2], s[3][2]));
        b.x = fmaxf(fmaxf(s[0][3], s[1][3]), fmaxf(s[2][3], s[3][3]));
        b.y = fmaxf(fmaxf(s[0][4], s[1][4]), fmaxf(s[2][4], s[3][4]));
        b.z = fmaxf(fmaxf(s[0][5], s[1][5]), fmaxf(s[2][5], s[3][5]));
        a.w = b.w = 0.f;
        boxes[2 * blockIdx.x] = a;
        boxes[2 * blockIdx.x + 1] = b;
    }
}

__device__ __forceinline__ void k_best(float d, float& b0, float& b1, float& b2) {  // simple_knn.cu:135-151
    const float n0 = fminf(b0, d);
    d = fmaxf(b0, d);
    const float n1 = fminf(b1, d);
    d = fmaxf(b1, d);
    b2 = fminf(b2, d);
    b0 = n0;
    b1 = n1;
}

// squared distance between a point and a box (simple_knn.cu:122-132)
__device__ __forceinline__ float box_point_d2(const float4& lo, const float4& hi, const float4& p) {
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
    return dx * dx + dy * dy + dz * dz;
}
// lower bound of the squared distance between any point of box A and any point of box B
__device__ __forceinline__ float box_box_d2(const float4& alo, const float4& ahi, const float4& blo, const float4& bhi) {
    const float dx = fmaxf(fmaxf(blo.x - ahi.x, alo.x - bhi.x), 0.f);
    const float dy = fmaxf(fmaxf(blo.y - ahi.y, alo.y - bhi.y), 0.f);
    const float dz = fmaxf(fmaxf(blo.z - ahi.z, alo.z - bhi.z), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

__global__ __launch_bounds__(KNN_BOX) void knn_search_k(int P, int nbox, const float4* __restrict__ sorted,
                                                        const float4* __restrict__ boxes, float* __restrict__ out) {
    __shared__ float4 s_cand[KNN_BOX];
    __shared__ float s_red[4];
    __shared__ unsigned long long s_mask[4];
    const int qb = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int self = qb * KNN_BOX + t;
    const float4 q = sorted[self];
    const bool live = self < P;
    const float4 qlo = boxes[2 * qb], qhi = boxes[2 * qb + 1];
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;

    auto scan_box = [&](int cb, bool want) {
        // all 256 threads stage the candidate box; lanes that cannot improve sit the scan out
        __syncthreads();
        s_cand[t] = sorted[(size_t)cb * KNN_BOX + t];
        __syncthreads();
        if (!want) return;
        const int base = cb * KNN_BOX;
        const int n = min(KNN_BOX, P - base);
        for (int j = 0; j < n; j++) {
            const float4 c = s_cand[j];
            const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
            const float d = fmaf(dz, dz, fmaf(dx, dx, dy * dy));
            if (base + j != self) k_best(d, b0, b1, b2);
        }
    };

    scan_box(qb, live);  // the own box first: it gives every live lane a tight third best

    for (int c0 = 0; c0 < nbox; c0 += KNN_BOX) {
        // workgroup's worst third-best bounds what any of its points can still accept
        float worst = live ? b2 : 0.f;
        worst = wave_max(worst);
        __syncthreads();
        if (lane == 0) s_red[wave] = worst;
        __syncthreads();
        worst = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        const int cb = c0 + t;
        bool near = false;
        if (cb < nbox && cb != qb) near = box_box_d2(qlo, qhi, boxes[2 * cb], boxes[2 * cb + 1]) * SLACK <= worst;
        const unsigned long long m = __ballot(near);
        if (lane == 0) s_mask[wave] = m;
        __syncthreads();
        for (int w = 0; w < 4; w++) {
            unsigned long long mw = s_mask[w];  // uniform across the workgroup
            while (mw) {
                const int bit = __builtin_ctzll(mw);
                mw &= mw - 1;
                const int cand = c0 + 64 * w + bit;
                const bool want = live && box_point_d2(boxes[2 * cand], boxes[2 * cand + 1], q) * SLACK <= b2;
                scan_box(cand, want);
            }
        }
    }
    if (live) out[__float_as_uint(q.w)] = (b0 + b1 + b2) / 3.0f;
}

// Workspace: bounds (6 encoded words) | Morton keys, ids and the sort's scratch | sorted points, padded to whole boxes | boxes
struct KnnView {
    uint32_t* enc;  // [8]
    SortBufs sb;    // [P]
    float4 *sorted, *boxes;
};
size_t knn_workspace_layout(int P, char* base, KnnView* v) {
    const size_t nbox = ((size_t)P + KNN_BOX - 1) / KNN_BOX;
    Carver c(base);
    KnnView t;
    t.enc = c.take<uint32_t>(8);
    carve_sort(c, (size_t)P, &t.sb);
    t.sorted = c.take<float4>(nbox * KNN_BOX);
    t.boxes = c.take<float4>(2 * nbox);
    if (v) *v = t;
    return c.bytes();
}

size_t knn_workspace_bytes(int P) { return knn_workspace_layout(P, nullptr, nullptr); }

int launch_knn(int P, const float* points, float* mean_dist2, void* workspace, hipStream_t s) {
    KnnView w;
    knn_workspace_layout(P, static_cast<char*>(workspace), &w);
    const int nbox = (P + KNN_BOX - 1) / KNN_BOX;
    (void)hipMemsetAsync(w.enc, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.enc + 3, 0x00, 3 * sizeof(uint32_t), s);
    const int rb = min(nbox, 1024);
    knn_bounds_k<<<dim3(rb), dim3(256), 0, s>>>(P, points, w.enc);
    knn_morton_k<<<dim3(nbox), dim3(256), 0, s>>>(P, points, w.enc, w.sb.keys[0], w.sb.vals[0]);
    const int fin = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)P, 0, 30, w.sb.scratch, s);
    knn_boxes_k<<<dim3(nbox), dim3(KNN_BOX), 0, s>>>(P, points, w.sb.vals[fin], w.sorted, w.boxes);
    knn_search_k<<<dim3(nbox), dim3(KNN_BOX), 0, s>>>(P, nbox, w.sorted, w.boxes, mean_dist2);
    return 0;
}

// ---- the k-NN graph: row i = the k smallest (dist2, reference id) pairs of query i, ascending ------------------
// A list entry is ONE ordered 64-bit word: the bits of the non-negative fp32 distance above the reference's id, so that the
// lexicographic order of the pairs is the unsigned order of the words (ties in distance go to the lower id) and the test against
// the lane's k-th pair is one compare.  An empty slot is (+inf, 0xFFFFFFFF): it is above every pair with a finite distance, its
// distance is the infinite bound a lane with fewer than k entries prunes with, and it is what a padded row holds.
constexpr unsigned long long KNN_EMPTY = 0x7F800000FFFFFFFFull;

// Each lane keeps KCAP words in registers, ascending.  Only the LAST k of them are the lane's list: the KCAP - k in front are
// zeros, below (or equal to) every pair and never moved, so the k-th pair is always the last, statically indexed, word.
// Queries: sq / qboxes / *nq_dev (Morton-sorted live queries in front, then -- up to Pq -- the ids of the masked-out ones);
// references: sr / rboxes / *nr_dev.  self_mode: the two are the same arrays and a query's own box is scanned first; otherwise
// the reference box whose centre is nearest to the query box's (thread 0 always offers box 0, so the minimum's low word is a box).
template <int KCAP>
__global__ __launch_bounds__(KNN_BOX) void knn_graph_k(int Pq, int k, int self_mode, int skip_self, const float4* __restrict__ sq,
                                                       const float4* __restrict__ qboxes, const uint32_t* __restrict__ nq_dev,
                                                       const float4* __restrict__ sr, const float4* __restrict__ rboxes,
                                                       const uint32_t* __restrict__ nr_dev, int32_t* __restrict__ idx,
                                                       float* __restrict__ dist2) {
    __shared__ float4 s_cand[KNN_BOX];
    __shared__ float s_red[4];
    __shared__ unsigned long long s_mask[4];
    const int qb = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int pos = qb * KNN_BOX + t;
    const int nq = (int)*nq_dev, nr = (int)*nr_dev;
    const int nbox = (nr + KNN_BOX - 1) / KNN_BOX;  // boxes that hold a reference: the ones behind are empty and never looked at
    const float4 q = sq[pos];
    const bool live = pos < nq;
    // skip_self: the reference whose ORIGINAL id is the query's is left out (ids are below 2^30: all ones matches none)
    const uint32_t skip = skip_self ? __float_as_uint(q.w) : 0xFFFFFFFFu;
    unsigned long long best[KCAP];
#pragma unroll
    for (int i = 0; i < KCAP; i++) best[i] = i < KCAP - k ? 0ull : KNN_EMPTY;
    auto bound = [&]() { return __uint_as_float((uint32_t)(best[KCAP - 1] >> 32)); };

    auto scan_box = [&](int cb, bool want) {
        __syncthreads();
        s_cand[t] = sr[(size_t)cb * KNN_BOX + t];
        __syncthreads();
        if (!want) return;
        const int n = min(KNN_BOX, nr - cb * KNN_BOX);
        auto pair_key = [&](int j) {
            const float4 c = s_cand[j];
            const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
            const float d = fmaf(dz, dz, fmaf(dx, dx, dy * dy));
            // the lane's own point never enters: all ones is above every list word
            return __float_as_uint(c.w) != skip ? ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(c.w) : ~0ull;
        };
        auto offer = [&](unsigned long long key) {
            const bool take = key < best[KCAP - 1];  // ONE compare against the lane's k-th pair
            if (__ballot(take)) {  // rare once the lists are warm: the chain runs only when some lane of the wave takes the pair
                if (take) best[KCAP - 1] = key;
#pragma unroll
                for (int i = KCAP - 1; i > 0; i--) {
                    const unsigned long long a = best[i - 1], b = best[i];
                    const bool lt = b < a;
                    best[i - 1] = lt ? b : a;
                    best[i] = lt ? a : b;
                }
            }
        };
        // four candidates per trip: their LDS reads are in flight together, and one ballot of "below the k-th pair as it was
        // when the trip began" (never smaller than it is later: conservative) lets the wave skip all four offers at once
        int j = 0;
        for (; j + 4 <= n; j += 4) {
            const unsigned long long k0 = pair_key(j), k1 = pair_key(j + 1), k2 = pair_key(j + 2), k3 = pair_key(j + 3);
            const unsigned long long last = best[KCAP - 1];
            if (__ballot((k0 < last) | (k1 < last) | (k2 < last) | (k3 < last))) {
                offer(k0);
                offer(k1);
                offer(k2);
                offer(k3);
            }
        }
        for (; j < n; j++) offer(pair_key(j));
    };

    if (qb * KNN_BOX < nq && nbox > 0) {  // (uniform: a block of masked-out queries only writes its padded rows)
        const float4 qlo = qboxes[2 * qb], qhi = qboxes[2 * qb + 1];
        int first = qb;
        if (!self_mode) {
            unsigned long long near = ~0ull;
            for (int cb = t; cb < nbox; cb += KNN_BOX) {
                const float4 lo = rboxes[2 * cb], hi = rboxes[2 * cb + 1];
                const float dx = (lo.x + hi.x) - (qlo.x + qhi.x), dy = (lo.y + hi.y) - (qlo.y + qhi.y), dz = (lo.z + hi.z) - (qlo.z + qhi.z);
                const float d = fmaf(dz, dz, fmaf(dx, dx, dy * dy));  // >= 0 or NaN: as bits, ordered like the lists' distances
                near = min(near, ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)cb);
            }
            near = wave_butterfly(near, [](unsigned long long a, unsigned long long b) { return min(a, b); });
            if (lane == 0) s_mask[wave] = near;
            __syncthreads();
            first = (int)(uint32_t)min(min(s_mask[0], s_mask[1]), min(s_mask[2], s_mask[3]));
        }
        scan_box(first, live);

        for (int c0 = 0; c0 < nbox; c0 += KNN_BOX) {
            // workgroup's worst k-th distance bounds what any of its queries can still accept
            float worst = live ? bound() : 0.f;
            worst = wave_max(worst);
            __syncthreads();
            if (lane == 0) s_red[wave] = worst;
            __syncthreads();
            worst = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
            const int cb = c0 + t;
            bool near = false;
            // <=: a box AT the k-th distance may hold a reference at that very distance with a lower id
            if (cb < nbox && cb != first) near = box_box_d2(qlo, qhi, rboxes[2 * cb], rboxes[2 * cb + 1]) * SLACK <= worst;
            const unsigned long long m = __ballot(near);
            if (lane == 0) s_mask[wave] = m;
            __syncthreads();
            for (int w = 0; w < 4; w++) {
                unsigned long long mw = s_mask[w];  // uniform across the workgroup
                while (mw) {
                    const int bit = __builtin_ctzll(mw);
                    mw &= mw - 1;
                    const int cand = c0 + 64 * w + bit;
                    const bool want = live && box_point_d2(rboxes[2 * cand], rboxes[2 * cand + 1], q) * SLACK <= bound();
                    scan_box(cand, want);
                }
            }
        }
    }
    if (pos < Pq) {  // rows by original id; a masked-out query's list is still all empty slots
        const size_t row = (size_t)__float_as_uint(q.w) * (size_t)k;
#pragma unroll
        for (int i = 0; i < KCAP; i++)
            if (i >= KCAP - k) {
                idx[row + (size_t)(i - (KCAP - k))] = (int32_t)(uint32_t)best[i];  // (0xFFFFFFFF of an empty slot is -1)
                dist2[row + (size_t)(i - (KCAP - k))] = __uint_as_float((uint32_t)(best[i] >> 32));
            }
    }
}

// Workspace: bounds of the references (6 words), the two live counts, bounds of the queries | ONE set of sort buffers, used for
// the references and then for the queries | sorted points and boxes of each side
struct KnnGraphView {
    uint32_t* hdr;  // [16]: 0..5 reference bounds, 6 live references, 7 live queries, 8..13 query bounds
    SortBufs sb;    // [max(Pq, Pr)]
    float4 *sorted_r, *boxes_r, *sorted_q, *boxes_q;
};
size_t knn_graph_workspace_layout(int Pq, int Pr, char* base, KnnGraphView* v) {
    const size_t nbr = ((size_t)Pr + KNN_BOX - 1) / KNN_BOX, nbq = ((size_t)Pq + KNN_BOX - 1) / KNN_BOX;
    Carver c(base);
    KnnGraphView t;
    t.hdr = c.take<uint32_t>(16);
    // (carve_sort's pieces, the scratch sized for whichever side's sort asks for more: the tile, hence the rows, go by n)
    const size_t n = (size_t)max(Pq, Pr);
    for (int i = 0; i < 2; i++) t.sb.keys[i] = c.take<uint32_t>(at_least_one(n));
    for (int i = 0; i < 2; i++) t.sb.vals[i] = c.take<uint32_t>(at_least_one(n));
    t.sb.scratch = c.take<uint32_t>(max(sort_scratch_words((size_t)Pq), sort_scratch_words((size_t)Pr)));
    t.sorted_r = c.take<float4>(nbr * KNN_BOX);
    t.boxes_r = c.take<float4>(2 * nbr);
    t.sorted_q = c.take<float4>(nbq * KNN_BOX);
    t.boxes_q = c.take<float4>(2 * nbq);
    if (v) *v = t;
    return c.bytes();
}

// one side: bounds, Morton codes (masked-out points behind the kept ones), sort, sorted points and boxes; *n_dev = kept count
void knn_graph_side(int P, const float* pts, const uint8_t* keep, uint32_t* enc, uint32_t* n_dev, const SortBufs& sb, float4* sorted,
                    float4* boxes, hipStream_t s) {
    const int nbox = (P + KNN_BOX - 1) / KNN_BOX;
    knn_bounds_k<<<dim3(min(nbox, 1024)), dim3(256), 0, s>>>(P, pts, enc, keep);
    knn_morton_k<<<dim3(nbox), dim3(256), 0, s>>>(P, pts, enc, sb.keys[0], sb.vals[0], keep, n_dev);
    const int fin = radix_sort_pairs(sb.keys, sb.vals, (size_t)P, 0, keep ? 31 : 30, sb.scratch, s);
    knn_boxes_k<<<dim3(nbox), dim3(KNN_BOX), 0, s>>>(P, pts, sb.vals[fin], sorted, boxes, n_dev);
}

int launch_knn_graph(int Pq, const float* queries, const uint8_t* query_keep, int Pr, const float* refs, const uint8_t* ref_keep,
                     int k, int exclude_self, int32_t* idx, float* dist2, void* workspace, hipStream_t s) {
    KnnGraphView w;
    knn_graph_workspace_layout(Pq, Pr, static_cast<char*>(workspace), &w);
    (void)hipMemsetAsync(w.hdr, 0x00, 16 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.hdr, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.hdr + 8, 0xFF, 3 * sizeof(uint32_t), s);
    uint32_t *nr = w.hdr + 6, *nq = w.hdr + 7;
    const bool self_mode = queries == refs && query_keep == ref_keep && Pq == Pr;
    if (Pr > 0) knn_graph_side(Pr, refs, ref_keep, w.hdr, nr, w.sb, w.sorted_r, w.boxes_r, s);
    if (self_mode) {
        nq = nr;
        w.sorted_q = w.sorted_r;
        w.boxes_q = w.boxes_r;
    } else {
        knn_graph_side(Pq, queries, query_keep, w.hdr + 8, nq, w.sb, w.sorted_q, w.boxes_q, s);
    }
    const dim3 grid((Pq + KNN_BOX - 1) / KNN_BOX), block(KNN_BOX);
    if (k <= 4)
        knn_graph_k<4><<<grid, block, 0, s>>>(Pq, k, self_mode, exclude_self, w.sorted_q, w.boxes_q, nq, w.sorted_r, w.boxes_r, nr, idx,
                                              dist2);
    else if (k <= 8)
        knn_graph_k<8><<<grid, block, 0, s>>>(Pq, k, self_mode, exclude_self, w.sorted_q, w.boxes_q, nq, w.sorted_r, w.boxes_r, nr, idx,
                                              dist2);
    else
        knn_graph_k<16><<<grid, block, 0, s>>>(Pq, k, self_mode, exclude_self, w.sorted_q, w.boxes_q, nq, w.sorted_r, w.boxes_r, nr, idx,
                                               dist2);
    return 0;
}

// label_out[i] = the label most entries of row i carry, the LOWEST among equals; an entry counts with 0 <= idx < Pr,
// labels[idx] >= 0 and (dist2 given) dist2 <= max_dist2.  Labels are compared as values: k * k integer compares per row.
__global__ __launch_bounds__(256) void knn_majority_k(int Pq, int k, const int32_t* __restrict__ idx, const float* __restrict__ dist2,
                                                      float max_dist2, int Pr, const int64_t* __restrict__ labels,
                                                      int64_t* __restrict__ label_out, int32_t* __restrict__ count_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Pq) return;
    const size_t row = (size_t)i * (size_t)k;
    auto label_of = [&](int j) -> int64_t {
        const int32_t r = idx[row + j];
        if (r < 0 || r >= Pr) return -1;
        if (dist2 && !(dist2[row + j] <= max_dist2)) return -1;
        return labels[r];
    };
    int64_t best = -1;
    int32_t best_n = 0;
    for (int a = 0; a < k; a++) {
        const int64_t la = label_of(a);
        if (la < 0) continue;
        int32_t n = 0;
        for (int b = 0; b < k; b++) n += label_of(b) == la;
        if (n > best_n || (n == best_n && la < best)) {
            best = la;
            best_n = n;
        }
    }
    label_out[i] = best;
    count_out[i] = best_n;
}

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_knn_workspace_bytes(int P) { return P > 0 && P < SORT_MAX_KEYS ? knn_workspace_bytes(P) : 0; }

int goi_knn_dist2(int P, const float* points, float* mean_dist2, void* workspace, void* stream) {
    if (P < 0) return fail("goi_knn_dist2: bad P");
    // (the Morton codes go through radix_sort_pairs, exact below 2^30 keys: common.h)
    if (P >= SORT_MAX_KEYS) return fail("goi_knn_dist2: need P < 2^30");
    if (P == 0) return 0;
    if (!points || !mean_dist2) return fail("goi_knn_dist2: a required pointer is NULL");
    if (check_workspace("goi_knn_dist2", workspace) < 0) return -1;
    launch_knn(P, points, mean_dist2, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_knn_graph_workspace_bytes(int Pq, int Pr) {
    return Pq >= 0 && Pr >= 0 && Pq < SORT_MAX_KEYS && Pr < SORT_MAX_KEYS ? knn_graph_workspace_layout(Pq, Pr, nullptr, nullptr) : 0;
}

int goi_knn_graph(int Pq, const float* queries, const uint8_t* query_keep, int Pr, const float* refs, const uint8_t* ref_keep, int k,
                  int exclude_self, int32_t* idx, float* dist2, void* workspace, void* stream) {
    if (Pq < 0 || Pr < 0) return fail("goi_knn_graph: bad Pq or Pr");
    if (Pq >= SORT_MAX_KEYS || Pr >= SORT_MAX_KEYS) return fail("goi_knn_graph: need Pq < 2^30 and Pr < 2^30");
    if (k < 1 || k > 16) return fail("goi_knn_graph: need 1 <= k <= 16");
    if (exclude_self && (queries != refs || Pq != Pr))
        return fail("goi_knn_graph: exclude_self needs queries == refs and Pq == Pr");
    if (Pq == 0) return 0;
    if (!queries || !idx || !dist2 || (Pr > 0 && !refs)) return fail("goi_knn_graph: a required pointer is NULL");
    if (check_workspace("goi_knn_graph", workspace) < 0) return -1;
    launch_knn_graph(Pq, queries, query_keep, Pr, refs, ref_keep, k, exclude_self != 0, idx, dist2, workspace,
                     static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_knn_majority(int Pq, int k, const int32_t* idx, const float* dist2, float max_dist2, int Pr, const int64_t* labels,
                     int64_t* label_out, int32_t* count_out, void* stream) {
    if (Pq < 0 || Pr < 0) return fail("goi_knn_majority: bad Pq or Pr");
    if (k < 1) return fail("goi_knn_majority: need k >= 1");
    if (max_dist2 != max_dist2) return fail("goi_knn_majority: max_dist2 is NaN");
    if (Pq == 0) return 0;
    if (!idx || !label_out || !count_out || (Pr > 0 && !labels)) return fail("goi_knn_majority: a required pointer is NULL");
    knn_majority_k<<<dim3((Pq + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(Pq, k, idx, dist2, max_dist2, Pr, labels,
                                                                                              label_out, count_out);
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
