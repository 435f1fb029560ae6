// Mesh clean-up on the device: connected components, the clean_mesh filters, vertex clustering and
// vertex normals of a triangle mesh (float32 [V, 3] vertices, int32 [F, 3] faces).  gfx950 only; compiled with
// -ffp-contract=off: every float operation below is rounded once, as the numpy restatement of tests/mesh_reference.py is.
//
// Shared properties: integer results are exact; floats are never accumulated with atomics (every sum has one fixed order), so
// two runs give the same bits; stages are separated by kernel boundaries, nothing spins on another workgroup.  A face that
// names an index outside [0, V) is treated as absent and sets MESH_STATUS_RANGE; a find_root walk or CAS retry loop that runs
// out of its bound sets MESH_STATUS_UNION (never reached: parents only decrease); a sort whose look-back timed out sets
// MESH_STATUS_SORT.
//
//   components   mesh_init_k: parent[v] = v; mesh_union_k: one lane per face hooks the larger root under the smaller with
//                atomicCAS (dbscan.hip's scheme), so the root of a component is its smallest vertex; mesh_flatten_k,
//                mesh_face_label_k.
//   dedup        three stable radix sorts of (key, face) on the largest, middle and smallest index of every face's sorted
//                triple leave equal triples adjacent in ascending face order; a face whose predecessor holds the same
//                triple is a duplicate.  Faces that are already gone carry the key `limit` and gather behind the rest.
//   clean        null faces, dedup, components of what is left, per-component face counts (integer atomics) and boxes (integer
//                atomic min / max on the order-preserving encoding), the two filters, then two scans that renumber.
//   decimate     member bounds, cell keys, a stable sort of (key, vertex), one lane per cell walking its run in fp64, the
//                faces mapped through the cells, dedup, two scans.
//   normals      a stable sort of (vertex, 3 face + corner); one lane per vertex finds its run by binary search and adds the
//                faces' cross products in ascending (face, corner) order.
// C entries, with the limits they enforce, at the end of the file: goi_mesh_* (declared in include/goi_raster.h).
#include "common.h"
#include "entry.h"
#include "wave_util.h"

#include <math.h>

namespace goi {
namespace {

constexpr int MESH_THREADS = 256;
constexpr uint32_t ENC_NONE = 0xFFFFFFFFu;

unsigned blocks_for(long long n) { return (unsigned)((n + MESH_THREADS - 1) / MESH_THREADS); }
__device__ __forceinline__ long long gid() { return (long long)blockIdx.x * MESH_THREADS + threadIdx.x; }
int bits_for(uint32_t limit) { return limit == 0 ? 1 : 32 - __builtin_clz(limit); }  // covers every key <= limit

__device__ __forceinline__ bool load_face(const int* __restrict__ faces, long long f, uint32_t V, uint32_t& a, uint32_t& b,
                                          uint32_t& c) {
    a = (uint32_t)faces[3 * f];
    b = (uint32_t)faces[3 * f + 1];
    c = (uint32_t)faces[3 * f + 2];
    return a < V && b < V && c < V;  // (a negative index is a huge unsigned one)
}

// ---- union-find (find_root: wave_util.h) -----------------------------------------------------------------------------------
constexpr uint32_t MESH_UNION = GOI_MESH_STATUS_UNION;
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t V, uint32_t* status) {
    for (uint32_t it = 0;; it++) {
        uint32_t ra = find_root(parent, a, V, status, MESH_UNION), rb = find_root(parent, b, V, status, MESH_UNION);
        if (ra == rb) return;
        if (ra > rb) {
            const uint32_t t = ra;
            ra = rb;
            rb = t;
        }
        if (atomicCAS(parent + rb, rb, ra) == rb) return;  // a failed CAS: that root was hooked meanwhile (at most V unions)
        a = ra;  // both are ancestors still: start the next walk from them
        b = rb;
        if (it >= V) {
            atomicOr(status, MESH_UNION);
            return;
        }
    }
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_init_k(uint32_t V, uint32_t* __restrict__ parent, uint8_t* __restrict__ named) {
    const long long v = gid();
    if (v >= V) return;
    parent[v] = (uint32_t)v;
    named[v] = 0;
}

// alive: NULL (every face) or one byte per face
__global__ void __launch_bounds__(MESH_THREADS) mesh_union_k(long long F, uint32_t V, const int* __restrict__ faces,
                                                            const uint8_t* __restrict__ alive, uint32_t* parent,
                                                            uint8_t* __restrict__ named, uint32_t* __restrict__ status) {
    const long long f = gid();
    if (f >= F || (alive && !alive[f])) return;
    uint32_t a, b, c;
    if (!load_face(faces, f, V, a, b, c)) {
        atomicOr(status, (uint32_t)GOI_MESH_STATUS_RANGE);
        return;
    }
    named[a] = 1;  // (several faces store the same byte)
    named[b] = 1;
    named[c] = 1;
    unite(parent, a, b, V, status);
    unite(parent, a, c, V, status);
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_flatten_k(uint32_t V, const uint32_t* __restrict__ parent,
                                                              const uint8_t* __restrict__ named, int* __restrict__ label,
                                                              uint32_t* __restrict__ status) {
    const long long v = gid();
    if (v >= V) return;
    label[v] = named[v] ? (int)find_root(parent, (uint32_t)v, V, status, MESH_UNION) : -1;
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_face_label_k(long long F, uint32_t V, const int* __restrict__ faces,
                                                                 const int* __restrict__ label, int* __restrict__ face_label) {
    const long long f = gid();
    if (f >= F) return;
    const uint32_t a = (uint32_t)faces[3 * f];
    face_label[f] = a < V ? label[a] : -1;
}

void run_components(long long F, uint32_t V, const int* faces, const uint8_t* alive, uint32_t* parent, uint8_t* named, int* label,
                    uint32_t* status, hipStream_t s) {
    if (V == 0) return;
    mesh_init_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(V, parent, named);
    if (F > 0) mesh_union_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, V, faces, alive, parent, named, status);
    mesh_flatten_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(V, parent, named, label, status);
}

// ---- duplicate faces -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sort3(uint32_t& a, uint32_t& b, uint32_t& c) {
    uint32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}
// the `which`-th smallest index of face f (0 smallest), or `limit` for a face that is gone
__device__ __forceinline__ uint32_t triple_key(const int* __restrict__ tri, const uint8_t* __restrict__ alive, uint32_t f, int which,
                                               uint32_t limit) {
    if (!alive[f]) return limit;
    uint32_t a = (uint32_t)tri[3 * (size_t)f], b = (uint32_t)tri[3 * (size_t)f + 1], c = (uint32_t)tri[3 * (size_t)f + 2];
    sort3(a, b, c);
    return which == 0 ? a : which == 1 ? b : c;
}
// first: the faces in their own order (this pass also writes the values); later passes re-key the order they are in
__global__ void __launch_bounds__(MESH_THREADS) mesh_dedup_key_k(uint32_t F, const int* __restrict__ tri,
                                                                const uint8_t* __restrict__ alive, int which, uint32_t limit,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                bool first) {
    const long long i = gid();
    if (i >= F) return;
    const uint32_t f = first ? (uint32_t)i : vals[i];
    if (first) vals[i] = f;
    keys[i] = triple_key(tri, alive, f, which, limit);
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_dedup_mark_k(uint32_t F, const int* __restrict__ tri,
                                                                 const uint8_t* __restrict__ alive_in,
                                                                 const uint32_t* __restrict__ order, uint8_t* __restrict__ alive_out) {
    const long long i = gid();
    if (i >= F) return;
    const uint32_t f = order[i];
    uint32_t keep = alive_in[f];  // (a 32-bit select: the byte is formed at the store)
    if (keep && i > 0) {
        const uint32_t g = order[i - 1];
        if (alive_in[g]) {
            uint32_t a = (uint32_t)tri[3 * (size_t)f], b = (uint32_t)tri[3 * (size_t)f + 1], c = (uint32_t)tri[3 * (size_t)f + 2];
            uint32_t d = (uint32_t)tri[3 * (size_t)g], e = (uint32_t)tri[3 * (size_t)g + 1], h = (uint32_t)tri[3 * (size_t)g + 2];
            sort3(a, b, c);
            sort3(d, e, h);
            if (a == d && b == e && c == h) keep = 0;  // g < f: the sorts are stable and started in face order
        }
    }
    alive_out[f] = (uint8_t)keep;
}

// alive_out[f] = alive_in[f] and no lower alive face holds the same set of three indices (all < limit)
void run_dedup(uint32_t F, const int* tri, const uint8_t* alive_in, uint8_t* alive_out, uint32_t limit, const SortBufs& sb,
               uint32_t* status, hipStream_t s) {
    if (F == 0) return;
    const int bits = bits_for(limit);
    uint32_t* k[2] = {sb.keys[0], sb.keys[1]};
    uint32_t* v[2] = {sb.vals[0], sb.vals[1]};
    for (int pass = 0; pass < 3; pass++) {
        mesh_dedup_key_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, tri, alive_in, 2 - pass, limit, k[0], v[0], pass == 0);
        const int fin = radix_sort_pairs(k, v, F, 0, bits, sb.scratch, s, false, false, nullptr, status);
        if (fin == 1) {
            uint32_t* t = k[0]; k[0] = k[1]; k[1] = t;
            t = v[0]; v[0] = v[1]; v[1] = t;
        }
    }
    mesh_dedup_mark_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, tri, alive_in, v[0], alive_out);
}

// ---- clean -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) mesh_null_k(long long F, uint32_t V, const float* __restrict__ vert,
                                                           const int* __restrict__ faces, uint8_t* __restrict__ alive,
                                                           uint32_t* __restrict__ status) {
    const long long f = gid();
    if (f >= F) return;
    uint32_t a, b, c;
    if (!load_face(faces, f, V, a, b, c)) {
        atomicOr(status, (uint32_t)GOI_MESH_STATUS_RANGE);
        alive[f] = 0;
        return;
    }
    bool null = a == b || b == c || a == c;
    float p[3][3];
    const uint32_t idx[3] = {a, b, c};
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) {
            p[k][d] = vert[3 * (size_t)idx[k] + d];
            null = null || !isfinite(p[k][d]);
        }
    const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const float wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    null = null || (nx == 0.f && ny == 0.f && nz == 0.f);
    const uint32_t keep = null ? 0u : 1u;
    alive[f] = (uint8_t)keep;
}

// per component (indexed by its root): faces, box; box of the whole mesh in mbox
__global__ void __launch_bounds__(MESH_THREADS) mesh_comp_init_k(uint32_t V, uint32_t* __restrict__ cfaces, uint32_t* __restrict__ cbox,
                                                                uint32_t* __restrict__ mbox, uint32_t* __restrict__ used) {
    const long long v = gid();
    if (v < 6) mbox[v] = v < 3 ? ENC_NONE : 0u;
    if (v >= V) return;
    cfaces[v] = 0;
    used[v] = 0;
    for (int d = 0; d < 3; d++) {
        cbox[6 * v + d] = ENC_NONE;
        cbox[6 * v + 3 + d] = 0u;
    }
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_comp_faces_k(long long F, const int* __restrict__ faces,
                                                                 const uint8_t* __restrict__ alive, const int* __restrict__ label,
                                                                 uint32_t* __restrict__ cfaces) {
    const long long f = gid();
    const bool mine = f < F && alive[f];
    const uint32_t r = mine ? (uint32_t)label[faces[3 * f]] : 0u;
    const unsigned long long act = __ballot(mine);
    if (wave_same(mine, r)) {  // a mesh is a few large components: one atomic per wave, not 64 on one word
        if ((threadIdx.x & 63) == __builtin_ctzll(act)) atomicAdd(cfaces + r, (uint32_t)__popcll(act));
    } else if (mine) {
        atomicAdd(cfaces + r, 1u);
    }
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_comp_box_k(uint32_t V, const float* __restrict__ vert, const int* __restrict__ label,
                                                               uint32_t* __restrict__ cbox, uint32_t* __restrict__ mbox) {
    const long long v = gid();
    const int r = v < V ? label[v] : -1;
    float p[3] = {0.f, 0.f, 0.f};
    if (r >= 0)
        for (int d = 0; d < 3; d++) p[d] = vert[3 * v + d];
    const bool same = wave_same(r >= 0, (uint32_t)r);  // the usual case: the wave's vertices are of one component
    if (r >= 0 && !same)
        for (int d = 0; d < 3; d++) {
            const uint32_t e = ord_enc(p[d]);
            atomicMin(cbox + 6 * (size_t)r + d, e);
            atomicMax(cbox + 6 * (size_t)r + 3 + d, e);
        }
    const int lead = __shfl(r, __builtin_ctzll(__ballot(r >= 0) | (1ull << 63)));
    for (int d = 0; d < 3; d++) {  // the wave's box: one pair of atomics for the mesh, and one for the component all share
        float mn = r >= 0 ? p[d] : INFINITY, mx = r >= 0 ? p[d] : -INFINITY;
        for (int o = 32; o >= 1; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o));
            mx = fmaxf(mx, __shfl_xor(mx, o));
        }
        if ((threadIdx.x & 63) == 0 && mn <= mx) {
            atomicMin(mbox + d, ord_enc(mn));
            atomicMax(mbox + 3 + d, ord_enc(mx));
            if (same) {
                atomicMin(cbox + 6 * (size_t)lead + d, ord_enc(mn));
                atomicMax(cbox + 6 * (size_t)lead + 3 + d, ord_enc(mx));
            }
        }
    }
}
// d2 of a box: the fp64 sum, x y z, of the squares of the fp32 extents
__device__ __forceinline__ double box_d2(const uint32_t* __restrict__ box) {
    double d2 = 0.0;
    for (int d = 0; d < 3; d++) {
        const float e = ord_dec(box[3 + d]) - ord_dec(box[d]);
        d2 += (double)e * (double)e;
    }
    return d2;
}
// cfaces[root] becomes 1 (the component stays) or 0
__global__ void __launch_bounds__(MESH_THREADS) mesh_comp_decide_k(uint32_t V, const int* __restrict__ label, long long min_faces,
                                                                  double min_diag2, const uint32_t* __restrict__ cbox,
                                                                  const uint32_t* __restrict__ mbox, uint32_t* __restrict__ cfaces) {
    const long long v = gid();
    if (v >= V || label[v] != (int)v) return;
    bool keep = (long long)cfaces[v] >= min_faces;
    keep = keep && !(box_d2(cbox + 6 * v) < min_diag2 * box_d2(mbox));
    cfaces[v] = keep ? 1u : 0u;
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_face_keep_k(long long F, const int* __restrict__ faces,
                                                                const uint8_t* __restrict__ alive, const int* __restrict__ label,
                                                                const uint32_t* __restrict__ ckeep, uint32_t* __restrict__ fflag,
                                                                uint32_t* __restrict__ used) {
    const long long f = gid();
    if (f >= F) return;
    uint32_t keep = 0;
    if (alive[f]) {
        const int a = faces[3 * f];
        keep = ckeep[label[a]];
        if (keep) {
            used[a] = 1;  // (several faces store the same word)
            used[faces[3 * f + 1]] = 1;
            used[faces[3 * f + 2]] = 1;
        }
    }
    fflag[f] = keep;
}
__global__ void mesh_counts_k(const uint32_t* __restrict__ tv, const uint32_t* __restrict__ tf, const uint32_t* __restrict__ status,
                              int* __restrict__ counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counts[0] = (int)*tv;
    counts[1] = (int)*tf;
    counts[2] = (int)*status;
}

// rows whose flag is set move to their scanned position (flags scanned in place: a set row's flag differs from its successor's)
__global__ void __launch_bounds__(MESH_THREADS) mesh_emit_vertices_k(uint32_t V, uint32_t total, const uint32_t* __restrict__ off,
                                                                    const float* __restrict__ vert, const float* __restrict__ col,
                                                                    float* __restrict__ out_v, float* __restrict__ out_c,
                                                                    int* __restrict__ index) {
    const long long v = gid();
    if (v >= V) return;
    const uint32_t o = off[v], next = v + 1 < V ? off[v + 1] : total;
    if (next == o) return;
    for (int d = 0; d < 3; d++) {
        out_v[3 * (size_t)o + d] = vert[3 * v + d];
        if (col) out_c[3 * (size_t)o + d] = col[3 * v + d];
    }
    index[o] = (int)v;
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_emit_faces_k(long long F, uint32_t total, const uint32_t* __restrict__ off,
                                                                 const int* __restrict__ tri, const uint32_t* __restrict__ voff,
                                                                 int* __restrict__ out_f, int* __restrict__ index) {
    const long long f = gid();
    if (f >= F) return;
    const uint32_t o = off[f], next = f + 1 < F ? off[f + 1] : total;
    if (next == o) return;
    for (int d = 0; d < 3; d++) out_f[3 * (size_t)o + d] = (int)voff[tri[3 * f + d]];
    if (index) index[o] = (int)f;
}

// (components and normals take an empty mesh, V = 0 or F = 0, and each of its arrays still gets a piece: at_least_one.  Clean and
// decimate need V, F >= 1.)
struct CompView {
    uint32_t* parent;
    uint8_t* named;
    uint32_t* status;
};
size_t comp_layout(size_t V, char* base, CompView* v) {
    Carver c(base);
    CompView t;
    t.parent = c.take<uint32_t>(at_least_one(V));
    t.named = c.take<uint8_t>(at_least_one(V));
    t.status = c.take<uint32_t>(4);
    if (v) *v = t;
    return c.bytes();
}

struct CleanView {
    uint32_t *parent, *cfaces, *cbox, *mbox, *used, *fflag, *ctl, *scan_scratch;  // ctl: 0 status, 1 vertices, 2 faces
    uint8_t *named, *alive0, *alive1;
    int* label;
    SortBufs sb;
};
size_t clean_layout(size_t V, size_t F, char* base, CleanView* v) {
    Carver c(base);
    CleanView t;
    t.parent = c.take<uint32_t>(V);
    t.cfaces = c.take<uint32_t>(V);
    t.cbox = c.take<uint32_t>(6 * V);
    t.mbox = c.take<uint32_t>(8);
    t.used = c.take<uint32_t>(V);
    t.fflag = c.take<uint32_t>(F);
    t.ctl = c.take<uint32_t>(4);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words(V > F ? V : F));
    t.named = c.take<uint8_t>(V);
    t.alive0 = c.take<uint8_t>(F);
    t.alive1 = c.take<uint8_t>(F);
    t.label = c.take<int>(V);
    carve_sort(c, F, &t.sb);
    if (v) *v = t;
    return c.bytes();
}

// ---- decimate --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) mesh_named_k(long long F, uint32_t V, const int* __restrict__ faces,
                                                            uint8_t* __restrict__ named, uint32_t* __restrict__ status) {
    const long long f = gid();
    if (f >= F) return;
    uint32_t a, b, c;
    if (!load_face(faces, f, V, a, b, c)) {
        atomicOr(status, (uint32_t)GOI_MESH_STATUS_RANGE);
        return;
    }
    named[a] = 1;
    named[b] = 1;
    named[c] = 1;
}
// member[v] = named and finite; box[0..2] / [3..5] = encoded min / max of the members
__global__ void __launch_bounds__(MESH_THREADS) mesh_member_k(uint32_t V, const float* __restrict__ vert, uint8_t* __restrict__ member,
                                                             uint32_t* __restrict__ box) {
    const long long v = gid();
    bool m = false;
    float p[3] = {0.f, 0.f, 0.f};
    if (v < V) {
        for (int d = 0; d < 3; d++) p[d] = vert[3 * v + d];
        m = member[v] && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        const uint32_t flag = m ? 1u : 0u;
        member[v] = (uint8_t)flag;
    }
    for (int d = 0; d < 3; d++) {
        float mn = m ? p[d] : INFINITY, mx = m ? p[d] : -INFINITY;
        for (int o = 32; o >= 1; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o));
            mx = fmaxf(mx, __shfl_xor(mx, o));
        }
        if ((threadIdx.x & 63) == 0 && mn <= mx) {
            atomicMin(box + d, ord_enc(mn));
            atomicMax(box + 3 + d, ord_enc(mx));
        }
    }
}
struct Cells {
    float lo[3], cell;
    bool flat;  // no extent (or no member): every member is in cell 0
};
__device__ __forceinline__ Cells load_cells(const uint32_t* __restrict__ box, int n) {
    Cells c;
    float e = 0.f;
    const bool none = box[0] == ENC_NONE;
    for (int d = 0; d < 3; d++) {
        c.lo[d] = none ? 0.f : ord_dec(box[d]);
        e = fmaxf(e, none ? 0.f : ord_dec(box[3 + d]) - c.lo[d]);
    }
    c.flat = !(e > 0.f);
    c.cell = e / (float)n;
    return c;
}
__device__ __forceinline__ uint32_t cell_key(const Cells& c, int n, const float* __restrict__ vert, size_t v) {
    if (c.flat) return 0u;
    uint32_t q[3];
    for (int d = 0; d < 3; d++) q[d] = (uint32_t)fminf(floorf((vert[3 * v + d] - c.lo[d]) / c.cell), (float)(n - 1));
    return (q[0] * (uint32_t)n + q[1]) * (uint32_t)n + q[2];
}
// faces whose three vertices are members in three distinct cells (one probe of the bisection)
__global__ void __launch_bounds__(MESH_THREADS) mesh_probe_k(long long F, uint32_t V, const float* __restrict__ vert,
                                                            const int* __restrict__ faces, const uint8_t* __restrict__ member,
                                                            const uint32_t* __restrict__ box, int n, uint32_t* __restrict__ count) {
    const Cells c = load_cells(box, n);
    uint32_t mine = 0;
    for (long long f = gid(); f < F; f += (long long)gridDim.x * MESH_THREADS) {
        uint32_t a, b, d;
        if (!load_face(faces, f, V, a, b, d) || !member[a] || !member[b] || !member[d]) continue;
        const uint32_t ka = cell_key(c, n, vert, a), kb = cell_key(c, n, vert, b), kd = cell_key(c, n, vert, d);
        mine += (ka != kb && kb != kd && ka != kd) ? 1u : 0u;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_cell_key_k(uint32_t V, const float* __restrict__ vert,
                                                               const uint8_t* __restrict__ member, const uint32_t* __restrict__ box,
                                                               int n, uint32_t none_key, uint32_t* __restrict__ keys,
                                                               uint32_t* __restrict__ vals) {
    const long long v = gid();
    if (v >= V) return;
    const Cells c = load_cells(box, n);
    keys[v] = member[v] ? cell_key(c, n, vert, v) : none_key;
    vals[v] = (uint32_t)v;
}
// head[i] = 1 where a cell's run starts in the sorted keys
__global__ void __launch_bounds__(MESH_THREADS) mesh_cell_head_k(uint32_t V, const uint32_t* __restrict__ skeys, uint32_t none_key,
                                                                uint32_t* __restrict__ head) {
    const long long i = gid();
    if (i >= V) return;
    head[i] = (skeys[i] != none_key && (i == 0 || skeys[i] != skeys[i - 1])) ? 1u : 0u;
}
// rank[i] = exclusive scan of head: a run's cell is rank[start]; vcell[v] = the cell of vertex v, or -1
__global__ void __launch_bounds__(MESH_THREADS) mesh_vertex_cell_k(uint32_t V, const uint32_t* __restrict__ skeys,
                                                                  const uint32_t* __restrict__ svals, uint32_t none_key,
                                                                  const uint32_t* __restrict__ rank, int* __restrict__ vcell,
                                                                  uint32_t* __restrict__ cused) {
    const long long i = gid();
    if (i >= V) return;
    cused[i] = 0;
    const bool head = i == 0 || skeys[i] != skeys[i - 1];  // rank counts the heads in front: a run's later members see their own
    vcell[svals[i]] = skeys[i] == none_key ? -1 : (int)(head ? rank[i] : rank[i] - 1u);
}
// tri[f] = the three cells; alive[f] = they are distinct (and every vertex is a member)
__global__ void __launch_bounds__(MESH_THREADS) mesh_cell_faces_k(long long F, uint32_t V, const int* __restrict__ faces,
                                                                 const int* __restrict__ vcell, int* __restrict__ tri,
                                                                 uint8_t* __restrict__ alive) {
    const long long f = gid();
    if (f >= F) return;
    uint32_t a, b, c;
    int ca = -1, cb = -1, cc = -1;
    if (load_face(faces, f, V, a, b, c)) {
        ca = vcell[a];
        cb = vcell[b];
        cc = vcell[c];
    }
    const bool ok = ca >= 0 && cb >= 0 && cc >= 0 && ca != cb && cb != cc && ca != cc;
    tri[3 * f] = ok ? ca : 0;
    tri[3 * f + 1] = ok ? cb : 0;
    tri[3 * f + 2] = ok ? cc : 0;
    const uint32_t flag = ok ? 1u : 0u;
    alive[f] = (uint8_t)flag;
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_cell_used_k(long long F, const int* __restrict__ tri,
                                                                const uint8_t* __restrict__ alive, uint32_t* __restrict__ fflag,
                                                                uint32_t* __restrict__ cused) {
    const long long f = gid();
    if (f >= F) return;
    const uint32_t keep = alive[f];
    fflag[f] = keep;
    if (keep)
        for (int d = 0; d < 3; d++) cused[tri[3 * f + d]] = 1;
}
// one lane per run: the mean of its members in ascending vertex order (fp64 sums, one division, one rounding)
__global__ void __launch_bounds__(MESH_THREADS) mesh_cell_mean_k(uint32_t V, uint32_t total, const uint32_t* __restrict__ skeys,
                                                                const uint32_t* __restrict__ svals, uint32_t none_key,
                                                                const uint32_t* __restrict__ rank, const uint32_t* __restrict__ coff,
                                                                const float* __restrict__ vert, const float* __restrict__ col,
                                                                float* __restrict__ out_v, float* __restrict__ out_c) {
    const long long i = gid();
    if (i >= V) return;
    const uint32_t key = skeys[i];
    if (key == none_key || (i > 0 && skeys[i - 1] == key)) return;
    const uint32_t cell = rank[i];
    const uint32_t o = coff[cell], next = cell + 1 < V ? coff[cell + 1] : total;
    if (next == o) return;  // no surviving face names this cell
    double sv[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    uint32_t cnt = 0;
    for (long long j = i; j < V && skeys[j] == key; j++, cnt++) {
        const size_t v = svals[j];
        for (int d = 0; d < 3; d++) {
            sv[d] += (double)vert[3 * v + d];
            if (col) sc[d] += (double)col[3 * v + d];
        }
    }
    for (int d = 0; d < 3; d++) {
        out_v[3 * (size_t)o + d] = (float)(sv[d] / (double)cnt);
        if (col) out_c[3 * (size_t)o + d] = (float)(sc[d] / (double)cnt);
    }
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_cluster_k(uint32_t V, uint32_t total, const int* __restrict__ vcell,
                                                              const uint32_t* __restrict__ coff, int* __restrict__ cluster) {
    const long long v = gid();
    if (v >= V) return;
    const int cell = vcell[v];
    int out = -1;
    if (cell >= 0) {
        const uint32_t o = coff[cell], next = (uint32_t)cell + 1 < V ? coff[cell + 1] : total;
        if (next != o) out = (int)o;
    }
    cluster[v] = out;
}

struct DecView {
    uint32_t *box, *ctl, *rank, *cused, *fflag, *scan_scratch;  // ctl: 0 status, 1 vertices, 2 faces
    uint8_t *member, *alive0, *alive1;
    int *vcell, *tri;
    SortBufs sbv, sbf;
};
size_t dec_layout(size_t V, size_t F, char* base, DecView* v) {
    Carver c(base);
    DecView t;
    t.box = c.take<uint32_t>(8);
    t.ctl = c.take<uint32_t>(4);
    t.rank = c.take<uint32_t>(V);
    t.cused = c.take<uint32_t>(V);
    t.fflag = c.take<uint32_t>(F);
    t.scan_scratch = c.take<uint32_t>(scan_scratch_words(V > F ? V : F));
    t.member = c.take<uint8_t>(V);
    t.alive0 = c.take<uint8_t>(F);
    t.alive1 = c.take<uint8_t>(F);
    t.vcell = c.take<int>(V);
    t.tri = c.take<int>(3 * F);
    carve_sort(c, V, &t.sbv);
    carve_sort(c, F, &t.sbf);
    if (v) *v = t;
    return c.bytes();
}

// ---- normals ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) mesh_corner_k(long long C, uint32_t V, const int* __restrict__ faces,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                             uint32_t* __restrict__ status) {
    const long long i = gid();
    if (i >= C) return;
    const long long f = i / 3;
    uint32_t a, b, c;
    uint32_t key = V;  // a face that names an index out of range adds nothing
    if (load_face(faces, f, V, a, b, c)) key = (uint32_t)faces[i];
    else atomicOr(status, (uint32_t)GOI_MESH_STATUS_RANGE);
    keys[i] = key;
    vals[i] = (uint32_t)i;
}
__global__ void __launch_bounds__(MESH_THREADS) mesh_normal_k(uint32_t V, uint32_t C, const float* __restrict__ vert,
                                                             const int* __restrict__ faces, const uint32_t* __restrict__ skeys,
                                                             const uint32_t* __restrict__ svals, float* __restrict__ out) {
    const long long v = gid();
    if (v >= V) return;
    uint32_t lo = 0, hi = C;  // the first sorted corner whose vertex is >= v
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (skeys[mid] < (uint32_t)v) lo = mid + 1;
        else hi = mid;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (uint32_t j = lo; j < C && skeys[j] == (uint32_t)v; j++) {  // ascending (face, corner): the sort is stable
        const size_t f = svals[j] / 3;
        const size_t a = (size_t)faces[3 * f], b = (size_t)faces[3 * f + 1], c = (size_t)faces[3 * f + 2];
        const float ux = vert[3 * b] - vert[3 * a], uy = vert[3 * b + 1] - vert[3 * a + 1], uz = vert[3 * b + 2] - vert[3 * a + 2];
        const float wx = vert[3 * c] - vert[3 * a], wy = vert[3 * c + 1] - vert[3 * a + 1], wz = vert[3 * c + 2] - vert[3 * a + 2];
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    float dot = sx * sx + sy * sy + sz * sz;
    if (!(dot > 1e-20f)) {  // auto_normal: torch.where(dot > 1e-20, vn, (0, 0, 1)); a NaN sum takes the default too
        sx = 0.f;
        sy = 0.f;
        sz = 1.f;
        dot = 1.f;
    }
    const float len = sqrtf(fmaxf(dot, 1e-20f));
    out[3 * v] = sx / len;
    out[3 * v + 1] = sy / len;
    out[3 * v + 2] = sz / len;
}

struct NormView {
    uint32_t* status;
    SortBufs sb;
};
size_t norm_layout(size_t C, char* base, NormView* v) {
    Carver c(base);
    NormView t;
    t.status = c.take<uint32_t>(4);
    carve_sort(c, C, &t.sb);
    if (v) *v = t;
    return c.bytes();
}

size_t mesh_components_workspace_bytes(long long V, long long F) { return comp_layout((size_t)V, nullptr, nullptr); }

void launch_mesh_components(long long V, long long F, const int* faces, int* vertex_label, int* face_label, int* status,
                            void* workspace, hipStream_t s) {
    CompView v;
    comp_layout((size_t)V, static_cast<char*>(workspace), &v);
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    (void)hipMemsetAsync(st, 0, sizeof(uint32_t), s);
    run_components(F, (uint32_t)V, faces, nullptr, v.parent, v.named, vertex_label, st, s);
    if (F > 0) mesh_face_label_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, (uint32_t)V, faces, vertex_label, face_label);
}

size_t mesh_clean_workspace_bytes(long long V, long long F) { return clean_layout((size_t)V, (size_t)F, nullptr, nullptr); }

void launch_mesh_clean_plan(long long V, long long F, const float* vertices, const int* faces, long long min_faces,
                            double min_diag2, void* workspace, int* counts, hipStream_t s) {
    CleanView w;
    clean_layout((size_t)V, (size_t)F, static_cast<char*>(workspace), &w);
    const uint32_t Vu = (uint32_t)V;
    (void)hipMemsetAsync(w.ctl, 0, 4 * sizeof(uint32_t), s);
    if (F > 0) mesh_null_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, Vu, vertices, faces, w.alive0, w.ctl);
    run_dedup((uint32_t)F, faces, w.alive0, w.alive1, Vu, w.sb, w.ctl, s);
    run_components(F, Vu, faces, w.alive1, w.parent, w.named, w.label, w.ctl, s);
    if (V > 0) {
        mesh_comp_init_k<<<dim3(blocks_for(V > 6 ? V : 6)), dim3(MESH_THREADS), 0, s>>>(Vu, w.cfaces, w.cbox, w.mbox, w.used);
        if (F > 0) mesh_comp_faces_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, faces, w.alive1, w.label, w.cfaces);
        mesh_comp_box_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, vertices, w.label, w.cbox, w.mbox);
        mesh_comp_decide_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, w.label, min_faces, min_diag2, w.cbox, w.mbox, w.cfaces);
        if (F > 0) mesh_face_keep_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, faces, w.alive1, w.label, w.cfaces, w.fflag, w.used);
        exclusive_scan_u32(w.used, nullptr, w.used, (size_t)V, w.ctl + 1, w.scan_scratch, s);
    }
    if (F > 0) exclusive_scan_u32(w.fflag, nullptr, w.fflag, (size_t)F, w.ctl + 2, w.scan_scratch, s);
    mesh_counts_k<<<dim3(1), dim3(64), 0, s>>>(w.ctl + 1, w.ctl + 2, w.ctl, counts);
}

void launch_mesh_clean_emit(long long V, long long F, const float* vertices, const int* faces, const float* colors,
                            const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                            float* out_colors, int* vertex_index, int* face_index, hipStream_t s) {
    CleanView w;
    clean_layout((size_t)V, (size_t)F, static_cast<char*>(const_cast<void*>(workspace)), &w);
    if (n_vertices > 0)
        mesh_emit_vertices_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>((uint32_t)V, (uint32_t)n_vertices, w.used, vertices, colors,
                                                                               out_vertices, out_colors, vertex_index);
    if (n_faces > 0)
        mesh_emit_faces_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, (uint32_t)n_faces, w.fflag, faces, w.used, out_faces,
                                                                            face_index);
}

size_t mesh_decimate_workspace_bytes(long long V, long long F) { return dec_layout((size_t)V, (size_t)F, nullptr, nullptr); }

void launch_mesh_decimate_members(long long V, long long F, const float* vertices, const int* faces, void* workspace, hipStream_t s) {
    DecView w;
    dec_layout((size_t)V, (size_t)F, static_cast<char*>(workspace), &w);
    (void)hipMemsetAsync(w.ctl, 0, 4 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.box, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.box + 3, 0x00, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(w.member, 0, (size_t)V, s);
    mesh_named_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, (uint32_t)V, faces, w.member, w.ctl);
    mesh_member_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>((uint32_t)V, vertices, w.member, w.box);
}

void launch_mesh_decimate_probe(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                                int* count, hipStream_t s) {
    DecView w;
    dec_layout((size_t)V, (size_t)F, static_cast<char*>(workspace), &w);
    (void)hipMemsetAsync(count, 0, sizeof(int), s);
    const unsigned g = blocks_for(F);
    mesh_probe_k<<<dim3(g < 2048 ? g : 2048), dim3(MESH_THREADS), 0, s>>>(F, (uint32_t)V, vertices, faces, w.member, w.box, divisions,
                                                                         reinterpret_cast<uint32_t*>(count));
}

// returns which of the two sort buffers holds the sorted (key, vertex) pairs: emit's `sorted_in`
int launch_mesh_decimate_plan(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                              int* counts, hipStream_t s) {
    DecView w;
    dec_layout((size_t)V, (size_t)F, static_cast<char*>(workspace), &w);
    const uint32_t Vu = (uint32_t)V, Fu = (uint32_t)F;
    const uint32_t none_key = (uint32_t)divisions * (uint32_t)divisions * (uint32_t)divisions;  // <= 2^30
    mesh_cell_key_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, vertices, w.member, w.box, divisions, none_key, w.sbv.keys[0],
                                                                      w.sbv.vals[0]);
    const int fin = radix_sort_pairs(w.sbv.keys, w.sbv.vals, (size_t)V, 0, bits_for(none_key), w.sbv.scratch, s, false, false, nullptr, w.ctl);
    mesh_cell_head_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, w.sbv.keys[fin], none_key, w.rank);
    exclusive_scan_u32(w.rank, nullptr, w.rank, (size_t)V, nullptr, w.scan_scratch, s);
    mesh_vertex_cell_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, w.sbv.keys[fin], w.sbv.vals[fin], none_key, w.rank, w.vcell, w.cused);
    mesh_cell_faces_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, Vu, faces, w.vcell, w.tri, w.alive0);
    run_dedup(Fu, w.tri, w.alive0, w.alive1, Vu, w.sbf, w.ctl, s);
    mesh_cell_used_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, w.tri, w.alive1, w.fflag, w.cused);
    exclusive_scan_u32(w.cused, nullptr, w.cused, (size_t)V, w.ctl + 1, w.scan_scratch, s);
    exclusive_scan_u32(w.fflag, nullptr, w.fflag, (size_t)F, w.ctl + 2, w.scan_scratch, s);
    mesh_counts_k<<<dim3(1), dim3(64), 0, s>>>(w.ctl + 1, w.ctl + 2, w.ctl, counts);
    return fin;
}

void launch_mesh_decimate_emit(long long V, long long F, const float* vertices, const float* colors, int divisions, int sorted_in,
                               const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                               float* out_colors, int* cluster, hipStream_t s) {
    DecView w;
    dec_layout((size_t)V, (size_t)F, static_cast<char*>(const_cast<void*>(workspace)), &w);
    const uint32_t Vu = (uint32_t)V;
    const uint32_t none_key = (uint32_t)divisions * (uint32_t)divisions * (uint32_t)divisions;
    if (n_vertices > 0)
        mesh_cell_mean_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, (uint32_t)n_vertices, w.sbv.keys[sorted_in],
                                                                           w.sbv.vals[sorted_in], none_key, w.rank, w.cused, vertices,
                                                                           colors, out_vertices, out_colors);
    mesh_cluster_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>(Vu, (uint32_t)n_vertices, w.vcell, w.cused, cluster);
    if (n_faces > 0)
        mesh_emit_faces_k<<<dim3(blocks_for(F)), dim3(MESH_THREADS), 0, s>>>(F, (uint32_t)n_faces, w.fflag, w.tri, w.cused, out_faces,
                                                                            nullptr);
}

size_t mesh_normals_workspace_bytes(long long V, long long F) { return norm_layout((size_t)(3 * F), nullptr, nullptr); }

void launch_mesh_normals(long long V, long long F, const float* vertices, const int* faces, float* normals, int* status,
                         void* workspace, hipStream_t s) {
    NormView w;
    norm_layout((size_t)(3 * F), static_cast<char*>(workspace), &w);
    uint32_t* st = reinterpret_cast<uint32_t*>(status);
    (void)hipMemsetAsync(st, 0, sizeof(uint32_t), s);
    const long long C = 3 * F;
    int fin = 0;
    if (C > 0) {
        mesh_corner_k<<<dim3(blocks_for(C)), dim3(MESH_THREADS), 0, s>>>(C, (uint32_t)V, faces, w.sb.keys[0], w.sb.vals[0], st);
        fin = radix_sort_pairs(w.sb.keys, w.sb.vals, (size_t)C, 0, bits_for((uint32_t)V), w.sb.scratch, s, false, false, nullptr, st);
    }
    if (V > 0)
        mesh_normal_k<<<dim3(blocks_for(V)), dim3(MESH_THREADS), 0, s>>>((uint32_t)V, (uint32_t)C, vertices, faces, w.sb.keys[fin],
                                                                        w.sb.vals[fin], normals);
}

bool mesh_sizes_ok(long long V, long long F, long long min_each) {
    return V >= min_each && F >= min_each && V < SORT_MAX_KEYS && 3 * F < SORT_MAX_KEYS;
}
int mesh_divisions(const char* fn, int divisions) {
    if (divisions < 1 || divisions > GOI_MESH_MAX_DIVISIONS) return fail(std::string(fn) + ": need 1 <= divisions <= 1024");
    return 0;
}

}  // namespace

int mesh_sizes(const char* fn, long long V, long long F, long long min_each) {
    if (!mesh_sizes_ok(V, F, min_each))
        return fail(std::string(fn) + ": need " + std::to_string(min_each) + " <= V, F and V, 3 F < 2^30");
    return 0;
}

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_mesh_components_workspace_bytes(long long V, long long F) {
    return mesh_sizes_ok(V, F, 0) ? mesh_components_workspace_bytes(V, F) : 0;
}

int goi_mesh_components(long long V, long long F, const int* faces, int* vertex_label, int* face_label, int* status,
                        void* workspace, void* stream) {
    const char* fn = "goi_mesh_components";
    if (mesh_sizes(fn, V, F, 0) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (!status || (V > 0 && !vertex_label) || (F > 0 && (!faces || !face_label)))
        return fail(std::string(fn) + ": a required pointer is NULL");
    launch_mesh_components(V, F, faces, vertex_label, face_label, status, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_mesh_clean_workspace_bytes(long long V, long long F) {
    return mesh_sizes_ok(V, F, 1) ? mesh_clean_workspace_bytes(V, F) : 0;
}

int goi_mesh_clean_plan(long long V, long long F, const float* vertices, const int* faces, long long min_faces, double min_diag2,
                        void* workspace, int* counts, void* stream) {
    const char* fn = "goi_mesh_clean_plan";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (!vertices || !faces || !counts) return fail(std::string(fn) + ": NULL vertices, faces or counts");
    if (!(min_diag2 >= 0.0)) return fail(std::string(fn) + ": need min_diag2 >= 0");
    launch_mesh_clean_plan(V, F, vertices, faces, min_faces, min_diag2, workspace, counts, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_mesh_clean_emit(long long V, long long F, const float* vertices, const int* faces, const float* colors,
                        const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                        float* out_colors, int* vertex_index, int* face_index, void* stream) {
    const char* fn = "goi_mesh_clean_emit";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (n_vertices < 0 || n_vertices > V || n_faces < 0 || n_faces > F) return fail(std::string(fn) + ": counts out of range");
    if (!vertices || !faces) return fail(std::string(fn) + ": NULL vertices or faces");
    if ((n_vertices > 0 && (!out_vertices || !vertex_index)) || (n_faces > 0 && (!out_faces || !face_index)))
        return fail(std::string(fn) + ": NULL output");
    if (colors && n_vertices > 0 && !out_colors) return fail(std::string(fn) + ": colors need out_colors");
    launch_mesh_clean_emit(V, F, vertices, faces, colors, workspace, n_vertices, n_faces, out_vertices, out_faces, out_colors,
                           vertex_index, face_index, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_mesh_decimate_workspace_bytes(long long V, long long F) {
    return mesh_sizes_ok(V, F, 1) ? mesh_decimate_workspace_bytes(V, F) : 0;
}

int goi_mesh_decimate_members(long long V, long long F, const float* vertices, const int* faces, void* workspace, void* stream) {
    const char* fn = "goi_mesh_decimate_members";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (!vertices || !faces) return fail(std::string(fn) + ": NULL vertices or faces");
    launch_mesh_decimate_members(V, F, vertices, faces, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_mesh_decimate_probe(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                            int* count, void* stream) {
    const char* fn = "goi_mesh_decimate_probe";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0 || mesh_divisions(fn, divisions) < 0) return -1;
    if (!vertices || !faces || !count) return fail(std::string(fn) + ": NULL vertices, faces or count");
    launch_mesh_decimate_probe(V, F, vertices, faces, divisions, workspace, count, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_mesh_decimate_plan(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                           int* counts, void* stream) {
    const char* fn = "goi_mesh_decimate_plan";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0 || mesh_divisions(fn, divisions) < 0) return -1;
    if (!vertices || !faces || !counts) return fail(std::string(fn) + ": NULL vertices, faces or counts");
    const int fin = launch_mesh_decimate_plan(V, F, vertices, faces, divisions, workspace, counts, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return fin;
}

int goi_mesh_decimate_emit(long long V, long long F, const float* vertices, const float* colors, int divisions, int sorted_in,
                           const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                           float* out_colors, int* cluster, void* stream) {
    const char* fn = "goi_mesh_decimate_emit";
    if (mesh_sizes(fn, V, F, 1) < 0 || check_workspace(fn, workspace) < 0 || mesh_divisions(fn, divisions) < 0) return -1;
    if (sorted_in != 0 && sorted_in != 1) return fail(std::string(fn) + ": sorted_in must be what goi_mesh_decimate_plan returned");
    if (n_vertices < 0 || n_vertices > V || n_faces < 0 || n_faces > F) return fail(std::string(fn) + ": counts out of range");
    if (!vertices || !cluster) return fail(std::string(fn) + ": NULL vertices or cluster");
    if ((n_vertices > 0 && !out_vertices) || (n_faces > 0 && !out_faces)) return fail(std::string(fn) + ": NULL output");
    if (colors && n_vertices > 0 && !out_colors) return fail(std::string(fn) + ": colors need out_colors");
    launch_mesh_decimate_emit(V, F, vertices, colors, divisions, sorted_in, workspace, n_vertices, n_faces, out_vertices, out_faces,
                              out_colors, cluster, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_mesh_normals_workspace_bytes(long long V, long long F) {
    return mesh_sizes_ok(V, F, 0) ? mesh_normals_workspace_bytes(V, F) : 0;
}

int goi_mesh_normals(long long V, long long F, const float* vertices, const int* faces, float* normals, int* status,
                     void* workspace, void* stream) {
    const char* fn = "goi_mesh_normals";
    if (mesh_sizes(fn, V, F, 0) < 0 || check_workspace(fn, workspace) < 0) return -1;
    if (!status || (V > 0 && (!vertices || !normals)) || (F > 0 && !faces)) return fail(std::string(fn) + ": a required pointer is NULL");
    launch_mesh_normals(V, F, vertices, faces, normals, status, workspace, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
