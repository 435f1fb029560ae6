// Non-rigid edits of a selection of Gaussians: as-rigid-as-possible deformation over a graph of control nodes (embedded
// deformation, Sumner et al. 2007; ARAP, Sorkine & Alexa 2007).  goi_hyperplane_amd/deform.py; DESIGN.md section 4.33.
//
//     E = sum_i sum_{j = idx[i,m], an edge} w[i,m] |(y_i - y_j) - R_i (x_i - x_j)|^2      x: rest, y: deformed, R_i = R(q_i)
//
// Entry (i, m) of the node graph idx [M,k] is an EDGE iff 0 <= idx[i,m] < M and idx[i,m] != i: a -1 tail, an id out of range and
// a self edge are skipped and never used as an address.  An edge that a row lists twice is two edges (smooth.hip's rule: the
// transpose lists it twice as well, so both ends see the same weights).
//
//   deform_positions_k   A lane per node, Jacobi: reads the OLD y and q of every node, writes the new y to the other buffer.  A
//                        constrained node takes its target.  A free node sums  w ((y_j - y_i) + R_i e_ij)  over its out-edges in row
//                        order, then  w ((y_m - y_i) - R_m e_mi)  over its in-edges in in_edge order (e_ab = x_a - x_b), divides by
//                        the summed weights W and adds `relax` times that: y_i + relax (yhat_i - y_i), which is (1 - relax) y_i +
//                        relax yhat_i written so that an undeformed graph gives exact zeros.  W <= 0 (no edge) keeps y.
//   deform_rotations_k   A lane per node: A_i = sum over out-edges of w (y_i - y_j)(x_i - x_j)^T, then polar_iters steps of the
//                        warm-started quaternion iteration of Mueller et al. 2016: omega = (sum_c r_c x a_c) / (|sum_c r_c . a_c|
//                        + 1e-9) over the columns of R(q) and A, q <- normalize(exp(omega) (x) q).  A zero torque (A = 0, rank-1 A)
//                        leaves q bit for bit where it was, and so does an |omega| that is not finite (the denominator can be
//                        1e-9 under a large torque): sin and cos of it would be NaN and poison every later iteration.
//   goi_deform_solve     enqueues `iterations` pairs (positions, then rotations: the q it returns are the rotations OF the y it
//                        returns), y ping-ponging between the caller's buffer and the workspace.  No read-back, no barrier.
//   deform_energy_k / deform_energy_final_k   E in float64: a thread adds the rows it owns in ascending order, the wave butterfly,
//                        the waves in order, ONE workgroup adds the partials the same way (pose.hip's order).
//   deform_apply_k<R>    The hot path.  A workgroup is ONE wave that owns 64 consecutive Gaussians (edit_transform_k's mapping).  A
//                        row that is selected and bound to a node blends its nodes' motions with weights exp(-(d_a^2 - d_0^2) /
//                        (2 sigma^2)): position from the REST row, q_g = normalize(sum w_a s_a q_a) times the REST quaternion, and
//                        every band of the REST _features_rest row times D_l(R(q_g)), built in the lane: the band is evaluated at
//                        2 l + 1 fixed directions turned by R^T, contracted with the row, and multiplied by the inverse of the basis
//                        at those directions (the constants arrive by value).  The wave's rest rows go through LDS as in edit.hip.
//                        A row whose q_g has a zero vector part copies the rest bits instead.  With `moments` the same q_g turns
//                        Adam first moments in place (R m, q_g (x) m, D_l m) and an identity row is not written.
//
// This TU is compiled with -ffp-contract=off: every product and every sum rounds once, in the order tests/deform_reference.py
// writes down.  No float atomics, no inline assembly.  C entries at the end of the file: goi_deform_* (include/goi_raster.h).
#include <type_traits>

#include "entry.h"
#include "rest_row.h"
#include "wave_util.h"
#include "workspace.h"

namespace goi {

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_WAVES = DF_THREADS / 64;
constexpr int DF_MAX_BLOCKS = 1024;             // the grid of deform_energy_k = the partials deform_energy_final_k sums
constexpr long long DF_MAX_ENTRIES = 1ll << 30;  // M * k below this, as for goi_knn_transpose
constexpr int DF_WAVE = 64;
constexpr int DF_KB_MAX = 8;

// R(q), row-major, of a (w, x, y, z) quaternion taken as unit
__device__ __forceinline__ void quat_matrix(const float* q, float* R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz);
    R[1] = 2.0f * (xy - wz);
    R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);
    R[4] = 1.0f - 2.0f * (xx + zz);
    R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);
    R[7] = 2.0f * (yz + wx);
    R[8] = 1.0f - 2.0f * (xx + yy);
}

// R(q) - I from the quaternion's terms: no `1 -` is written, so the identity gives nine exact zeros
__device__ __forceinline__ void quat_matrix_minus_identity(const float* q, float* R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = -2.0f * (yy + zz);
    R[1] = 2.0f * (xy - wz);
    R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);
    R[4] = -2.0f * (xx + zz);
    R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);
    R[7] = 2.0f * (yz + wx);
    R[8] = -2.0f * (xx + yy);
}

// r = R v, each component (R[i][0] v0 + R[i][1] v1) + R[i][2] v2
__device__ __forceinline__ void rotate3(const float* R, float v0, float v1, float v2, float* r) {
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = (R[3 * i] * v0 + R[3 * i + 1] * v1) + R[3 * i + 2] * v2;
}

// row <- a (x) row, the Hamilton product of (w, x, y, z) quaternions, each component summed left to right
__device__ __forceinline__ void quat_left(const float* a, float* __restrict__ row) {
    const float b0 = row[0], b1 = row[1], b2 = row[2], b3 = row[3];
    row[0] = ((a[0] * b0 - a[1] * b1) - a[2] * b2) - a[3] * b3;
    row[1] = ((a[0] * b1 + a[1] * b0) + a[2] * b3) - a[3] * b2;
    row[2] = ((a[0] * b2 - a[1] * b3) + a[2] * b0) + a[3] * b1;
    row[3] = ((a[0] * b3 + a[1] * b2) - a[2] * b1) + a[3] * b0;
}

// q / |q|, the norm summed left to right; a zero or non-finite norm leaves q as it is
__device__ __forceinline__ void quat_normalize(float* q) {
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(n > 0.0f) || n == INFINITY) return;
#pragma unroll
    for (int c = 0; c < 4; c++) q[c] = q[c] / n;
}

__device__ __forceinline__ bool node_edge(int M, int i, int32_t j) { return j >= 0 && j < M && j != i; }

// ---- the solve ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DF_THREADS) void deform_positions_k(int M, int k, const float* __restrict__ x,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                                 const int32_t* __restrict__ in_ptr,
                                                                 const int32_t* __restrict__ in_edge,
                                                                 const uint8_t* __restrict__ constrained,
                                                                 const float* __restrict__ target, float relax,
                                                                 const float* __restrict__ y, const float* __restrict__ q,
                                                                 float* __restrict__ y_new) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= M) return;
    float* out = y_new + 3 * (size_t)i;
    if (constrained && constrained[i]) {
        out[0] = target[3 * (size_t)i];
        out[1] = target[3 * (size_t)i + 1];
        out[2] = target[3 * (size_t)i + 2];
        return;
    }
    const float xi[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
    const float yi[3] = {y[3 * (size_t)i], y[3 * (size_t)i + 1], y[3 * (size_t)i + 2]};
    float Ri[9], acc[3] = {0.f, 0.f, 0.f}, W = 0.f, r[3];
    quat_matrix(q + 4 * (size_t)i, Ri);
    for (int m = 0; m < k; m++) {
        const size_t e = (size_t)i * (size_t)k + (size_t)m;
        const int32_t j = idx[e];
        if (!node_edge(M, i, j)) continue;
        const float w = weight ? weight[e] : 1.0f;
        const float* xj = x + 3 * (size_t)j;
        const float* yj = y + 3 * (size_t)j;
        rotate3(Ri, xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2], r);
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * ((yj[c] - yi[c]) + r[c]);
        W = W + w;
    }
    const int n = M * k;  // (below 2^30: the entry checks)
    const int lo = min(max(in_ptr[i], 0), n), hi = min(max(in_ptr[i + 1], lo), n);
    for (int p = lo; p < hi; p++) {
        const int32_t e = in_edge[p];
        if (e < 0 || e >= n) continue;
        const int m = e / k;
        if (m == i) continue;
        const float w = weight ? weight[e] : 1.0f;
        const float* xm = x + 3 * (size_t)m;
        const float* ym = y + 3 * (size_t)m;
        float Rm[9];
        quat_matrix(q + 4 * (size_t)m, Rm);
        rotate3(Rm, xm[0] - xi[0], xm[1] - xi[1], xm[2] - xi[2], r);
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * ((ym[c] - yi[c]) - r[c]);
        W = W + w;
    }
    if (W > 0.f) {  // (a zero step keeps y's bits, the sign of a zero included)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float step = relax * (acc[c] / W);
            out[c] = step == 0.f ? yi[c] : yi[c] + step;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = yi[c];
    }
}

__global__ __launch_bounds__(DF_THREADS) void deform_rotations_k(int M, int k, const float* __restrict__ x,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                                 const float* __restrict__ y, int polar_iters,
                                                                 float* __restrict__ q) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= M) return;
    const float xi[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
    const float yi[3] = {y[3 * (size_t)i], y[3 * (size_t)i + 1], y[3 * (size_t)i + 2]};
    float A[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < k; m++) {
        const size_t e = (size_t)i * (size_t)k + (size_t)m;
        const int32_t j = idx[e];
        if (!node_edge(M, i, j)) continue;
        const float w = weight ? weight[e] : 1.0f;
        const float* xj = x + 3 * (size_t)j;
        const float* yj = y + 3 * (size_t)j;
        const float ex[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
#pragma unroll
        for (int r = 0; r < 3; r++) {  // w (d_r e_c): with y = x the matrix is symmetric bit for bit and the torque exactly zero
            const float d = yi[r] - yj[r];
#pragma unroll
            for (int c = 0; c < 3; c++) A[3 * r + c] = A[3 * r + c] + w * (d * ex[c]);
        }
    }
    float qi[4] = {q[4 * (size_t)i], q[4 * (size_t)i + 1], q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]};
    for (int it = 0; it < polar_iters; it++) {
        float R[9], t[3] = {0.f, 0.f, 0.f}, s = 0.f;
        quat_matrix(qi, R);
#pragma unroll
        for (int c = 0; c < 3; c++) {  // column c of R against column c of A
            const float r0 = R[c], r1 = R[3 + c], r2 = R[6 + c], a0 = A[c], a1 = A[3 + c], a2 = A[6 + c];
            t[0] = t[0] + (r1 * a2 - r2 * a1);
            t[1] = t[1] + (r2 * a0 - r0 * a2);
            t[2] = t[2] + (r0 * a1 - r1 * a0);
            s = s + ((r0 * a0 + r1 * a1) + r2 * a2);
        }
        const float den = fabsf(s) + 1e-9f;
        const float o0 = t[0] / den, o1 = t[1] / den, o2 = t[2] / den;
        const float th = sqrtf((o0 * o0 + o1 * o1) + o2 * o2);
        if (!(th > 0.f) || th == INFINITY) break;  // no torque, or an omega that overflowed (sum r . a = 0): q stays where it is
        const float h = 0.5f * th;
        const float f = sinf(h) / th;
        const float dq[4] = {cosf(h), f * o0, f * o1, f * o2};
        quat_left(dq, qi);
        quat_normalize(qi);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) q[4 * (size_t)i + c] = qi[c];
}

// ---- the energy, float64 --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* waves) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = waves[0];
#pragma unroll
    for (int w = 1; w < DF_WAVES; w++) total = total + waves[w];
    return total;
}

__global__ __launch_bounds__(DF_THREADS) void deform_energy_k(int M, int k, const float* __restrict__ x,
                                                              const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                              const float* __restrict__ y, const float* __restrict__ q,
                                                              double* __restrict__ partial) {
    __shared__ double waves[DF_WAVES];
    double sum = 0.0;
    for (long long i64 = (long long)blockIdx.x * DF_THREADS + threadIdx.x; i64 < M; i64 += (long long)gridDim.x * DF_THREADS) {
        const int i = (int)i64;
        const double w0 = q[4 * (size_t)i], qx = q[4 * (size_t)i + 1], qy = q[4 * (size_t)i + 2], qz = q[4 * (size_t)i + 3];
        const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - w0 * qz), 2.0 * (qx * qz + w0 * qy),
                             2.0 * (qx * qy + w0 * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - w0 * qx),
                             2.0 * (qx * qz - w0 * qy), 2.0 * (qy * qz + w0 * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
        double row = 0.0;
        for (int m = 0; m < k; m++) {
            const size_t e = (size_t)i * (size_t)k + (size_t)m;
            const int32_t j = idx[e];
            if (!node_edge(M, i, j)) continue;
            const double w = weight ? (double)weight[e] : 1.0;
            double ex[3], d2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++) ex[c] = (double)x[3 * (size_t)i + c] - (double)x[3 * (size_t)j + c];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double rot = (R[3 * r] * ex[0] + R[3 * r + 1] * ex[1]) + R[3 * r + 2] * ex[2];
                const double d = ((double)y[3 * (size_t)i + r] - (double)y[3 * (size_t)j + r]) - rot;
                d2 = d2 + d * d;
            }
            row = row + w * d2;
        }
        sum = sum + row;
    }
    const double total = block_sum(sum, waves);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(DF_THREADS) void deform_energy_final_k(int nblk, const double* __restrict__ partial,
                                                                    double* __restrict__ energy) {
    __shared__ double waves[DF_WAVES];
    double sum = 0.0;
    for (int b = threadIdx.x; b < nblk; b += DF_THREADS) sum = sum + partial[b];
    const double total = block_sum(sum, waves);
    if (threadIdx.x == 0) *energy = total;
}

int energy_blocks(int M) { return min((M + DF_THREADS - 1) / DF_THREADS, DF_MAX_BLOCKS); }

// Workspace of the solve: the second y buffer.  Of the energy: the per-workgroup partials.
size_t solve_layout(int M, char* base, float** y2) {
    Carver c(base);
    float* p = c.take<float>(at_least_one(3 * (size_t)M));
    if (y2) *y2 = p;
    return c.bytes();
}
size_t energy_layout(char* base, double** partial) {
    Carver c(base);
    double* p = c.take<double>(DF_MAX_BLOCKS);
    if (partial) *partial = p;
    return c.bytes();
}

// ---- the apply ---------------------------------------------------------------------------------------------------------------------
struct DeformApply {
    const uint8_t* selection;
    int invert, n_nodes, kb, moments;
    const int32_t* bind_idx;
    const float* bind_dist2;
    float inv_two_sigma2;
    const float *node_x, *node_y, *node_q;
    const float *src_xyz, *src_rotation, *src_rest;
    float *xyz, *rotation, *rest;
};

// band l of this project's real SH basis (cuda_rasterizer/auxiliary.h) at the unit direction (x, y, z): 2 l + 1 values
__device__ __forceinline__ void sh_band(float x, float y, float z, float* b, std::integral_constant<int, 3>) {
    const float C1 = 0.4886025119029199f;
    b[0] = -C1 * y;
    b[1] = C1 * z;
    b[2] = -C1 * x;
}
__device__ __forceinline__ void sh_band(float x, float y, float z, float* b, std::integral_constant<int, 5>) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[0] = 1.0925484305920792f * xy;
    b[1] = -1.0925484305920792f * yz;
    b[2] = 0.31539156525252005f * ((2.0f * zz - xx) - yy);
    b[3] = -1.0925484305920792f * xz;
    b[4] = 0.5462742152960396f * (xx - yy);
}
__device__ __forceinline__ void sh_band(float x, float y, float z, float* b, std::integral_constant<int, 7>) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y;
    b[0] = -0.5900435899266435f * y * (3.0f * xx - yy);
    b[1] = 2.890611442640554f * xy * z;
    b[2] = -0.4570457994644658f * y * ((4.0f * zz - xx) - yy);
    b[3] = 0.3731763325901154f * z * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
    b[4] = -0.4570457994644658f * x * ((4.0f * zz - xx) - yy);
    b[5] = 1.445305721320277f * z * (xx - yy);
    b[6] = -0.5900435899266435f * x * (xx - 3.0f * yy);
}

// The band of N = 2 l + 1 coefficients starting at coefficient `first` of a [.][3] row held in c, in place: c <- D_l(R) c per
// channel.  v[n] = sum_k Y_k(R^T d_n) c_k (k ascending), then c_i = sum_n inv[i][n] v[n] (n ascending).
template <int N>
__device__ __forceinline__ void rotate_band(const float* R, const float* dirs, const float* inv, float* c, int first) {
    float v[N][3];
#pragma unroll
    for (int n = 0; n < N; n++) {
        const float d0 = dirs[3 * n], d1 = dirs[3 * n + 1], d2 = dirs[3 * n + 2];
        const float u0 = (R[0] * d0 + R[3] * d1) + R[6] * d2;  // R^T d
        const float u1 = (R[1] * d0 + R[4] * d1) + R[7] * d2;
        const float u2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
        float b[N];
        sh_band(u0, u1, u2, b, std::integral_constant<int, N>());
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float acc = b[0] * c[first * 3 + ch];
#pragma unroll
            for (int k = 1; k < N; k++) acc = acc + b[k] * c[(first + k) * 3 + ch];
            v[n][ch] = acc;
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            float acc = inv[i * N] * v[0][ch];
#pragma unroll
            for (int n = 1; n < N; n++) acc = acc + inv[i * N + n] * v[n][ch];
            c[(first + i) * 3 + ch] = acc;
        }
    }
}

// The wave's 64 rows of R floats from src through LDS to dst; only the rows in `ballot` are read and written, a row with `turn`
// multiplied by its D_l(Rg) on the way (the others are copied).  edit.hip's edit_rest with a rotation per lane.
template <int R>
__device__ __forceinline__ void apply_rest(const float* src, float* dst, long long base_row,  // (src may be dst)
                                           unsigned long long ballot, bool turn, int lane, const float* Rg, const GoiDeformSH& sh,
                                           float* __restrict__ lds) {
    constexpr int STRIDE = RestRow<R>::STRIDE;
    const long long e0 = base_row * R;
    const int safe = __builtin_ctzll(ballot) * R;  // a word of a row in the ballot: what the lanes of the other rows read instead
    float v[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * DF_WAVE + lane;
        v[k] = src[e0 + (((ballot >> (e / R)) & 1ull) ? e : safe)];
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * DF_WAVE + lane, row = e / R;
        lds[row * STRIDE + (e - row * R)] = v[k];
    }
    __syncthreads();
    if (turn) {
        float* mine = lds + lane * STRIDE;
        float c[R];
#pragma unroll
        for (int j = 0; j < R; j++) c[j] = mine[j];
        rotate_band<3>(Rg, sh.dirs1, sh.inv1, c, 0);
        if constexpr (R > 9) rotate_band<5>(Rg, sh.dirs2, sh.inv2, c, 3);
        if constexpr (R > 24) rotate_band<7>(Rg, sh.dirs3, sh.inv3, c, 8);
#pragma unroll
        for (int j = 0; j < R; j++) mine[j] = c[j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * DF_WAVE + lane, row = e / R;
        v[k] = lds[row * STRIDE + (e - row * R)];
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int e = k * DF_WAVE + lane;
        if ((ballot >> (e / R)) & 1ull) dst[e0 + e] = v[k];
    }
    __syncthreads();  // the buffer is free again
}

template <int R>
__global__ __launch_bounds__(DF_WAVE) void deform_apply_k(long long P, const GoiDeformSH sh, const DeformApply a) {
    __shared__ float lds[R ? DF_WAVE * RestRow<R>::STRIDE : 1];
    const int lane = threadIdx.x;
    const long long base = (long long)blockIdx.x * DF_WAVE;
    const long long g = base + lane;
    const bool sel = g < P && edit_selected(a.selection, a.invert, g);
    // the row's nodes: entry m is used iff its id is a node and its distance is finite; the first such entry is the reference
    int node[DF_KB_MAX];
    float wgt[DF_KB_MAX];
    int first = -1;
    if (sel) {
        float d0 = 0.f, wsum = 0.f;
#pragma unroll
        for (int m = 0; m < DF_KB_MAX; m++) {
            node[m] = -1;
            wgt[m] = 0.f;
            if (m < a.kb) {
                const int32_t id = a.bind_idx[g * a.kb + m];
                const float d = a.bind_dist2[g * a.kb + m];
                if (id >= 0 && id < a.n_nodes && fabsf(d) < INFINITY) {
                    if (first < 0) {
                        first = m;
                        d0 = d;
                    }
                    node[m] = id;
                    wgt[m] = expf(-((d - d0) * a.inv_two_sigma2));
                    wsum = wsum + wgt[m];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < DF_KB_MAX; m++) wgt[m] = wgt[m] / wsum;  // (unused entries: 0 / wsum, never looked at)
    }
    const bool bound = sel && first >= 0;
    const unsigned long long ballot = __ballot(bound);
    if (!ballot) return;
    bool turn = false;
    float Rg[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (bound) {
        float qg[4] = {0.f, 0.f, 0.f, 0.f}, q1[4] = {1.f, 0.f, 0.f, 0.f}, acc[3] = {0.f, 0.f, 0.f};
        const float* xs = a.src_xyz ? a.src_xyz + 3 * g : nullptr;
        const bool move = !a.moments && xs;
        float px[3] = {0.f, 0.f, 0.f};
        if (xs) {
            px[0] = xs[0];
            px[1] = xs[1];
            px[2] = xs[2];
        }
#pragma unroll
        for (int m = 0; m < DF_KB_MAX; m++) {
            if (node[m] < 0) continue;
            const float* qa = a.node_q + 4 * (size_t)node[m];
            const float qn[4] = {qa[0], qa[1], qa[2], qa[3]};
            if (m == first) {
#pragma unroll
                for (int c = 0; c < 4; c++) q1[c] = qn[c];
            }
            const float dot = ((qn[0] * q1[0] + qn[1] * q1[1]) + qn[2] * q1[2]) + qn[3] * q1[3];
            const float ws = dot < 0.f ? -wgt[m] : wgt[m];
#pragma unroll
            for (int c = 0; c < 4; c++) qg[c] = qg[c] + ws * qn[c];
            if (move) {
                const float* xa = a.node_x + 3 * (size_t)node[m];
                const float* ya = a.node_y + 3 * (size_t)node[m];
                float Rm[9], r[3];
                quat_matrix_minus_identity(qn, Rm);
                rotate3(Rm, px[0] - xa[0], px[1] - xa[1], px[2] - xa[2], r);
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] = acc[c] + wgt[m] * ((ya[c] - xa[c]) + r[c]);
            }
        }
        quat_normalize(qg);
        turn = qg[1] != 0.f || qg[2] != 0.f || qg[3] != 0.f;
        if (turn) quat_matrix(qg, Rg);
        if (move) {  // (a zero displacement keeps the rest bits, the sign of a zero included)
            float* xd = a.xyz + 3 * g;
#pragma unroll
            for (int c = 0; c < 3; c++) xd[c] = acc[c] == 0.f ? px[c] : px[c] + acc[c];
        } else if (a.moments && a.xyz && turn) {  // a moment gets the linear part only
            float* md = a.xyz + 3 * g;
            float r[3];
            rotate3(Rg, md[0], md[1], md[2], r);
            md[0] = r[0];
            md[1] = r[1];
            md[2] = r[2];
        }
        if (a.rotation && (turn || !a.moments)) {
            const float* rs = a.moments ? a.rotation + 4 * g : a.src_rotation + 4 * g;
            float row[4] = {rs[0], rs[1], rs[2], rs[3]};
            if (turn) quat_left(qg, row);
            float* rd = a.rotation + 4 * g;
#pragma unroll
            for (int c = 0; c < 4; c++) rd[c] = row[c];
        }
    }
    if constexpr (R > 0) {
        if (a.rest) {
            // with moments the identity rows are neither read nor written
            const unsigned long long rows = a.moments ? __ballot(bound && turn) : ballot;
            if (rows) apply_rest<R>(a.moments ? a.rest : a.src_rest, a.rest, base, rows, bound && turn, lane, Rg, sh, lds);
        }
    }
}

void launch_apply(long long P, int Msh, const GoiDeformSH& sh, const DeformApply& a, hipStream_t s) {
    if (P <= 0) return;
    const dim3 grid((unsigned)((P + DF_WAVE - 1) / DF_WAVE)), block(DF_WAVE);
    const int R = a.rest ? 3 * (Msh - 1) : 0;
    if (R == 45)
        deform_apply_k<45><<<grid, block, 0, s>>>(P, sh, a);
    else if (R == 24)
        deform_apply_k<24><<<grid, block, 0, s>>>(P, sh, a);
    else if (R == 9)
        deform_apply_k<9><<<grid, block, 0, s>>>(P, sh, a);
    else
        deform_apply_k<0><<<grid, block, 0, s>>>(P, sh, a);
}

// M and k of the node graph
int check_graph(const char* fn, int M, int k) {
    if (M < 0) return fail(std::string(fn) + ": need M >= 0");
    if (k < 1) return fail(std::string(fn) + ": need k >= 1");
    if ((long long)M * k >= DF_MAX_ENTRIES) return fail(std::string(fn) + ": need M * k < 2^30");
    return 0;
}

bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

size_t goi_deform_solve_workspace_bytes(int M) { return M >= 0 && M < (1 << 30) ? solve_layout(M, nullptr, nullptr) : 0; }

int goi_deform_solve(int M, int k, const float* x, const int32_t* idx, const float* weight, const int32_t* in_ptr,
                     const int32_t* in_edge, const unsigned char* constrained, const float* target, int iterations, int polar_iters,
                     float relax, float* y, float* q, void* workspace, void* stream) {
    const char* fn = "goi_deform_solve";
    if (check_graph(fn, M, k) < 0) return -1;
    if (iterations < 0) return fail(std::string(fn) + ": need iterations >= 0");
    if (polar_iters < 0) return fail(std::string(fn) + ": need polar_iters >= 0");
    if (!(relax > 0.f && relax <= 1.f)) return fail(std::string(fn) + ": need 0 < relax <= 1");
    if (M == 0 || iterations == 0) return 0;  // y and q are the warm start
    if (!x || !idx || !in_ptr || !in_edge || !y || !q || (constrained && !target))
        return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned4(x) || misaligned4(idx) || misaligned4(weight) || misaligned4(in_ptr) || misaligned4(in_edge) ||
        misaligned4(target) || misaligned4(y) || misaligned4(q))
        return fail(std::string(fn) + ": x, idx, weight, in_ptr, in_edge, target, y and q must be 4-byte aligned");
    if (check_workspace(fn, workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* y2;
    solve_layout(M, static_cast<char*>(workspace), &y2);
    const dim3 grid((unsigned)((M + DF_THREADS - 1) / DF_THREADS)), block(DF_THREADS);
    float *cur = y, *other = y2;
    for (int it = 0; it < iterations; it++) {
        deform_positions_k<<<grid, block, 0, s>>>(M, k, x, idx, weight, in_ptr, in_edge, constrained, target, relax, cur, q, other);
        deform_rotations_k<<<grid, block, 0, s>>>(M, k, x, idx, weight, other, polar_iters, q);
        float* t = cur;
        cur = other;
        other = t;
    }
    if (cur != y) GOI_HIP(hipMemcpyAsync(y, cur, 3 * (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
    GOI_HIP(hipGetLastError());
    return 0;
}

size_t goi_deform_energy_workspace_bytes(int M) { return M >= 0 && M < (1 << 30) ? energy_layout(nullptr, nullptr) : 0; }

int goi_deform_energy(int M, int k, const float* x, const int32_t* idx, const float* weight, const float* y, const float* q,
                      double* energy, void* workspace, void* stream) {
    const char* fn = "goi_deform_energy";
    if (check_graph(fn, M, k) < 0) return -1;
    if (!energy || (M > 0 && (!x || !idx || !y || !q))) return fail(std::string(fn) + ": a required pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(energy) & 7) != 0) return fail(std::string(fn) + ": energy must be 8-byte aligned");
    if (misaligned4(x) || misaligned4(idx) || misaligned4(weight) || misaligned4(y) || misaligned4(q))
        return fail(std::string(fn) + ": x, idx, weight, y and q must be 4-byte aligned");
    if (check_workspace(fn, workspace) < 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial;
    energy_layout(static_cast<char*>(workspace), &partial);
    const int nblk = energy_blocks(M);
    if (nblk > 0) deform_energy_k<<<dim3(nblk), dim3(DF_THREADS), 0, s>>>(M, k, x, idx, weight, y, q, partial);
    deform_energy_final_k<<<dim3(1), dim3(DF_THREADS), 0, s>>>(nblk, partial, energy);
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_deform_apply(long long P, int M_sh, int n_nodes, int kb, const unsigned char* selection, int invert, const int32_t* bind_idx,
                     const float* bind_dist2, float sigma, const float* node_x, const float* node_y, const float* node_q,
                     const GoiDeformSH* sh, const float* src_xyz, const float* src_rotation, const float* src_features_rest,
                     float* xyz, float* rotation, float* features_rest, int moments, void* stream) {
    const char* fn = "goi_deform_apply";
    if (P < 0 || P >= (1ll << 31)) return fail(std::string(fn) + ": need 0 <= P < 2^31");
    if (M_sh != 1 && M_sh != 4 && M_sh != 9 && M_sh != 16) return fail(std::string(fn) + ": M must be 1, 4, 9 or 16");
    if (n_nodes < 0 || n_nodes >= (1 << 30)) return fail(std::string(fn) + ": need 0 <= n_nodes < 2^30");
    if (kb < 1 || kb > DF_KB_MAX) return fail(std::string(fn) + ": need 1 <= kb <= 8");
    if (P * kb >= (1ll << 31)) return fail(std::string(fn) + ": need P * kb < 2^31");
    if (!(sigma > 0.f) || sigma == INFINITY) return fail(std::string(fn) + ": sigma must be finite and > 0");
    if (moments != 0 && moments != 1) return fail(std::string(fn) + ": moments must be 0 or 1");
    if (!sh) return fail(std::string(fn) + ": the SH constants are NULL");
    if (P == 0 || n_nodes == 0) return 0;  // nothing is bound
    if (M_sh == 1 && features_rest) return fail(std::string(fn) + ": M = 1 has no features_rest");
    if (!bind_idx || !bind_dist2 || !node_q) return fail(std::string(fn) + ": a required pointer is NULL");
    if (!moments && (!node_x || !node_y || !src_xyz || !src_rotation || !xyz || !rotation || (M_sh > 1 && (!src_features_rest || !features_rest))))
        return fail(std::string(fn) + ": a required pointer is NULL");
    if (misaligned4(bind_idx) || misaligned4(bind_dist2) || misaligned4(node_x) || misaligned4(node_y) || misaligned4(node_q) ||
        misaligned4(src_xyz) || misaligned4(src_rotation) || misaligned4(src_features_rest) || misaligned4(xyz) ||
        misaligned4(rotation) || misaligned4(features_rest))
        return fail(std::string(fn) + ": every tensor must be 4-byte aligned");
    DeformApply a;
    a.selection = selection;
    a.invert = invert;
    a.n_nodes = n_nodes;
    a.kb = kb;
    a.moments = moments;
    a.bind_idx = bind_idx;
    a.bind_dist2 = bind_dist2;
    a.inv_two_sigma2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    a.node_x = node_x;
    a.node_y = node_y;
    a.node_q = node_q;
    a.src_xyz = moments ? nullptr : src_xyz;
    a.src_rotation = src_rotation;
    a.src_rest = src_features_rest;
    a.xyz = xyz;
    a.rotation = rotation;
    a.rest = M_sh > 1 ? features_rest : nullptr;
    launch_apply(P, M_sh, *sh, a, static_cast<hipStream_t>(stream));
    GOI_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
