// Device helpers shared by the two per-Gaussian units, preprocess_fwd.hip and preprocess_bwd.hip: what BOTH kernels restate of
// the reference's projection (a helper only one of them uses lives in that unit).  Both units are compiled with
// -ffp-contract=off, so the statements below round the same way in the forward and in the backward that re-derives from them.
#pragma once

#include "gmath.h"

namespace goi {

__device__ __forceinline__ M3 rotation_from_quat(float r, float x, float y, float z) {
    return make_m3(1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                   2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                   2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y));
}

struct Cov2D {
    M3 T, Vrk, W;
    V3 t;
    float txtz, tytz, limx, limy;
    M3 cov;
};

__device__ __forceinline__ void ewa_cov2d(V3 mean, float fx, float fy, float tan_fovx, float tan_fovy,
                                          const float* cov3D, const float* view, Cov2D& c) {
    V3 t = xform_point_4x3(mean, view);
    c.limx = 1.3f * tan_fovx;
    c.limy = 1.3f * tan_fovy;
    c.txtz = t.x / t.z;
    c.tytz = t.y / t.z;
    t.x = fminf(c.limx, fmaxf(-c.limx, c.txtz)) * t.z;
    t.y = fminf(c.limy, fmaxf(-c.limy, c.tytz)) * t.z;
    c.t = t;
    M3 J = make_m3(fx / t.z, 0.0f, -(fx * t.x) / (t.z * t.z), 0.0f, fy / t.z, -(fy * t.y) / (t.z * t.z), 0.f, 0.f, 0.f);
    c.W = make_m3(view[0], view[4], view[8], view[1], view[5], view[9], view[2], view[6], view[10]);
    c.T = mul(c.W, J);
    c.Vrk = make_m3(cov3D[0], cov3D[1], cov3D[2], cov3D[1], cov3D[3], cov3D[4], cov3D[2], cov3D[4], cov3D[5]);
    c.cov = mul(mul(transpose(c.T), transpose(c.Vrk)), c.T);
}

// The camera arrays are tiny, uniform device arrays: every thread reads them through the scalar
// cache into registers once.
struct Camera {
    float view[16], proj[16], campos[3];
};
__device__ __forceinline__ Camera load_camera(const float* __restrict__ v, const float* __restrict__ p,
                                              const float* __restrict__ c) {
    Camera cam;
#pragma unroll
    for (int i = 0; i < 16; i++) cam.view[i] = v[i];
#pragma unroll
    for (int i = 0; i < 16; i++) cam.proj[i] = p[i];
#pragma unroll
    for (int i = 0; i < 3; i++) cam.campos[i] = c[i];
    return cam;
}

}  // namespace goi
