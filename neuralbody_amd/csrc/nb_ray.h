// Internal: the camera block, the per-pixel ray and the ray / box intersection shared by nb_raygen.hip (full images) and
// nb_train_rays.hip (sampled training rays).
//
// Restates (zju3dv/neuralbody):
//   lib/utils/if_nerf/if_nerf_data_utils.py:8-21   get_rays      (float64 like numpy: K is float64)
//   lib/utils/if_nerf/if_nerf_data_utils.py:54-69  get_near_far  (float32 on the cast rays of a full image, float64 on the
//                                                                 rays of a training batch; uses the FIRST ray's origin,
//                                                                 which is every ray's origin)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace nbray {

struct RayCam {
    double Kinv[9];  // inv(K), row-major
    double R[9];
    double T[3];
    double o[3];  // -R^T T
    float bmin[3], bmax[3];
};

// The arithmetic below is written with plain operators under a contraction pragma of its own (as in nb_march_common.h): the `_rn`
// intrinsics are the plain operators to hipcc, which contracts them into FMAs across the inlined calls, so the norm used to be
// fma(dx, dx, dy * dy) + dz * dz and near / far of an oblique view differed from the reference's by up to 2 ulp
// (tests/test_gpu_raygen.py).  Under the pragma each operation is ONE IEEE operation, as in numpy; `/` and sqrtf are the correctly
// rounded ones of this toolchain.

// fp64 direction of the ray through pixel (px, py): pixel_world - rays_o before the cast
__device__ __forceinline__ void pixel_ray_f64(const RayCam &c, int px, int py, double (&d)[3]) {
#pragma clang fp contract(off)
    // xy1 is float32 in the reference (np.arange(..., dtype=float32)), promoted to float64 by np.dot
    const double x = (double)(float)px, y = (double)(float)py;
    double pc[3], pw[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)  // xy1 @ inv(K).T
        pc[a] = (x * c.Kinv[a * 3 + 0] + y * c.Kinv[a * 3 + 1]) + c.Kinv[a * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = pc[a] - c.T[a];
#pragma unroll
    for (int a = 0; a < 3; ++a)  // (pixel_camera - T) @ R
        pw[a] = (pc[0] * c.R[0 * 3 + a] + pc[1] * c.R[1 * 3 + a]) + pc[2] * c.R[2 * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = pw[a] - c.o[a];
}

__device__ __forceinline__ void pixel_ray(const RayCam &c, int px, int py, float (&o)[3], float (&d)[3]) {
    double dd[3];
    pixel_ray_f64(c, px, py, dd);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (float)dd[a];
        o[a] = (float)c.o[a];
    }
}

// get_near_far on the float32 rays of a full image (render_utils.py:126-127 casts before it intersects)
__device__ __forceinline__ bool near_far(const RayCam &c, const float (&o)[3], const float (&d)[3], float *near,
                                         float *far) {
#pragma clang fp contract(off)
    const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    float tn = -INFINITY, tf = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v = d[a] / n;
        if (v < 1e-5f && v > -1e-10f) v = 1e-5f;   // if_nerf_data_utils.py:58
        if (v > -1e-5f && v < 1e-10f) v = -1e-5f;  // :59 (order matters)
        const float t0 = (c.bmin[a] - o[a]) / v;
        const float t1 = (c.bmax[a] - o[a]) / v;
        tn = fmaxf(tn, fminf(t0, t1));
        tf = fminf(tf, fmaxf(t0, t1));
    }
    *near = tn / n;
    *far = tf / n;
    return tn < tf;
}

// get_near_far on the float64 rays of a training batch (if_nerf_data_utils.py:116-120 hands it get_rays' own arrays; the
// float32 bounds are promoted); near and far leave as float64 and are rounded once where they are stored (:134-135)
__device__ __forceinline__ bool near_far(const RayCam &c, const double (&d)[3], double *near, double *far) {
#pragma clang fp contract(off)
    const double n = __dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    double tn = -INFINITY, tf = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double v = d[a] / n;
        if (v < 1e-5 && v > -1e-10) v = 1e-5;   // if_nerf_data_utils.py:58
        if (v > -1e-5 && v < 1e-10) v = -1e-5;  // :59 (order matters)
        const double t0 = ((double)c.bmin[a] - c.o[a]) / v;
        const double t1 = ((double)c.bmax[a] - c.o[a]) / v;
        tn = fmax(tn, fmin(t0, t1));
        tf = fmin(tf, fmax(t0, t1));
    }
    *near = tn / n;
    *far = tf / n;
    return tn < tf;
}

inline bool inv3(const double *m, double *out) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det == 0.0 || det != det) return false;
    const double r = 1.0 / det;
    out[0] = (e * i - f * h) * r;
    out[1] = (c * h - b * i) * r;
    out[2] = (b * f - c * e) * r;
    out[3] = (f * g - d * i) * r;
    out[4] = (a * i - c * g) * r;
    out[5] = (c * d - a * f) * r;
    out[6] = (d * h - e * g) * r;
    out[7] = (b * g - a * h) * r;
    out[8] = (a * e - b * d) * r;
    return true;
}

// host: K, R (row-major 3x3), T (3) and the world AABB -> the camera block; false when K is singular
inline bool make_cam(const double K[9], const double R[9], const double T[3], const float bounds[6], RayCam *c) {
    if (!inv3(K, c->Kinv)) return false;
    for (int k = 0; k < 9; ++k) c->R[k] = R[k];
    for (int a = 0; a < 3; ++a) {
        c->T[a] = T[a];
        c->o[a] = -(R[0 * 3 + a] * T[0] + R[1 * 3 + a] * T[1] + R[2 * 3 + a] * T[2]);  // -R^T T
        c->bmin[a] = bounds[a];
        c->bmax[a] = bounds[3 + a];
    }
    return true;
}

}  // namespace nbray
