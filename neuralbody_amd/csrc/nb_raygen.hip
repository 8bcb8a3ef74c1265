// nb_raygen.hip — full-image ray generation + SMPL-bbox intersection + compaction on device.
//
// Restates (zju3dv/neuralbody):
//   lib/utils/if_nerf/if_nerf_data_utils.py:8-21   get_rays      (float64 like numpy: K is float64)
//   lib/utils/if_nerf/if_nerf_data_utils.py:54-69  get_near_far  (float32; uses the FIRST ray's origin)
//   lib/utils/render_utils.py:120-137              image_rays    (cast to float32, compact by mask)
// One thread per pixel; mask -> exclusive scan -> ordered compaction, so the surviving rays keep
// the reference's row-major pixel order (visualizers re-assemble with img[mask_at_box] = rgb).
// nb_raygen_body is the same host function and the same two kernels, instantiated with the cut of [near, far] by the posed body's
// per-pixel depth interval (nb_body_depth_range of nb_silhouette.hip, widened by nb_ray_bounds.hip).
#include "nb_ray.h"
#include "nb_scan.h"

namespace {

using nbray::near_far;
using nbray::pixel_ray;
using nbray::RayCam;

// nb_raygen_body's cut of [near, far] by the pixel's depth interval: lo / hi are one fp32 operation each
__device__ __forceinline__ bool body_cut(float2 r, float margin, float &near, float &far) {
#pragma clang fp contract(off)
    const float lo = r.x - margin, hi = r.y + margin;
    near = fmaxf(near, lo);
    far = fminf(far, hi);
    return near < far;
}

// BODY: nb_raygen_body, the cut applied and a ray it empties dropped; without it `range` and `margin` are not read
template <bool BODY>
__global__ void ray_flag_kernel(RayCam c, int H, int W, const float2 *__restrict__ range, float margin, int *__restrict__ flags,
                                uint8_t *__restrict__ mask) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W) return;
    float o[3], d[3], near, far;
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
    bool hit = near_far(c, o, d, &near, &far);
    if (BODY) hit = body_cut(range[p], margin, near, far) && hit;  // a pixel outside the box stays dropped
    flags[p] = hit;
    mask[p] = hit;
}

template <bool BODY>
__global__ void ray_emit_kernel(RayCam c, int H, int W, const float2 *__restrict__ range, float margin, const int *__restrict__ flags,
                                const int *__restrict__ pos, float *__restrict__ ray_o, float *__restrict__ ray_d,
                                float *__restrict__ near_out, float *__restrict__ far_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W || !flags[p]) return;
    float o[3], d[3], near, far;
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
    near_far(c, o, d, &near, &far);
    if (BODY) body_cut(range[p], margin, near, far);
    const long long r = pos[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ray_o[r * 3 + a] = o[a];
        ray_d[r * 3 + a] = d[a];
    }
    near_out[r] = near;
    far_out[r] = far;
}

__global__ void mask_flag_kernel(const uint8_t *__restrict__ mask, long long n, int *__restrict__ flags) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) flags[p] = mask[p] != 0;
}

// img[p] = mask[p] ? rgb_map[pos[p]] * scale : background; optional channel flip (the demo visualizer writes BGR)
__global__ void image_assemble_kernel(const int *__restrict__ flags, const int *__restrict__ pos, long long n,
                                      long long n_rays, const float *__restrict__ rgb_map,
                                      const float *__restrict__ depth_map, float bkgd, int bgr, float scale,
                                      float *__restrict__ img, float *__restrict__ depth) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float c[3] = {bkgd, bkgd, bkgd}, d = 0.f;
    const long long r = pos[p];
    if (flags[p] && r < n_rays) {
        c[0] = rgb_map[r * 3 + 0];
        c[1] = rgb_map[r * 3 + 1];
        c[2] = rgb_map[r * 3 + 2];
        if (depth_map) d = depth_map[r];
    }
    img[p * 3 + 0] = (bgr ? c[2] : c[0]) * scale;
    img[p * 3 + 1] = c[1] * scale;
    img[p * 3 + 2] = (bgr ? c[0] : c[2]) * scale;
    if (depth) depth[p] = d;
}

// both entries: `what` names the caller in the messages; BODY: nb_raygen_body, with its three refusals and the cut in both kernels
template <bool BODY>
int raygen(const char *what, int32_t H, int32_t W, const double K[9], const double R[9], const double T[3], const float bounds[6],
           const float *range, float margin, float *ray_o, float *ray_d, float *near, float *far, uint8_t *mask_at_box, int32_t *n_rays,
           void *scratch, void *stream) {
    NB_REQUIRE(K && R && T && bounds && (range || !BODY) && ray_o && ray_d && near && far && mask_at_box && n_rays && scratch,
               "%s: NULL pointer", what);
    NB_REQUIRE(H > 0 && W > 0, "%s: H = %d, W = %d", what, H, W);
    if (BODY) {
        NB_REQUIRE(K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0,
                   "%s: K's last row is (%g, %g, %g), not (0, 0, 1): a ray's parameter is not its camera depth", what, K[6], K[7], K[8]);
        NB_REQUIRE(margin >= 0.f && margin <= 3.4028234e38f, "%s: margin = %g (finite, >= 0)", what, (double)margin);
        NB_REQUIRE(((uintptr_t)range & 7) == 0, "%s: range must be 8-byte aligned", what);
    }
    RayCam c;
    NB_REQUIRE(nbray::make_cam(K, R, T, bounds, &c), "%s: K is singular", what);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    int *flags, *pos, *bs;
    nb_scan_carve(scratch, n, &flags, &pos, &bs);
    const dim3 grd(nb_ceil_div(n, 256)), blk(256);
    hipLaunchKernelGGL(ray_flag_kernel<BODY>, grd, blk, 0, st, c, H, W, (const float2 *)range, margin, flags, mask_at_box);
    if (int rc = nb_exclusive_scan(flags, pos, n_rays, n, bs, st)) return rc;
    hipLaunchKernelGGL(ray_emit_kernel<BODY>, grd, blk, 0, st, c, H, W, (const float2 *)range, margin, flags, pos, ray_o, ray_d, near, far);
    NB_CHECK_LAUNCH(what);
    return NB_OK;
}

}  // namespace

extern "C" int nb_raygen(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3],
                         const float bounds[6], float *ray_o, float *ray_d, float *near, float *far,
                         uint8_t *mask_at_box, int32_t *n_rays, void *scratch, void *stream) {
    return raygen<false>("nb_raygen", H, W, K, R, T, bounds, nullptr, 0.f, ray_o, ray_d, near, far, mask_at_box, n_rays, scratch, stream);
}

// nb_raygen with near = max(near, lo - margin), far = min(far, hi + margin) of the pixel's depth interval in `range`
// (nb_body_depth_range, widened: nb_ray_bounds.hip has why the interval cuts [near, far] directly) and the rays it empties dropped
extern "C" int nb_raygen_body(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3], const float bounds[6],
                              const float *range, float margin, float *ray_o, float *ray_d, float *near, float *far,
                              uint8_t *mask_at_box, int32_t *n_rays, void *scratch, void *stream) {
    return raygen<true>("nb_raygen_body", H, W, K, R, T, bounds, range, margin, ray_o, ray_d, near, far, mask_at_box, n_rays, scratch,
                        stream);
}

extern "C" int nb_image_assemble(const uint8_t *mask_at_box, int64_t n_pixels, const float *rgb_map, const float *depth_map,
                                 int64_t n_rays, int white_bkgd, int bgr, float scale, float *img, float *depth,
                                 void *scratch, void *stream) {
    NB_REQUIRE(n_pixels >= 0 && n_rays >= 0, "nb_image_assemble: n_pixels = %lld, n_rays = %lld", (long long)n_pixels,
               (long long)n_rays);
    if (n_pixels == 0) return NB_OK;
    NB_REQUIRE(mask_at_box && img && scratch && (rgb_map || n_rays == 0), "nb_image_assemble: NULL pointer");
    NB_REQUIRE((depth == nullptr) == (depth_map == nullptr) || n_rays == 0, "nb_image_assemble: depth and depth_map go together");
    hipStream_t st = (hipStream_t)stream;
    int *flags, *pos, *bs;
    nb_scan_carve(scratch, n_pixels, &flags, &pos, &bs);
    const dim3 grd(nb_ceil_div(n_pixels, 256)), blk(256);
    hipLaunchKernelGGL(mask_flag_kernel, grd, blk, 0, st, mask_at_box, (long long)n_pixels, flags);
    // nobody needs the total on the host
    if (int rc = nb_exclusive_scan(flags, pos, nb_scan_total_slot(bs, n_pixels), n_pixels, bs, st)) return rc;
    hipLaunchKernelGGL(image_assemble_kernel, grd, blk, 0, st, flags, pos, (long long)n_pixels, (long long)n_rays, rgb_map,
                       depth_map, white_bkgd ? 1.f : 0.f, bgr, scale, img, depth);
    NB_CHECK_LAUNCH("nb_image_assemble");
    return NB_OK;
}
