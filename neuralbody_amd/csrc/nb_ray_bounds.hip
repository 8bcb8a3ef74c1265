// nb_ray_bounds.hip — rays bounded by the posed body instead of its box: nb_depth_range_widen and nb_raygen_body.
//
// nb_body_depth_range (nb_silhouette.hip) gives every pixel of the rendered camera the camera-depth interval of the body's triangles
// that cover it.  get_rays (zju3dv/neuralbody lib/utils/if_nerf/if_nerf_data_utils.py:8-21) does not normalise ray_d, so with K's last
// row (0, 0, 1) the point o + t ray_d has camera depth t: the interval cuts get_near_far's [near, far] directly.
//   nb_depth_range_widen  the clothing margin in pixels (a border x border window, nb_mask_dilate's) and one interval per aligned
//                         tile x tile block; min and max are exact, so the two steps are one min / max over a clipped rectangle,
//                         taken here as a pass along the rows into LDS and a pass down the columns out of it
//   nb_raygen_body        nb_raygen with near = max(near, lo - margin), far = min(far, hi + margin) and the rays without an interval
//                         left dropped
#include "nb_ray.h"
#include "nb_scan.h"

namespace {

using nbray::near_far;
using nbray::pixel_ray;
using nbray::RayCam;

constexpr int REGION = 16;                          // a workgroup's pixels: REGION x REGION, a multiple of every tile
constexpr int MAX_HALF = 127;                       // border <= 255
constexpr int MAX_ROWS = REGION + 2 * MAX_HALF;     // rows of the image a region's columns are folded over

// One workgroup per aligned 16 x 16 region of one image.  Pixel (x, y) of tile block [bx0, bx1] x [by0, by1] takes the min / max over
// the columns bx0 - half .. bx1 + half and the rows by0 - half .. by1 + half, both clipped to the image.
__global__ __launch_bounds__(256) void widen_kernel(const float2 *__restrict__ in, int H, int W, int half, int tile, int rx, int ry,
                                                    float2 *__restrict__ out) {
    __shared__ float2 rows[MAX_ROWS][REGION];
    const int img = blockIdx.x / (rx * ry), reg = blockIdx.x % (rx * ry);
    const int X0 = (reg % rx) * REGION, Y0 = (reg / rx) * REGION;
    const size_t base = (size_t)img * H * W;
    const int r0 = max(Y0 - half, 0), r1 = min(Y0 + REGION - 1 + half, H - 1);  // r1 - r0 < MAX_ROWS
    for (int e = threadIdx.x; e < (r1 - r0 + 1) * REGION; e += 256) {
        const int r = r0 + e / REGION, x = X0 + e % REGION;
        float2 m = make_float2(INFINITY, -INFINITY);
        if (x < W) {
            const int bx0 = x / tile * tile;
            const int c0 = max(bx0 - half, 0), c1 = min(bx0 + tile - 1 + half, W - 1);
            const float2 *__restrict__ row = in + base + (size_t)r * W;
            for (int c = c0; c <= c1; ++c) {
                const float2 v = row[c];
                m.x = fminf(m.x, v.x), m.y = fmaxf(m.y, v.y);
            }
        }
        rows[r - r0][e % REGION] = m;
    }
    __syncthreads();
    const int lx = threadIdx.x % REGION, x = X0 + lx, y = Y0 + threadIdx.x / REGION;
    if (x >= W || y >= H) return;
    const int by0 = y / tile * tile;
    const int a0 = max(by0 - half, 0), a1 = min(by0 + tile - 1 + half, H - 1);  // inside r0 .. r1: by0 >= Y0, by0 + tile <= Y0 + REGION
    float2 m = make_float2(INFINITY, -INFINITY);
    for (int r = a0; r <= a1; ++r) {
        const float2 v = rows[r - r0][lx];
        m.x = fminf(m.x, v.x), m.y = fmaxf(m.y, v.y);
    }
    out[base + (size_t)y * W + x] = m;
}

// nb_raygen's two kernels with the cut: lo / hi are one fp32 operation each
__device__ __forceinline__ bool body_cut(float2 r, float margin, float &near, float &far) {
#pragma clang fp contract(off)
    const float lo = r.x - margin, hi = r.y + margin;
    near = fmaxf(near, lo);
    far = fminf(far, hi);
    return near < far;
}

__global__ void body_flag_kernel(RayCam c, int H, int W, const float2 *__restrict__ range, float margin, int *__restrict__ flags,
                                 uint8_t *__restrict__ mask) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W) return;
    float o[3], d[3], near, far;
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
    bool hit = near_far(c, o, d, &near, &far);
    hit = body_cut(range[p], margin, near, far) && hit;
    flags[p] = hit;
    mask[p] = hit;
}

__global__ void body_emit_kernel(RayCam c, int H, int W, const float2 *__restrict__ range, float margin, const int *__restrict__ flags,
                                 const int *__restrict__ pos, float *__restrict__ ray_o, float *__restrict__ ray_d,
                                 float *__restrict__ near_out, float *__restrict__ far_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W || !flags[p]) return;
    float o[3], d[3], near, far;
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
    near_far(c, o, d, &near, &far);
    body_cut(range[p], margin, near, far);
    const long long r = pos[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ray_o[r * 3 + a] = o[a];
        ray_d[r * 3 + a] = d[a];
    }
    near_out[r] = near;
    far_out[r] = far;
}

}  // namespace

extern "C" int nb_depth_range_widen(const float *range_in, int32_t n, int32_t H, int32_t W, int32_t border, int32_t tile,
                                    float *range_out, void *stream) {
    NB_REQUIRE(range_in && range_out && range_in != range_out, "nb_depth_range_widen: NULL pointer, or range_out is range_in");
    NB_REQUIRE(n >= 1 && H >= 1 && W >= 1 && (long long)n * H * W <= 2147483647ll,
               "nb_depth_range_widen: n = %d, H = %d, W = %d (all >= 1, at most 2^31 - 1 pixels)", n, H, W);
    NB_REQUIRE(border >= 1 && border % 2 == 1 && border <= 2 * MAX_HALF + 1, "nb_depth_range_widen: border = %d (odd, 1..255)", border);
    NB_REQUIRE(tile == 1 || tile == 2 || tile == 4 || tile == 8 || tile == 16, "nb_depth_range_widen: tile = %d (1, 2, 4, 8 or 16)", tile);
    NB_REQUIRE((((uintptr_t)range_in | (uintptr_t)range_out) & 7) == 0, "nb_depth_range_widen: the ranges must be 8-byte aligned");
    const int rx = nb_ceil_div(W, REGION), ry = nb_ceil_div(H, REGION);
    NB_REQUIRE((long long)n * rx * ry <= 2147483647ll, "nb_depth_range_widen: n = %d images of %d x %d are too many", n, H, W);
    hipLaunchKernelGGL(widen_kernel, dim3(n * rx * ry), dim3(256), 0, (hipStream_t)stream, (const float2 *)range_in, H, W, border / 2, tile,
                       rx, ry, (float2 *)range_out);
    NB_CHECK_LAUNCH("nb_depth_range_widen");
    return NB_OK;
}

extern "C" int nb_raygen_body(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3], const float bounds[6],
                              const float *range, float margin, float *ray_o, float *ray_d, float *near, float *far,
                              uint8_t *mask_at_box, int32_t *n_rays, void *scratch, void *stream) {
    NB_REQUIRE(K && R && T && bounds && range && ray_o && ray_d && near && far && mask_at_box && n_rays && scratch,
               "nb_raygen_body: NULL pointer");
    NB_REQUIRE(H > 0 && W > 0, "nb_raygen_body: H = %d, W = %d", H, W);
    NB_REQUIRE(K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0,
               "nb_raygen_body: K's last row is (%g, %g, %g), not (0, 0, 1): a ray's parameter is not its camera depth", K[6], K[7], K[8]);
    NB_REQUIRE(margin >= 0.f && margin <= 3.4028234e38f, "nb_raygen_body: margin = %g (finite, >= 0)", (double)margin);
    NB_REQUIRE(((uintptr_t)range & 7) == 0, "nb_raygen_body: range must be 8-byte aligned");
    RayCam c;
    NB_REQUIRE(nbray::make_cam(K, R, T, bounds, &c), "nb_raygen_body: K is singular");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    int *flags, *pos, *bs;
    nb_scan_carve(scratch, n, &flags, &pos, &bs);
    const dim3 grd(nb_ceil_div(n, 256)), blk(256);
    hipLaunchKernelGGL(body_flag_kernel, grd, blk, 0, st, c, H, W, (const float2 *)range, margin, flags, mask_at_box);
    if (int rc = nb_exclusive_scan(flags, pos, n_rays, n, bs, st)) return rc;
    hipLaunchKernelGGL(body_emit_kernel, grd, blk, 0, st, c, H, W, (const float2 *)range, margin, flags, pos, ray_o, ray_d, near, far);
    NB_CHECK_LAUNCH("nb_raygen_body");
    return NB_OK;
}
