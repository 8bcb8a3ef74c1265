// nb_ray_bounds.hip — rays bounded by the posed body instead of its box: nb_depth_range_widen, between nb_body_depth_range
// (nb_silhouette.hip) and nb_raygen_body (nb_raygen.hip).
//
// nb_body_depth_range (nb_silhouette.hip) gives every pixel of the rendered camera the camera-depth interval of the body's triangles
// that cover it.  get_rays (zju3dv/neuralbody lib/utils/if_nerf/if_nerf_data_utils.py:8-21) does not normalise ray_d, so with K's last
// row (0, 0, 1) the point o + t ray_d has camera depth t: the interval cuts get_near_far's [near, far] directly.
//   nb_depth_range_widen  the clothing margin in pixels (a border x border window, nb_mask_dilate's) and one interval per aligned
//                         tile x tile block; min and max are exact, so the two steps are one min / max over a clipped rectangle,
//                         taken here as a pass along the rows into LDS and a pass down the columns out of it
//   nb_raygen_body        nb_raygen with near = max(near, lo - margin), far = min(far, hi + margin) and the rays without an interval
//                         left dropped: nb_raygen's kernels, in nb_raygen.hip
#include "nb_common.h"

namespace {

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
