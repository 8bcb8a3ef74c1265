// Internal: the one window kernel behind nb_mask_dilate (nb_lattice.hip) and nb_mask_band (nb_image_prep.hip): a thread per pixel of
// a uint8 [n_views,H,W] stack folds the border x border neighbourhood around it (anchor = centre), pixels outside the image ignored.
// A FOLD is a small functor struct, default-constructed per pixel:
//     void take(unsigned byte)                   one pixel of the window
//     unsigned result(unsigned centre) const     the output byte; centre = the pixel's own byte
#pragma once
#include "nb_common.h"

namespace nbwindow {

template <class Fold>
__global__ __launch_bounds__(256) void window_kernel(const unsigned char *__restrict__ in, int H, int W, int half, long long n,
                                                     unsigned char *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const unsigned char *__restrict__ img = in + (p - (long long)y * W - x);  // the pixel's view
    const int y0 = max(y - half, 0), y1 = min(y + half, H - 1), x0 = max(x - half, 0), x1 = min(x + half, W - 1);
    Fold f;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) f.take(img[(long long)yy * W + xx]);
    out[p] = (unsigned char)f.result(in[p]);
}

// the argument checks and the launch of the entry `name`, whose input is called `in_name`
template <class Fold>
int launch(const char *name, const char *in_name, const uint8_t *in, int32_t n_views, int32_t H, int32_t W, int32_t border, uint8_t *out,
           void *stream) {
    NB_REQUIRE(in && out && in != out, "%s: NULL pointer, or out is %s", name, in_name);
    NB_REQUIRE(n_views >= 1 && H >= 1 && W >= 1 && (long long)n_views * H * W <= 2147483647ll,
               "%s: n_views = %d, H = %d, W = %d (all >= 1, at most 2^31 - 1 pixels)", name, n_views, H, W);
    NB_REQUIRE(border >= 1 && border % 2 == 1 && border <= 255, "%s: border = %d (odd, 1..255)", name, border);
    const long long n = (long long)n_views * H * W;
    hipLaunchKernelGGL(window_kernel<Fold>, dim3(nb_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, H, W, border / 2, n, out);
    NB_CHECK_LAUNCH(name);
    return NB_OK;
}

}  // namespace nbwindow
