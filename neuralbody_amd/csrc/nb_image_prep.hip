// nb_image_prep.hip — nb_mask_band, nb_image_undistort: a photographed frame and its CIHP label image turned into what the ray
// and lattice kernels consume, on the device.
//
// Restates (zju3dv/neuralbody):
//   lib/datasets/light_stage/multi_view_dataset.py:58-64         get_mask: (label != 0), cv2.erode / cv2.dilate with a 5 x 5
//                                                                kernel, 100 on the band where they differ       (nb_mask_band)
//   lib/datasets/light_stage/multi_view_dataset.py:129-142       cv2.undistort of the float image and the uint8 mask, the INTER_AREA
//                                                                / INTER_NEAREST reduction by cfg.ratio, the background fill
//   lib/datasets/light_stage/multi_view_mesh_dataset.py:102-109  cv2.undistort of every view's mask        (nb_image_undistort)
// cv2.undistort is initUndistortRectifyMap (a float64 map per pixel, quantised to 1/32 pixel) followed by remap(INTER_LINEAR,
// BORDER_CONSTANT); include/nb_hip.h states the arithmetic operation by operation.  Nothing is stored between the stages: a thread
// owns one output pixel, evaluates the map of the n x n full-resolution pixels under it and reads their taps from the bytes.
//
// hipcc contracts a * b + c into an FMA by default and its `_rn` intrinsics are the plain operators, so contraction is switched off
// for this file: every operator below is one IEEE operation (fp64 and fp32 `/` are correctly rounded under hipcc's defaults), and
// tests/image_prep_ref.py rounds at the same places.
#include <math.h>

#include "nb_common.h"
#include "nb_window.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_VIEWS = 8;  // cameras per launch (96 bytes of kernel arguments each); a longer batch is several launches
constexpr int BLOCK_X = 64, BLOCK_Y = 4;

struct Cam {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;
};
struct Cams {
    Cam c[MAX_VIEWS];
};

// the fold of nb_window.h for nb_mask_band: msk = 100 where the window's maximum and minimum of (label != 0) differ, else (label != 0)
struct BandFold {
    unsigned any = 0, all = 1;
    __device__ __forceinline__ void take(unsigned b) { any |= b != 0, all &= b != 0; }
    __device__ __forceinline__ unsigned result(unsigned centre) const { return any != all ? 100u : (unsigned)(centre != 0); }
};

// rint(32 v) clamped into int32; a NaN becomes the lowest value (fmax returns its other operand)
__device__ __forceinline__ int fixed32(double v) {
    const double t = rint(v * 32.0);
    return (int)fmin(fmax(t, -2147483648.0), 2147483647.0);
}

struct Taps {
    int sx, sy, ax, ay;
};

// the source position of full-resolution pixel (column j, row i) in 1/32 pixel: initUndistortRectifyMap with R = I, newK = K
__device__ __forceinline__ Taps source_of(const Cam &c, int j, int i) {
    const double x = ((double)j - c.cx) / c.fx;
    const double y = ((double)i - c.cy) / c.fy;
    const double x2 = x * x;
    const double y2 = y * y;
    const double r2 = x2 + y2;
    const double _2xy = 2.0 * x * y;
    const double kr = (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double u = c.fx * (x * kr + c.p1 * _2xy + c.p2 * (r2 + 2.0 * x2)) + c.cx;
    const double v = c.fy * (y * kr + c.p1 * (r2 + 2.0 * y2) + c.p2 * _2xy) + c.cy;
    const int iu = fixed32(u), iv = fixed32(v);
    return {iu >> 5, iv >> 5, iu & 31, iv & 31};
}

__device__ __forceinline__ bool in_image(int y, int x, int H, int W) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; }

// remap of a uint8 plane: the 1/32 weights as integers, (sum + 512) >> 10
__device__ __forceinline__ unsigned remap_u8(const unsigned char *__restrict__ img, int H, int W, const Taps &t) {
    const unsigned w00 = (32 - t.ay) * (32 - t.ax), w01 = (32 - t.ay) * t.ax, w10 = t.ay * (32 - t.ax), w11 = t.ay * t.ax;
    const long long at = (long long)t.sy * W + t.sx;
    unsigned s = 512;
    if (in_image(t.sy, t.sx, H, W)) s += img[at] * w00;
    if (in_image(t.sy, t.sx + 1, H, W)) s += img[at + 1] * w01;
    if (in_image(t.sy + 1, t.sx, H, W)) s += img[at + W] * w10;
    if (in_image(t.sy + 1, t.sx + 1, H, W)) s += img[at + W + 1] * w11;
    return s >> 10;
}

// remap of the three byte channels as float32: S = unit[byte] = byte / 255.f, ((S00 w00 + S01 w01) + S10 w10) + S11 w11
__device__ __forceinline__ void remap_rgb(const unsigned char *__restrict__ img, int H, int W, const Taps &t,
                                          const float *__restrict__ unit, float out[3]) {
    const float fx = (float)t.ax / 32.f, fy = (float)t.ay / 32.f;
    const float gx = 1.f - fx, gy = 1.f - fy;
    const float w00 = gy * gx, w01 = gy * fx, w10 = fy * gx, w11 = fy * fx;
    const bool i00 = in_image(t.sy, t.sx, H, W), i01 = in_image(t.sy, t.sx + 1, H, W);
    const bool i10 = in_image(t.sy + 1, t.sx, H, W), i11 = in_image(t.sy + 1, t.sx + 1, H, W);
    const long long at = ((long long)t.sy * W + t.sx) * 3, row = (long long)W * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float s00 = i00 ? unit[img[at + ch]] : 0.f;
        const float s01 = i01 ? unit[img[at + 3 + ch]] : 0.f;
        const float s10 = i10 ? unit[img[at + row + ch]] : 0.f;
        const float s11 = i11 ? unit[img[at + row + 3 + ch]] : 0.f;
        out[ch] = ((s00 * w00 + s01 * w01) + s10 * w10) + s11 * w11;
    }
}

// one thread per output pixel (X, Y) of view blockIdx.z; rgb / msk may be NULL (then so is its output)
__global__ __launch_bounds__(BLOCK_X *BLOCK_Y) void image_undistort_kernel(const unsigned char *__restrict__ rgb,
                                                                           const unsigned char *__restrict__ msk, Cams cams, int H,
                                                                           int W, int n, int fill, float inv_area,
                                                                           float *__restrict__ img_out,
                                                                           unsigned char *__restrict__ msk_out) {
    static_assert(BLOCK_X * BLOCK_Y == 256, "one thread per byte value fills the table");
    __shared__ float unit[256];  // byte / 255.f, one correctly rounded division per entry instead of twelve per pixel
    unit[threadIdx.y * BLOCK_X + threadIdx.x] = (float)(threadIdx.y * BLOCK_X + threadIdx.x) / 255.0f;
    __syncthreads();
    const int X = blockIdx.x * BLOCK_X + threadIdx.x, Y = blockIdx.y * BLOCK_Y + threadIdx.y;
    const int Wo = W / n, Ho = H / n;
    if (X >= Wo || Y >= Ho) return;
    const Cam &cam = cams.c[blockIdx.z];
    const long long view = blockIdx.z;
    const long long o = (view * Ho + Y) * Wo + X;
    unsigned m = 1;
    if (msk) {  // INTER_NEAREST by an integer factor: the undistorted mask at (nY, nX)
        m = remap_u8(msk + view * H * W, H, W, source_of(cam, X * n, Y * n));
        msk_out[o] = (unsigned char)m;
    }
    if (!rgb) return;
    float acc[3];
    if (fill != NB_FILL_NONE && m == 0) {
        acc[0] = acc[1] = acc[2] = fill == NB_FILL_WHITE ? 1.f : 0.f;
    } else {  // INTER_AREA by an integer factor: the block's sum in row-major order, times 1 / n^2
        const unsigned char *__restrict__ src = rgb + view * H * W * 3;
        acc[0] = acc[1] = acc[2] = 0.f;
        for (int dy = 0; dy < n; ++dy)
            for (int dx = 0; dx < n; ++dx) {
                float px[3];
                remap_rgb(src, H, W, source_of(cam, X * n + dx, Y * n + dy), unit, px);
                acc[0] = acc[0] + px[0];
                acc[1] = acc[1] + px[1];
                acc[2] = acc[2] + px[2];
            }
        acc[0] = acc[0] * inv_area;
        acc[1] = acc[1] * inv_area;
        acc[2] = acc[2] * inv_area;
    }
    img_out[o * 3 + 0] = acc[0];
    img_out[o * 3 + 1] = acc[1];
    img_out[o * 3 + 2] = acc[2];
}

}  // namespace

extern "C" int nb_mask_band(const uint8_t *label, int32_t n_views, int32_t H, int32_t W, int32_t border, uint8_t *out,
                            void *stream) {
    return nbwindow::launch<BandFold>("nb_mask_band", "label", label, n_views, H, W, border, out, stream);
}

extern "C" int nb_image_undistort(const uint8_t *rgb, const uint8_t *msk, const double *cam, int32_t n_views, int32_t H, int32_t W,
                                  int32_t n, int fill, float *img_out, uint8_t *msk_out, void *stream) {
    NB_REQUIRE(rgb || msk, "nb_image_undistort: both rgb and msk are NULL");
    NB_REQUIRE(cam != nullptr, "nb_image_undistort: cam is NULL");
    NB_REQUIRE((rgb != nullptr) == (img_out != nullptr) && (msk != nullptr) == (msk_out != nullptr),
               "nb_image_undistort: an input without its output, or an output without its input");
    NB_REQUIRE(n_views >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (long long)n_views * H * W * 3 <= 2147483647ll,
               "nb_image_undistort: n_views = %d (>= 1), H = %d, W = %d (1..32768), 3 n_views H W at most 2^31 - 1", n_views, H, W);
    NB_REQUIRE(n >= 1 && H % n == 0 && W % n == 0, "nb_image_undistort: n = %d must be >= 1 and divide H = %d and W = %d", n, H, W);
    NB_REQUIRE(fill == NB_FILL_NONE || fill == NB_FILL_BLACK || fill == NB_FILL_WHITE, "nb_image_undistort: fill = %d", fill);
    NB_REQUIRE(fill == NB_FILL_NONE || msk, "nb_image_undistort: fill = %d needs a mask", fill);
    for (int32_t v = 0; v < n_views; ++v)
        for (int k = 0; k < NB_CAM_DOUBLES; ++k)
            NB_REQUIRE(isfinite(cam[v * NB_CAM_DOUBLES + k]) && (k > 1 || cam[v * NB_CAM_DOUBLES + k] != 0.0),
                       "nb_image_undistort: camera %d, constant %d is not finite, or a focal length is 0", v, k);
    const int Ho = H / n, Wo = W / n;
    const float inv_area = 1.0f / (float)((long long)n * n);
    for (int32_t v0 = 0; v0 < n_views; v0 += MAX_VIEWS) {
        const int nv = n_views - v0 < MAX_VIEWS ? n_views - v0 : MAX_VIEWS;
        Cams cams = {};
        for (int v = 0; v < nv; ++v) {
            const double *c = cam + (size_t)(v0 + v) * NB_CAM_DOUBLES;
            cams.c[v] = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11]};
        }
        const size_t in_px = (size_t)v0 * H * W, out_px = (size_t)v0 * Ho * Wo;
        hipLaunchKernelGGL(image_undistort_kernel, dim3(nb_ceil_div(Wo, BLOCK_X), nb_ceil_div(Ho, BLOCK_Y), nv),
                           dim3(BLOCK_X, BLOCK_Y), 0, (hipStream_t)stream, rgb ? rgb + in_px * 3 : nullptr,
                           msk ? msk + in_px : nullptr, cams, H, W, n, fill, inv_area, img_out ? img_out + out_px * 3 : nullptr,
                           msk_out ? msk_out + out_px : nullptr);
        NB_CHECK_LAUNCH("nb_image_undistort");
    }
    return NB_OK;
}
