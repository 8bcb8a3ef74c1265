// nb_metrics.hip — MSE, PSNR and SSIM of one rendered view on device.
//
// Restates (zju3dv/neuralbody):
//   lib/evaluators/if_nerf.py:47-74   Evaluator.evaluate   (scatter at mask_at_box, mse over the compacted fp32 rays, psnr)
//   lib/evaluators/if_nerf.py:20-45   ssim_metric          (crop to cv2.boundingRect(mask), compare_ssim(multichannel=True))
//   scikit-image 0.14.2 skimage/measure/_structural_similarity.py  (7x7 uniform window, sample covariance, K1 0.01, K2 0.03,
//                                                                    mean over the map without its 3-pixel border)
// No dense image exists: the SSIM kernel reads the compacted [n,3] arrays through the exclusive scan of the mask, as
// nb_image_assemble does.  Every floating-point sum runs in a fixed order (per-block fp64 partials in scratch, one last block
// adds them), so a view's numbers are reproducible bit for bit.
#include "nb_scan.h"

namespace {

// compare_ssim takes data_range from the dtype when the caller gives none: float images get dtype_range = (-1, 1), i.e. 2 —
// not the 1 the [0, 1] images actually span.  The reference (and the paper's table) is computed that way; keep it.
constexpr double SSIM_DATA_RANGE = 2.0;
constexpr double SSIM_C1 = (0.01 * SSIM_DATA_RANGE) * (0.01 * SSIM_DATA_RANGE);  // 4e-4
constexpr double SSIM_C2 = (0.03 * SSIM_DATA_RANGE) * (0.03 * SSIM_DATA_RANGE);  // 3.6e-3
constexpr int WIN = 7;
constexpr double WIN_N = WIN * WIN;
constexpr double COV_NORM = WIN_N / (WIN_N - 1.0);  // use_sample_covariance

constexpr int BLOCK = 256;
constexpr int PIX_PER_BLOCK = 1024;  // flag / box / MSE kernel: 4 pixels per thread

// SSIM tile: 64 x 16 windows per workgroup.  A wave takes 64 adjacent window columns (LDS reads of a wave are 64 consecutive
// floats: conflict free) and 4 window rows; the staged pixels are the tile plus the 6-pixel halo to the right and below.
constexpr int TILE_W = 64, TILE_H = 16;
constexpr int ROWS_PER_WAVE = TILE_H / (BLOCK / 64);  // 4
constexpr int ST_W = TILE_W + WIN - 1, ST_H = TILE_H + WIN - 1;  // 70 x 22 staged pixels
constexpr int ST_N = ST_W * ST_H;
// LDS: 6 planes (3 channels x {pred, gt}) of 70 x 22 fp32 = 36 960 B -> 4 workgroups per CU

// box[] holds four maxima so that a zero fill is "no pixel seen": W - xmin, H - ymin, xmax + 1, ymax + 1
struct Box {
    int x, y, w, h;
};

__device__ __forceinline__ Box load_box(const int *__restrict__ box, int H, int W, int whole_img) {
    Box b;
    if (whole_img) {
        b.x = 0, b.y = 0, b.w = W, b.h = H;
    } else if (box[2] == 0) {
        b.x = b.y = b.w = b.h = 0;  // cv2.boundingRect of an empty mask
    } else {
        b.x = W - box[0];
        b.y = H - box[1];
        b.w = box[2] - b.x;
        b.h = box[3] - b.y;
    }
    return b;
}

// sum over the block in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double wsum[BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) s += wsum[i];
    }
    __syncthreads();
    return s;
}

// per pixel: scan flag and bounding box; per block: one fp64 partial of sum (pred - gt)^2 over its share of the compacted rays
__global__ __launch_bounds__(BLOCK) void metrics_flag_kernel(const uint8_t *__restrict__ mask, int H, int W,
                                                             int *__restrict__ flags, int *__restrict__ box,
                                                             const float *__restrict__ pred, const float *__restrict__ gt,
                                                             long long n_elem, long long chunk,
                                                             double *__restrict__ mse_part) {
    const long long n = (long long)H * W;
    int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
#pragma unroll
    for (int i = 0; i < PIX_PER_BLOCK / BLOCK; ++i) {
        const long long p = (long long)blockIdx.x * PIX_PER_BLOCK + i * BLOCK + threadIdx.x;
        if (p >= n) break;
        const int f = mask[p] != 0;
        flags[p] = f;
        if (f) {
            const int y = (int)(p / W), x = (int)(p - (long long)y * W);
            bx0 = max(bx0, W - x);
            by0 = max(by0, H - y);
            bx1 = max(bx1, x + 1);
            by1 = max(by1, y + 1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bx0 = max(bx0, __shfl_xor(bx0, off));
        by0 = max(by0, __shfl_xor(by0, off));
        bx1 = max(bx1, __shfl_xor(bx1, off));
        by1 = max(by1, __shfl_xor(by1, off));
    }
    if ((threadIdx.x & 63) == 0 && bx1 > 0) {  // integer maxima: order-independent
        atomicMax(box + 0, bx0);
        atomicMax(box + 1, by0);
        atomicMax(box + 2, bx1);
        atomicMax(box + 3, by1);
    }

    // (pred - gt) and its square in fp32 like the reference's fp32 arrays, accumulated in fp64
    const long long beg = (long long)blockIdx.x * chunk;
    const long long end = min(beg + chunk, n_elem);
    const bool vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & 15) == 0;
    double s = 0.0;
    for (long long i = beg + 4 * threadIdx.x; i < end; i += 4 * BLOCK) {  // chunk % 4 == 0: i stays 16-byte aligned
        if (vec && i + 4 <= end) {
            const float4 a = *reinterpret_cast<const float4 *>(pred + i);
            const float4 b = *reinterpret_cast<const float4 *>(gt + i);
            const float d0 = __fsub_rn(a.x, b.x), d1 = __fsub_rn(a.y, b.y), d2 = __fsub_rn(a.z, b.z), d3 = __fsub_rn(a.w, b.w);
            s += (double)__fmul_rn(d0, d0);
            s += (double)__fmul_rn(d1, d1);
            s += (double)__fmul_rn(d2, d2);
            s += (double)__fmul_rn(d3, d3);
        } else {
            for (long long k = i; k < min(i + 4, end); ++k) {
                const float d = __fsub_rn(pred[k], gt[k]);
                s += (double)__fmul_rn(d, d);
            }
        }
    }
    s = block_sum(s);
    if (threadIdx.x == 0) mse_part[blockIdx.x] = s;
}

// One workgroup per 64 x 16 tile of window origins (image coordinates).  A window is counted when it lies fully inside the
// crop box.  Writes ssim_part[tile] = sum of S over the tile's windows and 3 channels and, for whole_img, wmse_part[tile] =
// sum of float64 (pred - gt)^2 over the tile's own 64 x 16 pixels.
__global__ __launch_bounds__(BLOCK) void metrics_ssim_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ pos, int H,
                                                             int W, const float *__restrict__ pred,
                                                             const float *__restrict__ gt, long long n_rays, float bkgd,
                                                             int whole_img, const int *__restrict__ box,
                                                             double *__restrict__ ssim_part, double *__restrict__ wmse_part) {
    __shared__ float st[6][ST_N];
    const int tile = blockIdx.y * gridDim.x + blockIdx.x;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const Box b = load_box(box, H, W, whole_img);
    // window origins of the crop: [b.x, b.x + b.w - 7] x [b.y, b.y + b.h - 7]
    const int ox0 = b.x, ox1 = b.x + b.w - WIN, oy0 = b.y, oy1 = b.y + b.h - WIN;
    const bool has_windows = ox1 >= ox0 && oy1 >= oy0 && tx0 <= ox1 && tx0 + TILE_W > ox0 && ty0 <= oy1 && ty0 + TILE_H > oy0;
    if (!has_windows && !whole_img) {  // block-uniform
        if (threadIdx.x == 0) ssim_part[tile] = 0.0;
        return;
    }

    for (int i = threadIdx.x; i < ST_N; i += BLOCK) {
        const int sy = i / ST_W, sx = i - sy * ST_W;
        const int x = tx0 + sx, y = ty0 + sy;
        float c[6] = {bkgd, bkgd, bkgd, bkgd, bkgd, bkgd};
        if (x < W && y < H) {
            const long long p = (long long)y * W + x;
            const long long r = pos[p];
            if (mask[p] != 0 && r < n_rays) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    c[2 * a] = pred[r * 3 + a];
                    c[2 * a + 1] = gt[r * 3 + a];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) st[a][i] = c[a];
    }
    __syncthreads();

    if (whole_img) {  // the float64 images of the reference: differences in fp64, background included
        double s = 0.0;
        for (int i = threadIdx.x; i < TILE_W * TILE_H; i += BLOCK) {
            const int sy = i / TILE_W, sx = i - sy * TILE_W;
            if (tx0 + sx < W && ty0 + sy < H) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double d = (double)st[2 * a][sy * ST_W + sx] - (double)st[2 * a + 1][sy * ST_W + sx];
                    s += d * d;
                }
            }
        }
        s = block_sum(s);
        if (threadIdx.x == 0) wmse_part[tile] = s;
    }

    const int col = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * ROWS_PER_WAVE;
    const int wx = tx0 + col;
    double acc = 0.0;
    if (has_windows && wx >= ox0 && wx <= ox1 && ty0 + row0 <= oy1 && ty0 + row0 + ROWS_PER_WAVE > oy0) {
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            const float *__restrict__ px = &st[2 * ch][row0 * ST_W + col];
            const float *__restrict__ py = &st[2 * ch + 1][row0 * ST_W + col];
            double h[WIN][5];  // row-pass sums of the last 7 pixel rows: x, y, xx, yy, xy
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE + WIN - 1; ++r) {
                double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {  // 7-tap row pass
                    const double u = (double)px[r * ST_W + k], v = (double)py[r * ST_W + k];
                    sx += u;
                    sy += v;
                    sxx = fma(u, u, sxx);  // the same operation for all three: pred == gt gives vx == vy == vxy bit for bit
                    syy = fma(v, v, syy);
                    sxy = fma(u, v, sxy);
                }
                h[r % WIN][0] = sx, h[r % WIN][1] = sy, h[r % WIN][2] = sxx, h[r % WIN][3] = syy, h[r % WIN][4] = sxy;
                if (r >= WIN - 1) {  // 7-tap column pass over the rows r - 6 .. r
                    double m[5];
#pragma unroll
                    for (int q = 0; q < 5; ++q) {
                        double t = 0.0;
#pragma unroll
                        for (int k = 0; k < WIN; ++k) t += h[(r + 1 + k) % WIN][q];
                        m[q] = t / WIN_N;
                    }
                    // every operation rounded on its own, in compare_ssim's order: with contraction into FMAs the numerator
                    // and the denominator of identical images would round differently and S would miss 1 by an ulp
                    const double ux = m[0], uy = m[1];
                    const double vx = __dmul_rn(COV_NORM, __dsub_rn(m[2], __dmul_rn(ux, ux)));
                    const double vy = __dmul_rn(COV_NORM, __dsub_rn(m[3], __dmul_rn(uy, uy)));
                    const double vxy = __dmul_rn(COV_NORM, __dsub_rn(m[4], __dmul_rn(ux, uy)));
                    const double a1 = __dadd_rn(__dmul_rn(__dmul_rn(2.0, ux), uy), SSIM_C1);
                    const double a2 = __dadd_rn(__dmul_rn(2.0, vxy), SSIM_C2);
                    const double b1 = __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), SSIM_C1);
                    const double b2 = __dadd_rn(__dadd_rn(vx, vy), SSIM_C2);
                    const double S = __ddiv_rn(__dmul_rn(a1, a2), __dmul_rn(b1, b2));
                    const int wy = ty0 + row0 + r - (WIN - 1);
                    if (wy >= oy0 && wy <= oy1) acc += S;
                }
            }
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) ssim_part[tile] = acc;
}

// adds the partials in a fixed order and writes out = {mse, psnr, ssim, x, y, w, h, n_windows}
__global__ __launch_bounds__(BLOCK) void metrics_final_kernel(const double *__restrict__ mse_part, int n_mse,
                                                              const double *__restrict__ ssim_part, int n_ssim, double mse_count,
                                                              int H, int W, int whole_img, const int *__restrict__ box,
                                                              double *__restrict__ out) {
    double s = 0.0, t = 0.0;
    for (int i = threadIdx.x; i < n_mse; i += BLOCK) s += mse_part[i];
    for (int i = threadIdx.x; i < n_ssim; i += BLOCK) t += ssim_part[i];
    s = block_sum(s);
    t = block_sum(t);
    if (threadIdx.x != 0) return;
    const Box b = load_box(box, H, W, whole_img);
    const double n_win = (b.w >= WIN && b.h >= WIN) ? (double)(b.w - WIN + 1) * (double)(b.h - WIN + 1) : 0.0;
    const double mse = s / mse_count;  // 0 / 0 = NaN: no rays
    out[0] = mse;
    out[1] = -10.0 * log(mse) / log(10.0);  // if_nerf.py:17; mse = 0 gives +inf
    out[2] = n_win > 0.0 ? t / (3.0 * n_win) : __longlong_as_double(0x7ff8000000000000LL);  // compare_ssim raises there
    out[3] = b.x, out[4] = b.y, out[5] = b.w, out[6] = b.h;
    out[7] = n_win;
}

constexpr long long MAX_PIXELS = 1LL << 30;  // int32 positions and flag sums of the scan

inline long long flag_blocks(long long n) { return (n + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK; }
inline long long ssim_tiles(int H, int W) { return (long long)nb_ceil_div(W, TILE_W) * nb_ceil_div(H, TILE_H); }

}  // namespace

extern "C" int64_t nb_eval_metrics_scratch_size(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return 0;
    const long long n = (long long)H * W;
    // [scan: flags | positions | block sums] [box 4 x int32] [mse partials] [ssim partials] [whole-image mse partials]  (fp64)
    return nb_align256(nb_scan_scratch_size(n)) + 256 + nb_align256(8 * flag_blocks(n)) + 2 * nb_align256(8 * ssim_tiles(H, W));
}

extern "C" int nb_eval_metrics(const uint8_t *mask_at_box, int32_t H, int32_t W, const float *rgb_pred, const float *rgb_gt,
                               int64_t n_rays, int white_bkgd, int whole_img, double *out, void *scratch, void *stream) {
    NB_REQUIRE(H >= 1 && W >= 1, "nb_eval_metrics: H = %d, W = %d", H, W);
    NB_REQUIRE((long long)H * W <= MAX_PIXELS, "nb_eval_metrics: %d x %d pixels exceed the scan's %lld", H, W, MAX_PIXELS);
    NB_REQUIRE(n_rays >= 0, "nb_eval_metrics: n_rays = %lld", (long long)n_rays);
    NB_REQUIRE(mask_at_box && out && scratch && ((rgb_pred && rgb_gt) || n_rays == 0), "nb_eval_metrics: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    int *flags, *pos, *bs;
    nb_scan_carve(scratch, n, &flags, &pos, &bs);
    char *p = static_cast<char *>(scratch) + nb_align256(nb_scan_scratch_size(n));
    int *box = reinterpret_cast<int *>(p);
    p += 256;
    const int n_fb = (int)flag_blocks(n), n_tiles = (int)ssim_tiles(H, W);
    double *mse_part = reinterpret_cast<double *>(p);
    p += nb_align256(8LL * n_fb);
    double *ssim_part = reinterpret_cast<double *>(p);
    p += nb_align256(8LL * n_tiles);
    double *wmse_part = reinterpret_cast<double *>(p);

    const long long n_elem = 3 * (long long)n_rays;
    const long long chunk = ((n_elem + n_fb - 1) / n_fb + 4 * BLOCK - 1) / (4 * BLOCK) * (4 * BLOCK);
    NB_HIP(hipMemsetAsync(box, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(metrics_flag_kernel, dim3(n_fb), dim3(BLOCK), 0, st, mask_at_box, H, W, flags, box, rgb_pred, rgb_gt,
                       n_elem, chunk, mse_part);
    // nobody needs the total on the host
    if (int rc = nb_exclusive_scan(flags, pos, nb_scan_total_slot(bs, n), n, bs, st)) return rc;
    hipLaunchKernelGGL(metrics_ssim_kernel, dim3(nb_ceil_div(W, TILE_W), nb_ceil_div(H, TILE_H)), dim3(BLOCK), 0, st,
                       mask_at_box, pos, H, W, rgb_pred, rgb_gt, (long long)n_rays, white_bkgd ? 1.f : 0.f, whole_img ? 1 : 0,
                       box, ssim_part, wmse_part);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(BLOCK), 0, st, whole_img ? wmse_part : mse_part,
                       whole_img ? n_tiles : n_fb, ssim_part, n_tiles, whole_img ? 3.0 * (double)n : (double)n_elem, H, W,
                       whole_img ? 1 : 0, box, out);
    NB_CHECK_LAUNCH("nb_eval_metrics");
    return NB_OK;
}
