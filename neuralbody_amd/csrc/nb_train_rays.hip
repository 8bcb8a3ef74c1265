// nb_train_rays.hip — one training batch of rays drawn on the device from a resident image and mask.
//
// Restates (zju3dv/neuralbody):
//   lib/utils/if_nerf/if_nerf_data_utils.py:153-219  sample_ray_h36m, train branch  (NB_SAMPLE_H36M)
//   lib/utils/if_nerf/if_nerf_data_utils.py:72-137   sample_ray, train branch       (NB_SAMPLE_PLAIN)
//   lib/utils/if_nerf/if_nerf_data_utils.py:40-51    get_bound_2d_mask: the six filled quads are the silhouette of the box,
//                                                    here one convex hull handed over by the host (train_rays.bound_hull)
// Classification (one thread per pixel) -> two exclusive scans -> ONE workgroup that restates the reference's
// `while nsampled_rays < nrays` loop: draw, intersect in float64, keep the hits in draw order, go round again with the
// deficit.  No atomics, no host round trip, no launch whose size depends on the data.
#include "nb_ray.h"
#include "nb_scan.h"

namespace {

using nbray::near_far;
using nbray::pixel_ray_f64;
using nbray::RayCam;

constexpr int MAX_HULL = 8;
constexpr int SAMPLE_BLOCK = 512;
constexpr int SAMPLE_WAVES = SAMPLE_BLOCK / 64;

struct Hull {
    int n;
    int x[MAX_HULL], y[MAX_HULL];
};

// body / bound candidate flags of every pixel (if_nerf_data_utils.py:79,99,108 and :160-161,181,190)
__global__ void classify_kernel(Hull h, int H, int W, int mode, const uint8_t *__restrict__ msk, int *__restrict__ f_body,
                                int *__restrict__ f_bound) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W) return;
    const long long px = p % W, py = p / W;
    bool in_hull = true;
    for (int e = 0; e < h.n; ++e) {  // edge functions of the CCW hull, exact in int64
        const int f = e + 1 < h.n ? e + 1 : 0;
        const long long ax = h.x[e], ay = h.y[e], bx = h.x[f], by = h.y[f];
        in_hull = in_hull && ((bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0);
    }
    const int m = in_hull ? (int)msk[p] : 0;  // msk * bound_mask
    bool body, bound;
    if (mode == NB_SAMPLE_H36M) {
        body = m == 1;
        bound = in_hull && m != 100;
    } else {
        body = m != 0;
        bound = in_hull;
    }
    f_body[p] = body;
    f_bound[p] = bound;
}

// index of the k-th set pixel in row-major order: upper_bound(pos, k) - 1 in the exclusive scan of the flags
__device__ __forceinline__ long long kth_set(const int *__restrict__ pos, long long n, int k) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (pos[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;  // >= 0: pos[0] = 0 <= k
}

__device__ __forceinline__ int pick(float u, int count) {
    const double t = (double)u * (double)count;  // exact: 24 x 31 bits
    const int k = t >= 0.0 ? (int)fmin(t, 2147483520.0) : 0;
    return k < count - 1 ? k : count - 1;
}

__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_kernel(
    RayCam c, int H, int W, const int *__restrict__ pos_body, const int *__restrict__ pos_bound,
    const int *__restrict__ n_body_ptr, const int *__restrict__ n_bound_ptr, const float *__restrict__ img, double body_ratio,
    const float *__restrict__ u, int n_rounds, int n_rays, float *__restrict__ rgb, float *__restrict__ ray_o,
    float *__restrict__ ray_d, float *__restrict__ near_out, float *__restrict__ far_out, int *__restrict__ pixel,
    uint8_t *__restrict__ mask_at_box, int *__restrict__ status) {
    __shared__ int wave_hits[SAMPLE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_pix = (long long)H * W;
    const int count_body = *n_body_ptr, count_bound = *n_bound_ptr;
    int filled = 0, round = 0;  // the same in every thread
    while (round < n_rounds && filled < n_rays) {
        const int deficit = n_rays - filled;
        const int n_body = (int)((double)deficit * body_ratio);  // int((nrays - nsampled_rays) * body_sample_ratio)
        int base = filled;
        for (int j0 = 0; j0 < deficit; j0 += SAMPLE_BLOCK) {
            const int j = j0 + tid;
            bool hit = false;
            long long p = 0;
            double d[3], tn = 0.0, tf = 0.0;
            if (j < deficit) {
                const bool is_body = j < n_body;
                const int count = is_body ? count_body : count_bound;
                if (count > 0) {
                    p = kth_set(is_body ? pos_body : pos_bound, n_pix, pick(u[(long long)round * n_rays + j], count));
                    pixel_ray_f64(c, (int)(p % W), (int)(p / W), d);
                    hit = near_far(c, d, &tn, &tf);
                }
            }
            // ordered compaction: rank inside the wave by ballot + popcount, waves in front through LDS
            const unsigned long long vote = __ballot(hit);
            const int rank = __popcll(vote & ((1ull << lane) - 1ull));
            if (lane == 0) wave_hits[wave] = __popcll(vote);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < SAMPLE_WAVES; ++w) {
                if (w < wave) before += wave_hits[w];
                total += wave_hits[w];
            }
            __syncthreads();
            if (hit) {
                const long long r = base + before + rank;  // < n_rays: a round keeps at most `deficit` rays
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    ray_o[r * 3 + a] = (float)c.o[a];
                    ray_d[r * 3 + a] = (float)d[a];
                    rgb[r * 3 + a] = img[p * 3 + a];
                }
                near_out[r] = (float)tn;
                far_out[r] = (float)tf;
                pixel[r * 2 + 0] = (int)(p / W);
                pixel[r * 2 + 1] = (int)(p % W);
                mask_at_box[r] = 1;
            }
            base += total;
        }
        filled = base;
        ++round;
    }
    // short batch: finite, renderable rows that the loss's [mask_at_box] drops
    double d0[3];
    pixel_ray_f64(c, 0, 0, d0);
    for (int r = filled + tid; r < n_rays; r += SAMPLE_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ray_o[(long long)r * 3 + a] = (float)c.o[a];
            ray_d[(long long)r * 3 + a] = (float)d0[a];
            rgb[(long long)r * 3 + a] = 0.f;
        }
        near_out[r] = 0.f;
        far_out[r] = 0.f;
        pixel[(long long)r * 2 + 0] = -1;
        pixel[(long long)r * 2 + 1] = -1;
        mask_at_box[r] = 0;
    }
    if (tid == 0) {
        status[0] = filled;
        status[1] = round;
        status[2] = count_body;
        status[3] = count_bound;
    }
}

bool size_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (long long)H * W <= (1ll << 30); }

}  // namespace

extern "C" int64_t nb_train_rays_scratch_size(int32_t H, int32_t W) {
    if (!size_ok(H, W)) return 0;
    return 2 * nb_scan_scratch_size((int64_t)H * W);  // [flags, positions, block sums] of the body and of the bound class
}

extern "C" int nb_train_rays(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3],
                             const float bounds[6], const int32_t *hull_xy, int32_t n_hull, const uint8_t *msk,
                             const float *img, int32_t mode, double body_ratio, const float *u, int32_t n_rounds,
                             int32_t n_rays, float *rgb, float *ray_o, float *ray_d, float *near, float *far, int32_t *pixel,
                             uint8_t *mask_at_box, int32_t *status, void *scratch, void *stream) {
    NB_REQUIRE(K && R && T && bounds && hull_xy, "nb_train_rays: NULL host pointer");
    NB_REQUIRE(size_ok(H, W), "nb_train_rays: H = %d, W = %d (both >= 1, H*W <= 2^30)", H, W);
    NB_REQUIRE(n_rays >= 1 && n_rounds >= 1, "nb_train_rays: n_rays = %d, n_rounds = %d", n_rays, n_rounds);
    NB_REQUIRE(n_hull >= 3 && n_hull <= MAX_HULL, "nb_train_rays: n_hull = %d (3..%d)", n_hull, MAX_HULL);
    NB_REQUIRE(body_ratio >= 0.0 && body_ratio <= 1.0, "nb_train_rays: body_ratio = %g (0..1)", body_ratio);
    NB_REQUIRE(mode == NB_SAMPLE_H36M || mode == NB_SAMPLE_PLAIN, "nb_train_rays: unknown mode %d", mode);
    Hull h;
    h.n = n_hull;
    for (int i = 0; i < MAX_HULL; ++i) h.x[i] = h.y[i] = 0;
    for (int i = 0; i < n_hull; ++i) {
        h.x[i] = hull_xy[2 * i + 0];
        h.y[i] = hull_xy[2 * i + 1];
        NB_REQUIRE(h.x[i] > -(1 << 30) && h.x[i] < (1 << 30) && h.y[i] > -(1 << 30) && h.y[i] < (1 << 30),
                   "nb_train_rays: hull point %d = (%d, %d), magnitude >= 2^30", i, h.x[i], h.y[i]);
    }
    RayCam c;
    NB_REQUIRE(nbray::make_cam(K, R, T, bounds, &c), "nb_train_rays: K is singular");
    NB_REQUIRE(msk && img && u && rgb && ray_o && ray_d && near && far && pixel && mask_at_box && status && scratch,
               "nb_train_rays: NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    int *f_body, *pos_body, *bs_body, *f_bound, *pos_bound, *bs_bound;
    nb_scan_carve(scratch, n, &f_body, &pos_body, &bs_body);
    nb_scan_carve(static_cast<char *>(scratch) + nb_scan_scratch_size(n), n, &f_bound, &pos_bound, &bs_bound);
    // the two totals stay on the device
    int *n_body = nb_scan_total_slot(bs_body, n), *n_bound = nb_scan_total_slot(bs_bound, n);
    hipLaunchKernelGGL(classify_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, st, h, H, W, mode, msk, f_body, f_bound);
    if (int rc = nb_exclusive_scan(f_body, pos_body, n_body, n, bs_body, st)) return rc;
    if (int rc = nb_exclusive_scan(f_bound, pos_bound, n_bound, n, bs_bound, st)) return rc;
    hipLaunchKernelGGL(sample_kernel, dim3(1), dim3(SAMPLE_BLOCK), 0, st, c, H, W, pos_body, pos_bound, n_body, n_bound, img,
                       body_ratio, u, n_rounds, n_rays, rgb, ray_o, ray_d, near, far, pixel, mask_at_box, status);
    NB_CHECK_LAUNCH("nb_train_rays");
    return NB_OK;
}
