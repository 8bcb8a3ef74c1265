// nb_ray_loss.hip — per-ray regularisers of the training step that have no counterpart in the reference.
//
//   nb_ray_distortion   compactness of a ray's weights: the distortion loss of Mip-NeRF 360 (Barron et al. 2022, eq. 15) restated for
//                       this renderer's samples, with its gradient with respect to the weights (include/nb_hip.h has the formulas)
//
// Sample i stands for the interval [z_i, z_{i+1}) as raw2outputs uses it (dist_i = z_{i+1} - z_i), the last sample is a point at the
// far end.  With s_i = (z_i - z_0) / (z_{S-1} - z_0), m_i the interval's midpoint and delta_i its length:
//   A_k = sum_j w_j |m_k - m_j|      L = sum_k w_k A_k + (1/3) sum_k w_k^2 delta_k      G_k = 2 A_k + (2/3) w_k delta_k
// z is non-decreasing, so m is: every j < k has m_j <= m_k and every j > k has m_j >= m_k (ties add 0 on either side), hence
//   A_k = m_k (W<k - W>k) - M<k + M>k      with W = sum w_j, M = sum w_j m_j over the samples in front of / behind k.
// One thread per ray, two sweeps, O(S), no [S,S] table, no atomics, no scratch: sweep 1 forms the totals W, M; sweep 2 carries the
// front sums and takes the back sums as total - front - own term.  Everything is float64 (fp32 inputs convert exactly), products and
// sums are rounded one by one (none contracted: the own term w_k m_k must leave the total with the bits it entered with, so that a
// one-hot ray gives A_k = 0 exactly); loss and G are rounded to fp32 once, on store.
#include "nb_common.h"

namespace {

struct Interval {
    double m, delta;
};

// midpoint and length of sample i in normalised depth; s_i is recomputed from z the same way wherever it is needed
__device__ __forceinline__ Interval interval_of(const float *__restrict__ zz, int i, int S, double z0, double span) {
    const double si = __ddiv_rn(__dsub_rn((double)zz[i], z0), span);
    if (i + 1 < S) {
        const double sn = __ddiv_rn(__dsub_rn((double)zz[i + 1], z0), span);
        return {__dmul_rn(__dadd_rn(si, sn), 0.5), __dsub_rn(sn, si)};
    }
    return {si, 0.0};
}

__global__ void ray_distortion_kernel(const float *__restrict__ weights, const float *__restrict__ z, long long n_rays, int S,
                                      float *__restrict__ loss, float *__restrict__ d_weights) {
    const long long ray = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= n_rays) return;
    const float *w = weights + ray * S;
    const float *zz = z + ray * S;
    float *g = d_weights ? d_weights + ray * S : nullptr;
    const double z0 = (double)zz[0], span = __dsub_rn((double)zz[S - 1], z0);
    if (!(span > 0.0)) {  // one sample, near == far, or a NaN depth
        loss[ray] = 0.f;
        if (g)
            for (int i = 0; i < S; ++i) g[i] = 0.f;
        return;
    }
    double Wt = 0.0, Mt = 0.0;
    for (int i = 0; i < S; ++i) {
        const double wi = (double)w[i];
        const Interval iv = interval_of(zz, i, S, z0, span);
        Wt = __dadd_rn(Wt, wi);
        Mt = __dadd_rn(Mt, __dmul_rn(wi, iv.m));
    }
    double Wf = 0.0, Mf = 0.0, L = 0.0;
    for (int k = 0; k < S; ++k) {
        const double wk = (double)w[k];
        const Interval iv = interval_of(zz, k, S, z0, span);
        const double wm = __dmul_rn(wk, iv.m);
        const double Wb = __dsub_rn(__dsub_rn(Wt, Wf), wk), Mb = __dsub_rn(__dsub_rn(Mt, Mf), wm);
        const double A = __dadd_rn(__dsub_rn(__dmul_rn(iv.m, __dsub_rn(Wf, Wb)), Mf), Mb);
        const double own = __dmul_rn(wk, iv.delta);  // w_k delta_k
        L = __dadd_rn(L, __dadd_rn(__dmul_rn(wk, A), __ddiv_rn(__dmul_rn(wk, own), 3.0)));
        if (g) g[k] = (float)__dadd_rn(__dmul_rn(2.0, A), __ddiv_rn(__dmul_rn(2.0, own), 3.0));
        Wf = __dadd_rn(Wf, wk);
        Mf = __dadd_rn(Mf, wm);
    }
    loss[ray] = (float)L;
}

}  // namespace

extern "C" {

int nb_ray_distortion(const float *weights, const float *z_vals, int64_t n_rays, int32_t n_samples, float *loss, float *d_weights,
                      void *stream) {
    NB_REQUIRE(n_rays >= 0, "nb_ray_distortion: n_rays = %lld is negative", (long long)n_rays);
    NB_REQUIRE(n_samples >= 1 && n_samples <= 512, "nb_ray_distortion: n_samples = %d is outside [1, 512]", (int)n_samples);
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(n_rays <= ((1LL << 31) - 1) * 64, "nb_ray_distortion: n_rays = %lld needs more than 2^31 - 1 workgroups", (long long)n_rays);
    NB_REQUIRE(weights && z_vals && loss, "nb_ray_distortion: NULL pointer");
    hipLaunchKernelGGL(ray_distortion_kernel, dim3(nb_ceil_div(n_rays, 64)), dim3(64), 0, (hipStream_t)stream, weights, z_vals,
                       (long long)n_rays, n_samples, loss, d_weights);
    NB_CHECK_LAUNCH("ray_distortion_kernel");
    return NB_OK;
}

}  // extern "C"
