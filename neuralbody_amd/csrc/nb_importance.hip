// nb_importance.hip — hierarchical sampling behind the march: the importance depths of every ray (nb_importance_sample) and the
// stable merge of the coarse and the fine samples of a ray by depth (nb_importance_merge; nb_importance_merge_z for depths alone).  The decode of the new points is
// nb_decode_points, the second quadrature nb_composite: this file is the per-ray work between them.
//
// Restates (zju3dv/neuralbody):
//   lib/networks/renderer/nerf_net_utils.py:55-90    sample_pdf, operation by operation                     (nb_importance_sample)
//   lib/networks/renderer/volume_renderer.py:86-90   bins = midpoints of z_vals, weights[..., 1:-1], det = (perturb == 0)
//   lib/networks/renderer/volume_renderer.py:117     z_std = std(z_samples, unbiased=False)
//   lib/networks/renderer/if_clight_renderer.py:25,68  o + d * z and d / |d| for the new points
//   lib/networks/renderer/volume_renderer.py:93      sort(cat([z_vals, z_samples]))                         (nb_importance_merge)
//   lib/networks/renderer/if_clight_renderer_mmsk.py:54-59  raw = 0 for a sample outside a silhouette       (keep, merge)
//
// One wave per ray, four rays per 256-thread workgroup (nb_composite_kernel's layout).  The coarse depths are the march's own
// (z_sample of nb_march_common.h, jitter included), the projection of a culled renderer is the march's cull_inside.
//
// SUMMATION ORDER of nb_importance_sample, with K = S - 2 weights w_i = weights[i + 1] (+) 1e-5f:
//   sum:    lane l adds w_l, w_{l+64}, ... in ascending order starting from 0, then the 64 partial sums meet in a butterfly
//           (xor 32, 16, 8, 4, 2, 1): every lane holds the same bits;
//   pdf:    pdf_i = w_i (/) sum, an IEEE division;
//   knots:  c_0 = 0; the pdf goes through in chunks of 64: inside a chunk an inclusive Hillis-Steele scan over the lanes (offsets 1, 2, 4,
//           8, 16, 32, lane l adds the value of lane l - offset), c_{i+1} = carry (+) scan_i, and the carry grows by the chunk's total
//           (lane 63's scan value).
// Adjacent knots therefore come from differently associated sums: the sequence is non-decreasing up to one rounding.  The bisection
// keeps c[lo] <= u < c[hi] (virtual knots -inf and +inf outside) down to hi = lo + 1, so it ends on a bin that brackets u whatever
// the last bit of its neighbours; on a non-decreasing sequence hi is searchsorted(side='right').
// Everything else is one IEEE operation per line (no contraction).  z_std is formed in float64 from the fp32 depths and rounded once.
// No atomics: the same inputs give the same bits.
#include "nb_march_common.h"
#include "nb_merge_rank.h"

namespace {

using namespace nbm;

constexpr int IMP_MAX = 128;      // importance samples per ray: two per lane
constexpr int MERGED_MAX = 512;   // S + N_importance: eight entries per lane in the merge
constexpr int RAYS_PER_BLOCK = 4;

struct SampleArgs {
    const float *ray_o, *ray_d, *near, *far, *t_vals, *t_rand, *weights, *u;
    long long n_rays;
    int S, N, u_per_ray;
    CullDev cull;
    const float *pose;
    float *z_coarse, *z_fine, *wpts, *viewdir, *z_std;
    unsigned char *keep;
};

__global__ __launch_bounds__(256) void importance_sample_kernel(SampleArgs a) {
#pragma clang fp contract(off)
    __shared__ float s_c[RAYS_PER_BLOCK][MERGED_MAX];  // knots c[0..K]
    __shared__ float s_b[RAYS_PER_BLOCK][MERGED_MAX];  // bins b[0..K]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray_raw = (long long)blockIdx.x * RAYS_PER_BLOCK + wv;
    const bool live = ray_raw < a.n_rays;
    const long long ray = live ? ray_raw : a.n_rays - 1;  // a padding wave repeats the last ray and stores nothing
    const int S = a.S, K = S - 2, N = a.N;
    float *c = s_c[wv], *b = s_b[wv];
    const float near = a.near[ray], far = a.far[ray];
    const float *tr = a.t_rand ? a.t_rand + ray * S : nullptr;
    const float *w_ray = a.weights + ray * S + 1;  // weights[..., 1:-1]

    // bins: the S - 1 midpoints of the coarse depths (volume_renderer.py:86)
    for (int j = lane; j <= K; j += 64) {
        const float z0 = z_sample(near, far, a.t_vals, tr, j, S), z1 = z_sample(near, far, a.t_vals, tr, j + 1, S);
        b[j] = 0.5f * __fadd_rn(z1, z0);
        if (live && a.z_coarse) {
            a.z_coarse[ray * S + j] = z0;
            if (j == K) a.z_coarse[ray * S + j + 1] = z1;
        }
    }
    // sum of weights + 1e-5 (nerf_net_utils.py:59-60)
    float sum = 0.f;
    for (int i = lane; i < K; i += 64) sum = __fadd_rn(sum, __fadd_rn(w_ray[i], 1e-5f));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum = __fadd_rn(sum, __shfl_xor(sum, off));
    // knots: inclusive prefix sum of the pdf with a leading 0 (:60-63)
    float carry = 0.f;
    if (lane == 0) c[0] = 0.f;
    for (int base = 0; base < K; base += 64) {
        const int i = base + lane;
        float p = i < K ? __fdiv_rn(__fadd_rn(w_ray[i], 1e-5f), sum) : 0.f;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float o = __shfl_up(p, off);
            if (lane >= off) p = __fadd_rn(p, o);
        }
        if (i < K) c[i + 1] = __fadd_rn(carry, p);
        carry = __fadd_rn(carry, __shfl(p, 63));
    }
    __syncthreads();  // (every wave of the workgroup runs the same loops: S and N are the launch's)

    const float ox = a.ray_o[ray * 3], oy = a.ray_o[ray * 3 + 1], oz = a.ray_o[ray * 3 + 2];
    const float dx = a.ray_d[ray * 3], dy = a.ray_d[ray * 3 + 1], dz = a.ray_d[ray * 3 + 2];
    // if_clight_renderer.py:68, d / |d|: formed in float64 and rounded once, so within an ulp of the direction itself (the fp32
    // quotient of the march, three roundings under a root and a division, is within two)
    const double dn = sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    const float vx = (float)((double)dx / dn), vy = (float)((double)dy / dn), vz = (float)((double)dz / dn);
    SceneDev sc = {};
    sc.pose = a.pose;  // cull_inside reads the pose alone, and only with pre_affine
    double dev[IMP_MAX / 64], dsum = 0.0;
#pragma unroll
    for (int r = 0; r < IMP_MAX / 64; ++r) {
        const int m = r * 64 + lane;
        dev[r] = 0.0;
        if (m >= N) continue;
        const float u = a.u[(a.u_per_ray ? ray * N : 0) + m];
        int lo = -1, hi = K + 1;  // c[lo] <= u < c[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] <= u) lo = mid;
            else hi = mid;
        }
        const int below = max(hi - 1, 0), above = min(K, hi);  // :75-76
        const float cb = c[below];
        float denom = __fsub_rn(c[above], cb);
        if (denom < 1e-5f) denom = 1.f;  // :86
        const float t = __fdiv_rn(__fsub_rn(u, cb), denom);
        const float bb = b[below];
        const float z = __fadd_rn(bb, __fmul_rn(t, __fsub_rn(b[above], bb)));  // :88
        dev[r] = (double)z - (double)near;  // (the std does not see the shift; the differences are exact in float64)
        dsum += dev[r];
        if (!live) continue;
        const long long o = ray * N + m;
        const float px = ray_point(ox, dx, z), py = ray_point(oy, dy, z), pz = ray_point(oz, dz, z);
        a.z_fine[o] = z;
        a.wpts[o * 3] = px;
        a.wpts[o * 3 + 1] = py;
        a.wpts[o * 3 + 2] = pz;
        a.viewdir[o * 3] = vx;
        a.viewdir[o * 3 + 1] = vy;
        a.viewdir[o * 3 + 2] = vz;
        if (a.keep) a.keep[o] = cull_inside(a.cull, sc, px, py, pz) ? 1 : 0;
    }
    // population standard deviation of the ray's importance depths (volume_renderer.py:117)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
    const double mean = dsum / (double)N;
    double dsq = 0.0;
#pragma unroll
    for (int r = 0; r < IMP_MAX / 64; ++r)
        if (r * 64 + lane < N) dsq += (dev[r] - mean) * (dev[r] - mean);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dsq += __shfl_xor(dsq, off);
    if (live && lane == 0) a.z_std[ray] = (float)sqrt(dsq / (double)N);
}

// (merge_load, merge_rank: nb_merge_rank.h, shared by the two merge kernels)
__global__ __launch_bounds__(256) void importance_merge_kernel(const float *__restrict__ z_coarse, const float *__restrict__ raw_coarse,
                                                               const float *__restrict__ z_fine, const float *__restrict__ raw_fine,
                                                               const unsigned char *__restrict__ keep, long long n_rays, int S, int N,
                                                               float *__restrict__ z_out, float *__restrict__ raw_out) {
    __shared__ float s_z[RAYS_PER_BLOCK][MERGED_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray_raw = (long long)blockIdx.x * RAYS_PER_BLOCK + wv;
    const bool live = ray_raw < n_rays;
    const long long ray = live ? ray_raw : n_rays - 1;
    const int T = S + N;
    float *z = s_z[wv];
    merge_load(z, z_coarse, z_fine, ray, S, N, lane);
    __syncthreads();
    if (!live) return;
    for (int e = lane; e < T; e += 64) {
        const float ze = z[e];
        const int rank = merge_rank(z, T, e);
        f32x4 r;
        if (e < S) {
            r = *reinterpret_cast<const f32x4 *>(raw_coarse + (ray * S + e) * 4);
        } else {
            const long long f = ray * N + (e - S);
            r = *reinterpret_cast<const f32x4 *>(raw_fine + f * 4);
            if (keep && !keep[f]) r = f32x4{0.f, 0.f, 0.f, 0.f};  // if_clight_renderer_mmsk.py:54-59
        }
        z_out[ray * T + rank] = ze;
        *reinterpret_cast<f32x4 *>(raw_out + (ray * T + rank) * 4) = r;
    }
}

// nb_importance_merge without the raw: the depths alone (volume_renderer.py:93 as the baseline's fine pass uses it)
__global__ __launch_bounds__(256) void importance_merge_z_kernel(const float *__restrict__ z_coarse, const float *__restrict__ z_fine,
                                                                 long long n_rays, int S, int N, float *__restrict__ z_out) {
    __shared__ float s_z[RAYS_PER_BLOCK][MERGED_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray_raw = (long long)blockIdx.x * RAYS_PER_BLOCK + wv;
    const bool live = ray_raw < n_rays;
    const long long ray = live ? ray_raw : n_rays - 1;
    const int T = S + N;
    float *z = s_z[wv];
    merge_load(z, z_coarse, z_fine, ray, S, N, lane);
    __syncthreads();
    if (!live) return;
    for (int e = lane; e < T; e += 64) z_out[ray * T + merge_rank(z, T, e)] = z[e];
}

// the sizes the entries accept
int importance_sizes(const char *who, int64_t n_rays, int32_t S, int32_t N) {
    NB_REQUIRE(n_rays >= 0 && n_rays < (1ll << 31), "%s: n_rays = %lld (0..2^31 - 1)", who, (long long)n_rays);
    NB_REQUIRE(S >= 3, "%s: n_samples = %d (>= 3: weights[1:-1] must not be empty)", who, S);
    NB_REQUIRE(N >= 1 && N <= IMP_MAX, "%s: n_importance = %d (1..%d)", who, N, IMP_MAX);
    NB_REQUIRE(S + N <= MERGED_MAX, "%s: n_samples + n_importance = %d (<= %d)", who, S + N, MERGED_MAX);
    return NB_OK;
}

}  // namespace

extern "C" int nb_importance_sample(const float *ray_o, const float *ray_d, const float *near, const float *far, int64_t n_rays,
                                    int32_t n_samples, const float *t_vals, const float *t_rand, const float *weights,
                                    int32_t n_importance, const float *u, int u_per_ray, const nb_cull *cull, const float *pose,
                                    float *z_coarse, float *z_fine, float *wpts, float *viewdir, uint8_t *keep, float *z_std,
                                    void *stream) {
    if (int rc = importance_sizes("nb_importance_sample", n_rays, n_samples, n_importance)) return rc;
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(ray_o && ray_d && near && far && t_vals && weights && u && z_fine && wpts && viewdir && z_std,
               "nb_importance_sample: NULL pointer");
    NB_REQUIRE((cull != nullptr) == (keep != nullptr), "nb_importance_sample: keep goes with cull (both or neither)");
    SampleArgs a = {};
    if (int rc = fill_cull(cull, &a.cull)) return rc;
    NB_REQUIRE(!cull || !cull->pre_affine || pose, "nb_importance_sample: pre_affine needs the pose block (nb_scene.pose)");
    a.ray_o = ray_o, a.ray_d = ray_d, a.near = near, a.far = far, a.t_vals = t_vals, a.t_rand = t_rand, a.weights = weights, a.u = u;
    a.n_rays = n_rays, a.S = n_samples, a.N = n_importance, a.u_per_ray = u_per_ray ? 1 : 0;
    a.pose = pose;
    a.z_coarse = z_coarse, a.z_fine = z_fine, a.wpts = wpts, a.viewdir = viewdir, a.z_std = z_std, a.keep = keep;
    hipLaunchKernelGGL(importance_sample_kernel, dim3(nb_ceil_div(n_rays, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, a);
    NB_CHECK_LAUNCH("nb_importance_sample");
    return NB_OK;
}

extern "C" int nb_importance_merge(const float *z_coarse, const float *raw_coarse, const float *z_fine, const float *raw_fine,
                                   const uint8_t *keep, int64_t n_rays, int32_t n_samples, int32_t n_importance, float *z_vals,
                                   float *raw, void *stream) {
    if (int rc = importance_sizes("nb_importance_merge", n_rays, n_samples, n_importance)) return rc;
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(z_coarse && raw_coarse && z_fine && raw_fine && z_vals && raw, "nb_importance_merge: NULL pointer");
    NB_REQUIRE((((uintptr_t)raw_coarse | (uintptr_t)raw_fine | (uintptr_t)raw) & 15) == 0,
               "nb_importance_merge: raw_coarse, raw_fine and raw must be 16-byte aligned");
    hipLaunchKernelGGL(importance_merge_kernel, dim3(nb_ceil_div(n_rays, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream,
                       z_coarse, raw_coarse, z_fine, raw_fine, keep, (long long)n_rays, n_samples, n_importance, z_vals, raw);
    NB_CHECK_LAUNCH("nb_importance_merge");
    return NB_OK;
}

extern "C" int nb_importance_merge_z(const float *z_coarse, const float *z_fine, int64_t n_rays, int32_t n_samples,
                                     int32_t n_importance, float *z_vals, void *stream) {
    if (int rc = importance_sizes("nb_importance_merge_z", n_rays, n_samples, n_importance)) return rc;
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(z_coarse && z_fine && z_vals, "nb_importance_merge_z: NULL pointer");
    hipLaunchKernelGGL(importance_merge_z_kernel, dim3(nb_ceil_div(n_rays, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream,
                       z_coarse, z_fine, (long long)n_rays, n_samples, n_importance, z_vals);
    NB_CHECK_LAUNCH("nb_importance_merge_z");
    return NB_OK;
}
