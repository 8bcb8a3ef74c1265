// nb_field_normal.hip — the surface normal of the density field, n(p) = -grad sigma(p) / |grad sigma(p)|, for rendered views and for
// mesh vertices: the one step of d sigma / d p that no other kernel takes (the gradient of the 4-level trilinear lookup with respect
// to the POINT, nb_trilinear_grad), the list of a marched view's samples that are worth a gradient (nb_normal_select) and the
// per-ray blend of their normals (nb_normal_composite).  The MLP part of the chain is nb_decode_points' tap and nb_gemm_fused.
//
// replaces: nothing in the reference (zju3dv/neuralbody has no normal output; tools/render_mesh.py shades with face normals).
//
// The coordinates are the forward gather's own: grid_coords, unnorm_clamped and cell_weights of nb_march_common.h; the sample
// positions are that header's z_sample (z_lin, z_jitter) and ray_point; the selection is a sequence of the one count-and-place tile
// body (nb_scan_dev.h).  No atomics anywhere: the same inputs give the same bits.
#include "nb_march_common.h"
#include "nb_scan_dev.h"

namespace {

using namespace nbm;

// ------------------------------------------------------------------ nb_trilinear_grad
struct GradArgs {
    SceneDev sc;          // vol[] unused
    const int *grid[4];   // index grid of each dense level (row id or -1)
    const float *rows[4]; // the active rows [n_rows_l, C_l]
    const float *wpts;    // [n,3]
    const float *dF;      // [n,352]
    float *grad;          // [n,3]
    long long n;
    float scale[4][3];    // d(index coordinate) / d(canonical coordinate) of level l along x, y, z: (size - 1) / (voxel_size * out_sh)
};

constexpr int GRP = 8;             // lanes per point: lane j of a group takes the 16-byte pieces j, j + 8, ... of every row
constexpr int GRAD_BLOCK = 256;    // 32 consecutive points per workgroup, 8 per wave (neighbours share voxels: the rows stay in L1 / L2)

// One level of one point, the share of lane j of its group: the three directional differences of the cell's trilinear blend, each
// already multiplied with d_feat and summed over the lane's channels, added to gc scaled to canonical units.
//   p(corner) = sum_c d_feat[c] v(corner)[c]           (0 for a corner out of bounds or with grid entry -1)
//   t_x = sum_{dy,dz} wy[dy] wz[dz] (p(1,dy,dz) - p(0,dy,dz)),  t_y, t_z alike
// A clamped index coordinate (outside [-2, size + 1]) has every corner out of bounds, so such a level adds nothing.
template <int L>
__device__ __forceinline__ void grad_level(const GradArgs &a, const GridCoord &g, const float *__restrict__ dF_p, int j, float (&gc)[3]) {
    constexpr int C = lvl_c(L), PER = C / 4 / GRP;
    const int D = a.sc.dhw[L][0], H = a.sc.dhw[L][1], W = a.sc.dhw[L][2];
    const AxisCell cx = cell_weights(unnorm_clamped(g.gw, W)), cy = cell_weights(unnorm_clamped(g.gh, H)),
                   cz = cell_weights(unnorm_clamped(g.gd, D));
    const int x0 = cx.i0, y0 = cy.i0, z0 = cz.i0;
    const float(&wx)[2] = cx.w, (&wy)[2] = cy.w, (&wz)[2] = cz.w;
    f32x4 d[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) d[k] = *reinterpret_cast<const f32x4 *>(dF_p + lvl_chan_base(L) + 4 * (j + GRP * k));
    float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
        const int xx = x0 + dx, yy = y0 + dy, zz = z0 + dz;
        const bool inb = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D;
        const int row = inb ? a.grid[L][((long long)zz * H + yy) * W + xx] : -1;
        if (row < 0) continue;  // outside the volume, or an inactive voxel: a constant zero
        const f32x4 *__restrict__ r = reinterpret_cast<const f32x4 *>(a.rows[L] + (size_t)row * C);
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const f32x4 v = r[j + GRP * k];
            p = fmaf(d[k].x, v.x, p);
            p = fmaf(d[k].y, v.y, p);
            p = fmaf(d[k].z, v.z, p);
            p = fmaf(d[k].w, v.w, p);
        }
        t[0] = fmaf(dx ? p : -p, wy[dy] * wz[dz], t[0]);
        t[1] = fmaf(dy ? p : -p, wx[dx] * wz[dz], t[1]);
        t[2] = fmaf(dz ? p : -p, wx[dx] * wy[dy], t[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) gc[k] = fmaf(t[k], a.scale[L][k], gc[k]);
}

__global__ __launch_bounds__(GRAD_BLOCK) void trilinear_grad_kernel(GradArgs a) {
    const long long t = (long long)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    const long long pt_raw = t / GRP;
    const bool live = pt_raw < a.n;
    const long long pt = live ? pt_raw : a.n - 1;  // padding lanes repeat the last point (the group sums below need every lane)
    const int j = (int)(t % GRP);
    const GridCoord g = grid_coords(a.sc, a.wpts[pt * 3], a.wpts[pt * 3 + 1], a.wpts[pt * 3 + 2]);
    const float *dF_p = a.dF + pt * 352;
    float gc[3] = {0.f, 0.f, 0.f};
    grad_level<0>(a, g, dF_p, j, gc);
    grad_level<1>(a, g, dF_p, j, gc);
    grad_level<2>(a, g, dF_p, j, gc);
    grad_level<3>(a, g, dF_p, j, gc);
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // the eight lanes of a group are neighbours in the wave
        gc[k] += __shfl_xor(gc[k], 1);
        gc[k] += __shfl_xor(gc[k], 2);
        gc[k] += __shfl_xor(gc[k], 4);
    }
    if (!live || j != 0) return;
    // canonical = (p - Th) @ R, so d/dp_i = sum_j R[i][j] d/dc_j
    const Pose ps = load_pose(a.sc.pose);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        a.grad[pt * 3 + i] = fmaf(ps.R[i * 3 + 2], gc[2], fmaf(ps.R[i * 3 + 1], gc[1], ps.R[i * 3] * gc[0]));
}

// ------------------------------------------------------------------ nb_normal_select
// The samples (ray, s) with weights >= w_min in (ray, s) order, under the capacity: their linear index and their position, the
// latter by the march's own sampling steps (z_sample, ray_point).
struct SelectSeq {
    const float *__restrict__ ray_o, *__restrict__ ray_d, *__restrict__ near, *__restrict__ far, *__restrict__ t_vals,
        *__restrict__ t_rand, *__restrict__ weights;
    float w_min;
    int S;
    float *__restrict__ wpts;
    int *__restrict__ idx, *__restrict__ n_out;
    int cap;
    __device__ __forceinline__ int value(long long i) const { return weights[i] >= w_min; }  // (a NaN weight is not selected)
    __device__ __forceinline__ void place(long long i, int selected, int r) const {
        if (!selected || r >= cap) return;
        const long long ray = i / S;
        const int s = (int)(i - ray * S);
        const float z = z_sample(near[ray], far[ray], t_vals, t_rand ? t_rand + ray * S : nullptr, s, S);
#pragma unroll
        for (int k = 0; k < 3; ++k) wpts[(size_t)r * 3 + k] = ray_point(ray_o[ray * 3 + k], ray_d[ray * 3 + k], z);
        idx[r] = (int)i;
    }
    __device__ __forceinline__ void total(int t) const {
        n_out[0] = min(t, cap);
        n_out[1] = t;
    }
};

// ------------------------------------------------------------------ nb_normal_composite
// One thread per ray: its run in the sorted idx is found by bisection and walked in sample order, so the sums are the same bits in
// every call.  Each step is one IEEE operation (no contraction), which is what the numpy model of the tests restates.
__global__ __launch_bounds__(256) void normal_composite_kernel(const int *__restrict__ idx, const float *__restrict__ grad, long long m,
                                                               const float *__restrict__ weights, long long n_rays, int S,
                                                               float *__restrict__ normal_map, float *__restrict__ normal_acc) {
#pragma clang fp contract(off)
    const long long ray = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= n_rays) return;
    const long long first = ray * S, last = first + S;
    long long lo = 0, hi = m;  // the first k with idx[k] >= first
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (idx[mid] < first) lo = mid + 1;
        else hi = mid;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f, acc = 0.f;
    for (long long k = lo; k < m; ++k) {
        const long long i = idx[k];
        if (i >= last) break;
        const float w = weights[i];
        const float gx = grad[k * 3], gy = grad[k * 3 + 1], gz = grad[k * 3 + 2];
        const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
        acc = acc + w;
        if (!(len >= 1e-12f) || !(len <= 3.4028234664e38f)) continue;  // a zero, NaN or overflowing gradient has no direction
        sx = sx + w * __fdiv_rn(-gx, len);
        sy = sy + w * __fdiv_rn(-gy, len);
        sz = sz + w * __fdiv_rn(-gz, len);
    }
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    const bool unit = len >= 1e-6f && len <= 3.4028234664e38f;
    normal_map[ray * 3 + 0] = unit ? __fdiv_rn(sx, len) : 0.f;
    normal_map[ray * 3 + 1] = unit ? __fdiv_rn(sy, len) : 0.f;
    normal_map[ray * 3 + 2] = unit ? __fdiv_rn(sz, len) : 0.f;
    normal_acc[ray] = acc;
}

constexpr long long SAMPLE_LIMIT = 2147483648ll - 256;  // n_rays * S below this: 32-bit linear sample indices
inline bool samples_fit(int64_t n_rays, int32_t S) {
    return n_rays >= 0 && S >= 0 && n_rays < SAMPLE_LIMIT && (long long)n_rays * S < SAMPLE_LIMIT;
}

}  // namespace

extern "C" int nb_trilinear_grad(const nb_scene *scene, const int32_t *const grids[4], const float *const rows[4], const float *wpts,
                                 const float *d_feat, int64_t n, float *grad, void *stream) {
    NB_REQUIRE(n >= 0 && n < SAMPLE_LIMIT, "nb_trilinear_grad: n = %lld (0..2^31 - 257)", (long long)n);
    if (n == 0) return NB_OK;
    NB_REQUIRE(scene && grids && rows && wpts && d_feat && grad, "nb_trilinear_grad: NULL pointer");
    NB_REQUIRE(((uintptr_t)d_feat & 15) == 0, "nb_trilinear_grad: d_feat must be 16-byte aligned");
    GradArgs a = {};
    nb_scene tmp = *scene;
    for (int l = 0; l < 4; ++l) {
        NB_REQUIRE(grids[l] && rows[l], "nb_trilinear_grad: NULL grid / rows at level %d", l);
        NB_REQUIRE(((uintptr_t)rows[l] & 15) == 0, "nb_trilinear_grad: rows[%d] must be 16-byte aligned", l);
        a.grid[l] = grids[l];
        a.rows[l] = rows[l];
        if (!tmp.vol[l]) tmp.vol[l] = wpts;  // the dense volumes are not read here; any non-NULL pointer passes the check
    }
    if (int rc = fill_scene(&tmp, &a.sc)) return rc;
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 3; ++k)  // x <- W and [2], y <- H and [1], z <- D and [0]
            a.scale[l][k] = a.sc.fm1[l][2 - k] / (a.sc.vs[2 - k] * a.sc.osh[2 - k]);
    a.wpts = wpts;
    a.dF = d_feat;
    a.grad = grad;
    a.n = n;
    hipLaunchKernelGGL(trilinear_grad_kernel, dim3(nb_ceil_div(n * GRP, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, (hipStream_t)stream, a);
    NB_CHECK_LAUNCH("nb_trilinear_grad");
    return NB_OK;
}

extern "C" int nb_normal_select(const float *ray_o, const float *ray_d, const float *near, const float *far, int64_t n_rays,
                                int32_t n_samples, const float *t_vals, const float *t_rand, const float *weights, float w_min,
                                int32_t cap, int32_t *idx, float *wpts, int32_t *n_out, void *scratch, void *stream) {
    NB_REQUIRE(samples_fit(n_rays, n_samples),
               "nb_normal_select: n_rays = %lld, n_samples = %d (n_rays * n_samples < 2^31 - 256)", (long long)n_rays, n_samples);
    const long long n = (long long)n_rays * n_samples;
    if (n == 0) return NB_OK;
    NB_REQUIRE(ray_o && ray_d && near && far && t_vals && weights && n_out && scratch, "nb_normal_select: NULL pointer");
    NB_REQUIRE(cap >= 0 && (cap == 0 || (idx && wpts)), "nb_normal_select: cap = %d, or NULL output with cap > 0", cap);
    const SelectSeq seq = {ray_o, ray_d, near, far, t_vals, t_rand, weights, w_min, n_samples, wpts, idx, n_out, cap};
    int *tile_sums;
    nb_scan_carve(scratch, n, nullptr, nullptr, &tile_sums);
    return nbscan::count_and_place("nb_normal_select", seq, seq, n, tile_sums, (hipStream_t)stream);
}

extern "C" int nb_normal_composite(const int32_t *idx, const float *grad, int64_t m, const float *weights, int64_t n_rays,
                                   int32_t n_samples, float *normal_map, float *normal_acc, void *stream) {
    NB_REQUIRE(samples_fit(n_rays, n_samples),
               "nb_normal_composite: n_rays = %lld, n_samples = %d (n_rays * n_samples < 2^31 - 256)", (long long)n_rays, n_samples);
    NB_REQUIRE(m >= 0 && m <= (long long)n_rays * n_samples, "nb_normal_composite: m = %lld selected of %lld samples", (long long)m,
               (long long)n_rays * n_samples);
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(normal_map && normal_acc && (m == 0 || (idx && grad && weights)), "nb_normal_composite: NULL pointer");
    hipLaunchKernelGGL(normal_composite_kernel, dim3(nb_ceil_div(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, idx, grad,
                       (long long)m, weights, (long long)n_rays, n_samples, normal_map, normal_acc);
    NB_CHECK_LAUNCH("nb_normal_composite");
    return NB_OK;
}
