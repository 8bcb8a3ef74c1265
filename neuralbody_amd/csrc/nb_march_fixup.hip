// nb_march_fixup.hip — the last-sample fix-up behind an NB_PREC_F16F6 march (nb_march_fold.hip), gfx950.
//
// The LAST sample's interval is 1e10 (nerf_net_utils.py:28): its alpha is a step function of the sign of its density, and the
// f16f6 arithmetic's density error can put a ray on the other side of the step.  The march lists such rays (list_ill_ray); this
// kernel runs once per view behind it, in 256-thread fp64 workgroups, on the same stream and with no host involved.
#include "nb_fold_level.h"
#include "nb_pack_layout.h"

using namespace nbm;

namespace {

// ---------------------------------------------------------------- last-sample fix-up
// The rays composite_step listed (their last density within NB_ILL_SIGMA of zero): one workgroup per record recomputes that ONE
// density at fp32 level — fc_0 through the same folded planes (head + remainder = 22 bits of fc_0 . V, trilinear weights in fp32,
// fp64 accumulation), fc_1 / fc_2 / alpha_fc from the fp32 fragments of the packed blob (fp64 accumulation, activations rounded to
// fp32 between the layers like the reference's) — and composites the last sample again from the listed state, exactly as
// RayAccum::add / store do.  Thread f owns natural feature f.
__device__ __forceinline__ int frag_bias_index(int f) {  // natural feature f inside a [tile][hi][16] block (b_pack, nb_march.hip)
    const int t = f >> 5, i = f & 31;
    return (t * 2 + tile_hi(i)) * 16 + tile_reg(i);
}
// row `row` of a 256 x 256 layer stored as fp32 A fragments (a_pack kind 1): the 16 bytes at ((tile * 32 + g) * 64 + hi * 32 + row % 32)
// hold the weights of input columns 8 g + 4 hi .. + 3 (col_hidden(4 g + i, hi) = 8 g + 4 hi + i)
__device__ __forceinline__ double frag_row_dot(const float *wfrag, const float *h, int row) {
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(wfrag) + (size_t)(row >> 5) * 32 * 64 + (row & 31);
    double s = 0.0;
    for (int g = 0; g < 32; ++g)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) {
            const f32x4 w = w4[g * 64 + hi * 32];
            const float *hh = h + 8 * g + 4 * hi;
            s = fma((double)w.x, (double)hh[0], s);
            s = fma((double)w.y, (double)hh[1], s);
            s = fma((double)w.z, (double)hh[2], s);
            s = fma((double)w.w, (double)hh[3], s);
        }
    return s;
}
__global__ __launch_bounds__(256) void nb_march_fixup_kernel(MarchArgs a) {
    __shared__ float rec[NB_ILL_RECORD_FLOATS];
    __shared__ float cw[32];
    __shared__ int crow[32];
    __shared__ float h[2][256];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    int *hdr = reinterpret_cast<int *>(a.ill);
    const int n = min(hdr[0], a.ill_cap);
    const int S = a.n_samples;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        __syncthreads();
        if (tid < NB_ILL_RECORD_FLOATS) rec[tid] = a.ill[NB_ILL_HEADER_FLOATS + (long long)it * NB_ILL_RECORD_FLOATS + tid];
        __syncthreads();
        const long long ray = __float_as_int(rec[0]);
        const float z = rec[4];
        if (tid < 32) {  // (level, corner): weight and U row, with the march's own arithmetic (prep_sequential, wt_build)
            const int L = tid >> 3, corner = tid & 7;
            const float px = ray_point(a.ray_o[ray * 3 + 0], a.ray_d[ray * 3 + 0], z), py = ray_point(a.ray_o[ray * 3 + 1], a.ray_d[ray * 3 + 1], z),
                        pz = ray_point(a.ray_o[ray * 3 + 2], a.ray_d[ray * 3 + 2], z);
            const GridCoord g = grid_coords(a.sc, px, py, pz);
            Lvl lv;
            lv.D = a.sc.dhw[L][0]; lv.H = a.sc.dhw[L][1]; lv.W = a.sc.dhw[L][2];
            lv.fmx = a.sc.fm1[L][2]; lv.fmy = a.sc.fm1[L][1]; lv.fmz = a.sc.fm1[L][0];
            lv.fpx = a.sc.fp1[L][2]; lv.fpy = a.sc.fp1[L][1]; lv.fpz = a.sc.fp1[L][0];
            const LvlIdx q = level_index(lv, g);
            const float fx = (float)q.x0, fy = (float)q.y0, fz = (float)q.z0;
            const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
            const float wx = dx ? q.ix - fx : (fx + 1.f) - q.ix, wy = dy ? q.iy - fy : (fy + 1.f) - q.iy, wz = dz ? q.iz - fz : (fz + 1.f) - q.iz;
            const int xx = q.x0 + dx, yy = q.y0 + dy, zz = q.z0 + dz;
            const bool inb = (unsigned)xx < (unsigned)lv.W && (unsigned)yy < (unsigned)lv.H && (unsigned)zz < (unsigned)lv.D;
            int row = -1;
            if (inb) {
                const int rid = a.fold.grid[L][((size_t)zz * lv.H + yy) * lv.W + xx];
                if (rid >= 0) row = a.fold.row_base[L] + rid;
            }
            cw[tid] = (wx * wy) * wz;
            crow[tid] = row;
        }
        __syncthreads();
        {
            double s = (double)a.pk[OFF_B0 + frag_bias_index(tid)];
            for (int c = 0; c < 32; ++c) {
                if (crow[c] < 0) continue;  // uniform
                const _Float16 *u = reinterpret_cast<const _Float16 *>(a.fold.urows) + (size_t)crow[c] * 512;
                s = fma((double)cw[c], (double)(float)u[tid] + (double)(float)u[256 + tid], s);
            }
            h[0][tid] = fmaxf((float)s, 0.f);
        }
        __syncthreads();
        h[1][tid] = fmaxf((float)((double)a.pk[OFF_B1 + frag_bias_index(tid)] + frag_row_dot(a.pk + OFF_L1, h[0], tid)), 0.f);
        __syncthreads();
        const float h3 = fmaxf((float)((double)a.pk[OFF_B2 + frag_bias_index(tid)] + frag_row_dot(a.pk + OFF_L2, h[1], tid)), 0.f);
        {
            // alpha_fc: [hi][q] with column col_hidden(q, hi)
            double p = (double)a.pk[OFF_AW + tile_hi(tid & 31) * 128 + hidden_q(tid)] * (double)h3;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) p += __shfl_xor(p, m);
            if ((tid & 63) == 0) red[tid >> 6] = p;
        }
        __syncthreads();
        if (tid == 0) {
            const float sigma = (float)(((red[0] + red[1]) + (red[2] + red[3])) + (double)a.pk[OFF_AB]);
            RayAccum ra;
            ra.T = rec[1]; ra.depth = rec[2]; ra.accw = rec[3];
            ra.cr = rec[8]; ra.cg = rec[9]; ra.cb = rec[10];
            const float out4[4] = {rec[12], rec[13], rec[14], sigma};
            const float w = ra.add(out4, z, rec[5]);
            ra.store(a, ray);
            a.weights[ray * S + (S - 1)] = w;
            if (a.raw) a.raw[(ray * S + (S - 1)) * 4 + 3] = sigma;
            if ((sigma > 0.f) != (rec[6] > 0.f)) atomicAdd(&hdr[1], 1);  // the march had taken the other branch of the step
        }
    }
}

}  // namespace

namespace nbm {

int launch_march_fixup(const MarchArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(nb_march_fixup_kernel, dim3(NB_ILL_FIXUP_BLOCKS), dim3(256), 0, st, a);
    NB_CHECK_LAUNCH("nb_march_fixup_kernel");
    return NB_OK;
}

}  // namespace nbm
