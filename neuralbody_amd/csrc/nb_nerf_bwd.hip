// nb_nerf_bwd.hip — the input-gradient chain of the vanilla-NeRF MLP (nb_nerf.hip is the forward) as one kernel: a workgroup
// carries the gradients of 64 samples from d raw back to the first layer's pre-activation, the gradient image never leaves LDS,
// the transposed weights stream from a blob packed once in MFMA fragment order (nb_nerf_pack_bwd), the relu masks are the
// forward's own stored activations (the tap of nb_nerf_decode_tap), and every pre-activation gradient goes to the d-tap, from
// which the parameter gradients are plain GEMMs and column sums (neuralbody_amd/nerf.py).
//
// Restates what autograd does for lib/networks/nerf.py:45-65 (zju3dv/neuralbody) up to the parameters' own gradients.
//
// LAYOUT.  LDS holds the tile's gradient transposed, g[row][sample] with 64 samples per row, 256 rows: the image of nb_nerf.hip
// without its embedding rows.  A step is out^T[j][sample] = W^T[j][k] . g[k][sample], the transposed matrix packed like a forward
// matrix of 256 output features (nb_nerf_mm.h: bw_*), so the layer body, the publish and the fragment-to-row stores are the
// forward's.  Wave w of four owns output features [64 w, 64 w + 64) of all 64 samples.
//
// ARITHMETIC, exact fp32 (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain), accumulators start at 0, k ascending:
//   dV[i]    = [V[i] > 0] . fmaf(Wrgb[2][i], d_rgb[2], fmaf(Wrgb[1][i], d_rgb[1], Wrgb[0][i] * d_rgb[0]))             i < 128
//   dfeat[j] = sum_{i = 0..127} Wv[i][j] dV[i]                                                                          j < 256
//   dz7[j]   = [h7[j] > 0] . fmaf(Walpha[j], d_sigma, sum_{i = 0..255} Wf[i][j] dfeat[i])
//   dz_{L-1}[j] = [h_{L-1}[j] > 0] . sum_{i = 0..255} W_L[i][c(j)] dz_L[i]       L = 7 .. 1, c(j) = 63 + j for the skip layer 5, else j
// [x > 0] is 1 where the stored post-activation value is greater than 0 and 0 otherwise (an activation that is exactly 0 passes no
// gradient, as torch.relu's backward).  No atomics: the same inputs give the same bits.  A padding sample of the last tile
// repeats the last point's masks, has d raw = 0, and stores nothing.
#include "nb_nerf_mm.h"

namespace {

using namespace nbnerf;

constexpr int LDS_BYTES_BWD = 256 * TILE * 4;

struct PackBwdArgs {
    const float *w[N_BW], *rgb_w, *alpha_w;
    float *packed;
};

// source of transposed matrix j: row stride and first column of its 256 output features in the reference's weight
__host__ __device__ constexpr int bw_ld(int j) { return j == 0 ? mm_in(MM_VIEWS) : (j == 1 ? 256 : mm_in(9 - j)); }
__host__ __device__ constexpr int bw_c0(int j) { return j == 9 - MM_SKIP ? N_PTS_EMB : 0; }  // nerf.py:53: the input first

// packed transposed matrix j: [wave 4][chunk bw_k / 16][feature tile 2][lane 64][k-step 8]; j == N_BW: the two heads' weights
__global__ __launch_bounds__(256) void nerf_pack_bwd_kernel(PackBwdArgs a, int j) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (j == N_BW) {
        if (idx < 384) a.packed[BW_OFF_RGB + idx] = a.rgb_w[idx];
        if (idx < 256) a.packed[BW_OFF_ALPHA + idx] = a.alpha_w[idx];
        return;
    }
    const int C = bw_k(j) / 16;
    if (idx >= 256 * bw_k(j)) return;
    const int e = idx & 7, lane = (idx >> 3) & 63;
    int rest = idx >> 9;
    const int ft = rest & 1;
    rest >>= 1;
    const int c = rest % C, wv = rest / C;
    const int feature = (wv * 2 + ft) * 32 + (lane & 31);
    const int kk = 16 * c + 2 * e + (lane >> 5);  // k-step e of the chunk, k = 2 e + lane half: an OUTPUT feature of the forward
    a.packed[bw_off(j) + idx] = a.w[j][(size_t)kk * bw_ld(j) + bw_c0(j) + feature];
}

struct ChainArgs {
    const float *bw, *tap, *d_raw;
    long long n_pts;
    float *dtap;
};

__global__ __launch_bounds__(256) void nerf_bwd_chain_kernel(ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float g[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5;
    const long long last = a.n_pts - 1;
    // the two samples whose D fragments this lane holds (sample tiles 0 and 1): tap rows to read the masks from (a padding sample
    // reads the last point's), d-tap rows to write (NULL = padding), d sigma
    const long long p0 = (long long)blockIdx.x * TILE + (lane & 31), p1 = p0 + 32;
    const bool l0 = p0 <= last, l1 = p1 <= last;
    const float *tp0 = a.tap + (l0 ? p0 : last) * NT_COLS, *tp1 = a.tap + (l1 ? p1 : last) * NT_COLS;
    float *dt0 = l0 ? a.dtap + p0 * NDT_COLS : nullptr, *dt1 = l1 ? a.dtap + p1 * NDT_COLS : nullptr;
    const float ds0 = l0 ? a.d_raw[p0 * 4 + 3] : 0.f, ds1 = l1 ? a.d_raw[p1 * 4 + 3] : 0.f;

    {  // dV on the VALU: thread (sample s, quarter q) forms features [32 q, 32 q + 32), four at a time
        const int s = lane, q = wave;
        const long long pt_raw = (long long)blockIdx.x * TILE + s;
        const bool live = pt_raw <= last;
        const long long pt = live ? pt_raw : last;
        const float d0 = live ? a.d_raw[pt * 4] : 0.f, d1 = live ? a.d_raw[pt * 4 + 1] : 0.f, d2 = live ? a.d_raw[pt * 4 + 2] : 0.f;
        const float *rw = a.bw + BW_OFF_RGB;
        for (int i0 = 32 * q; i0 < 32 * q + 32; i0 += 4) {
            const f32x4 m = *reinterpret_cast<const f32x4 *>(a.tap + pt * NT_COLS + NT_V + i0);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = fmaf(rw[256 + i0 + i], d2, fmaf(rw[128 + i0 + i], d1, __fmul_rn(rw[i0 + i], d0)));
                v[i] = m[i] > 0.f ? t : 0.f;
                g[(i0 + i) * TILE + s] = v[i];
            }
            if (live) *reinterpret_cast<f32x4 *>(a.dtap + pt * NDT_COLS + NDT_V + i0) = v;
        }
    }
    __syncthreads();

    f32x16 acc[2][2];
    // dfeat = Wv[:, :256]^T dV: no mask (feature_linear has no activation)
    mm_layer<2, false>(a.bw + bw_off(0) + wave * (bw_k(0) * 64), nullptr, g, 0, bw_k(0) / 16, 0, 0, acc, lane);
    store_rows<2, false>(acc, dt0 ? dt0 + NDT_FEATURE + 64 * wave : nullptr, dt1 ? dt1 + NDT_FEATURE + 64 * wave : nullptr, lane);
    publish<2, false>(acc, g, 64 * wave, lane);

#pragma unroll 1
    for (int j = 1; j < N_BW; ++j) {  // feature_linear^T (+ alpha_linear^T), then pts_linears[7..1]^T: the gradient of z_i, i = 8 - j
        const int i = 8 - j, c = 256 * i + 64 * wave;
        f32x4 mk[2][2][4];  // h_i of the lane's fragments: in flight while the MFMAs run
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    mk[st][ft][gq] = *reinterpret_cast<const f32x4 *>((st == 0 ? tp0 : tp1) + NT_H + c + 32 * ft + 8 * gq + 4 * hi);
        mm_layer<2, false>(a.bw + bw_off(j) + wave * (bw_k(j) * 64), nullptr, g, 0, bw_k(j) / 16, 0, 0, acc, lane);
        if (j == 1) {  // alpha_linear reads h7 too (nerf.py:56)
            const float *aw = a.bw + BW_OFF_ALPHA + 64 * wave;
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float w = aw[32 * ft + tile_row(r, hi)];
                    acc[ft][0][r] = fmaf(w, ds0, acc[ft][0][r]);
                    acc[ft][1][r] = fmaf(w, ds1, acc[ft][1][r]);
                }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ft][st][r] = mk[st][ft][r >> 2][r & 3] > 0.f ? acc[ft][st][r] : 0.f;
        store_rows<2, false>(acc, dt0 ? dt0 + NDT_Z + c : nullptr, dt1 ? dt1 + NDT_Z + c : nullptr, lane);
        if (i > 0) publish<2, false>(acc, g, 64 * wave, lane);  // (block-uniform: the barriers inside are met by all or none)
    }
}

}  // namespace

extern "C" int64_t nb_nerf_pack_bwd_size(void) { return BW_PACK_FLOATS; }

extern "C" int nb_nerf_pack_bwd(const nb_nerf_params *params, float *packed_bwd, void *stream) {
    NB_REQUIRE(params && packed_bwd, "nb_nerf_pack_bwd: NULL pointer");
    NB_REQUIRE(((uintptr_t)packed_bwd & 15) == 0, "nb_nerf_pack_bwd: packed_bwd must be 16-byte aligned");
    PackBwdArgs a = {};
    a.w[0] = params->views_w, a.w[1] = params->feature_w;
    for (int j = 2; j < N_BW; ++j) a.w[j] = params->pts_w[9 - j];
    a.rgb_w = params->rgb_w, a.alpha_w = params->alpha_w;
    a.packed = packed_bwd;
    uintptr_t bits = (uintptr_t)a.rgb_w | (uintptr_t)a.alpha_w;
    for (int j = 0; j < N_BW; ++j) {
        NB_REQUIRE(a.w[j], "nb_nerf_pack_bwd: NULL weight (transposed matrix %d)", j);
        bits |= (uintptr_t)a.w[j];
    }
    NB_REQUIRE(a.rgb_w && a.alpha_w, "nb_nerf_pack_bwd: NULL alpha_linear / rgb_linear weight");
    NB_REQUIRE((bits & 3) == 0, "nb_nerf_pack_bwd: every parameter must be 4-byte aligned");
    for (int j = 0; j <= N_BW; ++j) {
        const int n = j == N_BW ? 384 : 256 * bw_k(j);
        hipLaunchKernelGGL(nerf_pack_bwd_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, j);
        NB_CHECK_LAUNCH("nb_nerf_pack_bwd");
    }
    return NB_OK;
}

extern "C" int nb_nerf_bwd_chain(const float *packed_bwd, const float *tap, const float *d_raw, int64_t n_pts, float *dtap,
                                 void *stream) {
    NB_REQUIRE(n_pts >= 0 && n_pts / TILE < (1ll << 31) - 1, "nb_nerf_bwd_chain: n_pts = %lld (0 .. < 2^37)", (long long)n_pts);
    if (n_pts == 0) return NB_OK;
    NB_REQUIRE(packed_bwd && tap && d_raw && dtap, "nb_nerf_bwd_chain: NULL pointer");
    NB_REQUIRE((((uintptr_t)packed_bwd | (uintptr_t)tap | (uintptr_t)dtap) & 15) == 0,
               "nb_nerf_bwd_chain: packed_bwd, tap and dtap must be 16-byte aligned");
    NB_REQUIRE(((uintptr_t)d_raw & 3) == 0, "nb_nerf_bwd_chain: d_raw must be 4-byte aligned");
    NB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nerf_bwd_chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               LDS_BYTES_BWD));
    ChainArgs a = {packed_bwd, tap, d_raw, (long long)n_pts, dtap};
    hipLaunchKernelGGL(nerf_bwd_chain_kernel, dim3(nb_ceil_div(n_pts, TILE)), dim3(256), LDS_BYTES_BWD, (hipStream_t)stream, a);
    NB_CHECK_LAUNCH("nb_nerf_bwd_chain");
    return NB_OK;
}
