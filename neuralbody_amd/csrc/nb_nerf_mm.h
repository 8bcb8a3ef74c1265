// nb_nerf_mm.h — what the forward (nb_nerf.hip) and the backward (nb_nerf_bwd.hip) of the vanilla-NeRF MLP share: the LDS image's
// row numbers, the layout functions of the packed blob (mm_*), the fp32 matrix layer on v_mfma_f32_32x32x2_f32 and the publish of
// a wave's D fragments into the image.  One copy, so both kernels stream weights in the same [wave][chunk][feature tile][lane]
// [k-step] order.  The layout itself is described at the top of nb_nerf.hip.
#pragma once
#include "nb_march_common.h"

namespace nbnerf {

using namespace nbm;

constexpr int TILE = 64;  // samples per workgroup
constexpr int ROW_PTS = 256, ROW_VIEW = 320, ROW_ALPHA = 352, N_ROWS = 356;
constexpr int N_PTS_EMB = 63, N_VIEW_EMB = 27;  // xyz_res 10, view_res 4

// the ten matrix layers: 0..7 pts_linears, 8 feature_linear, 9 views_linears[0]
constexpr int N_MM = 10, MM_FEATURE = 8, MM_VIEWS = 9, MM_SKIP = 5;
__host__ __device__ constexpr int mm_out(int L) { return L == MM_VIEWS ? 128 : 256; }
__host__ __device__ constexpr int mm_in(int L) { return L == 0 ? 63 : (L == MM_SKIP ? 319 : (L == MM_VIEWS ? 283 : 256)); }
__host__ __device__ constexpr int mm_row0(int L) { return L == 0 ? ROW_PTS : 0; }
__host__ __device__ constexpr int mm_c0(int L) { return L == 0 ? 4 : 16; }  // chunks (16 rows) of the first segment
__host__ __device__ constexpr int mm_row1(int L) { return L == MM_SKIP ? ROW_PTS : ROW_VIEW; }
__host__ __device__ constexpr int mm_c1(int L) { return L == MM_SKIP ? 4 : (L == MM_VIEWS ? 2 : 0); }
__host__ __device__ constexpr int mm_k(int L) { return 16 * (mm_c0(L) + mm_c1(L)); }
__host__ __device__ constexpr int mm_w_off(int L) {
    int o = 0;
    for (int i = 0; i < L; ++i) o += mm_out(i) * mm_k(i);
    return o;
}
constexpr int W_TOTAL = mm_w_off(N_MM);
__host__ __device__ constexpr int mm_b_off(int L) { return W_TOTAL + 256 * L; }
constexpr int OFF_ALPHA_W = mm_b_off(MM_VIEWS) + 128, OFF_ALPHA_B = OFF_ALPHA_W + 256, OFF_RGB_W = OFF_ALPHA_B + 4,
              OFF_RGB_B = OFF_RGB_W + 384, PACK_FLOATS = OFF_RGB_B + 4;
static_assert(W_TOTAL == 593920 && W_TOTAL % 4 == 0, "ten matrices, K padded to whole chunks");

// the weight column that row `row` of the LDS image meets in layer L, -1 = a zero row
__host__ __device__ constexpr int mm_col(int L, int row) {
    if (L == 0) return row - ROW_PTS < N_PTS_EMB ? row - ROW_PTS : -1;
    if (L == MM_SKIP) return row < 256 ? N_PTS_EMB + row : (row - ROW_PTS < N_PTS_EMB ? row - ROW_PTS : -1);  // nerf.py:53
    if (L == MM_VIEWS) return row < 256 ? row : (row - ROW_VIEW < N_VIEW_EMB ? 256 + row - ROW_VIEW : -1);   // nerf.py:58
    return row;
}

// The activation tap of nb_nerf_decode_tap, row-major [n_pts, NT_COLS] fp32: h0 .. h7 after the relu, feature_linear's output,
// the view hidden V after the relu, the 63 point-embedding columns and a zero, the 27 direction-embedding columns and five zeros.
// Every slice starts on a 16-byte boundary of a 16-byte-multiple row.  The d-tap of nb_nerf_bwd_chain, [n_pts, NDT_COLS]: the
// gradients of the loss by the pre-activations z0 .. z7, by feature_linear's output and by views_linears[0]'s pre-activation.
constexpr int NT_H = 0, NT_FEATURE = 2048, NT_V = 2304, NT_PTS = 2432, NT_VIEW = 2496, NT_COLS = 2528;
constexpr int NDT_Z = 0, NDT_FEATURE = 2048, NDT_V = 2304, NDT_COLS = 2432;
static_assert(NT_COLS % 4 == 0 && NDT_COLS % 4 == 0 && NT_VIEW == NT_PTS + 64 && NT_COLS == NT_VIEW + 32, "16-byte slices");

// The transposed matrices of the input-gradient chain (nb_nerf_pack_bwd), in the order the chain runs them: 0 views_linears[0]
// [:, :256]^T (K = 128), 1 feature_linear^T, 2..8 pts_linears[7..1]^T (K = 256; of pts_linears[5] the 256 h columns).  Each is
// packed as a forward matrix with 256 output features and bw_k(j) / 16 chunks, so mm_layer streams it unchanged.  Behind them
// rgb_linear's weight [3,128] and alpha_linear's [256] as they are.
constexpr int N_BW = 9;
__host__ __device__ constexpr int bw_k(int j) { return j == 0 ? 128 : 256; }
__host__ __device__ constexpr int bw_off(int j) { return j == 0 ? 0 : 256 * 128 + (j - 1) * 256 * 256; }
constexpr int BW_TOTAL = bw_off(N_BW), BW_OFF_RGB = BW_TOTAL, BW_OFF_ALPHA = BW_OFF_RGB + 384, BW_PACK_FLOATS = BW_OFF_ALPHA + 256;
static_assert(BW_TOTAL == 557056 && BW_PACK_FLOATS % 4 == 0, "nine transposed matrices");

// One matrix layer of this wave: acc[ft][st] = bias + W . act over the layer's row segments.  wp: the wave's packed weights,
// bias: the bias of the wave's first feature (BIAS = false: not read, the accumulators start at 0).  The next chunk's fragments
// are in flight while a chunk's sixteen MFMAs run.
template <int FT, bool BIAS = true>
__device__ __forceinline__ void mm_layer(const float *__restrict__ wp, const float *__restrict__ bias, const float *act, int row0,
                                         int c0, int row1, int c1, f32x16 (&acc)[FT][2], int lane) {
    const int hi = lane >> 5, col = lane & 31;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b = BIAS ? bias[32 * ft + tile_row(r, hi)] : 0.f;
            acc[ft][0][r] = b;
            acc[ft][1][r] = b;
        }
    const f32x4 *wq = reinterpret_cast<const f32x4 *>(wp) + lane * 2;
    const int C = c0 + c1;
    f32x4 cur[FT][2], nxt[FT][2];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) cur[ft][0] = wq[ft * 128], cur[ft][1] = wq[ft * 128 + 1];
    for (int c = 0; c < C; ++c) {
        const int cn = c + 1 < C ? c + 1 : c;  // (the last chunk reloads itself: no branch around the loads)
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) nxt[ft][0] = wq[(cn * FT + ft) * 128], nxt[ft][1] = wq[(cn * FT + ft) * 128 + 1];
        const int row = c < c0 ? row0 + 16 * c : row1 + 16 * (c - c0);
        const float *b = act + (row + hi) * TILE + col;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float b0 = b[2 * e * TILE], b1 = b[2 * e * TILE + 32];
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                const float w = cur[ft][e >> 2][e & 3];
                acc[ft][0] = NB_MFMA(w, b0, acc[ft][0]);
                acc[ft][1] = NB_MFMA(w, b1, acc[ft][1]);
            }
        }
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) cur[ft][0] = nxt[ft][0], cur[ft][1] = nxt[ft][1];
    }
}

// The wave's tiles go to rows [f0, f0 + 32 FT) of the image, between two barriers: every wave has read the old rows before any
// wave writes, and every row is written before the next layer reads.
template <int FT, bool RELU>
__device__ __forceinline__ void publish(const f32x16 (&acc)[FT][2], float *act, int f0, int lane) {
    const int hi = lane >> 5, col = lane & 31;
    __syncthreads();
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[ft][st][r];
                act[(f0 + 32 * ft + tile_row(r, hi)) * TILE + 32 * st + col] = RELU ? fmaxf(v, 0.f) : v;
            }
    __syncthreads();
}

// A wave's D fragments as rows of a row-major matrix in global memory: registers 4 g .. 4 g + 3 of a lane are the four consecutive
// features 8 g + 4 hi .. + 3 of its tile, so they leave as one 16-byte store.  dst0 / dst1: the row of the lane's sample in sample
// tile 0 / 1 at the wave's first feature, NULL = a padding sample, which stores nothing.
template <int FT, bool RELU>
__device__ __forceinline__ void store_rows(const f32x16 (&acc)[FT][2], float *dst0, float *dst1, int lane) {
    const int hi = lane >> 5;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        float *dst = st == 0 ? dst0 : dst1;
        if (dst == nullptr) continue;
#pragma unroll
        for (int ft = 0; ft < FT; ++ft)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = RELU ? fmaxf(acc[ft][st][4 * g + i], 0.f) : acc[ft][st][4 * g + i];
                *reinterpret_cast<f32x4 *>(dst + 32 * ft + 8 * g + 4 * hi) = v;
            }
    }
}

}  // namespace nbnerf
