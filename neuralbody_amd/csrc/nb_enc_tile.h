// nb_enc_tile.h — what the sparse-convolution kernels of nb_encoder.hip and nb_encoder_bwd.hip share (device code, and the list of
// channel pairs their dispatchers walk): the 32-row MFMA tile and its fragments, the spconv index rule, a tile's prologue, the split
// (head / remainder) row loads and the BatchNorm sums' way out.
#pragma once
#include "nb_tile32.h"

// the (Cin, Cout) pairs of SparseConvNet's layers.  The 16-bit forward kernels also run each pair's backward-input convolution
// (Cout -> Cin) and leave out the pairs with a 16-channel side; the 16-bit weight gradient leaves out Cin = 16.
#define NB_FOR_CONV_SHAPES(X) X(16, 16) X(16, 32) X(32, 32) X(32, 64) X(64, 64) X(64, 128) X(128, 128)

typedef _Float16 bf16x8 __attribute__((ext_vector_type(8)));  // 8 fp16 — or the bits of 8 bf16 (the name predates the switch to fp16)
typedef _Float16 nb_h16;
typedef __bf16 nb_bf16x8 __attribute__((ext_vector_type(8)));

// BF: the operands are bf16 head / remainder pairs (the backward-input convolution: gradients span more binades than an
// un-scaled fp16 head holds; a bf16 pair carries 16 mantissa bits, ~2^-16 relative per product) instead of fp16 pairs
template <bool BF>
__device__ __forceinline__ f32x16 nb_mfma16(const bf16x8 a, const bf16x8 b, const f32x16 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nb_bf16x8, a), __builtin_bit_cast(nb_bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
#define NB_MFMA16(a, b, c) nb_mfma16<BF>((a), (b), (c))

namespace {

struct Dims {
    int d, h, w;
};

__device__ __forceinline__ bf16x8 zero_fragment() {
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (nb_h16)0.f;
    return z;
}

// THE spconv index rule (k = 3, p = 1): row of the input level under kernel offset o of output voxel (z, y, x), or -1.
// stride > 0: the forward gather, input voxel = stride * out - 1 + k.
// stride < 0: the TRANSPOSED gather of a layer of stride -stride, "input" voxel = (out - 1 + k) / -stride where that divides.
// One rule, because a layer's backward-input product is itself a convolution: input voxel p receives dx[u] . W[k]^T from every
// output voxel u with s u - 1 + k = p, i.e. u = (p + 1 - k) / s = (p - 1 + (2 - k)) / s — the transposed gather of p under the
// MIRRORED offset 26 - o (tests/test_spconv_restatements.py: test_backward_input_of_a_strided_layer_is_a_convolution_with_a_
// transposed_gather).  conv_bwd_in_kernel asks with (26 - o, -stride); the 16-bit backward-input convolution with (o, -stride) on
// weights whose offsets nb_enc_conv_pack16 mode 1 has already mirrored; conv_rulebook_kernel and the forward kernels with (o, stride).
__device__ __forceinline__ int neighbour_row(const int *__restrict__ in_grid, Dims gi, int z, int y, int x, int o, int stride, bool valid) {
    const int kd = o / 9, kh = (o / 3) % 3, kw = o % 3;
    const int mul = stride > 0 ? stride : 1, low = stride > 0 ? 0 : -stride - 1, sh = stride > 0 ? 0 : (-stride) >> 1;  // -stride in {1, 2}
    int iz = z * mul - 1 + kd, iy = y * mul - 1 + kh, ix = x * mul - 1 + kw;
    if (!valid || ((iz | iy | ix) & low) != 0 || iz < 0 || iy < 0 || ix < 0) return -1;
    iz >>= sh, iy >>= sh, ix >>= sh;
    if (iz >= gi.d || iy >= gi.h || ix >= gi.w) return -1;
    return in_grid[((long long)iz * gi.h + iy) * gi.w + ix];
}

// A wave's tile of 32 rows of a level: lane (i, hi) looks up the neighbours of row row0 + i (both halves of the wave hold the same
// 32 rows; hi selects the half of the K chunk the lane loads and the D rows it holds, tile_row).
struct ConvTile {
    int lane, i, hi;
    int row0, n;  // the tile's first row; live rows of the level
    bool valid;   // row0 + i is a live row
    int z, y, x;  // ... and its voxel
    // false: the whole workgroup (rows from wg_row0 on) is past the live rows — workgroup-uniform, so the waves of a live workgroup
    // all reach its barriers
    __device__ __forceinline__ bool init(int row0_, int wg_row0, const int *__restrict__ n_rows, const int *__restrict__ rows_lin, Dims g) {
        lane = threadIdx.x & 63, i = lane & 31, hi = lane >> 5;
        row0 = row0_;
        n = *n_rows;
        if (wg_row0 >= n) return false;
        valid = row0 + i < n;
        const int lin = valid ? rows_lin[row0 + i] : 0;
        x = lin % g.w, y = (lin / g.w) % g.h, z = lin / (g.w * g.h);
        return true;
    }
    // the row under kernel offset o (`live` false: -1).  MIRROR: the transposed gather under the mirrored offset (see neighbour_row),
    // stride = the layer's.
    template <bool MIRROR = false>
    __device__ __forceinline__ int neighbour(const int *__restrict__ grid, Dims g, int o, int stride, bool live = true) const {
        return neighbour_row(grid, g, z, y, x, MIRROR ? 26 - o : o, MIRROR ? -stride : stride, live && valid);
    }
    template <bool MIRROR = false>
    __device__ __forceinline__ void fill_neighbours(int (&nbrs)[27], const int *__restrict__ grid, Dims g, int stride) const {
#pragma unroll
        for (int o = 0; o < 27; ++o) nbrs[o] = neighbour<MIRROR>(grid, g, o, stride);
    }
};

// The fp32 kernels' A operand: half hi of the C channels of a lane's neighbour row (row 0 for a lane without one), 16 bytes a load
template <int C>
__device__ __forceinline__ void load_row_half(const float *__restrict__ rows, int nbr, int hi, f32x4 (&dst)[C / 8]) {
    const f32x4 *p = reinterpret_cast<const f32x4 *>(rows + (size_t)(nbr >= 0 ? nbr : 0) * C + hi * (C / 2));
#pragma unroll
    for (int q = 0; q < C / 8; ++q) dst[q] = p[q];
}
// ... as the MFMA's K values, zeros for a lane without a neighbour
template <int C>
__device__ __forceinline__ void mask_row_half(const f32x4 (&src)[C / 8], bool has, float (&A)[C / 2]) {
#pragma unroll
    for (int q = 0; q < C / 8; ++q) {
        const f32x4 v = src[q];
        A[4 * q] = has ? v.x : 0.f;
        A[4 * q + 1] = has ? v.y : 0.f;
        A[4 * q + 2] = has ? v.z : 0.f;
        A[4 * q + 3] = has ? v.w : 0.f;
    }
}

// K chunk c (16 channels) of the A fragments of split rows ([cap, CIN] heads | in_plane further on: remainders): lane (row i, half
// hi) holds channels 16 c + 8 hi .. + 7 of its neighbour row (row 0 for a lane without one: the consumer zeroes it)
template <int CIN>
__device__ __forceinline__ void load_split_chunk(const unsigned short *__restrict__ in_split, long long in_plane, int nbr, int hi, int c,
                                                 bf16x8 &ah, bf16x8 &al) {
    const size_t r = (size_t)(nbr >= 0 ? nbr : 0) * CIN + 8 * hi + 16 * c;
    ah = *reinterpret_cast<const bf16x8 *>(in_split + r);
    al = *reinterpret_cast<const bf16x8 *>(in_split + in_plane + r);
}
template <int CIN>
__device__ __forceinline__ void load_split_rows(const unsigned short *__restrict__ in_split, long long in_plane, int nbr, int hi,
                                                bf16x8 (&ah)[CIN / 16], bf16x8 (&al)[CIN / 16]) {
#pragma unroll
    for (int c = 0; c < CIN / 16; ++c) load_split_chunk<CIN>(in_split, in_plane, nbr, hi, c, ah[c], al[c]);
}

// ------------------------------------------------------------------ a tile's way out
// The BatchNorm sums (fp64: sum and sum of squares per channel) of a workgroup's waves meet in LDS and leave as ONE atomic per
// channel and workgroup.  As one pair of atomics per WAVE the ~900 waves of a 29 k-row level queued on the layer's 2 COUT addresses:
// 14 of the 52 us of a 64 -> 64 launch (profiles/r05_conv_stamps.log).  `red`: NW * NT * 64 doubles of LDS, [wave][tile][sum, sum of
// squares][channel of the tile], written by the waves before the call (each lane's sums over the rows of its half, the two halves
// added by a shuffle; that half stays in the callers: as a helper of its own it cost the two-tile kernels 13-20 registers and a copy
// of the accumulators per offset).  Every wave of the workgroup calls this: the slots summed in wave order, one atomic per sum.
template <int COUT, int NT, int NW>
__device__ __forceinline__ void add_channel_sums(const double *red, int ct, double *__restrict__ stats) {
    __syncthreads();
    if (threadIdx.x < NT * 64) {  // thread = (tile, which sum, channel of the tile)
        const int t = threadIdx.x >> 6, which = (threadIdx.x >> 5) & 1, co = (ct + t) * 32 + (threadIdx.x & 31);
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[((w * NT + t) * 2 + which) * 32 + (threadIdx.x & 31)];
        if ((COUT % 32 == 0) || co < COUT) atomicAdd(&stats[which * COUT + co], v);
    }
}

// The tile is stored and its sums go the way above.  Every wave of the workgroup calls this (a wave without rows brings zeros;
// `active` false: a wave beyond the NW that hold tiles, for the barrier only); `red` must be LDS that nobody reads or writes any more.
template <int COUT, int NT, int NW>
__device__ __forceinline__ void store_tile_and_sums(const f32x16 (&acc)[NT], int row0, int n, int ct, float *__restrict__ out_rows,
                                                    double *__restrict__ stats, double *red, int wv, int lane,
                                                    bool active = true) {
    const int i = lane & 31, hi = lane >> 5;
    // D fragment: lane (j = i, hi) holds channel (ct + t) * 32 + j of rows row0 + tile_row(r, hi)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (!active) break;  // (wave-uniform) a wave that only keeps the barrier company
        const int co = (ct + t) * 32 + i;
        const bool cok = (COUT % 32 == 0) || co < COUT;
        double s = 0.0, ss = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = row0 + tile_row(r, hi);
            const float v = acc[t][r];
            if (orow < n && cok) {
                out_rows[(size_t)orow * COUT + co] = v;
                s += (double)v;
                ss += (double)v * (double)v;
            }
        }
        s += __shfl_xor(s, 32);
        ss += __shfl_xor(ss, 32);
        if (hi == 0) {
            red[((wv * NT + t) * 2) * 32 + i] = s;
            red[((wv * NT + t) * 2 + 1) * 32 + i] = ss;
        }
    }
    add_channel_sums<COUT, NT, NW>(red, ct, stats);
}

}  // namespace
