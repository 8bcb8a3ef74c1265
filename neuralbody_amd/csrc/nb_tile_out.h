// nb_tile_out.h — the two ways a 32x32 D tile of the backward matrix kernels (nb_backward.hip, nb_encoder_bwd.hip) leaves: fp32 atomics
// (the A^T.B kernels gemm_tn_kernel, conv_bwd_w_kernel, conv_bwd_w16_kernel) and the row epilogue of gemm_rows_kernel and
// gemm_rows_fast_kernel.  gemm_tn16_kernel and gemm_rows16_kernel keep their own copies: on these pieces they compile to other code
// than before and measured 1 - 4 % slower (profiles/backward_tile_refactor.md).  Both pieces take the lane's half hi = lane >> 5 and
// its column from threadIdx.x: the workgroup is one-dimensional and made of whole waves, as every kernel of these files is launched.
#pragma once
#include "nb_tile32.h"

namespace nbto {

// C[row0 + tile_row(r, hi)][col] += alpha val(r) for the NR accumulator registers from r0 on, lane (j = lane & 31, hi) holding column
// col = (the tile's first column) + j.  CHECK_ROWS false: every row of the tile lies below row_limit (a row count that is a multiple
// of 32), no test is compiled.
template <int NR, bool CHECK_ROWS = true, class Val>
__device__ __forceinline__ void tile_atomic_add_regs(Val val, int r0, float *__restrict__ C, int ld, int row0, int col, int row_limit,
                                                     bool col_ok, float alpha) {
    if (!col_ok) return;
    const int hi = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int row = row0 + tile_row(r0 + q, hi);
        if (!CHECK_ROWS || row < row_limit) atomicAdd(&C[(size_t)row * ld + col], alpha * val(r0 + q));
    }
}
template <bool CHECK_ROWS = true>
__device__ __forceinline__ void tile_atomic_add(const f32x16 &acc, float *__restrict__ C, int ld, int row0, int col, int row_limit,
                                                bool col_ok, float alpha) {
    tile_atomic_add_regs<16, CHECK_ROWS>([&](int r) { return acc[r]; }, 0, C, ld, row0, col, row_limit, col_ok, alpha);
}

// A wave's 32 rows (from row0 = the workgroup's first row + 32 x wave) x four 32-column tiles (from col0) of C[R, N]:
//   C = alpha acc + beta C;  mask_y: C = 0 where not Y[row, col] > 0 (the ReLU that followed the layer whose input gradient this is);
//   colsum[col] += sum_rows C (after the mask: that layer's bias gradient), as one fp32 atomic per column per WORKGROUP: the four
//   waves meet in cs_lds (128 floats, zeroed by the kernel at least one barrier earlier) — one atomic per wave made 4096 per address
//   per product and dominated the kernel.  Every thread of the workgroup calls this (a barrier when colsum is given).
__device__ __forceinline__ void rows_epilogue(const f32x16 (&acc)[4], long long row0, int col0, long long R, int N, float alpha, float beta,
                                              float *__restrict__ C, int ldc, const float *__restrict__ mask_y, int ldy,
                                              float *__restrict__ colsum, float *cs_lds) {
    const int i = threadIdx.x & 31, hi = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = col0 + 32 * t + i;
        if (col >= N || row0 >= R) continue;
        float cs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long row = row0 + tile_row(r, hi);
            if (row >= R) continue;
            float v = alpha * acc[t][r];
            float *cp = C + row * ldc + col;
            if (beta != 0.f) v += beta * *cp;
            if (mask_y && !(mask_y[row * ldy + col] > 0.f)) v = 0.f;
            *cp = v;
            cs += v;
        }
        if (colsum) atomicAdd(&cs_lds[32 * t + i], cs);
    }
    if (colsum) {
        __syncthreads();
        if (threadIdx.x < 128 && col0 + (int)threadIdx.x < N) atomicAdd(&colsum[col0 + threadIdx.x], cs_lds[threadIdx.x]);
    }
}

}  // namespace nbto
