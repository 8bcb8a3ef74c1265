// nb_tile32.h — the vocabulary of a 32x32 MFMA tile, shared by the march (nb_march_common.h), the encoder (nb_enc_tile.h) and the
// backward matrix kernels (nb_tile_out.h): the vector types, the exact-fp32 MFMA, the D fragment's row order, a zeroed accumulator.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define NB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// row of a 32x32 D fragment that accumulator register r of a lane of half hi (= lane >> 5) holds; the lane's column is lane & 31
__host__ __device__ constexpr int tile_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ f32x16 zero_acc() {
    f32x16 a;
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
    return a;
}
