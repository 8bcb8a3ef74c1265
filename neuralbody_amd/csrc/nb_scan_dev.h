// Internal: the one count-and-place tile body behind the exclusive scan (nb_scan.hip) and behind every kernel pair that
// folds a scan into the predicate in front of it and the numbering behind it (encoder index sets, nb_sparsify).
//
// A SEQUENCE is a small functor struct, passed by value:
//     int  value(long long i) const             the count of item i (0 / 1 for a predicate, any int >= 0 for a scan)
//     void place(long long i, int value, int prefix) const     prefix = the sum of the values in front of item i
//     void total(int t) const                   the sum of all values, called once
// The count pass needs `value` only, and may take another functor than the place pass.  Each pass calls `value` exactly once per
// item (i < n), so a `value` may write what the other pass reads (the voxeliser's count pass stores its flag); never call it twice.
// Device side first (block scan, tile body, the two kernels), then the host-side launcher count_and_place, which is why this header
// includes nb_scan.h (nb_scan_tops, NB_CHECK_LAUNCH), and the one sequence that more than one file uses (MarkedGrid).
#pragma once
#include <hip/hip_runtime.h>

#include "nb_scan.h"

namespace nbscan {

constexpr int BLOCK = 256;
constexpr int ITEMS = 4;
constexpr int TILE = BLOCK * ITEMS;  // 1024 elements per block
constexpr int FUSED_MAX_BLOCKS = 4096;  // up to here every block sums the block totals in front of it itself (<= 16 KiB from L2)

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

// inclusive scan of one value per thread across a 256-thread block; returns the exclusive prefix of the thread and the block
// total through `total`
__device__ __forceinline__ int block_excl_scan(int v, int *total) {
    __shared__ int wsum[BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        if (i < w) base += wsum[i];
        tot += wsum[i];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// sum of block_sums[0 .. b) by the whole block (the exclusive prefix of block b without a pass over the block totals)
__device__ __forceinline__ int blocks_before(const int *__restrict__ block_sums, int b) {
    int s = 0;
    for (int i = threadIdx.x; i < b; i += BLOCK) s += block_sums[i];
    int tot;
    block_excl_scan(s, &tot);
    return tot;
}

// ------------------------------------------------------------------ the tile body
// how many of a thread's ITEMS items from i0 on lie inside a sequence of n (<= 0: none).  For the place pass: one 64-bit comparison
// per thread and 32-bit guards per item (four 64-bit comparisons kept live across the block scan cost it 7 VGPRs); the count pass
// compiles shorter with the plain comparisons
__device__ __forceinline__ int items_inside(long long i0, long long n) { return (int)min(n - i0, (long long)ITEMS); }

// the values of tile `tile` of a sequence of n items summed into tile_sums[tile]
template <class Seq>
__device__ __forceinline__ void tile_count(Seq seq, long long n, int tile, int *__restrict__ tile_sums) {
    const long long i0 = (long long)tile * TILE + threadIdx.x * ITEMS;
    int s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
        if (i0 + k < n) s += seq.value(i0 + k);
    int tot;
    block_excl_scan(s, &tot);
    if (threadIdx.x == 0) tile_sums[tile] = tot;
}

// every item of the tile placed at its exclusive prefix; `before`: the sum of the tiles in front of this one — blocks_before() of the
// tile sums, or the tile's entry once scan_tops_kernel has scanned them; the sequence's last tile writes the total
template <class Seq>
__device__ __forceinline__ void tile_place(Seq seq, long long n, int tile, int before, bool is_last) {
    const long long i0 = (long long)tile * TILE + threadIdx.x * ITEMS;
    const int m = items_inside(i0, n);
    int v[ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        v[k] = k < m ? seq.value(i0 + k) : 0;
        s += v[k];
    }
    int tot;
    int prefix = block_excl_scan(s, &tot) + before;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (k < m) seq.place(i0 + k, v[k], prefix);
        prefix += v[k];
    }
    if (is_last && threadIdx.x == 0) seq.total(before + tot);
}

template <class Seq>
__global__ __launch_bounds__(BLOCK) void tile_count_kernel(Seq seq, long long n, int *__restrict__ tile_sums) {
    tile_count(seq, n, (int)blockIdx.x, tile_sums);
}

// SELF_SUM: every block sums the tile totals in front of it itself — no pass over the totals, one launch less in every chain
template <bool SELF_SUM, class Seq>
__global__ __launch_bounds__(BLOCK) void tile_place_kernel(Seq seq, long long n, const int *__restrict__ tile_sums) {
    const int tile = (int)blockIdx.x;
    const int before = SELF_SUM ? blocks_before(tile_sums, tile) : tile_sums[tile];
    tile_place(seq, n, tile, before, tile == (int)gridDim.x - 1);
}

// One sequence of n >= 1 items counted and placed: two launches, three (the tile totals get their own pass) beyond
// FUSED_MAX_BLOCKS tiles.  tile_sums: nb_scan_blocks(n) ints.
template <class Count, class Place>
int count_and_place(const char *what, Count count, Place place, long long n, int *tile_sums, hipStream_t st) {
    const int nt = (int)nb_scan_blocks(n);
    const dim3 tiles((unsigned)nt), blk(BLOCK);
    hipLaunchKernelGGL(tile_count_kernel<Count>, tiles, blk, 0, st, count, n, tile_sums);
    if (nt <= FUSED_MAX_BLOCKS) {
        hipLaunchKernelGGL((tile_place_kernel<true, Place>), tiles, blk, 0, st, place, n, tile_sums);
    } else {
        nb_scan_tops(tile_sums, nt, st);
        hipLaunchKernelGGL((tile_place_kernel<false, Place>), tiles, blk, 0, st, place, n, tile_sums);
    }
    NB_CHECK_LAUNCH(what);
    return NB_OK;
}

// ------------------------------------------------------------------ the marked cells of an int32 grid
// Cells >= 0 numbered in linear order: the row id into the cell, the cell into out_lin, both under the capacity (a marked cell beyond
// it becomes -1), the count clamped to it.  A cell is read and rewritten by one thread only.
struct MarkedGrid {
    int *__restrict__ grid, *__restrict__ out_lin, *__restrict__ n_out;
    int cap;
    __device__ __forceinline__ int value(long long i) const { return grid[i] >= 0; }
    __device__ __forceinline__ void place(long long i, int marked, int r) const {
        if (!marked) return;
        grid[i] = r < cap ? r : -1;
        if (r < cap) out_lin[r] = (int)i;
    }
    __device__ __forceinline__ void total(int t) const { *n_out = min(t, cap); }
};

}  // namespace nbscan
