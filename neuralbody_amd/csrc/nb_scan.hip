// Device-wide exclusive scan of int32 counts (two small kernels, three beyond 4 M elements): the tile body of nb_scan_dev.h on a
// plain array.  Deterministic stream compaction wherever the positions are needed afterwards, for random access: ray generation
// and image assembly (mask_at_box, lib/utils/render_utils.py:128-132), the evaluator's metrics, the training-ray sampler (0 / 1
// flags) and marching cubes (edge flags, and 0..5 triangles per cell).  The encoder's index sets and nb_sparsify run the same
// tile body on their own sequences, without a flags or a positions array.
#include "nb_scan.h"

#include "nb_scan_dev.h"

namespace {

struct ArraySeq {
    const int *__restrict__ in;
    int *__restrict__ out, *__restrict__ total_out;
    __device__ __forceinline__ int value(long long i) const { return in[i]; }
    __device__ __forceinline__ void place(long long i, int, int prefix) const { out[i] = prefix; }
    __device__ __forceinline__ void total(int t) const { *total_out = t; }
};

// single block: exclusive scan of the block sums in place
__global__ __launch_bounds__(nbscan::BLOCK) void scan_tops_kernel(int *__restrict__ block_sums, int n_blocks) {
    int carry = 0;
    for (int base = 0; base < n_blocks; base += nbscan::BLOCK) {
        const int i = base + threadIdx.x;
        const int v = i < n_blocks ? block_sums[i] : 0;
        int tot;
        const int ex = nbscan::block_excl_scan(v, &tot);
        if (i < n_blocks) block_sums[i] = carry + ex;
        carry += tot;
    }
}

}  // namespace

long long nb_scan_blocks(long long n) { return (n + nbscan::TILE - 1) / nbscan::TILE; }

void nb_scan_tops(int *block_sums, int n_blocks, hipStream_t st) {
    hipLaunchKernelGGL(scan_tops_kernel, dim3(1), dim3(nbscan::BLOCK), 0, st, block_sums, n_blocks);
}

int nb_exclusive_scan(const int *flags, int *out, int *total, long long n, int *block_sums, hipStream_t st) {
    if (n <= 0) {
        NB_HIP(hipMemsetAsync(total, 0, sizeof(int), st));
        return NB_OK;
    }
    const ArraySeq seq = {flags, out, total};
    return nbscan::count_and_place("nb_exclusive_scan", seq, seq, n, block_sums, st);
}

extern "C" int64_t nb_scan_scratch_size(int64_t n) {
    if (n < 0) n = 0;
    // [flags n][positions n][block sums][total slot]  (int32), 256-byte aligned sections.  The last 256 bytes are the spare int
    // behind the block sums (nb_scan_total_slot): where a caller that needs the scan's total on the device only lets it land.
    return 2 * nb_align256(n * 4) + nb_align256(nb_scan_blocks(n) * 4) + 256;
}

void nb_scan_carve(void *scratch, long long n, int **flags, int **pos, int **block_sums) {
    const long long a = nb_align256(n * 4);
    char *p = static_cast<char *>(scratch);
    if (flags) *flags = reinterpret_cast<int *>(p);
    if (pos) *pos = reinterpret_cast<int *>(p + a);
    if (block_sums) *block_sums = reinterpret_cast<int *>(p + 2 * a);
}
