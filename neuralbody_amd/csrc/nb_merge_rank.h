// nb_merge_rank.h — the device body of the depth merges (nb_importance_merge, nb_importance_merge_z of nb_importance.hip): the load of a
// ray's concatenated depths into LDS and the stable rank of one entry by counting.
#pragma once
#include <hip/hip_runtime.h>

namespace nbm {

// Rank by counting: entry e of the concatenation (coarse 0..S-1, then fine) goes to the slot whose number is the count of entries
// with a smaller depth plus the earlier entries with the same depth — a stable sort, whatever order the inputs come in.
__device__ __forceinline__ int merge_rank(const float *z, int T, int e) {
    const float ze = z[e];
    int rank = 0;
    for (int j = 0; j < T; ++j) {  // (every lane reads the same word: an LDS broadcast)
        const float zj = z[j];
        rank += (zj < ze || (zj == ze && j < e)) ? 1 : 0;
    }
    return rank;
}

// the wave's ray: the concatenated depths into LDS (a padding wave repeats the last ray and stores nothing)
__device__ __forceinline__ void merge_load(float *z, const float *__restrict__ z_coarse, const float *__restrict__ z_fine,
                                           long long ray, int S, int N, int lane) {
    for (int e = lane; e < S + N; e += 64) z[e] = e < S ? z_coarse[ray * S + e] : z_fine[ray * N + (e - S)];
}

}  // namespace nbm
