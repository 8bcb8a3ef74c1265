// Internal: the one triangle walker, and its two kernels, behind the silhouette and depth-range rasterisers (nb_silhouette.hip) and the
// z-buffered one (nb_mesh_render.hip).
//
// Triangles are binned by their clipped pixel box.  A box up to SMALL_BOX x SMALL_BOX is walked by the thread that set the triangle
// up; the others go on a device-side list, which a fixed grid of LARGE_BLOCKS workgroups strides over, a workgroup per triangle.
// What a triangle is and what happens at a pixel is the caller's TRIANGLE JOB, a small functor struct, passed by value:
//     bool setup(int g)           triangle g (0 <= g < n) set up in the job's own members; false: nothing to draw.  After true, the
//                                 clipped pixel box (not empty, inclusive) is in the members x0, x1, y0, y1 (Box below)
//     void pixel(int x, int y)    called once for every pixel of the box, by some thread, in no order
// The large pass sets a listed triangle up again, so `setup` is a function of g alone.  The one atomic (a wave's slice of the list)
// orders list entries, which no output bit depends on when `pixel` does not care about order.
// The pointer `pixel` writes through is the job's member `out`.  small_kernel / large_kernel, which every rasteriser instantiates with
// its job, take the job by value but that pointer as a __restrict__ parameter of their own, stored into the job before the pass
// (members cannot carry the qualifier; with the output only a member both rasterisers measured 3 to 6 % slower).
// Integer and control flow only: the callers round their floats in their own files, under their own contraction pragma.
#pragma once
#include <hip/hip_runtime.h>

namespace nbraster {

constexpr int SUB = 256, HALF = SUB / 2;  // sub-pixel units per pixel: vertices are snapped to 1 / SUB pixel
static_assert(SUB == 1 << 8, "Box::clip divides by SUB with >> 8");
constexpr float MAX_PIXEL = 32768.0f;     // nothing beyond it is snapped: |coordinate| <= 2^23, every edge-function product < 2^50
constexpr int SMALL_BOX = 16;             // clipped boxes up to SMALL_BOX x SMALL_BOX are walked by one thread
constexpr int LARGE_BLOCKS = 512;         // the large-triangle launch: a fixed grid striding over the device-side count

template <class T>  // for what belongs to the vertices b and c of a triangle of negative area
__device__ __forceinline__ void swap(T &a, T &b) { const T s = a; a = b, b = s; }

struct Box {
    int x0, x1, y0, y1;
    // Per axis the pixels ceil((min - HALF) / SUB) .. floor((max + up) / SUB) of the triangle's extent, clipped to the image; false:
    // none.  up = +HALF: the closed squares centre -+ HALF that meet the extent; up = -HALF: the centres SUB i + HALF inside it
    __device__ __forceinline__ bool clip(int ax, int ay, int bx, int by, int cx, int cy, int up, int H, int W) {
        x0 = max((min(ax, min(bx, cx)) + HALF - 1) >> 8, 0), x1 = min((max(ax, max(bx, cx)) + up) >> 8, W - 1);
        y0 = max((min(ay, min(by, cy)) + HALF - 1) >> 8, 0), y1 = min((max(ay, max(by, cy)) + up) >> 8, H - 1);
        return x0 <= x1 && y0 <= y1;
    }
};

// One thread per triangle, 256 per workgroup: small boxes are walked here, the others listed for large_pass.
template <class Job>
__device__ __forceinline__ void small_pass(Job &job, int n, int *__restrict__ count, int *__restrict__ large) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool draw = g < n && job.setup(g);
    const bool big = draw && (job.x1 - job.x0 >= SMALL_BOX || job.y1 - job.y0 >= SMALL_BOX);
    // the wave's large triangles take consecutive list places: one atomic per wave that has any
    const unsigned long long m = __ballot(big);
    if (m) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(count, __popcll(m));
        base = __shfl(base, leader, 64);
        if (big) large[base + __popcll(m & ((1ull << lane) - 1ull))] = g;  // < n places in all: every g is listed at most once
    }
    if (!draw || big) return;
    for (int y = job.y0; y <= job.y1; ++y)
        for (int x = job.x0; x <= job.x1; ++x) job.pixel(x, y);
}

// One workgroup per listed triangle, its 256 threads striding over the clipped box; launched with LARGE_BLOCKS workgroups.
template <class Job>
__device__ __forceinline__ void large_pass(Job &job, int n, const int *__restrict__ count, const int *__restrict__ large) {
    const int listed = min(*count, n);
    for (int i = blockIdx.x; i < listed; i += gridDim.x) {
        const int g = large[i];
        if ((unsigned)g >= (unsigned)n || !job.setup(g)) continue;
        const int bw = job.x1 - job.x0 + 1;
        const long long px = (long long)bw * (job.y1 - job.y0 + 1);
        for (long long p = threadIdx.x; p < px; p += 256) job.pixel(job.x0 + (int)(p % bw), job.y0 + (int)(p / bw));
    }
}

// The two launches of a rasteriser: small_kernel with a thread per triangle, then large_kernel with LARGE_BLOCKS workgroups.
template <class Job>
__global__ __launch_bounds__(256) void small_kernel(Job job, decltype(Job::out) __restrict__ out, int n, int *__restrict__ count,
                                                    int *__restrict__ large) {
    job.out = out;  // a parameter for its __restrict__ (above)
    small_pass(job, n, count, large);
}

template <class Job>
__global__ __launch_bounds__(256) void large_kernel(Job job, decltype(Job::out) __restrict__ out, int n, const int *__restrict__ count,
                                                    const int *__restrict__ large) {
    job.out = out;
    large_pass(job, n, count, large);
}

}  // namespace nbraster
