// nb_silhouette.hip — nb_smpl_silhouette: the posed body's triangles rasterised into a handful of cull cameras, conservatively and
// exactly, as a stand-in for the training-view masks a pose that was never photographed does not have; and nb_body_depth_range: the
// same triangles in the same cameras, every pixel given the camera-depth interval of the triangles that cover it.
//
// Stands where (zju3dv/neuralbody):
//   lib/datasets/light_stage/multi_view_perform_dataset.py:105-127  get_mask: the CIHP masks of real images, read from disk
//   lib/networks/renderer/if_clight_renderer_mmsk.py:12-45          the consumer: round -> clamp lookup of a sample's pixel
// Vertices go through the cull's projection (cull_project, beside cull_inside in nb_march_common.h) and are snapped to 1/256 pixel; everything
// behind the snap is integer arithmetic (edge functions in int64, |coordinate| <= 2^23, every product < 2^48), so the mask is a
// function of the inputs alone.  The output is a union of 1 bytes: racing identical stores, no ordering, the same bits every time.
// The one atomic (a wave's slice of the large-triangle list) orders list entries, which no output bit depends on.
// The two entries are one host function (raster<Job>) and one set of kernels: project_kernel<DEPTH>, a fill kernel each (they write
// different types) and nb_raster.h's small_kernel / large_kernel with the entry's triangle job, SilJob or RangeJob.
#include "nb_march_common.h"
#include "nb_raster.h"

namespace {

// a pixel is the closed square centre -+ HALF; |u|, |w| beyond MAX_PIXEL: the view does not cull
using nbraster::HALF, nbraster::MAX_PIXEL, nbraster::SUB;
constexpr float MIN_DEPTH = 0.01f;            // metres in front of the camera
constexpr int HDR_COUNT = 0, HDR_FLAGS = 4;   // scratch header, int32: large-triangle count | pad | flag of every (frame, view)

struct Scratch {
    int *hdr;     // [HDR_FLAGS + F * nv]
    int2 *snap;   // [F * nv, V] snapped pixel coordinates
    int *large;   // [F * nv * Nf] (frame, view, triangle) ids of the triangles one thread does not walk
    float *depth; // [F * nv, V] camera depths (nb_body_depth_range alone)
    long long hdr_bytes, total_bytes;
};

// 0 total_bytes: dimensions the entry refuses
Scratch carve(void *base, long long F, long long V, long long Nf, long long nv, bool with_depth = false) {
    Scratch s = {};
    if (F < 1 || V < 1 || Nf < 1 || nv < 1 || nv > NB_MAX_CULL_VIEWS || F > 65535) return s;
    const long long fv = F * nv;
    // a whole workgroup past the last id must still fit an int: the grids index vertices and triangles with int
    if (fv * V > 2147483647ll - 256 || fv * Nf > 2147483647ll - 256) return s;
    s.hdr_bytes = nb_align256(4 * (HDR_FLAGS + fv));
    const long long snap_bytes = nb_align256(8 * fv * V), large_bytes = nb_align256(4 * fv * Nf);
    char *p = (char *)base;
    s.hdr = (int *)p;
    s.snap = (int2 *)(p + s.hdr_bytes);
    s.large = (int *)(p + s.hdr_bytes + snap_bytes);
    s.depth = (float *)(p + s.hdr_bytes + snap_bytes + large_bytes);
    s.total_bytes = s.hdr_bytes + snap_bytes + large_bytes + (with_depth ? nb_align256(4 * fv * V) : 0);
    return s;
}

// Vertex v of frame f through the camera `view`: the cull's projection, the snap to 1 / SUB pixel and the camera depth (R v + T).z.
// false: the view does not cull (a vertex nearer than MIN_DEPTH, a projection beyond MAX_PIXEL, NaN); s is then (0, 0)
__device__ __forceinline__ bool project_snap(const float *__restrict__ verts, const float *__restrict__ cam, int V, int f, int view, int v,
                                             int2 &s, float &depth) {
    const float *__restrict__ pv = verts + ((size_t)f * V + v) * 3;
    const float p[3] = {pv[0], pv[1], pv[2]};
    float t[3], q[3];
    nbm::cull_project((nbm::cfloat_ptr)(cam + view * 21), p, t, q);
    const float u = __fdiv_rn(q[0], q[2]), w = __fdiv_rn(q[1], q[2]);
    // written so that a NaN anywhere lands on the safe side
    const bool ok = t[2] >= MIN_DEPTH && fabsf(u) <= MAX_PIXEL && fabsf(w) <= MAX_PIXEL;
    s = {0, 0};
    if (ok) {
        s.x = (int)rintf((float)SUB * u);  // |256 u| <= 2^23: exact in fp32, half to even
        s.y = (int)rintf((float)SUB * w);
    }
    depth = t[2];
    return ok;
}

// One workgroup = 256 vertices of one (frame, view): the camera is wave-uniform.  DEPTH: the vertex's camera depth is kept beside its
// snapped coordinates (without it `depth` is not touched).
template <bool DEPTH>
__global__ __launch_bounds__(256) void project_kernel(const float *__restrict__ verts, const float *__restrict__ cam, int V, int nv,
                                                      int chunks, int2 *__restrict__ snap, float *__restrict__ depth,
                                                      int *__restrict__ flags) {
    const int fv = blockIdx.x / chunks, v = (blockIdx.x % chunks) * 256 + threadIdx.x;
    if (v >= V) return;
    int2 s;
    float z;
    if (!project_snap(verts, cam, V, fv / nv, fv % nv, v, s, z)) flags[fv] = 1;  // racing stores of the same value
    snap[(size_t)fv * V + v] = s;
    if (DEPTH) depth[(size_t)fv * V + v] = z;
}

// range = (+inf, -inf) where the rasteriser will draw, (-inf, +inf) where the view does not bound.  A pixel per thread.
__global__ __launch_bounds__(256) void range_fill_kernel(const int *__restrict__ flags, long long HW, long long n, float2 *__restrict__ range) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    range[p] = flags[p / HW] ? make_float2(-INFINITY, INFINITY) : make_float2(INFINITY, -INFINITY);
}

// out = the flag of its (frame, view): 0 where the rasteriser will draw, 1 where the view does not cull.  16 bytes per thread.
__global__ __launch_bounds__(256) void sil_fill_kernel(const int *__restrict__ flags, long long HW, long long n, int aligned,
                                                       unsigned char *__restrict__ out) {
    const long long b = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (b >= n) return;
    const long long e = min(b + 16, n);
    const long long i0 = b / HW, i1 = (e - 1) / HW;
    if (aligned && e - b == 16 && i0 == i1) {
        const unsigned w = flags[i0] ? 0x01010101u : 0u;
        *reinterpret_cast<uint4 *>(out + b) = make_uint4(w, w, w, w);
        return;
    }
    for (long long k = b; k < e; ++k) out[k] = flags[k / HW] ? 1 : 0;
}

// A triangle of one (frame, view), set up from the snapped vertices: oriented to positive area, its bounding box in pixels
// clipped to the image, the three edge functions.  Pixel (x, y) is covered iff for every edge
//   E_i(256 x, 256 y) + 128 (|dx_i| + |dy_i|) >= 0,
// the largest value E_i takes on the closed square: the separating-axis test of square against triangle (the box is the other
// two axes).
struct Tri : nbraster::Box {
    long long dx[3], dy[3], c[3];  // E_i(X, Y) = dx_i Y - dy_i X + c_i, the slack already in c_i
    __device__ __forceinline__ bool covers(int x, int y) const {
        const long long X = (long long)x * SUB, Y = (long long)y * SUB;
        return (dx[0] * Y - dy[0] * X + c[0] >= 0) & (dx[1] * Y - dy[1] * X + c[1] >= 0) & (dx[2] * Y - dy[2] * X + c[2] >= 0);
    }
};

// false: nothing to draw (a flagged view, an index outside the vertices, zero area, a box off the image)
__device__ __forceinline__ bool tri_setup(int g, int Nf, int V, int H, int W, const int *__restrict__ faces,
                                          const int2 *__restrict__ snap, const int *__restrict__ flags, Tri &T, int &fv) {
    fv = g / Nf;
    const int tri = g - fv * Nf;
    if (flags[fv]) return false;
    const int ia = faces[3 * (size_t)tri], ib = faces[3 * (size_t)tri + 1], ic = faces[3 * (size_t)tri + 2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return false;
    const int2 *__restrict__ sv = snap + (size_t)fv * V;
    const int2 a = sv[ia];
    int2 b = sv[ib], c = sv[ic];
    const long long area = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
    if (area == 0) return false;
    if (area < 0) nbraster::swap(b, c);
    // the squares 256 x -+ 128 that meet the triangle's extent
    if (!T.clip(a.x, a.y, b.x, b.y, c.x, c.y, +HALF, H, W)) return false;
    const int2 P[3] = {a, b, c}, Q[3] = {b, c, a};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T.dx[i] = (long long)Q[i].x - P[i].x;
        T.dy[i] = (long long)Q[i].y - P[i].y;
        const long long adx = T.dx[i] < 0 ? -T.dx[i] : T.dx[i], ady = T.dy[i] < 0 ? -T.dy[i] : T.dy[i];
        T.c[i] = T.dy[i] * P[i].x - T.dx[i] * P[i].y + HALF * (adx + ady);
    }
    return true;
}

// The triangle job of nb_raster.h: triangle g of the (frame, view, triangle) ids, a 1 byte wherever its pixel's square meets it.
struct SilJob : Tri {
    static constexpr bool DEPTH = false;
    const int *faces, *flags;
    const int2 *snap;
    int Nf, V, H, W;
    unsigned char *out;
    int fv;  // the triangle's (frame, view), set by setup like the Tri
    __device__ __forceinline__ bool setup(int g) { return tri_setup(g, Nf, V, H, W, faces, snap, flags, *this, fv); }
    __device__ __forceinline__ void pixel(int x, int y) { if (covers(x, y)) out[((size_t)fv * H + y) * W + x] = 1; }
};

// The triangle job of nb_raster.h: triangle g of the (frame, view, triangle) ids, its vertex-depth interval folded into every pixel
// whose square meets it.  Depths are >= MIN_DEPTH, so their fp32 bits order like signed integers, and so do the bits of the two
// infinities the fill left: integer atomic min / max, the result free of the order of arrival.
struct RangeJob : Tri {
    static constexpr bool DEPTH = true;
    const int *faces, *flags;
    const int2 *snap;
    const float *depth;
    int Nf, V, H, W;
    int *out;     // the [F,nv,H,W,2] fp32 range as its bits
    int fv;       // the triangle's (frame, view), set by setup like the Tri
    int zlo, zhi; // bits of the smallest and the largest of its three vertex depths
    __device__ __forceinline__ bool setup(int g) {
        if (!tri_setup(g, Nf, V, H, W, faces, snap, flags, *this, fv)) return false;
        const int tri = g - fv * Nf;  // its indices passed tri_setup's check
        const float *__restrict__ dv = depth + (size_t)fv * V;
        const float za = dv[faces[3 * (size_t)tri]], zb = dv[faces[3 * (size_t)tri + 1]], zc = dv[faces[3 * (size_t)tri + 2]];
        zlo = __float_as_int(fminf(za, fminf(zb, zc)));
        zhi = __float_as_int(fmaxf(za, fmaxf(zb, zc)));
        return true;
    }
    __device__ __forceinline__ void pixel(int x, int y) {
        if (!covers(x, y)) return;
        int *__restrict__ r = out + 2 * (((size_t)fv * H + y) * W + x);
        atomicMin(r, zlo);
        atomicMax(r + 1, zhi);
    }
};

// Both entries: `what` names the caller in every message, the Job says which rasteriser runs.  DEPTH: the vertex depths are kept and
// `out` is the fp32 range as its bits; the fills differ in what they write, and with it the grid-size refusal.
template <class Job>
int raster(const char *what, const float *verts, const int32_t *faces, const float *cam, int32_t F, int32_t V, int32_t Nf, int32_t nv,
           int32_t H, int32_t W, void *scratch, int64_t scratch_bytes, decltype(Job::out) out, void *stream) {
    constexpr bool DEPTH = Job::DEPTH;
    NB_REQUIRE(verts && faces && cam && scratch && out, "%s: NULL pointer", what);
    const Scratch s = carve(scratch, F, V, Nf, nv, DEPTH);
    NB_REQUIRE(s.total_bytes > 0, "%s: F = %d (1..65535), V = %d, Nf = %d (>= 1), nv = %d (1..%d), F nv V and F nv Nf below 2^31 - 256",
               what, F, V, Nf, nv, NB_MAX_CULL_VIEWS);
    NB_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: H = %d, W = %d (1..32768)", what, H, W);
    NB_REQUIRE(scratch_bytes >= s.total_bytes, "%s: scratch holds %lld bytes, %lld needed", what, (long long)scratch_bytes, s.total_bytes);
    NB_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", what);
    if constexpr (DEPTH) NB_REQUIRE(((uintptr_t)out & 7) == 0, "%s: range must be 8-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    const int fv = F * nv, chunks = nb_ceil_div(V, 256), n_tri = fv * Nf;
    const long long HW = (long long)H * W, n_px = HW * fv;
    if constexpr (DEPTH)
        NB_REQUIRE((n_px + 255) / 256 <= 2147483647ll, "%s: %lld pixels are too many", what, n_px);
    else
        NB_REQUIRE((n_px + 16 * 256 - 1) / (16 * 256) <= 2147483647ll, "%s: %lld output bytes are too many", what, n_px);
    char where[64];  // "<what> (<step>)", written only when a launch failed
    const auto at = [&](const char *step) { return snprintf(where, sizeof(where), "%s (%s)", what, step), where; };
    int *flags = s.hdr + HDR_FLAGS, *count = s.hdr + HDR_COUNT;
    NB_HIP(hipMemsetAsync(s.hdr, 0, (size_t)s.hdr_bytes, st));  // the count and every flag
    hipLaunchKernelGGL(project_kernel<DEPTH>, dim3(fv * chunks), dim3(256), 0, st, verts, cam, V, nv, chunks, s.snap,
                       DEPTH ? s.depth : nullptr, flags);
    NB_CHECK_LAUNCH(at("project"));
    Job job = {};
    job.faces = faces, job.flags = flags, job.snap = s.snap, job.Nf = Nf, job.V = V, job.H = H, job.W = W;
    if constexpr (DEPTH) {
        job.depth = s.depth;
        hipLaunchKernelGGL(range_fill_kernel, dim3(nb_ceil_div(n_px, 256)), dim3(256), 0, st, flags, HW, n_px, (float2 *)out);
    } else {
        hipLaunchKernelGGL(sil_fill_kernel, dim3(nb_ceil_div(n_px, 16 * 256)), dim3(256), 0, st, flags, HW, n_px,
                           ((uintptr_t)out & 15) == 0 ? 1 : 0, out);
    }
    NB_CHECK_LAUNCH(at("fill"));
    hipLaunchKernelGGL(nbraster::small_kernel<Job>, dim3(nb_ceil_div(n_tri, 256)), dim3(256), 0, st, job, out, n_tri, count, s.large);
    NB_CHECK_LAUNCH(at("triangles"));
    hipLaunchKernelGGL(nbraster::large_kernel<Job>, dim3(nbraster::LARGE_BLOCKS), dim3(256), 0, st, job, out, n_tri, count, s.large);
    NB_CHECK_LAUNCH(at("large triangles"));
    return NB_OK;
}

}  // namespace

extern "C" int64_t nb_smpl_silhouette_scratch_size(int32_t F, int32_t V, int32_t Nf, int32_t nv) {
    return carve(nullptr, F, V, Nf, nv).total_bytes;
}

extern "C" int nb_smpl_silhouette(const float *verts, const int32_t *faces, const float *cam, int32_t F, int32_t V, int32_t Nf,
                                  int32_t nv, int32_t H, int32_t W, void *scratch, int64_t scratch_bytes, uint8_t *out,
                                  void *stream) {
    return raster<SilJob>("nb_smpl_silhouette", verts, faces, cam, F, V, Nf, nv, H, W, scratch, scratch_bytes, out, stream);
}

extern "C" int64_t nb_body_depth_range_scratch_size(int32_t F, int32_t V, int32_t Nf, int32_t nv) {
    return carve(nullptr, F, V, Nf, nv, true).total_bytes;
}

extern "C" int nb_body_depth_range(const float *verts, const int32_t *faces, const float *cam, int32_t F, int32_t V, int32_t Nf,
                                   int32_t nv, int32_t H, int32_t W, void *scratch, int64_t scratch_bytes, float *range, void *stream) {
    return raster<RangeJob>("nb_body_depth_range", verts, faces, cam, F, V, Nf, nv, H, W, scratch, scratch_bytes, (int *)range, stream);
}
