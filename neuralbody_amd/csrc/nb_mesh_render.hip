// nb_mesh_render.hip — nb_mesh_vertex_normals, nb_mesh_render: the normal-shaded orthographic pictures of an indexed mesh, z-buffered
// on the device, for the turntable a headless node cannot ask an OpenGL context for.
//
// Stands where (zju3dv/neuralbody):
//   tools/render_mesh.py:21-51      normalize_v3, compute_normal: unit face normals summed unweighted per vertex, normalised
//   tools/render_mesh.py:120-170    the 91-view loop: set_mesh(vertices, faces, 0.5 * normals + 0.5), display, get_color
//   tools/render/camera.py:160-190  get_gl_matrix with ortho_ratio set; tools/render/glm.py:114-123 ortho
//   tools/render/color.vs, color.fs the vertex colour interpolated over the triangle; GL_LESS depth test, no culling, ms_rate 1
// Every output is a function of the inputs alone (include/nb_hip.h has the definition).  Normals: the face normals are quantised
// to integers before they are summed, and integer atomics do not care about arrival order.  Pictures: vertices are snapped to
// 1/256 pixel and coverage is integer (int64 edge functions at the pixel centre); each covered centre offers one 64-bit key
// (depth in order-preserving bits << 32 | triangle) to atomicMin, whose result does not depend on the order of the offers either.
//
// The `_rn` device intrinsics of this toolchain are the plain operators, which hipcc contracts into FMAs across inlined calls
// (__fadd_rn(__fmul_rn(a, b), c) assembles to v_fmac_f32), and __fsqrt_rn is the 1-ulp v_sqrt_f32.  So contraction is switched off
// for this file and every rounded operation below is an operator between two named values (sqrtf and `/` are correctly rounded
// under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt): the kernels and tests/mesh_render_ref.py round at the same places.
#include <float.h>
#include <math.h>

#include "nb_common.h"
#include "nb_raster.h"

#pragma clang fp contract(off)

namespace {

// pixel (i, j) is sampled at (256 i + 128, 256 j + 128); a triangle with a vertex beyond MAX_PIXEL is skipped
using nbraster::HALF, nbraster::MAX_PIXEL, nbraster::SUB;
constexpr int CAM_FLOATS = 24;            // affine 3 x 4 | normal rotation 3 x 3 | 3 of padding
constexpr float QUANT = 1048576.0f;       // 2^20: a unit face normal's component as an integer
constexpr float NORM_EPS = 1e-8f;         // render_mesh.py:24
constexpr unsigned long long EMPTY = ~0ull;

__device__ __forceinline__ float mul(float a, float b) { return a * b; }
__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ float sub(float a, float b) { return a - b; }
__device__ __forceinline__ float quo(float a, float b) { return a / b; }
__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return add(add(mul(a0, b0), mul(a1, b1)), mul(a2, b2));
}
__device__ __forceinline__ float length3(float x, float y, float z) { return fmaxf(sqrtf(dot3(x, y, z, x, y, z)), NORM_EPS); }

// ----------------------------------------------------------------------------------------------------------- vertex normals
// One thread per face.  |component| <= 2^20 + 1 after the rounded divide, so a vertex of valence up to 2047 cannot overflow
// its int32 sums: 2047 (2^20 + 1) < 2^31.
__global__ __launch_bounds__(256) void normals_face_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V, int T,
                                                           int *__restrict__ acc) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int i[3] = {faces[3 * (size_t)t], faces[3 * (size_t)t + 1], faces[3 * (size_t)t + 2]};
    if ((unsigned)i[0] >= (unsigned)V || (unsigned)i[1] >= (unsigned)V || (unsigned)i[2] >= (unsigned)V) return;
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[k][c] = verts[3 * (size_t)i[k] + c];
    const float ux = sub(p[1][0], p[0][0]), uy = sub(p[1][1], p[0][1]), uz = sub(p[1][2], p[0][2]);
    const float wx = sub(p[2][0], p[0][0]), wy = sub(p[2][1], p[0][1]), wz = sub(p[2][2], p[0][2]);
    const float nx = sub(mul(uy, wz), mul(uz, wy)), ny = sub(mul(uz, wx), mul(ux, wz)), nz = sub(mul(ux, wy), mul(uy, wx));
    const float len = length3(nx, ny, nz);
    const float q[3] = {mul(quo(nx, len), QUANT), mul(quo(ny, len), QUANT), mul(quo(nz, len), QUANT)};
    // a face with a non-finite vertex adds nothing (written so that a NaN lands on the safe side)
    if (!(fabsf(q[0]) <= 2.0f * QUANT && fabsf(q[1]) <= 2.0f * QUANT && fabsf(q[2]) <= 2.0f * QUANT)) return;
    const int n[3] = {(int)rintf(q[0]), (int)rintf(q[1]), (int)rintf(q[2])};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (n[c]) atomicAdd(acc + 3 * (size_t)i[k] + c, n[c]);
}

// One thread per vertex: the integer sums back in units of one, normalised with the reference's clamp.
__global__ __launch_bounds__(256) void normals_vertex_kernel(const int *__restrict__ acc, int V, float *__restrict__ normals) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float s = 1.0f / QUANT;  // a power of two: the products are exact
    const float x = mul((float)acc[3 * (size_t)v], s), y = mul((float)acc[3 * (size_t)v + 1], s), z = mul((float)acc[3 * (size_t)v + 2], s);
    const float len = length3(x, y, z);
    normals[3 * (size_t)v] = quo(x, len), normals[3 * (size_t)v + 1] = quo(y, len), normals[3 * (size_t)v + 2] = quo(z, len);
}

// ----------------------------------------------------------------------------------------------------------- pictures
constexpr int HDR_BYTES = 256;  // scratch header: int32 large-triangle count

struct Scratch {
    int *hdr;
    unsigned long long *keys;  // [n_views, H, W]
    int *large;                // [n_views * T] (view, triangle) ids of the triangles one thread does not walk
    long long keys_bytes, total_bytes;
};

// 0 total_bytes: dimensions the entry refuses
Scratch carve(void *base, long long nv, long long H, long long W, long long T) {
    Scratch s = {};
    if (nv < 1 || H < 1 || W < 1 || T < 0 || H > 32768 || W > 32768) return s;
    // a whole workgroup past the last id must still fit an int: the grids index pixels and (view, triangle) pairs with int
    if (nv * H * W > 2147483647ll - 256 || nv * T > 2147483647ll - 256) return s;
    s.keys_bytes = nb_align256(8 * nv * H * W);
    char *p = (char *)base;
    s.hdr = (int *)p;
    s.keys = (unsigned long long *)(p + HDR_BYTES);
    s.large = (int *)(p + HDR_BYTES + s.keys_bytes);
    s.total_bytes = HDR_BYTES + s.keys_bytes + nb_align256(4 * nv * T);
    return s;
}

// float bits whose unsigned order is the floats' order (-0 below +0)
__device__ __forceinline__ unsigned ordered_bits(float d) {
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A triangle of one view: its vertices through the view's affine, snapped, oriented to positive area; the attributes follow the
// orientation.  The raster kernels and the resolve kernel both call this and so get the same bits.
struct Tri : nbraster::Box {    // the box: the pixel centres inside the bounding box, clipped to the image
    int idx[3];                 // vertex indices in oriented order
    int px[3], py[3];           // snapped coordinates
    float d[3];                 // depths
    // the three edge functions at pixel (x, y)'s centre: e[i] belongs to the edge opposite vertex i, all >= 0 inside
    __device__ __forceinline__ void edges(int x, int y, long long e[3]) const {
        const long long X = (long long)x * SUB + HALF, Y = (long long)y * SUB + HALF;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int p = (i + 1) % 3, q = (i + 2) % 3;
            e[i] = (long long)(px[q] - px[p]) * (Y - py[p]) - (long long)(py[q] - py[p]) * (X - px[p]);
        }
    }
    // a_0 + l_1 (a_1 - a_0) + l_2 (a_2 - a_0)
    static __device__ __forceinline__ float mix(float a0, float a1, float a2, float l1, float l2) {
        return add(add(a0, mul(l1, sub(a1, a0))), mul(l2, sub(a2, a0)));
    }
};

// false: nothing to draw (an index outside the vertices, a non-finite or far-off vertex, zero area, no pixel centre in the box)
__device__ __forceinline__ bool tri_setup(int tri, const int *__restrict__ faces, const float *__restrict__ verts, int V,
                                          const float *__restrict__ cam, int H, int W, Tri &t) {
    t.idx[0] = faces[3 * (size_t)tri], t.idx[1] = faces[3 * (size_t)tri + 1], t.idx[2] = faces[3 * (size_t)tri + 2];
    if ((unsigned)t.idx[0] >= (unsigned)V || (unsigned)t.idx[1] >= (unsigned)V || (unsigned)t.idx[2] >= (unsigned)V) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *__restrict__ v = verts + 3 * (size_t)t.idx[k];
        const float vx = v[0], vy = v[1], vz = v[2];
        float r[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = add(dot3(cam[4 * i], cam[4 * i + 1], cam[4 * i + 2], vx, vy, vz), cam[4 * i + 3]);
        // written so that a NaN lands on the safe side
        if (!(fabsf(r[0]) <= MAX_PIXEL && fabsf(r[1]) <= MAX_PIXEL && fabsf(r[2]) <= FLT_MAX)) return false;
        t.px[k] = (int)rintf(mul((float)SUB, r[0]));  // |256 x| <= 2^23: exact in fp32, half to even
        t.py[k] = (int)rintf(mul((float)SUB, r[1]));
        t.d[k] = r[2];
    }
    const long long area = (long long)(t.px[1] - t.px[0]) * (t.py[2] - t.py[0]) - (long long)(t.py[1] - t.py[0]) * (t.px[2] - t.px[0]);
    if (area == 0) return false;
    if (area < 0)
        nbraster::swap(t.idx[1], t.idx[2]), nbraster::swap(t.px[1], t.px[2]), nbraster::swap(t.py[1], t.py[2]), nbraster::swap(t.d[1], t.d[2]);
    // the centres 256 i + 128 inside the triangle's extent
    return t.clip(t.px[0], t.py[0], t.px[1], t.py[1], t.px[2], t.py[2], -HALF, H, W);
}

// The sample of triangle t at pixel (x, y): false when the centre is not covered or the depth there is not finite.
__device__ __forceinline__ bool sample(const Tri &t, int x, int y, float &l1, float &l2, float &d) {
    long long e[3];
    t.edges(x, y, e);
    if ((e[0] < 0) | (e[1] < 0) | (e[2] < 0)) return false;
    const float sum = (float)(e[0] + e[1] + e[2]);  // int64 -> fp32, to nearest
    l1 = quo((float)e[1], sum), l2 = quo((float)e[2], sum);
    d = Tri::mix(t.d[0], t.d[1], t.d[2], l1, l2);
    return fabsf(d) <= FLT_MAX;
}

__device__ __forceinline__ void offer(const Tri &t, int tri, int x, int y, unsigned long long *__restrict__ row) {
    float l1, l2, d;
    if (!sample(t, x, y, l1, l2, d)) return;
    const unsigned long long key = ((unsigned long long)ordered_bits(d) << 32) | (unsigned)tri;
    if (key < row[x]) atomicMin(row + x, key);  // the read is a hint (keys only fall): the atomic alone decides
}

// The triangle job of nb_raster.h: triangle g of the (view, triangle) ids, a key offered wherever it covers a pixel's centre.
struct RasterJob : Tri {
    const float *verts, *cams;
    const int *faces;
    int T, V, H, W;
    unsigned long long *out, *img;  // out: the keys [n_views, H, W]; img, tri: the triangle's view and index, set by setup like the Tri
    int tri;
    __device__ __forceinline__ bool setup(int g) {
        const int view = g / T;
        tri = g - view * T, img = out + (size_t)view * H * W;
        return tri_setup(tri, faces, verts, V, cams + (size_t)view * CAM_FLOATS, H, W, *this);
    }
    __device__ __forceinline__ void pixel(int x, int y) { offer(*this, tri, x, y, img + (size_t)y * W); }
};

// One thread per pixel: the winner's sample again, by the functions that made the key, then its colour.  ATTR: `normals` holds the
// vertex colours themselves (nb_mesh_render_attr) instead of the normals they are computed from.
template <bool ATTR>
__global__ __launch_bounds__(256) void resolve_kernel(const float *__restrict__ verts, const float *__restrict__ normals,
                                                      const int *__restrict__ faces, const float *__restrict__ cams, int n_px, int T,
                                                      int V, int H, int W, const unsigned long long *__restrict__ keys,
                                                      float *__restrict__ rgb, int *__restrict__ face_id, float *__restrict__ depth) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_px) return;
    const int HW = H * W, view = g / HW, p = g - view * HW, y = p / W, x = p - y * W;
    const float *__restrict__ cam = cams + (size_t)view * CAM_FLOATS;
    const unsigned long long key = keys[g];
    const int tri = (int)(unsigned)(key & 0xffffffffull);
    float c[3] = {1.0f, 1.0f, 1.0f}, d = INFINITY, l1, l2;
    int id = -1;
    Tri t;
    if (key != EMPTY && (unsigned)tri < (unsigned)T && tri_setup(tri, faces, verts, V, cam, H, W, t) && x >= t.x0 && x <= t.x1 &&
        y >= t.y0 && y <= t.y1 && sample(t, x, y, l1, l2, d)) {
        id = tri;
        float col[3][3];  // [vertex][channel]: 0.5 n' + 0.5, n' the normal through the view's rotation; or the attribute as it is
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *__restrict__ nv = normals + 3 * (size_t)t.idx[k];
            const float nx = nv[0], ny = nv[1], nz = nv[2];
            if (ATTR) {
                col[k][0] = nx, col[k][1] = ny, col[k][2] = nz;
                continue;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
                col[k][i] = add(mul(0.5f, dot3(cam[12 + 3 * i], cam[12 + 3 * i + 1], cam[12 + 3 * i + 2], nx, ny, nz)), 0.5f);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = Tri::mix(col[0][i], col[1][i], col[2][i], l1, l2);
    } else {
        d = INFINITY;
    }
    rgb[3 * (size_t)g] = c[0], rgb[3 * (size_t)g + 1] = c[1], rgb[3 * (size_t)g + 2] = c[2];
    if (face_id) face_id[g] = id;
    if (depth) depth[g] = d;
}

}  // namespace

extern "C" int nb_mesh_vertex_normals(const float *verts, const int32_t *faces, int32_t V, int32_t T, int32_t *acc, float *normals,
                                      void *stream) {
    NB_REQUIRE(V >= 0 && T >= 0 && V <= (2147483647 - 256) / 3 && T <= 2147483647 - 256,
               "nb_mesh_vertex_normals: V = %d (0..%d), T = %d (0..2^31 - 257)", V, (2147483647 - 256) / 3, T);
    NB_REQUIRE(V == 0 || (verts && acc && normals), "nb_mesh_vertex_normals: NULL pointer");
    NB_REQUIRE(T == 0 || faces, "nb_mesh_vertex_normals: NULL faces");
    if (V == 0) return NB_OK;
    hipStream_t st = (hipStream_t)stream;
    NB_HIP(hipMemsetAsync(acc, 0, 12 * (size_t)V, st));
    if (T > 0) {
        hipLaunchKernelGGL(normals_face_kernel, dim3(nb_ceil_div(T, 256)), dim3(256), 0, st, verts, faces, V, T, acc);
        NB_CHECK_LAUNCH("nb_mesh_vertex_normals (faces)");
    }
    hipLaunchKernelGGL(normals_vertex_kernel, dim3(nb_ceil_div(V, 256)), dim3(256), 0, st, acc, V, normals);
    NB_CHECK_LAUNCH("nb_mesh_vertex_normals (vertices)");
    return NB_OK;
}

extern "C" int64_t nb_mesh_render_scratch_size(int32_t n_views, int32_t H, int32_t W, int32_t T) {
    return carve(nullptr, n_views, H, W, T).total_bytes;
}

namespace {

// both entries: `what` names the caller in the refusals, ATTR says what `normals` holds (resolve_kernel)
template <bool ATTR>
int render(const char *what, const float *verts, const float *normals, const int32_t *faces, int32_t V, int32_t T, const float *cams,
           int32_t n_views, int32_t H, int32_t W, float *rgb, int32_t *face_id, float *depth, void *scratch, int64_t scratch_bytes,
           void *stream) {
    NB_REQUIRE(cams && rgb && scratch, "%s: NULL pointer", what);
    NB_REQUIRE(V >= 0 && T >= 0 && (T == 0 || (verts && normals && faces)), "%s: V = %d, T = %d with a NULL mesh pointer", what,
               V, T);
    const Scratch s = carve(scratch, n_views, H, W, T);
    NB_REQUIRE(s.total_bytes > 0,
               "%s: n_views = %d (>= 1), H = %d, W = %d (1..32768), T = %d (>= 0), n_views H W and n_views T below 2^31 - 256", what,
               n_views, H, W, T);
    NB_REQUIRE(scratch_bytes >= s.total_bytes, "%s: scratch holds %lld bytes, %lld needed", what, (long long)scratch_bytes,
               s.total_bytes);
    NB_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    const int n_tri = n_views * T, n_px = n_views * H * W;
    NB_HIP(hipMemsetAsync(s.hdr, 0, HDR_BYTES, st));                       // the large-triangle count
    NB_HIP(hipMemsetAsync(s.keys, 0xFF, 8 * (size_t)n_px, st));            // every key: nothing drawn
    if (n_tri > 0) {
        const RasterJob job = {{}, verts, cams, faces, T, V, H, W};
        hipLaunchKernelGGL(nbraster::small_kernel<RasterJob>, dim3(nb_ceil_div(n_tri, 256)), dim3(256), 0, st, job, s.keys, n_tri, s.hdr,
                           s.large);
        NB_CHECK_LAUNCH("nb_mesh_render (triangles)");
        hipLaunchKernelGGL(nbraster::large_kernel<RasterJob>, dim3(nbraster::LARGE_BLOCKS), dim3(256), 0, st, job, s.keys, n_tri, s.hdr,
                           s.large);
        NB_CHECK_LAUNCH("nb_mesh_render (large triangles)");
    }
    hipLaunchKernelGGL(resolve_kernel<ATTR>, dim3(nb_ceil_div(n_px, 256)), dim3(256), 0, st, verts, normals, faces, cams, n_px, T, V, H, W,
                       s.keys, rgb, face_id, depth);
    NB_CHECK_LAUNCH("nb_mesh_render (resolve)");
    return NB_OK;
}

}  // namespace

extern "C" int nb_mesh_render(const float *verts, const float *normals, const int32_t *faces, int32_t V, int32_t T, const float *cams,
                              int32_t n_views, int32_t H, int32_t W, float *rgb, int32_t *face_id, float *depth, void *scratch,
                              int64_t scratch_bytes, void *stream) {
    return render<false>("nb_mesh_render", verts, normals, faces, V, T, cams, n_views, H, W, rgb, face_id, depth, scratch, scratch_bytes,
                         stream);
}

extern "C" int nb_mesh_render_attr(const float *verts, const float *attr, const int32_t *faces, int32_t V, int32_t T, const float *cams,
                                   int32_t n_views, int32_t H, int32_t W, float *rgb, int32_t *face_id, float *depth, void *scratch,
                                   int64_t scratch_bytes, void *stream) {
    return render<true>("nb_mesh_render_attr", verts, attr, faces, V, T, cams, n_views, H, W, rgb, face_id, depth, scratch, scratch_bytes,
                        stream);
}
