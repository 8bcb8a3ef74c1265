// nb_mesh_rig.hip — an extracted mesh bound to the SMPL body it clothes, so that nb_smpl_pose can repose it: the closest point of
// the posed body's surface for every mesh vertex (nb_mesh_closest), and there the transfer of the skinning weights and shape
// directions and the inverse skin to the rest pose (nb_mesh_rig_bind).
//
// Restates (zju3dv/neuralbody): lib/utils/blend_utils.py:73-82 ppts_to_pts (the inverse skin; the reference has it for the sample
// points of its T-pose variant and has no mesh counterpart).  The closest point is the region walk of C. Ericson, Real-Time Collision
// Detection, 5.1.5 (ClosestPtPointTriangle).
//
// "a (+) b" is ONE fp32 operation rounded to nearest.  As in nb_mesh_render.hip, hipcc contracts the plain operators into FMAs across
// inlined calls, so contraction is switched off for this file and every rounded operation is an operator between two named values;
// `/` and sqrtf are correctly rounded under hipcc's default.  dot(x, y) = (x0 (*) y0 (+) x1 (*) y1) (+) x2 (*) y2 everywhere.
//
// nb_mesh_closest, per point p and triangle (a, b, c) with ab = b (-) a, ac = c (-) a (made once per call, by the prepass):
//   ap = p (-) a, d1 = dot(ab, ap), d2 = dot(ac, ap);            d1 <= 0 and d2 <= 0                 -> (v, w) = (0, 0)      vertex a
//   bp = p (-) b, d3 = dot(ab, bp), d4 = dot(ac, bp);            d3 >= 0 and d4 <= d3                -> (1, 0)               vertex b
//   vc = d1 (*) d4 (-) d3 (*) d2;                                vc <= 0, d1 >= 0, d3 <= 0           -> (d1 (/) (d1 (-) d3), 0)    edge ab
//   cp = p (-) c, d5 = dot(ab, cp), d6 = dot(ac, cp);            d6 >= 0 and d5 <= d6                -> (0, 1)               vertex c
//   vb = d5 (*) d2 (-) d1 (*) d6;                                vb <= 0, d2 >= 0, d6 <= 0           -> (0, d2 (/) (d2 (-) d6))    edge ac
//   va = d3 (*) d6 (-) d5 (*) d4, e1 = d4 (-) d3, e2 = d5 (-) d6; va <= 0, e1 >= 0, e2 >= 0           -> w = e1 (/) (e1 (+) e2), v = 1 (-) w   edge bc
//   otherwise, with each of va, vb, vc replaced by 0 where it is < 0:  denom = 1 (/) ((va (+) vb) (+) vc), v = vb (*) denom, w = vc (*) denom.
// The tests are taken in this order (the book's) and the first that holds decides; a comparison with a NaN is false.  Then, for
// every region alike,  bary = ((1 (-) v) (-) w, v, w),  q = (a (+) ab (*) v) (+) ac (*) w  per coordinate,  dist2 = dot(p (-) q, p (-) q).
// The replacement by 0 in the interior is the one thing added to the book.  It changes nothing in exact arithmetic (there the
// interior is reached with all three positive) and it makes 0 <= v, w and v + w <= 1 + 2^-22 hold in EVERY region whatever the
// rounding did to the region tests, which the skip rule below leans on (0 (/) 0 and 0 (*) inf give a NaN: that face is skipped).
// The point's triangle is the one with the smallest finite dist2, the lower ORIGINAL face index on a tie: every candidate is
// compared as the pair (dist2, index), so the order the triangles are visited in does not matter.
//
// The prepass orders the faces whose indices are in range by the Morton code of a 16^3 lattice over their centroids (a counting
// sort: integer atomics count and place, so the order inside a cell varies from run to run — and, by the sentence above, nothing
// in the output does), cuts the order into tiles of 64 triangles and gives each tile a sphere (centre, R).  A wave of 64 points
// (marching cubes emits neighbours together) skips a tile when EVERY lane with a finite point finds
//       D = sqrtf(dot(p (-) centre, p (-) centre)) finite   and   D > (R (+) sqrtf(best)) (*) 1.002f,          best = the lane's current dist2.
// Why that is conservative in fp32: R = 1.002 r + 4e-6 S + 1e-15 with r the largest computed distance of a tile vertex from the
// centre and S the tile's largest |coordinate|.  By the bounds on v, w the exact a + ab v + ac w lies within (1 + 2^-21) r of the
// centre; the at most six roundings of ab, ac and q (each <= 2^-24 of a magnitude <= 3 S) move the computed q by less than
// 2^-20 S < 4e-6 S; computed distances carry a relative error below 2^-21.  So |q - centre| < R - 0.0019 r - 1e-15 exactly, and
// |p - q| >= |p - centre| - |q - centre| > 1.0019 (R + sqrt(best)) - R >= 1.0019 sqrt(best) + 1.9e-18.  The computed dist2 is at least
// (1 - 2^-21) |p - q|^2 (the 1e-15 keeps that square far above the subnormals, where the relative bound would end) > best: STRICTLY
// larger, so no triangle of a skipped tile could have replaced the lane's candidate, tie or not.  A tile with a non-finite vertex
// has R = +inf and is never skipped; best = +inf skips nothing.  The branch is wave-uniform (a ballot), the tile is staged in LDS by
// the wave's own lanes and read back at one address per instruction (a broadcast).  Before the sweep the wave visits the tile
// whose sphere is nearest to its first finite point, so that `best` is small from the start.  One thread per point where the
// points alone fill the device; for fewer points several waves share the tiles of the same 64 points (closest_kernel says how).
//
// nb_mesh_rig_bind, per mesh vertex x with the closest triangle (v0, v1, v2) of the body and bary (b0, b1, b2):
//   w_j = (b0 (*) W[j,v0] (+) b1 (*) W[j,v1]) (+) b2 (*) W[j,v2]                                         the rig's weight of joint j
//   T = [I|0] + sum_j w_j (A_j - [I|0]), j ascending, each term T (+) w_j (*) (.)                       smpl_vertex_kernel's blend, from ws
//   y_k = (rot[k] (*) (x_0 (-) Th_0) (+) rot[3+k] (*) (x_1 (-) Th_1)) (+) rot[6+k] (*) (x_2 (-) Th_2)       the inverse of rot . s + Th
//   v_shaped = M^-1 (y (-) t), M = T[:, :3], t = T[:, 3]; M^-1 = adj(M) (/) det(M) per element           blend_utils.py:79-81
//   S_l = the shape direction l interpolated with the expression of w_j;  v_template = v_shaped (-) sum_l S_l (*) beta_l, l ascending.
// !(|det M| >= 2^-10) (two joints turned against each other can blend to a singular M; a NaN lands here too): the vertex is bound
// rigidly to its largest-weight joint (the lowest j on a tie) — one-hot weights, T = A_j, determinant 1 by construction — and
// counted in status[1].  face = -1 (or any index outside the body): one-hot on joint 0, T = A_0, zero shape directions, counted in
// status[0].  Pose blend shapes are NOT transferred: a rig has posedirs = NULL and is driven with new_params = 0; a bind frame that
// was posed with new_params = 1 simply has its corrective offsets baked into v_template.
#include <float.h>

#include <algorithm>

#include "nb_common.h"
#include "nb_smpl_ws.h"

#pragma clang fp contract(off)

namespace {

constexpr int NJ = NB_SMPL_JOINTS, NBETA = NB_SMPL_BETAS;  // params row: poses 72 | shapes 10 | Rh 3 | Th 3
constexpr int TILE = 64;           // triangles per tile = lanes of the wave that stages it
constexpr int TRI_F4 = 4;          // float4 per triangle: a.xyz b.x | b.yz c.xy | c.z ab.xyz | ac.xyz index
constexpr int AXIS = 16, BINS = AXIS * AXIS * AXIS;
constexpr int HDR_INTS = 64;       // header of the scratch, int32
constexpr int H_LO = 0, H_HI = 3, H_NVALID = 6, H_COUNTERS = 8;  // counters: two uint64 at ints 8..11 (tiles skipped, tiles met)
constexpr float CULL_FACTOR = 1.002f, CULL_R = 1.002f, CULL_S = 4e-6f, CULL_FLOOR = 1e-15f;
constexpr long long MAX3 = 2147483648ll - 256;  // 3 P, 3 V, 3 Nf stay below it

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

// int whose signed order is the floats' order
__device__ __forceinline__ int ordered_int(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

struct Scratch {
    int *hdr, *bins, *order;
    float4 *spheres, *tris;
    long long bytes;
};

inline Scratch carve(void *base, int n_faces) {
    const long long n_tiles = ((long long)n_faces + TILE - 1) / TILE;
    char *p = (char *)base;
    Scratch s;
    s.hdr = (int *)p, p += nb_align256(HDR_INTS * 4);
    s.bins = (int *)p, p += nb_align256(BINS * 4);
    s.order = (int *)p, p += nb_align256((long long)n_faces * 4);
    s.spheres = (float4 *)p, p += nb_align256(n_tiles * 16);
    s.tris = (float4 *)p, p += nb_align256(n_tiles * TILE * TRI_F4 * 16);
    s.bytes = (long long)(p - (char *)base);
    return s;
}

__global__ __launch_bounds__(256) void closest_init_kernel(int *__restrict__ hdr, int *__restrict__ bins) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < BINS) bins[i] = 0;
    if (i < HDR_INTS) hdr[i] = i < H_HI ? 0x7fffffff : i < H_NVALID ? (int)0x80000000 : 0;
}

__device__ __forceinline__ bool face_in_range(const int *__restrict__ faces, int f, int V, int &i0, int &i1, int &i2) {
    i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    return (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
}

// the sum of the three corners stands for the centroid
__device__ __forceinline__ void corner_sum(const float *__restrict__ verts, int i0, int i1, int i2, float s[3]) {
    for (int k = 0; k < 3; ++k) s[k] = (verts[3 * (size_t)i0 + k] + verts[3 * (size_t)i1 + k]) + verts[3 * (size_t)i2 + k];
}

// box of the corner sums of the faces in range: integer atomics on order-preserving bits, min and max do not depend on the order
__global__ __launch_bounds__(256) void closest_box_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V, int Nf,
                                                          int *__restrict__ hdr) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int i0, i1, i2;
    if (f < Nf && face_in_range(faces, (int)f, V, i0, i1, i2)) {
        float s[3];
        corner_sum(verts, i0, i1, i2, s);
        for (int k = 0; k < 3; ++k)
            if (fabsf(s[k]) <= FLT_MAX) lo[k] = hi[k] = s[k];
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off, 64));
        }
    if (threadIdx.x % 64 == 0)
        for (int k = 0; k < 3; ++k) {
            if (lo[k] <= FLT_MAX) atomicMin(hdr + H_LO + k, ordered_int(lo[k]));
            if (hi[k] >= -FLT_MAX) atomicMax(hdr + H_HI + k, ordered_int(hi[k]));
        }
}

// Morton cell 0 .. BINS - 1 of a corner sum; anything that is not a number of the box lands in a cell all the same
__device__ __forceinline__ int cell_of(const float s[3], const int *__restrict__ hdr) {
    int key = 0;
    for (int k = 0; k < 3; ++k) {
        const float lo = ordered_float(hdr[H_LO + k]), hi = ordered_float(hdr[H_HI + k]);
        const float t = (s[k] - lo) * ((float)AXIS / (hi - lo));
        const int q = t >= (float)(AXIS - 1) ? AXIS - 1 : t >= 0.0f ? (int)t : 0;  // a NaN (an empty or flat box) -> 0
        for (int b = 0; b < 4; ++b) key |= ((q >> b) & 1) << (3 * b + k);
    }
    return key;
}

// place = 0: count the faces of every cell; place = 1: hand every face a slot of its cell (bins then hold the cells' cursors)
__global__ __launch_bounds__(256) void closest_bin_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V, int Nf,
                                                          const int *__restrict__ hdr, int *__restrict__ bins, int *__restrict__ order,
                                                          int place) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    int i0, i1, i2;
    if (f >= Nf || !face_in_range(faces, (int)f, V, i0, i1, i2)) return;
    float s[3];
    corner_sum(verts, i0, i1, i2, s);
    const int slot = atomicAdd(bins + cell_of(s, hdr), 1);
    if (place && (unsigned)slot < (unsigned)Nf) order[slot] = (int)f;  // the cells' counts sum to the faces in range <= Nf
}

// one workgroup: counts -> exclusive offsets (the cursors of the placement), their total -> hdr[H_NVALID]
__global__ __launch_bounds__(1024) void closest_offsets_kernel(int *__restrict__ bins, int *__restrict__ hdr) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    int c[BINS / 1024], sum = 0;
    for (int k = 0; k < BINS / 1024; ++k) c[k] = bins[t * (BINS / 1024) + k], sum += c[k];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int k = 0; k < BINS / 1024; ++k) bins[t * (BINS / 1024) + k] = run, run += c[k];
    if (t == 1023) hdr[H_NVALID] = part[t];
}

// one wave per tile: its triangles' a, b, c, ab, ac and original index, and its sphere
__global__ __launch_bounds__(64) void closest_tile_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int Nf,
                                                          const int *__restrict__ hdr, const int *__restrict__ order,
                                                          float4 *__restrict__ spheres, float4 *__restrict__ tris) {
    const int n_valid = min(hdr[H_NVALID], Nf);
    const long long k = (long long)blockIdx.x * TILE + threadIdx.x;
    if ((long long)blockIdx.x * TILE >= n_valid) return;
    const bool live = k < n_valid;
    float P[9];
    for (int e = 0; e < 9; ++e) P[e] = 0.0f;
    int f = -1;
    if (live) {
        f = order[k];
        for (int c = 0; c < 3; ++c) {
            const int i = faces[3 * (size_t)f + c];  // in range: only such faces were placed
            for (int e = 0; e < 3; ++e) P[3 * c + e] = verts[3 * (size_t)i + e];
        }
    }
    float4 *__restrict__ out = tris + (size_t)k * TRI_F4;
    out[0] = make_float4(P[0], P[1], P[2], P[3]);
    out[1] = make_float4(P[4], P[5], P[6], P[7]);
    out[2] = make_float4(P[8], P[3] - P[0], P[4] - P[1], P[5] - P[2]);
    out[3] = make_float4(P[6] - P[0], P[7] - P[1], P[8] - P[2], __int_as_float(f));
    // the sphere: centre of the corners' box, the largest computed distance from it, the largest |coordinate|
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, S = 0.0f;
    bool good = true;
    if (live)
        for (int c = 0; c < 3; ++c) {
            good = good && finite3(P[3 * c], P[3 * c + 1], P[3 * c + 2]);
            for (int e = 0; e < 3; ++e) {
                lo[e] = fminf(lo[e], P[3 * c + e]), hi[e] = fmaxf(hi[e], P[3 * c + e]);
                S = fmaxf(S, fabsf(P[3 * c + e]));
            }
        }
    for (int off = 32; off >= 1; off >>= 1) {
        for (int e = 0; e < 3; ++e) {
            lo[e] = fminf(lo[e], __shfl_xor(lo[e], off, 64));
            hi[e] = fmaxf(hi[e], __shfl_xor(hi[e], off, 64));
        }
        S = fmaxf(S, __shfl_xor(S, off, 64));
    }
    good = __all(good);
    float ctr[3], r = 0.0f;
    for (int e = 0; e < 3; ++e) ctr[e] = 0.5f * lo[e] + 0.5f * hi[e];
    if (live)
        for (int c = 0; c < 3; ++c) {
            const float dx = P[3 * c] - ctr[0], dy = P[3 * c + 1] - ctr[1], dz = P[3 * c + 2] - ctr[2];
            r = fmaxf(r, sqrtf(dot3(dx, dy, dz, dx, dy, dz)));
        }
    for (int off = 32; off >= 1; off >>= 1) r = fmaxf(r, __shfl_xor(r, off, 64));
    float R = (CULL_R * r + CULL_S * S) + CULL_FLOOR;
    if (!good || !finite3(ctr[0], ctr[1], ctr[2]) || !(R <= FLT_MAX)) R = INFINITY;
    if (threadIdx.x == 0) spheres[blockIdx.x] = make_float4(ctr[0], ctr[1], ctr[2], R);
}

// the region walk of the header: (v, w) of the closest point of one triangle
__device__ __forceinline__ void closest_vw(float px, float py, float pz, const float4 t0, const float4 t1, const float4 t2, const float4 t3,
                                           float &v, float &w) {
    const float ax = t0.x, ay = t0.y, az = t0.z, bx = t0.w, by = t1.x, bz = t1.y, cx = t1.z, cy = t1.w, cz = t2.x;
    const float abx = t2.y, aby = t2.z, abz = t2.w, acx = t3.x, acy = t3.y, acz = t3.z;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0f && d2 <= 0.0f) {
        v = 0.0f, w = 0.0f;
        return;
    }
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) {
        v = 1.0f, w = 0.0f;
        return;
    }
    const float m14 = d1 * d4, m32 = d3 * d2;
    float vc = m14 - m32;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float den = d1 - d3;
        v = d1 / den, w = 0.0f;
        return;
    }
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0f && d5 <= d6) {
        v = 0.0f, w = 1.0f;
        return;
    }
    const float m52 = d5 * d2, m16 = d1 * d6;
    float vb = m52 - m16;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float den = d2 - d6;
        v = 0.0f, w = d2 / den;
        return;
    }
    const float m36 = d3 * d6, m54 = d5 * d4;
    float va = m36 - m54;
    const float e1 = d4 - d3, e2 = d5 - d6;
    if (va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
        const float den = e1 + e2;
        w = e1 / den, v = 1.0f - w;
        return;
    }
    va = va < 0.0f ? 0.0f : va, vb = vb < 0.0f ? 0.0f : vb, vc = vc < 0.0f ? 0.0f : vc;
    const float sab = va + vb, sum = sab + vc;
    const float denom = 1.0f / sum;
    v = vb * denom, w = vc * denom;
}

constexpr int FLAG_EXHAUSTIVE = NB_CLOSEST_EXHAUSTIVE, FLAG_COUNT = NB_CLOSEST_COUNT_TILES;

// 64 points per workgroup, one lane per point in each of its waves.  With one wave (a large mesh: there are workgroups enough to
// fill the device) this is one thread per point.  A small mesh would leave most of the device idle, so its workgroups get up to
// MAX_WAVES waves: wave w of W sweeps the tiles w, w + W, ... for the same 64 points, every wave with its own LDS tile, `best`
// and skip decisions, and the W candidates of a point meet in LDS at the end under the same (dist2, index) order.  The waves
// run different numbers of tiles, so inside the sweep a wave orders its own LDS traffic (a fence; the wave runs in lockstep)
// and the workgroup's only barriers are the two of the final merge.
constexpr int MAX_WAVES = 16, TARGET_WAVES = 2048;

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(64 * MAX_WAVES) void closest_kernel(const float *__restrict__ points, int P, int Nf, int *__restrict__ hdr,
                                                                 const float4 *__restrict__ spheres, const float4 *__restrict__ tris,
                                                                 int flags, int *__restrict__ face, float *__restrict__ bary,
                                                                 float *__restrict__ dist2) {
    extern __shared__ float4 lds[];  // W tiles of TILE * TRI_F4 float4; the merge reuses the first W * 64
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, W = blockDim.x / 64;
    float4 *__restrict__ tl = lds + wave * (TILE * TRI_F4);
    const long long i = (long long)blockIdx.x * 64 + lane;
    float px = NAN, py = NAN, pz = NAN;
    if (i < P) px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    const bool ok = finite3(px, py, pz);
    const int n_valid = min(hdr[H_NVALID], Nf), n_tiles = (n_valid + TILE - 1) / TILE;
    const bool cull = !(flags & FLAG_EXHAUSTIVE);
    float best = INFINITY, root = INFINITY, bv = 0.0f, bw = 0.0f;
    int bidx = -1, skipped = 0, met = 0;

    int start = -1;  // the tile whose sphere is nearest to the first finite point: every wave visits it first
    const unsigned long long oks = __ballot(ok);
    if (cull && n_tiles > 1 && oks) {
        const int src = __ffsll((long long)oks) - 1;
        const float rx = __shfl(px, src, 64), ry = __shfl(py, src, 64), rz = __shfl(pz, src, 64);
        float gap = INFINITY;
        int gt = 0x7fffffff;
        for (int t = lane; t < n_tiles; t += 64) {
            const float4 s = spheres[t];
            const float dx = rx - s.x, dy = ry - s.y, dz = rz - s.z;
            const float g = sqrtf(dot3(dx, dy, dz, dx, dy, dz)) - s.w;
            if (g < gap) gap = g, gt = t;  // a NaN or +inf is never taken
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const float og = __shfl_xor(gap, off, 64);
            const int ot = __shfl_xor(gt, off, 64);
            if (og < gap || (og == gap && ot < gt)) gap = og, gt = ot;
        }
        if (gt != 0x7fffffff) start = gt;
    }

    for (int k = start >= 0 ? wave - W : wave; k < n_tiles; k += W) {  // k < 0: the start tile; everything here is wave-uniform
        if (k >= 0 && k == start) continue;
        const int t = k < 0 ? start : k;
        ++met;
        if (cull) {
            const float4 s = spheres[t];
            const float dx = px - s.x, dy = py - s.y, dz = pz - s.z;
            const float D = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
            const float reach = s.w + root;
            const bool far = D <= FLT_MAX && D > reach * CULL_FACTOR;
            if (!__any(ok && !far)) {
                ++skipped;
                continue;
            }
        }
        wave_lds_fence();  // the wave has finished with its tile before
        for (int e = 0; e < TRI_F4; ++e) tl[e * TILE + lane] = tris[(size_t)t * TILE * TRI_F4 + e * TILE + lane];
        wave_lds_fence();
        const int cnt = min(TILE, n_valid - t * TILE);
        for (int j = 0; j < cnt; ++j) {
            const float4 t0 = tl[TRI_F4 * j], t1 = tl[TRI_F4 * j + 1], t2 = tl[TRI_F4 * j + 2], t3 = tl[TRI_F4 * j + 3];
            float v, w;
            closest_vw(px, py, pz, t0, t1, t2, t3, v, w);
            const float abvx = t2.y * v, abvy = t2.z * v, abvz = t2.w * v, acwx = t3.x * w, acwy = t3.y * w, acwz = t3.z * w;
            const float hx = t0.x + abvx, hy = t0.y + abvy, hz = t0.z + abvz;
            const float qx = hx + acwx, qy = hy + acwy, qz = hz + acwz;
            const float ex = px - qx, ey = py - qy, ez = pz - qz;
            const float d = dot3(ex, ey, ez, ex, ey, ez);
            const int idx = __float_as_int(t3.w);
            if (d <= FLT_MAX && (d < best || (d == best && idx < bidx))) best = d, bidx = idx, bv = v, bw = w;
        }
        root = sqrtf(best);
    }
    if (W > 1) {  // uniform over the workgroup
        __syncthreads();
        lds[wave * 64 + lane] = make_float4(best, __int_as_float(bidx), bv, bw);
        __syncthreads();
        if (wave == 0)
            for (int o = 1; o < W; ++o) {
                const float4 c = lds[o * 64 + lane];
                const int idx = __float_as_int(c.y);
                if (idx >= 0 && (c.x < best || (c.x == best && idx < bidx))) best = c.x, bidx = idx, bv = c.z, bw = c.w;
            }
    }
    if (wave == 0 && i < P) {
        face[i] = bidx;
        const float u = 1.0f - bv;
        bary[3 * i] = bidx < 0 ? 0.0f : u - bw, bary[3 * i + 1] = bv, bary[3 * i + 2] = bw;
        dist2[i] = best;
    }
    if ((flags & FLAG_COUNT) && lane == 0) {  // bench only: integer sums, order-independent
        unsigned long long *__restrict__ c = (unsigned long long *)(hdr + H_COUNTERS);
        atomicAdd(c, (unsigned long long)skipped);
        atomicAdd(c + 1, (unsigned long long)met);
    }
}

// ------------------------------------------------------------------------------------------------------------------ bind
__global__ __launch_bounds__(64) void rig_bind_kernel(const float *__restrict__ params, const float *__restrict__ ws,
                                                      const float *__restrict__ W, const float *__restrict__ Sd,
                                                      const int *__restrict__ faces, int V, int Nf, const float *__restrict__ points,
                                                      const int *__restrict__ face, const float *__restrict__ bary, int P,
                                                      float *__restrict__ weights, float *__restrict__ shapedirs,
                                                      float *__restrict__ v_template, int *__restrict__ status) {
    __shared__ float wsl[WS_FLOATS];
    __shared__ float par[16];  // betas [10] | Th [3]
    const int t = threadIdx.x;
    for (int e = t; e < WS_FLOATS; e += 64) wsl[e] = ws[e];
    if (t < NBETA + 3) par[t] = params[t < NBETA ? 72 + t : 72 + 3 + t];  // Th follows Rh
    __syncthreads();
    const long long p = (long long)blockIdx.x * 64 + t;
    if (p >= P) return;
    const size_t n3v = 3 * (size_t)V, n3p = 3 * (size_t)P;
    const int f = face[p];
    int i0 = 0, i1 = 0, i2 = 0;
    const bool bound = (unsigned)f < (unsigned)Nf && face_in_range(faces, f, V, i0, i1, i2);
    const float b0 = bound ? bary[3 * p] : 0.0f, b1 = bound ? bary[3 * p + 1] : 0.0f, b2 = bound ? bary[3 * p + 2] : 0.0f;

    float w[NJ], T[12];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (bound) {
            const float m0 = b0 * W[(size_t)j * V + i0], m1 = b1 * W[(size_t)j * V + i1], m2 = b2 * W[(size_t)j * V + i2];
            w[j] = (m0 + m1) + m2;
        } else {
            w[j] = j == 0 ? 1.0f : 0.0f;
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const float m = w[j] * wsl[WS_A + 12 * j + e];
            T[e] = T[e] + m;
        }
    float M[9];
    auto matrix = [&]() {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[3 * r + c] = r == c ? 1.0f + T[4 * r + c] : T[4 * r + c];
    };
    matrix();
    // cofactors: C[3 r + c] = the cofactor of M[r][c]
    float Cf[9];
    auto cofactors = [&]() {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                const float x = M[3 * r1 + c1] * M[3 * r2 + c2], y = M[3 * r1 + c2] * M[3 * r2 + c1];
                Cf[3 * r + c] = x - y;
            }
    };
    cofactors();
    const float t0 = M[0] * Cf[0], t1 = M[1] * Cf[1], t2 = M[2] * Cf[2];
    float det = (t0 + t1) + t2;
    const bool degenerate = bound && !(fabsf(det) >= 0.0009765625f);
    if (!bound || degenerate) {
        int jm = 0;
        if (degenerate) {
            float wm = w[0];
#pragma unroll
            for (int j = 1; j < NJ; ++j)
                if (w[j] > wm) wm = w[j], jm = j;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) w[j] = j == jm ? 1.0f : 0.0f;
        for (int e = 0; e < 12; ++e) T[e] = wsl[WS_A + 12 * jm + e];
        matrix();
        cofactors();
        det = 1.0f;
        atomicAdd(status + (bound ? 1 : 0), 1);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) weights[(size_t)j * P + p] = w[j];

    const float *__restrict__ rot = wsl + WS_ROT;
    float dx[3], y[3], vs[3];
    for (int k = 0; k < 3; ++k) dx[k] = points[3 * p + k] - par[NBETA + k];
    for (int k = 0; k < 3; ++k) {
        const float m0 = rot[k] * dx[0], m1 = rot[3 + k] * dx[1], m2 = rot[6 + k] * dx[2];
        y[k] = ((m0 + m1) + m2) - T[4 * k + 3];
    }
    for (int r = 0; r < 3; ++r) {  // M^-1[r][c] = cofactor of M[c][r] over det
        const float n0 = Cf[r] / det, n1 = Cf[3 + r] / det, n2 = Cf[6 + r] / det;
        const float m0 = n0 * y[0], m1 = n1 * y[1], m2 = n2 * y[2];
        vs[r] = (m0 + m1) + m2;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < NBETA; ++l)
        for (int k = 0; k < 3; ++k) {
            float sd = 0.0f;
            if (bound) {
                const float m0 = b0 * Sd[l * n3v + 3 * (size_t)i0 + k], m1 = b1 * Sd[l * n3v + 3 * (size_t)i1 + k],
                            m2 = b2 * Sd[l * n3v + 3 * (size_t)i2 + k];
                sd = (m0 + m1) + m2;
            }
            shapedirs[l * n3p + 3 * p + k] = sd;
            const float m = sd * par[l];
            acc[k] = acc[k] + m;
        }
    for (int k = 0; k < 3; ++k) v_template[3 * p + k] = vs[k] - acc[k];
}

bool sizes_ok(long long P, long long V, long long Nf) { return P >= 1 && V >= 1 && Nf >= 1 && 3 * P < MAX3 && 3 * V < MAX3 && 3 * Nf < MAX3; }

}  // namespace

extern "C" int64_t nb_mesh_closest_scratch_size(int32_t n_verts, int32_t n_faces) {
    if (!sizes_ok(1, n_verts, n_faces)) return 0;
    return carve(nullptr, n_faces).bytes;
}

extern "C" int nb_mesh_closest(const float *points, const float *verts, const int32_t *faces, int32_t n_points, int32_t n_verts,
                               int32_t n_faces, int flags, void *scratch, int64_t scratch_bytes, int32_t *face, float *bary,
                               float *dist2, void *stream) {
    NB_REQUIRE(sizes_ok(n_points, n_verts, n_faces), "nb_mesh_closest: P = %d, V = %d, Nf = %d (each >= 1, 3 P, 3 V, 3 Nf < 2^31 - 256)",
               n_points, n_verts, n_faces);
    NB_REQUIRE(points && verts && faces && scratch && face && bary && dist2, "nb_mesh_closest: NULL pointer");
    NB_REQUIRE((flags & ~(FLAG_EXHAUSTIVE | FLAG_COUNT)) == 0, "nb_mesh_closest: flags = %d", flags);
    const Scratch s = carve(scratch, n_faces);
    NB_REQUIRE(scratch_bytes >= s.bytes, "nb_mesh_closest: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, s.bytes);
    NB_REQUIRE(((size_t)scratch & 15) == 0, "nb_mesh_closest: scratch is not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int fb = nb_ceil_div(n_faces, 256), n_tiles = nb_ceil_div(n_faces, TILE);
    hipLaunchKernelGGL(closest_init_kernel, dim3(BINS / 256), dim3(256), 0, st, s.hdr, s.bins);
    hipLaunchKernelGGL(closest_box_kernel, dim3(fb), dim3(256), 0, st, verts, faces, n_verts, n_faces, s.hdr);
    hipLaunchKernelGGL(closest_bin_kernel, dim3(fb), dim3(256), 0, st, verts, faces, n_verts, n_faces, s.hdr, s.bins, s.order, 0);
    hipLaunchKernelGGL(closest_offsets_kernel, dim3(1), dim3(1024), 0, st, s.bins, s.hdr);
    hipLaunchKernelGGL(closest_bin_kernel, dim3(fb), dim3(256), 0, st, verts, faces, n_verts, n_faces, s.hdr, s.bins, s.order, 1);
    hipLaunchKernelGGL(closest_tile_kernel, dim3(n_tiles), dim3(64), 0, st, verts, faces, n_faces, s.hdr, s.order, s.spheres, s.tris);
    NB_CHECK_LAUNCH("nb_mesh_closest (prepass)");
    const int blocks = nb_ceil_div(n_points, 64), waves = std::max(1, std::min({MAX_WAVES, TARGET_WAVES / blocks, n_tiles}));
    hipLaunchKernelGGL(closest_kernel, dim3(blocks), dim3(64 * waves), (size_t)waves * TILE * TRI_F4 * sizeof(float4), st, points,
                       n_points, n_faces, s.hdr, s.spheres, s.tris, flags, face, bary, dist2);
    NB_CHECK_LAUNCH("nb_mesh_closest");
    return NB_OK;
}

extern "C" int nb_mesh_rig_bind(const nb_smpl_model *model, const float *params, const float *ws, const int32_t *faces,
                                int32_t n_faces, const float *points, const int32_t *face, const float *bary, int32_t n_points,
                                float *weights, float *shapedirs, float *v_template, int32_t *status, void *stream) {
    NB_REQUIRE(model, "nb_mesh_rig_bind: NULL model");
    NB_REQUIRE(sizes_ok(n_points, model->n_verts, n_faces),
               "nb_mesh_rig_bind: P = %d, V = %d, Nf = %d (each >= 1, 3 P, 3 V, 3 Nf < 2^31 - 256)", n_points, model->n_verts, n_faces);
    NB_REQUIRE(params && ws && faces && points && face && bary && weights && shapedirs && v_template && status,
               "nb_mesh_rig_bind: NULL pointer");
    NB_REQUIRE(model->weights && model->shapedirs, "nb_mesh_rig_bind: a model array is NULL");
    hipStream_t st = (hipStream_t)stream;
    NB_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(rig_bind_kernel, dim3(nb_ceil_div(n_points, 64)), dim3(64), 0, st, params, ws, model->weights, model->shapedirs,
                       faces, model->n_verts, n_faces, points, face, bary, n_points, weights, shapedirs, v_template, status);
    NB_CHECK_LAUNCH("nb_mesh_rig_bind");
    return NB_OK;
}
