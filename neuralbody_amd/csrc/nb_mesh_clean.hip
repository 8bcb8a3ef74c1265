// nb_mesh_clean.hip — what stands between marching cubes and the mesh a user wants, on the device: connected components of an
// indexed triangle list, the choice of the components to keep, the order-preserving compaction of vertices, faces and one per-vertex
// attribute, and the two small kernels around the colour head that give every vertex a colour.
//
// Stands where the reference has nothing (zju3dv/neuralbody writes every stray blob of lib/networks/renderer/if_mesh_renderer.py:46-52
// into the .ply, in grey; its users clean the file by hand): the host equivalent is a download, scipy.sparse.csgraph
// .connected_components, numpy fancy indexing and an upload.
//
// Rules of every kernel here (include/nb_hip.h states them for the caller): no allocation, no synchronisation, integer atomics only
// and only where the result does not depend on arrival order, every loop counted, no thread ever waits for another; a loop that
// hits its limit raises the give-up word of the scratch header and the thread leaves.
//
// Components: union-find in global memory under the invariant parent[v] <= v.  A root is hooked under a smaller root with atomicMin,
// so whatever the order of the hooks, a set's root ends as its smallest vertex: the labels are unique although the execution is not.
// A stale read of parent[] is harmless: every value parent[v] ever held is a vertex of v's set and <= v, and the atomicMin that
// decides returns what the word really holds.
#include "nb_scan_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int HDR_BYTES = 256, HDR_WORDS = HDR_BYTES / 4;
constexpr int ROUNDS = NB_MESH_HOOK_ROUNDS;
// header words
constexpr int H_STATUS = 0;    // the give-up word: 0, or 1 when the labels could not be finished (the outputs then stay unwritten)
constexpr int H_ROUND = 1;     // [ROUNDS] give-up of hook round r; round r + 1 runs iff word r is set
constexpr int H_FLAT = 12;     // give-up of the flatten pass
constexpr int H_TOTALS = 16;   // kept vertices, kept faces (the two scans' totals)
constexpr int H_BEST = 32;     // 64-bit, 8-byte aligned: (faces << 32) | ~label of the largest component
static_assert(H_ROUND + ROUNDS <= H_FLAT && (H_BEST * 4) % 8 == 0 && H_BEST + 2 <= HDR_WORDS, "header layout");

constexpr int HOOK_STEPS = 1 << 14;   // parent reads and hook attempts one face may spend per round
constexpr int FLAT_STEPS = 1 << 20;   // parent reads one vertex may spend on its way to the root

struct Scratch {
    int *hdr, *parent, *count, *vpos, *fpos, *sums_v, *sums_f;
    long long bytes;
};

// bytes = 0: sizes the entries refuse
Scratch carve(void *base, long long V, long long T) {
    Scratch s = {};
    if (V < 0 || T < 0 || V > 2147483647ll - 256 || T > 2147483647ll - 256) return s;
    const long long v = nb_align256(4 * V), t = nb_align256(4 * T);
    const long long bv = nb_align256(4 * nb_scan_blocks(V)), bt = nb_align256(4 * nb_scan_blocks(T));
    s.bytes = HDR_BYTES + 3 * v + t + bv + bt;
    char *p = (char *)base;
    s.hdr = (int *)p;
    s.parent = (int *)(p + HDR_BYTES);
    s.count = (int *)(p + HDR_BYTES + v);
    s.vpos = (int *)(p + HDR_BYTES + 2 * v);
    s.fpos = (int *)(p + HDR_BYTES + 3 * v);
    s.sums_v = (int *)(p + HDR_BYTES + 3 * v + t);
    s.sums_f = (int *)(p + HDR_BYTES + 3 * v + t + bv);
    return s;
}

// the face's three indices; false: one lies outside 0..V-1 (the rule of nb_mesh_vertex_normals)
__device__ __forceinline__ bool face_of(const int *__restrict__ faces, int t, int V, int i[3]) {
    i[0] = faces[3 * (size_t)t], i[1] = faces[3 * (size_t)t + 1], i[2] = faces[3 * (size_t)t + 2];
    return (unsigned)i[0] < (unsigned)V && (unsigned)i[1] < (unsigned)V && (unsigned)i[2] < (unsigned)V;
}

// ----------------------------------------------------------------------------------------------------------- components
__device__ __forceinline__ int load_parent(const int *parent, int v) { return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above v, halving the path on the way (parent[v] = min(parent[v], grandparent): still an ancestor, still <= v).
// Counted: every parent read costs one of `steps`; false when they ran out.
__device__ __forceinline__ bool find_root(int *parent, int &v, int &steps) {
    int p = load_parent(parent, v);
    while (p != v) {
        if (--steps < 0) return false;
        const int g = load_parent(parent, p);
        if (g != p) atomicMin(parent + v, g);
        v = p, p = g;
    }
    return true;
}

// the sets of a and b made one; false: out of steps (the pass is idempotent: a later round takes the pair up again)
__device__ __forceinline__ bool unite(int *parent, int a, int b, int &steps) {
    while (true) {
        if (!find_root(parent, a, steps) || !find_root(parent, b, steps)) return false;
        if (a == b) return true;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return true;  // hi was a root and now hangs under lo
        // hi had been hooked meanwhile, under old < hi, and now hangs under min(old, lo); the other of the two has to join it.
        // max(old, lo) < hi: the larger of the pair strictly decreases
        a = old, b = lo;
        if (--steps < 0) return false;
    }
}

__global__ __launch_bounds__(BLOCK) void init_kernel(int *__restrict__ parent, int V, int *__restrict__ hdr) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < V) parent[v] = v;
    if (blockIdx.x == 0 && threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = 0;
}

// One thread per face.  Round 0 always runs; round r > 0 runs iff a thread of round r - 1 gave up (block-uniform).
__global__ __launch_bounds__(BLOCK) void hook_kernel(const int *__restrict__ faces, int V, int T, int *parent, int *hdr, int round) {
    if (round > 0 && hdr[H_ROUND + round - 1] == 0) return;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    int i[3];
    if (t >= T || !face_of(faces, t, V, i)) return;
    int steps = HOOK_STEPS;
    if (!unite(parent, i[0], i[1], steps) || !unite(parent, i[0], i[2], steps)) atomicMax(hdr + H_ROUND + round, 1);
}

// One thread per vertex: parent[v] = root(v), in place (a walker that passes v meets the old parent or the root, both above it).
__global__ __launch_bounds__(BLOCK) void flatten_kernel(int *parent, int V, int *hdr) {
    if (hdr[H_ROUND + ROUNDS - 1] != 0) return;
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    int r = v, steps = FLAT_STEPS, p = load_parent(parent, r);
    while (p != r) {
        if (--steps < 0) {
            atomicMax(hdr + H_FLAT, 1);
            return;
        }
        r = p, p = load_parent(parent, r);
    }
    if (r != v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the labels leave the scratch only when they are finished; the give-up word says which
__global__ __launch_bounds__(BLOCK) void publish_kernel(const int *__restrict__ parent, int V, int *hdr, int *__restrict__ label) {
    const bool failed = hdr[H_ROUND + ROUNDS - 1] != 0 || hdr[H_FLAT] != 0;
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (!failed && v < V) label[v] = parent[v];
    // every block read the two words it decides by before any block can have written the status: they are other words
    if (v == 0) hdr[H_STATUS] = failed;
}

// ----------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(BLOCK) void face_count_kernel(const int *__restrict__ label, const int *__restrict__ faces, int V, int T,
                                                           const int *__restrict__ hdr, int *__restrict__ count) {
    if (hdr[H_STATUS] != 0) return;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    int i[3];
    if (t >= T || !face_of(faces, t, V, i)) return;
    const int l = label[i[0]];
    if ((unsigned)l < (unsigned)V) atomicAdd(count + l, 1);
}

__device__ __forceinline__ bool is_root_with_faces(const int *__restrict__ label, const int *__restrict__ count, int v) {
    return label[v] == v && count[v] > 0;
}

__global__ __launch_bounds__(BLOCK) void best_kernel(const int *__restrict__ label, const int *__restrict__ count, int V, int *hdr,
                                                     int *stats) {
    if (hdr[H_STATUS] != 0) return;
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V || !is_root_with_faces(label, count, v)) return;
    // the largest count; among equal counts the largest ~label, the smallest label
    atomicMax((unsigned long long *)(hdr + H_BEST), ((unsigned long long)(unsigned)count[v] << 32) | (unsigned)~v);
    atomicAdd(stats + 0, 1);
}

__global__ __launch_bounds__(BLOCK) void keep_kernel(const int *__restrict__ label, const int *__restrict__ count, int V, float min_fraction,
                                                     const int *__restrict__ hdr, unsigned char *__restrict__ keep, int *stats) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (hdr[H_STATUS] != 0) {
        if (v < 4) stats[v] = NB_EINTERNAL;
        return;
    }
    if (v >= V) return;
    const unsigned long long best = *(const unsigned long long *)(hdr + H_BEST);
    const int largest = (int)(best >> 32), winner = (int)~(unsigned)(best & 0xffffffffull);
    const int l = label[v];
    const int n = (unsigned)l < (unsigned)V ? count[l] : 0;
    bool k;
    if (min_fraction >= 1.0f) {
        k = n > 0 && l == winner;
    } else {
        const int need = max((int)ceil((double)min_fraction * (double)largest), 1);  // fp64: the product of an fp32 and an int32 is exact
        k = n >= need;
    }
    keep[v] = k;
    if (l == v && n > 0) {  // once per component that has a face
        if (v == winner) stats[2] = largest;
        if (k) atomicAdd(stats + 1, 1), atomicAdd(stats + 3, n);
    }
}

// ----------------------------------------------------------------------------------------------------------- compact
struct VertSeq {
    const unsigned char *__restrict__ keep;
    int *__restrict__ vpos, *__restrict__ total_out;
    __device__ __forceinline__ int value(long long i) const { return keep[i] != 0; }
    __device__ __forceinline__ void place(long long i, int kept, int prefix) const { vpos[i] = kept ? prefix : -1; }
    __device__ __forceinline__ void total(int t) const { *total_out = t; }
};

struct FaceSeq {
    const int *__restrict__ faces;
    const unsigned char *__restrict__ keep;
    int V;
    int *__restrict__ fpos, *__restrict__ total_out;
    __device__ __forceinline__ int value(long long t) const {
        int i[3];
        return face_of(faces, (int)t, V, i) && keep[i[0]] != 0;
    }
    __device__ __forceinline__ void place(long long t, int kept, int prefix) const { fpos[t] = kept ? prefix : -1; }
    __device__ __forceinline__ void total(int t) const { *total_out = t; }
};

__global__ void counts_kernel(const int *__restrict__ hdr, int *__restrict__ counts) {
    if (threadIdx.x < 2) counts[threadIdx.x] = hdr[H_STATUS] != 0 ? NB_EINTERNAL : hdr[H_TOTALS + threadIdx.x];
}

// false (block-uniform): the counts do not fit the buffers or the labels were never finished; nothing is written then
__device__ __forceinline__ bool may_emit(const int *__restrict__ hdr, int vert_cap, int tri_cap) {
    return hdr[H_STATUS] == 0 && hdr[H_TOTALS] <= vert_cap && hdr[H_TOTALS + 1] <= tri_cap;
}

__global__ __launch_bounds__(BLOCK) void emit_verts_kernel(const float *__restrict__ verts, const float *__restrict__ attr,
                                                           const int *__restrict__ vpos, int V, const int *__restrict__ hdr, int vert_cap,
                                                           int tri_cap, float *__restrict__ verts_out, float *__restrict__ attr_out) {
    if (!may_emit(hdr, vert_cap, tri_cap)) return;
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int o = vpos[v];
    if ((unsigned)o >= (unsigned)vert_cap) return;  // not kept
#pragma unroll
    for (int c = 0; c < 3; ++c) verts_out[3 * (size_t)o + c] = verts[3 * (size_t)v + c];
    if (attr)
#pragma unroll
        for (int c = 0; c < 3; ++c) attr_out[3 * (size_t)o + c] = attr[3 * (size_t)v + c];
}

__global__ __launch_bounds__(BLOCK) void emit_faces_kernel(const int *__restrict__ faces, const int *__restrict__ vpos,
                                                           const int *__restrict__ fpos, int V, int T, const int *__restrict__ hdr,
                                                           int vert_cap, int tri_cap, int *__restrict__ faces_out) {
    if (!may_emit(hdr, vert_cap, tri_cap)) return;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    const int o = fpos[t];
    int i[3];
    if ((unsigned)o >= (unsigned)tri_cap || !face_of(faces, t, V, i)) return;  // not kept
#pragma unroll
    for (int c = 0; c < 3; ++c) faces_out[3 * (size_t)o + c] = vpos[i[c]];
}

// ----------------------------------------------------------------------------------------------------------- colours
__global__ __launch_bounds__(BLOCK) void color_query_kernel(const float *__restrict__ verts_idx, const float *__restrict__ normals,
                                                            const float *__restrict__ step, const float *__restrict__ origin, float pad,
                                                            int V, float *__restrict__ wpts, float *__restrict__ viewdir) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    float n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float shifted = verts_idx[3 * (size_t)v + c] - pad;
        const float scaled = shifted * step[c];
        wpts[3 * (size_t)v + c] = scaled + origin[c];
        n[c] = normals[3 * (size_t)v + c];
    }
    const bool none = n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f;  // a vertex no face uses: look down -z
    viewdir[3 * (size_t)v] = none ? 0.0f : -n[0];
    viewdir[3 * (size_t)v + 1] = none ? 0.0f : -n[1];
    viewdir[3 * (size_t)v + 2] = none ? -1.0f : -n[2];
}

__global__ __launch_bounds__(BLOCK) void color_finish_kernel(const float *__restrict__ raw, int V, float *__restrict__ rgb_f,
                                                             unsigned char *__restrict__ rgb_u8) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = 1.f / (1.f + expf(-raw[4 * (size_t)v + c]));  // the sigmoid of nb_composite
        rgb_f[3 * (size_t)v + c] = s;
        const float b = rintf(255.0f * s);  // half to even
        rgb_u8[3 * (size_t)v + c] = (unsigned char)(b >= 0.0f ? (b <= 255.0f ? (int)b : 255) : 0);  // a NaN gives 0
    }
}

inline dim3 grid_of(int n) { return dim3((unsigned)nb_ceil_div(n > 0 ? n : 1, BLOCK)); }

}  // namespace

extern "C" int64_t nb_mesh_clean_scratch_size(int32_t V, int32_t T) { return carve(nullptr, V, T).bytes; }

#define NB_MESH_SCRATCH(what)                                                                                                     \
    const Scratch s = carve(scratch, V, T);                                                                                       \
    NB_REQUIRE(s.bytes > 0, what ": n_verts = %d, n_faces = %d (0..2^31 - 257)", V, T);                                            \
    NB_REQUIRE(scratch && ((uintptr_t)scratch & 15) == 0, what ": scratch is NULL or not 16-byte aligned");                       \
    hipStream_t st = (hipStream_t)stream

extern "C" int nb_mesh_components(const int32_t *faces, int32_t V, int32_t T, int32_t *label, void *scratch, void *stream) {
    NB_MESH_SCRATCH("nb_mesh_components");
    NB_REQUIRE((V == 0 || label) && (T == 0 || faces), "nb_mesh_components: NULL pointer");
    hipLaunchKernelGGL(init_kernel, grid_of(V), dim3(BLOCK), 0, st, s.parent, V, s.hdr);
    NB_CHECK_LAUNCH("nb_mesh_components (init)");
    if (V > 0 && T > 0) {
        for (int r = 0; r < ROUNDS; ++r) hipLaunchKernelGGL(hook_kernel, grid_of(T), dim3(BLOCK), 0, st, faces, V, T, s.parent, s.hdr, r);
        NB_CHECK_LAUNCH("nb_mesh_components (hook)");
        hipLaunchKernelGGL(flatten_kernel, grid_of(V), dim3(BLOCK), 0, st, s.parent, V, s.hdr);
        NB_CHECK_LAUNCH("nb_mesh_components (flatten)");
    }
    hipLaunchKernelGGL(publish_kernel, grid_of(V), dim3(BLOCK), 0, st, s.parent, V, s.hdr, label);
    NB_CHECK_LAUNCH("nb_mesh_components (publish)");
    return NB_OK;
}

extern "C" int nb_mesh_component_select(const int32_t *label, const int32_t *faces, int32_t V, int32_t T, float min_fraction,
                                        uint8_t *keep_vertex, int32_t *stats, void *scratch, void *stream) {
    NB_MESH_SCRATCH("nb_mesh_component_select");
    NB_REQUIRE(min_fraction > 0.0f && min_fraction <= 1.0f, "nb_mesh_component_select: min_fraction = %g, not in (0, 1]", (double)min_fraction);
    NB_REQUIRE(stats && (V == 0 || (label && keep_vertex)) && (T == 0 || faces), "nb_mesh_component_select: NULL pointer");
    NB_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int), st));
    NB_HIP(hipMemsetAsync(s.hdr + H_BEST, 0, 8, st));
    if (V > 0) NB_HIP(hipMemsetAsync(s.count, 0, 4 * (size_t)V, st));
    if (V > 0 && T > 0) {
        hipLaunchKernelGGL(face_count_kernel, grid_of(T), dim3(BLOCK), 0, st, label, faces, V, T, s.hdr, s.count);
        hipLaunchKernelGGL(best_kernel, grid_of(V), dim3(BLOCK), 0, st, label, s.count, V, s.hdr, stats);
        NB_CHECK_LAUNCH("nb_mesh_component_select (count)");
    }
    hipLaunchKernelGGL(keep_kernel, grid_of(V), dim3(BLOCK), 0, st, label, s.count, V, min_fraction, s.hdr, keep_vertex, stats);
    NB_CHECK_LAUNCH("nb_mesh_component_select (keep)");
    return NB_OK;
}

extern "C" int nb_mesh_compact_count(const int32_t *faces, const uint8_t *keep_vertex, int32_t V, int32_t T, int32_t *counts,
                                     void *scratch, void *stream) {
    NB_MESH_SCRATCH("nb_mesh_compact_count");
    NB_REQUIRE(counts && (V == 0 || keep_vertex) && (T == 0 || faces), "nb_mesh_compact_count: NULL pointer");
    NB_HIP(hipMemsetAsync(s.hdr + H_TOTALS, 0, 2 * sizeof(int), st));
    if (V > 0) {
        const VertSeq vs = {keep_vertex, s.vpos, s.hdr + H_TOTALS};
        if (int rc = nbscan::count_and_place("nb_mesh_compact_count (vertices)", vs, vs, V, s.sums_v, st)) return rc;
    }
    if (V > 0 && T > 0) {
        const FaceSeq fs = {faces, keep_vertex, V, s.fpos, s.hdr + H_TOTALS + 1};
        if (int rc = nbscan::count_and_place("nb_mesh_compact_count (faces)", fs, fs, T, s.sums_f, st)) return rc;
    }
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, st, s.hdr, counts);
    NB_CHECK_LAUNCH("nb_mesh_compact_count");
    return NB_OK;
}

extern "C" int nb_mesh_compact(const float *verts, const int32_t *faces, const float *attr, int32_t V, int32_t T, float *verts_out,
                               int32_t *faces_out, float *attr_out, int32_t vert_cap, int32_t tri_cap, void *scratch, void *stream) {
    NB_MESH_SCRATCH("nb_mesh_compact");
    NB_REQUIRE(vert_cap >= 0 && tri_cap >= 0 && (V == 0 || verts) && (T == 0 || faces), "nb_mesh_compact: NULL pointer or negative capacity");
    NB_REQUIRE((verts_out || vert_cap == 0) && (faces_out || tri_cap == 0), "nb_mesh_compact: NULL output with capacity");
    NB_REQUIRE(!attr == !attr_out || vert_cap == 0, "nb_mesh_compact: attr and attr_out go together");
    if (V > 0 && vert_cap > 0) {
        hipLaunchKernelGGL(emit_verts_kernel, grid_of(V), dim3(BLOCK), 0, st, verts, attr, s.vpos, V, s.hdr, vert_cap, tri_cap, verts_out,
                           attr_out);
        NB_CHECK_LAUNCH("nb_mesh_compact (vertices)");
    }
    if (V > 0 && T > 0 && tri_cap > 0) {
        hipLaunchKernelGGL(emit_faces_kernel, grid_of(T), dim3(BLOCK), 0, st, faces, s.vpos, s.fpos, V, T, s.hdr, vert_cap, tri_cap, faces_out);
        NB_CHECK_LAUNCH("nb_mesh_compact (faces)");
    }
    return NB_OK;
}

extern "C" int nb_mesh_color_query(const float *verts_idx, const float *normals, const float *step, const float *origin, float pad,
                                   int32_t V, float *wpts, float *viewdir, void *stream) {
    NB_REQUIRE(V >= 0 && V <= (2147483647 - 256) / 3, "nb_mesh_color_query: n_verts = %d (0..%d)", V, (2147483647 - 256) / 3);
    if (V == 0) return NB_OK;
    NB_REQUIRE(verts_idx && normals && step && origin && wpts && viewdir, "nb_mesh_color_query: NULL pointer");
    hipLaunchKernelGGL(color_query_kernel, grid_of(V), dim3(BLOCK), 0, (hipStream_t)stream, verts_idx, normals, step, origin, pad, V, wpts,
                       viewdir);
    NB_CHECK_LAUNCH("nb_mesh_color_query");
    return NB_OK;
}

extern "C" int nb_mesh_color_finish(const float *raw, int32_t V, float *rgb_f, uint8_t *rgb_u8, void *stream) {
    NB_REQUIRE(V >= 0 && V <= (2147483647 - 256) / 4, "nb_mesh_color_finish: n_verts = %d (0..%d)", V, (2147483647 - 256) / 4);
    if (V == 0) return NB_OK;
    NB_REQUIRE(raw && rgb_f && rgb_u8, "nb_mesh_color_finish: NULL pointer");
    hipLaunchKernelGGL(color_finish_kernel, grid_of(V), dim3(BLOCK), 0, (hipStream_t)stream, raw, V, rgb_f, rgb_u8);
    NB_CHECK_LAUNCH("nb_mesh_color_finish");
    return NB_OK;
}
