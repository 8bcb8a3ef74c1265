// nb_lattice.hip — the mesh pass's query lattice on the device: mask dilation, silhouette carving, the list of carved points and
// the scatter of their densities into the padded cube.
//
// Restates (zju3dv/neuralbody):
//   lib/datasets/light_stage/multi_view_mesh_dataset.py:111-113  get_mask: cv2.dilate(msk, ones((5, 5)))       (nb_mask_dilate)
//   lib/datasets/light_stage/multi_view_mesh_dataset.py:117-140  prepare_inside_pts                            (nb_lattice_carve)
//   lib/datasets/light_stage/multi_view_mesh_dataset.py:151-158  the 'ij' meshgrid of the three axes, never materialised
//   lib/networks/renderer/if_mesh_renderer.py:30-31,42-46        pts[inside], cube[inside] = alpha, np.pad(cube, 10)
//                                                                                       (nb_lattice_gather, nb_lattice_scatter)
// A lattice is three axis vectors; point (i, j, k) = (ax[i], ay[j], az[k]) has the linear index (i*Y + j)*Z + k.  The projection
// and mask test is the march's cull_inside (nb_march_common.h), not a second copy; the two numberings are sequences of the one
// count-and-place tile body (nb_scan_dev.h).  No atomics: the same inputs give the same bits.
#include "nb_march_common.h"
#include "nb_scan_dev.h"
#include "nb_window.h"

namespace {

struct Lattice {
    const float *__restrict__ ax, *__restrict__ ay, *__restrict__ az;
    unsigned Y, Z;
    // linear index (< 2^31) -> (i, j, k)
    __device__ __forceinline__ void index(unsigned lin, unsigned &i, unsigned &j, unsigned &k) const {
        const unsigned t = lin / Z;
        k = lin - t * Z;
        i = t / Y;
        j = t - i * Y;
    }
};

// count pass of nb_lattice_carve: the flag of point i, stored as it is counted
struct CarveSeq {
    Lattice lat;
    nbm::CullDev cull;  // pre = 0
    unsigned char *__restrict__ inside;
    __device__ __forceinline__ int value(long long i) const {
        unsigned a, b, c;
        lat.index((unsigned)i, a, b, c);
        nbm::CullDev cd = cull;
        cd.pre = 0;  // known here, so that cull_inside's pose branch (the only reader of the scene) is compiled away
        const nbm::SceneDev no_scene = {};
        const int f = nbm::cull_inside(cd, no_scene, lat.ax[a], lat.ay[b], lat.az[c]) ? 1 : 0;
        inside[i] = (unsigned char)f;
        return f;
    }
};

// place pass of nb_lattice_carve: nothing to place, the total lands in n_inside
struct FlagTotalSeq {
    const unsigned char *__restrict__ inside;
    int *__restrict__ n_inside;
    __device__ __forceinline__ int value(long long i) const { return inside[i]; }
    __device__ __forceinline__ void place(long long, int, int) const {}
    __device__ __forceinline__ void total(int t) const { *n_inside = t; }
};

// the flagged points in linear order, under the capacity
struct GatherSeq {
    Lattice lat;
    const unsigned char *__restrict__ inside;
    float *__restrict__ wpts;
    int *__restrict__ lin, *__restrict__ n_out;
    int cap;
    __device__ __forceinline__ int value(long long i) const { return inside[i] != 0; }
    __device__ __forceinline__ void place(long long i, int flagged, int r) const {
        if (!flagged || r >= cap) return;
        unsigned a, b, c;
        lat.index((unsigned)i, a, b, c);
        wpts[(size_t)r * 3 + 0] = lat.ax[a];
        wpts[(size_t)r * 3 + 1] = lat.ay[b];
        wpts[(size_t)r * 3 + 2] = lat.az[c];
        lin[r] = (int)i;
    }
    __device__ __forceinline__ void total(int t) const {
        n_out[0] = min(t, cap);
        n_out[1] = t;
    }
};

// the fold of nb_window.h for nb_mask_dilate: out = max of the window's bytes
struct MaxFold {
    unsigned m = 0;
    __device__ __forceinline__ void take(unsigned b) { m = max(m, b); }
    __device__ __forceinline__ unsigned result(unsigned) const { return m; }
};

__global__ __launch_bounds__(256) void lattice_scatter_kernel(const float *__restrict__ alpha, long long stride,
                                                              const int *__restrict__ lin, long long n, Lattice lat, unsigned n_pts,
                                                              int pad, float *__restrict__ cube) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned l = (unsigned)lin[r];
    if (l >= n_pts) return;  // not a lattice point (a negative entry included): nothing to write
    unsigned i, j, k;
    lat.index(l, i, j, k);
    const long long Yp = (long long)lat.Y + 2 * pad, Zp = (long long)lat.Z + 2 * pad;
    cube[((long long)(i + pad) * Yp + (j + pad)) * Zp + (k + pad)] = alpha[r * stride];
}

// dims of a lattice the calls accept -> its point count, 0 otherwise
long long lattice_points(const int32_t dims[3]) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return 0;
    const long long xy = (long long)dims[0] * dims[1];  // < 2^62; the third factor only once this one is small
    if (xy > 2147483647ll || xy * dims[2] > 2147483647ll) return 0;
    return xy * dims[2];
}

}  // namespace

extern "C" int nb_mask_dilate(const uint8_t *msk, int32_t n_views, int32_t H, int32_t W, int32_t border, uint8_t *out,
                              void *stream) {
    return nbwindow::launch<MaxFold>("nb_mask_dilate", "msk", msk, n_views, H, W, border, out, stream);
}

extern "C" int nb_lattice_carve(const float *ax, const float *ay, const float *az, const int32_t dims[3], const nb_cull *cull,
                                uint8_t *inside, int32_t *n_inside, void *scratch, void *stream) {
    NB_REQUIRE(ax && ay && az && inside && n_inside && scratch, "nb_lattice_carve: NULL pointer");
    const long long n = lattice_points(dims);
    NB_REQUIRE(n >= 1, "nb_lattice_carve: dims must be >= 1 with at most 2^31 - 1 points");
    NB_REQUIRE(cull != nullptr, "nb_lattice_carve: cull is NULL");
    NB_REQUIRE(cull->pre_affine == 0, "nb_lattice_carve: pre_affine = %d (the lattice is carved in world space)", cull->pre_affine);
    CarveSeq carve;
    if (int rc = nbm::fill_cull(cull, &carve.cull)) return rc;
    carve.lat = {ax, ay, az, (unsigned)dims[1], (unsigned)dims[2]};
    carve.inside = inside;
    const FlagTotalSeq flags = {inside, n_inside};
    int *tile_sums;
    nb_scan_carve(scratch, n, nullptr, nullptr, &tile_sums);
    return nbscan::count_and_place("nb_lattice_carve", carve, flags, n, tile_sums, (hipStream_t)stream);
}

extern "C" int nb_lattice_gather(const float *ax, const float *ay, const float *az, const int32_t dims[3], const uint8_t *inside,
                                 int32_t cap, float *wpts, int32_t *lin, int32_t *n_out, void *scratch, void *stream) {
    NB_REQUIRE(ax && ay && az && inside && n_out && scratch, "nb_lattice_gather: NULL pointer");
    const long long n = lattice_points(dims);
    NB_REQUIRE(n >= 1, "nb_lattice_gather: dims must be >= 1 with at most 2^31 - 1 points");
    NB_REQUIRE(cap >= 0 && (cap == 0 || (wpts && lin)), "nb_lattice_gather: cap = %d, or NULL output with cap > 0", cap);
    const GatherSeq seq = {{ax, ay, az, (unsigned)dims[1], (unsigned)dims[2]}, inside, wpts, lin, n_out, cap};
    int *tile_sums;
    nb_scan_carve(scratch, n, nullptr, nullptr, &tile_sums);
    return nbscan::count_and_place("nb_lattice_gather", seq, seq, n, tile_sums, (hipStream_t)stream);
}

extern "C" int nb_lattice_scatter(const float *alpha, int64_t alpha_stride, const int32_t *lin, int64_t n, const int32_t dims[3],
                                  int32_t pad, float *cube, void *stream) {
    const long long n_pts = lattice_points(dims);
    NB_REQUIRE(n_pts >= 1, "nb_lattice_scatter: dims must be >= 1 with at most 2^31 - 1 points");
    NB_REQUIRE(n >= 0 && n <= n_pts && alpha_stride >= 1 && pad >= 0 && pad <= 1024,
               "nb_lattice_scatter: n = %lld (0..%lld), alpha_stride = %lld (>= 1), pad = %d (0..1024)", (long long)n, n_pts,
               (long long)alpha_stride, pad);
    if (n == 0) return NB_OK;
    NB_REQUIRE(alpha && lin && cube, "nb_lattice_scatter: NULL pointer");
    const Lattice lat = {nullptr, nullptr, nullptr, (unsigned)dims[1], (unsigned)dims[2]};
    hipLaunchKernelGGL(lattice_scatter_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, alpha,
                       (long long)alpha_stride, lin, (long long)n, lat, (unsigned)n_pts, pad, cube);
    NB_CHECK_LAUNCH("nb_lattice_scatter");
    return NB_OK;
}
