// nb_smpl.hip — a frame's geometry on the device: SMPL linear blend skinning from pose parameters, and the voxelisation of the
// posed vertices into the sparse encoder's input.
//
// Restates (zju3dv/neuralbody):
//   zju_smpl/smplmodel/body_model.py:89-153   SMPLlayer.forward, return_verts=True, scale=1            (nb_smpl_pose)
//   zju_smpl/smplmodel/lbs.py:142-233         lbs: shape blend, joints, pose blend, skinning           (nb_smpl_pose)
//   zju_smpl/smplmodel/lbs.py:280-311         batch_rodrigues                                          (rodrigues_f32)
//   zju_smpl/smplmodel/lbs.py:327-378         batch_rigid_transform                                    (smpl_prologue_kernel)
//   lib/datasets/light_stage/multi_view_dataset.py:68-118, monocular_dataset.py:32-71  prepare_input   (nb_smpl_voxelize)
// Plain fp32, wave64, no atomics, every sum in a fixed order: the same inputs give the same bits.  Products and sums that have to
// give the same bits in two places (the SMPL-space coordinates of nb_smpl_voxelize's two passes) are written with fmaf.
#include "nb_common.h"
#include "nb_smpl_ws.h"

namespace {

constexpr int NJ = NB_SMPL_JOINTS;         // 24
constexpr int NPF = NB_SMPL_POSE_BASIS;    // 207 = 23 * 9
constexpr int NB_BETAS = NB_SMPL_BETAS;    // 10
constexpr int PSTRIDE = NB_SMPL_PARAMS;    // 88 floats per frame: poses 72 | shapes 10 | Rh 3 | Th 3
// per-frame workspace: WS_A, WS_PF, WS_ROT, WS_FLOATS of nb_smpl_ws.h

// lbs.py:295-310 as written there: the angle is the norm of the SHIFTED vector, the direction the unshifted vector over it
__device__ __forceinline__ void rodrigues_f32(const float *__restrict__ r, float *__restrict__ R) {
    const float sx = r[0] + 1e-8f, sy = r[1] + 1e-8f, sz = r[2] + 1e-8f;
    const float angle = sqrtf(sx * sx + sy * sy + sz * sz);
    const float x = r[0] / angle, y = r[1] / angle, z = r[2] / angle;
    const float s = sinf(angle), c1 = 1.0f - cosf(angle);
    const float K[9] = {0.0f, -z, y, z, 0.0f, -x, -y, x, 0.0f};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const float kk = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = ((i == j ? 1.0f : 0.0f) + s * K[i * 3 + j]) + c1 * kk;
        }
}

struct Parents {
    int p[NJ];
};

// One wave per frame: 25 Rodrigues, the joints of the shaped body, the kinematic chain, the relative transforms.
//   G_j = G_parent . [R_j | J_j - J_parent]   (the reference's chain; its last column is the posed joint)
//   A_j = G_j . [I | -J_j]: rotation G_j.R, translation A_parent.t + G_parent.R . ((I - R_j) J_j) — the reference's
//   G_j.t - G_j.R J_j without the cancellation of two numbers the size of a joint (in the rest pose I - R_j is 0 and A_j.t is 0
//   exactly, where the subtraction leaves the rounding of the chain's sums).
// The skinning weights of a vertex sum to 1 (SmplModel refuses a model whose rows do not), so
//   T_v = sum_j W[v,j] A_j = [I | 0] + sum_j W[v,j] (A_j - [I | 0]):
// the vertex kernel blends the differences, which are 0 in the rest pose and small in a mild one, instead of letting the
// float32 sum of the weights (1 - 2^-23 .. 1 + 2^-23) scale the vertex.
__global__ __launch_bounds__(64) void smpl_prologue_kernel(const float *__restrict__ params, const float *__restrict__ j_template,
                                                           const float *__restrict__ j_shapedirs, Parents parents,
                                                           float *__restrict__ ws, float *__restrict__ joints) {
    __shared__ float R[(NJ + 1) * 9];  // joint rotations, then rot(Rh)
    __shared__ float J[NJ * 3];
    __shared__ float G[NJ * 12];       // rows of [R | t]
    __shared__ float At[NJ * 3];
    __shared__ int par[NJ];
    const int f = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) par[j] = parents.p[j];
    }
    const float *__restrict__ p = params + (size_t)f * PSTRIDE;
    float *__restrict__ w = ws + (size_t)f * WS_FLOATS;
    if (t < NJ) rodrigues_f32(p + 3 * t, R + 9 * t);
    if (t == NJ) rodrigues_f32(p + 72 + NB_BETAS, R + 9 * NJ);
    for (int e = t; e < NJ * 3; e += 64) {  // J = J_regressor . (v_template + shapedirs . beta), regressed once on the host
        float acc = 0.0f;
        for (int l = 0; l < NB_BETAS; ++l) acc += j_shapedirs[e * NB_BETAS + l] * p[72 + l];
        J[e] = j_template[e] + acc;
    }
    __syncthreads();
    for (int e = t; e < NPF; e += 64) w[WS_PF + e] = R[9 + e] - ((e % 9) % 4 == 0 ? 1.0f : 0.0f);
    if (t < 9) w[WS_ROT + t] = R[9 * NJ + t];
    // the chain: parents[j] < j, so joint j's parent is finished when its turn comes; lanes 0..11 hold one element of G_j each
    const int r = (t % 12) / 4, c = t % 4;
    for (int j = 0; j < NJ; ++j) {
        const int pa = par[j];
        if (t < 12) {
            float g;
            if (pa < 0) {
                g = c < 3 ? R[9 * j + 3 * r + c] : J[3 * j + r];
            } else {
                const float *__restrict__ Gp = G + 12 * pa + 4 * r;
                if (c < 3)
                    g = Gp[0] * R[9 * j + c] + Gp[1] * R[9 * j + 3 + c] + Gp[2] * R[9 * j + 6 + c];
                else
                    g = Gp[0] * (J[3 * j] - J[3 * pa]) + Gp[1] * (J[3 * j + 1] - J[3 * pa + 1]) + Gp[2] * (J[3 * j + 2] - J[3 * pa + 2]) +
                        Gp[3];
            }
            G[12 * j + 4 * r + c] = g;
        } else if (t < 15) {  // lanes 12..14: A_j.t, one row each
            const int i = t - 12;
            float d[3];  // (I - R_j) J_j
            for (int k = 0; k < 3; ++k) {
                const float *__restrict__ Rj = R + 9 * j + 3 * k;
                d[k] = -((Rj[0] - (k == 0 ? 1.0f : 0.0f)) * J[3 * j] + (Rj[1] - (k == 1 ? 1.0f : 0.0f)) * J[3 * j + 1] +
                         (Rj[2] - (k == 2 ? 1.0f : 0.0f)) * J[3 * j + 2]);
            }
            At[3 * j + i] = pa < 0 ? d[i] : At[3 * pa + i] + (G[12 * pa + 4 * i] * d[0] + G[12 * pa + 4 * i + 1] * d[1] + G[12 * pa + 4 * i + 2] * d[2]);
        }
        __syncthreads();
    }
    // stored as A_j - [I | 0]: the blend of the vertex kernel sums the transforms' differences from the identity
    for (int e = t; e < NJ * 12; e += 64)
        w[WS_A + e] = (e % 4) < 3 ? G[e] - ((e % 12) % 5 == 0 ? 1.0f : 0.0f) : At[3 * (e / 12) + (e % 12) / 4];
    if (joints)
        for (int e = t; e < NJ * 3; e += 64) joints[(size_t)f * NJ * 3 + e] = G[12 * (e / 3) + 4 * (e % 3) + 3];
}

// 64 vertices (192 consecutive coordinates) per workgroup of four waves.  With the pose blend, wave w sums the basis vectors
// [52 w, 52 w + 52) for the 192 coordinates: for one basis index the wave's lanes read consecutive floats of posedirs [207, 3V], and
// every element of posedirs is read by exactly one lane of the frame.  The four partial sums meet in a fixed order.
constexpr int VB = 64, EB = 3 * VB, PF_PER_WAVE = 52;
static_assert(4 * PF_PER_WAVE >= NPF, "the four waves cover the basis");

__global__ __launch_bounds__(256) void smpl_vertex_kernel(const float *__restrict__ params, const float *__restrict__ ws,
                                                          const float *__restrict__ v_template, const float *__restrict__ shapedirs,
                                                          const float *__restrict__ posedirs, const float *__restrict__ weights,
                                                          int V, int new_params, float *__restrict__ verts) {
    __shared__ float wsl[WS_FLOATS];
    __shared__ float part[4 * EB];
    __shared__ float vp[EB];
    const int f = blockIdx.y, t = threadIdx.x;
    const long long n3 = 3ll * V, base = (long long)blockIdx.x * EB;
    const float *__restrict__ p = params + (size_t)f * PSTRIDE;
    for (int e = t; e < WS_FLOATS; e += 256) wsl[e] = ws[(size_t)f * WS_FLOATS + e];
    __syncthreads();
    if (new_params) {  // lbs.py:199-202,211; skipped entirely otherwise (:213), posedirs is then never read
        const int w = t / 64, lane = t % 64;
        const int p0 = w * PF_PER_WAVE, p1 = min(p0 + PF_PER_WAVE, NPF);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        const bool in0 = base + lane < n3, in1 = base + lane + 64 < n3, in2 = base + lane + 128 < n3;
        const float *__restrict__ row = posedirs + (size_t)p0 * n3 + base + lane;
        for (int q = p0; q < p1; ++q, row += n3) {
            const float pf = wsl[WS_PF + q];
            if (in0) acc[0] += pf * row[0];
            if (in1) acc[1] += pf * row[64];
            if (in2) acc[2] += pf * row[128];
        }
        for (int k = 0; k < 3; ++k) part[w * EB + lane + 64 * k] = acc[k];
        __syncthreads();
    }
    if (t < EB && base + t < n3) {  // lbs.py:186: v_shaped, then :211 or :213
        float acc = 0.0f;
        for (int l = 0; l < NB_BETAS; ++l) acc += shapedirs[(size_t)l * n3 + base + t] * p[72 + l];
        float v = v_template[base + t] + acc;
        if (new_params) v = ((part[t] + part[EB + t]) + (part[2 * EB + t] + part[3 * EB + t])) + v;
        vp[t] = v;
    }
    __syncthreads();
    const long long v = (long long)blockIdx.x * VB + t;
    if (t < VB && v < V) {  // lbs.py:220-231, body_model.py:148
        float T[12];
        for (int e = 0; e < 12; ++e) T[e] = 0.0f;
        for (int j = 0; j < NJ; ++j) {
            const float wj = weights[(size_t)j * V + v];
            for (int e = 0; e < 12; ++e) T[e] += wj * wsl[WS_A + 12 * j + e];
        }
        const float x = vp[3 * t], y = vp[3 * t + 1], z = vp[3 * t + 2];
        float s[3];
        const float xyz[3] = {x, y, z};
        for (int i = 0; i < 3; ++i) s[i] = xyz[i] + (T[4 * i] * x + T[4 * i + 1] * y + T[4 * i + 2] * z + T[4 * i + 3]);
        const float *__restrict__ rot = wsl + WS_ROT;
        float *__restrict__ out = verts + ((size_t)f * V + v) * 3;
        for (int i = 0; i < 3; ++i) out[i] = (s[0] * rot[3 * i] + s[1] * rot[3 * i + 1] + s[2] * rot[3 * i + 2]) + p[72 + NB_BETAS + 3 + i];
    }
}

// ------------------------------------------------------------------------------------------------- voxelisation
constexpr int VOX_THREADS = 1024;

// cv2.Rodrigues(Rh)[0].astype(np.float32): the exact formula in double, rounded once
__device__ void rodrigues_f64(const float *__restrict__ r, float *__restrict__ R) {
    const double x = r[0], y = r[1], z = r[2];
    const double th = sqrt(x * x + y * y + z * z);
    if (th < 1e-12) {
        for (int e = 0; e < 9; ++e) R[e] = e % 4 == 0 ? 1.0f : 0.0f;
        return;
    }
    const double kx = x / th, ky = y / th, kz = z / th, s = sin(th), c1 = 1.0 - cos(th);
    const double K[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double kk = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = (float)(((i == j ? 1.0 : 0.0) + s * K[i * 3 + j]) + c1 * kk);
        }
}

// (v - Th) . R, column i: the one expression both passes evaluate
__device__ __forceinline__ float smpl_space(const float d[3], const float *__restrict__ R, int i) {
    return fmaf(d[2], R[6 + i], fmaf(d[1], R[3 + i], d[0] * R[i]));
}

// min over the workgroup of lo[0..5], max of hi[0..5]; the result is in red[0..11] after the call (min and max do not depend on
// the order they are taken in)
__device__ void block_min_max(float lo[6], float hi[6], float *__restrict__ red /* [16 * 12] */) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int e = 0; e < 6; ++e) {
            lo[e] = fminf(lo[e], __shfl_xor(lo[e], off, 64));
            hi[e] = fmaxf(hi[e], __shfl_xor(hi[e], off, 64));
        }
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0)
        for (int e = 0; e < 6; ++e) {
            red[12 * wave + e] = lo[e];
            red[12 * wave + 6 + e] = hi[e];
        }
    __syncthreads();
    if (threadIdx.x < 12) {
        float a = red[threadIdx.x];
        for (int w = 1; w < VOX_THREADS / 64; ++w) a = threadIdx.x < 6 ? fminf(a, red[12 * w + threadIdx.x]) : fmaxf(a, red[12 * w + threadIdx.x]);
        red[threadIdx.x] = a;
    }
    __syncthreads();
}

struct VoxPad {
    float x, y, z;  // subtracted from the minimum and added to the maximum of the axis; 0 = that axis is not padded
};

// One workgroup per frame: bounds of the world vertices and of their SMPL-space images, then the voxel coordinates.
__global__ __launch_bounds__(VOX_THREADS) void smpl_voxelize_kernel(const float *__restrict__ verts, int V, const float *__restrict__ Rh,
                                                                    const float *__restrict__ Th, long long rt_stride, double vs0,
                                                                    double vs1, double vs2, VoxPad pad, int *__restrict__ coord,
                                                                    int *__restrict__ out_sh, float *__restrict__ bounds,
                                                                    float *__restrict__ R_out, int *__restrict__ summary) {
    __shared__ float R[9];
    __shared__ float th[3];
    __shared__ float red[(VOX_THREADS / 64) * 12];
    __shared__ float mn[3];  // padded minimum of the SMPL-space coordinates
    const int f = blockIdx.x, t = threadIdx.x;
    const float *__restrict__ xyz = verts + (size_t)f * V * 3;
    if (t == 0) rodrigues_f64(Rh + (size_t)f * rt_stride, R);
    if (t < 3) th[t] = Th[(size_t)f * rt_stride + t];
    __syncthreads();
    float lo[6], hi[6];
    for (int e = 0; e < 6; ++e) lo[e] = INFINITY, hi[e] = -INFINITY;
    for (int v = t; v < V; v += VOX_THREADS) {
        const float w[3] = {xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2]};
        const float d[3] = {w[0] - th[0], w[1] - th[1], w[2] - th[2]};
        for (int i = 0; i < 3; ++i) {
            const float s = smpl_space(d, R, i);
            lo[i] = fminf(lo[i], w[i]), hi[i] = fmaxf(hi[i], w[i]);
            lo[3 + i] = fminf(lo[3 + i], s), hi[3 + i] = fmaxf(hi[3 + i], s);
        }
    }
    block_min_max(lo, hi, red);
    // red: world min [0..2], SMPL-space min [3..5], world max [6..8], SMPL-space max [9..11]; the padding is a float32 operation
    if (t < 3) {
        const float pd = t == 0 ? pad.x : t == 1 ? pad.y : pad.z;  // x - 0 is x
        const float wlo = red[t] - pd, whi = red[6 + t] + pd, slo = red[3 + t] - pd, shi = red[9 + t] + pd;
        summary[(size_t)f * 9 + t] = __float_as_int(wlo);
        summary[(size_t)f * 9 + 3 + t] = __float_as_int(whi);
        bounds[(size_t)f * 6 + t] = slo;
        bounds[(size_t)f * 6 + 3 + t] = shi;
        mn[t] = slo;
        // out_sh in dhw order: entry 2 - t belongs to axis t
        const double vs = t == 2 ? vs0 : t == 1 ? vs1 : vs2;
        const int sh = ((int)ceil((double)(shi - slo) / vs) | 31) + 1;
        out_sh[(size_t)f * 3 + (2 - t)] = sh;
        summary[(size_t)f * 9 + 6 + (2 - t)] = sh;
    }
    if (t < 9) R_out[(size_t)f * 9 + t] = R[t];
    __syncthreads();
    int *__restrict__ co = coord + (size_t)f * V * 3;
    for (int v = t; v < V; v += VOX_THREADS) {
        const float d[3] = {xyz[3 * (size_t)v] - th[0], xyz[3 * (size_t)v + 1] - th[1], xyz[3 * (size_t)v + 2] - th[2]};
        co[3 * (size_t)v + 0] = (int)rint((double)(smpl_space(d, R, 2) - mn[2]) / vs0);
        co[3 * (size_t)v + 1] = (int)rint((double)(smpl_space(d, R, 1) - mn[1]) / vs1);
        co[3 * (size_t)v + 2] = (int)rint((double)(smpl_space(d, R, 0) - mn[0]) / vs2);
    }
}

}  // namespace

extern "C" int nb_smpl_pose(const nb_smpl_model *model, const float *params, int32_t n_frames, int new_params, float *ws,
                            float *verts, float *joints, void *stream) {
    NB_REQUIRE(model && params && ws && verts, "nb_smpl_pose: NULL pointer");
    NB_REQUIRE(model->n_verts >= 1 && model->n_verts <= 2147483647 / 3 / 4, "nb_smpl_pose: V = %d (1 .. 178956970)", model->n_verts);
    NB_REQUIRE(n_frames >= 1 && n_frames <= 65535, "nb_smpl_pose: F = %d (1 .. 65535)", n_frames);
    NB_REQUIRE(model->v_template && model->shapedirs && model->weights && model->j_template && model->j_shapedirs,
               "nb_smpl_pose: a model array is NULL");
    NB_REQUIRE(!new_params || model->posedirs, "nb_smpl_pose: new_params needs posedirs");
    NB_REQUIRE(model->parents[0] == -1, "nb_smpl_pose: parents[0] = %d (the root has parent -1)", model->parents[0]);
    for (int j = 1; j < NJ; ++j)
        NB_REQUIRE(model->parents[j] >= 0 && model->parents[j] < j, "nb_smpl_pose: parents[%d] = %d (0 .. %d: a parent comes first)",
                   j, model->parents[j], j - 1);
    const int V = model->n_verts;
    Parents parents;
    for (int j = 0; j < NJ; ++j) parents.p[j] = model->parents[j];
    hipLaunchKernelGGL(smpl_prologue_kernel, dim3(n_frames), dim3(64), 0, (hipStream_t)stream, params, model->j_template,
                       model->j_shapedirs, parents, ws, joints);
    NB_CHECK_LAUNCH("nb_smpl_pose (prologue)");
    hipLaunchKernelGGL(smpl_vertex_kernel, dim3(nb_ceil_div(V, VB), n_frames), dim3(256), 0, (hipStream_t)stream, params, ws,
                       model->v_template, model->shapedirs, model->posedirs, model->weights, V, new_params ? 1 : 0, verts);
    NB_CHECK_LAUNCH("nb_smpl_pose (vertices)");
    return NB_OK;
}

extern "C" int nb_smpl_voxelize(const float *verts, int32_t n_verts, int32_t n_frames, const float *Rh, const float *Th,
                                int64_t rt_stride, const double voxel_size[3], int pad_mode, int32_t *coord, int32_t *out_sh,
                                float *bounds, float *R, int32_t *summary, void *stream) {
    NB_REQUIRE(verts && Rh && Th && voxel_size && coord && out_sh && bounds && R && summary, "nb_smpl_voxelize: NULL pointer");
    NB_REQUIRE(n_verts >= 1 && n_verts <= 2147483647 / 3 / 4, "nb_smpl_voxelize: V = %d (1 .. 178956970)", n_verts);
    NB_REQUIRE(n_frames >= 1, "nb_smpl_voxelize: F = %d (>= 1)", n_frames);
    NB_REQUIRE(rt_stride >= 3, "nb_smpl_voxelize: rt_stride = %lld floats (>= 3)", (long long)rt_stride);
    for (int a = 0; a < 3; ++a)
        NB_REQUIRE(voxel_size[a] > 0.0 && voxel_size[a] <= 1e30, "nb_smpl_voxelize: voxel_size[%d] = %g (> 0)", a, voxel_size[a]);
    VoxPad pad = {0.0f, 0.0f, 0.0f};
    if (pad_mode == NB_PAD_ZJU)
        pad.z = 0.05f;
    else if (pad_mode == NB_PAD_BIG_BOX)
        pad.x = pad.y = pad.z = 0.05f;
    else if (pad_mode == NB_PAD_SNAPSHOT)
        pad.y = 0.1f;
    else
        NB_REQUIRE(false, "nb_smpl_voxelize: pad_mode = %d (NB_PAD_ZJU, NB_PAD_BIG_BOX or NB_PAD_SNAPSHOT)", pad_mode);
    hipLaunchKernelGGL(smpl_voxelize_kernel, dim3(n_frames), dim3(VOX_THREADS), 0, (hipStream_t)stream, verts, n_verts, Rh, Th,
                       (long long)rt_stride, voxel_size[0], voxel_size[1], voxel_size[2], pad, coord, out_sh, bounds, R, summary);
    NB_CHECK_LAUNCH("nb_smpl_voxelize");
    return NB_OK;
}
