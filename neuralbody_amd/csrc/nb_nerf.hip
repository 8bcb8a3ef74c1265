// nb_nerf.hip — the vanilla-NeRF baseline's coordinate MLP (8 x 256, one skip, a view branch) as one kernel: a workgroup carries
// 64 samples from the positional encoding to raw, the activations never leave LDS, the weights stream from a blob packed once in
// MFMA fragment order (nb_nerf_pack).
//
// Restates (zju3dv/neuralbody):
//   lib/networks/embedder.py:26-36                    [x, sin(2^k x), cos(2^k x)]_k, three columns each
//   lib/networks/nerf.py:27-43, 45-65                 Nerf: pts_linears (skip [input_pts, h] after layer 4), alpha_linear,
//                                                     feature_linear, views_linears[0] on [feature, input_views], rgb_linear
//   lib/networks/nerf.py:140-158                      Network.forward: embed, concatenate, run
//   lib/networks/renderer/volume_renderer.py:72,151   pts = o + d * z, viewdirs = d / |d|
//
// LAYOUT.  LDS holds the tile's activations transposed, act[row][sample] with 64 samples per row:
//   rows   0..255  h, the hidden vector (each layer overwrites it in place, between two barriers)
//   rows 256..319  the 63 embedding columns of the point, then a zero row
//   rows 320..351  the 27 embedding columns of the direction, then five zero rows
//   rows 352..355  the four partial sums of alpha_linear
// A layer is out^T[feature][sample] = W[feature][k] . act[k][sample] on v_mfma_f32_32x32x2_f32: the A operand is the weight (lane
// l: feature l & 31 of the tile, k = 2 e + (l >> 5) of k-step e), the B operand the activation (lane l: row k, sample l & 31), so a
// D fragment has its sample on the lane and its features in the registers (tile_row) and goes back to act[feature][sample] with
// conflict-free stores.  Wave w of four owns features [64 w, 64 w + 64) (views_linears[0]: [32 w, 32 w + 32)) of all 64 samples:
// 2 x 2 (1 x 2) accumulator tiles.  A layer's k runs over one or two row segments in chunks of 16 rows: layer 0 over rows 256..319,
// the skip layer over 0..255 then 256..319 (its weight columns are permuted to that order when packed: the reference has the
// input first), the view layer over 0..255 then 320..351.  The zero rows meet zero weights.
//
// ARITHMETIC, NB_PREC_F32.  Every product is an fp32 fma into an fp32 accumulator that starts at the bias:
// the matrix layers in ascending k of the row order above (the MFMA is a k-ordered fmaf chain), alpha_linear as four fmaf chains
// over 64 columns each, added as (p0 + p1) + (p2 + p3) and then to the bias, rgb_linear as one chain over its 128 columns.  The
// point is fl32(o + fl32(d * z)), the direction d / |d| formed in float64 and rounded once (nb_importance_sample's definitions),
// the encoding sin_rev of nb_march_common.h.  No atomics: the same inputs give the same bits.
//
// NB_PREC_F16X3 (nerf_decode16_kernel): the same layers on v_mfma_f32_32x32x16_f16 with fp32 accumulation, every operand split into
// an fp16 head and an fp16 remainder (x = h + l, l = fp16(x - h)) and three products per k-step: Wh.xh + Wh.xl + Wl.xh; the
// remainder x remainder term (2^-22 of the product) is dropped.  The B operand of that MFMA is eight consecutive k of one sample,
// so the image has the OTHER orientation, act16[sample][row] in fp16 with 360 halves per sample (352 rows + 8 of padding), heads
// and remainders in two such arrays; a D fragment's registers 4 g .. 4 g + 3 are four consecutive features of the lane's sample and
// go back as one 8-byte store of heads and one of remainders.  A k-step is a chunk: 16 rows, the weights packed per lane as eight
// heads then eight remainders in the same [wave][chunk][feature tile][lane] order and the same number of bytes as the fp32 blob.
// Biases, alpha_linear and rgb_linear stay fp32 (fma chains over head + remainder).  The accumulation order inside the MFMA is the
// hardware's; the result is still a function of the inputs alone.
#include "nb_nerf_mm.h"

namespace {

using namespace nbnerf;

constexpr int LDS_BYTES = N_ROWS * TILE * 4;
constexpr int STRIDE16 = 360;                  // halves per sample of the fp16 image: 352 rows + 8, so 16-byte reads stay aligned
constexpr int LO16 = TILE * STRIDE16;          // the remainders' array follows the heads'
constexpr int ALPHA16 = 2 * LO16 / 2;          // float index of the four alpha_linear partial sums behind both arrays
constexpr int LDS_BYTES16 = 2 * LO16 * 2 + 4 * TILE * 4;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct PackArgs {
    const float *w[N_MM], *b[N_MM], *alpha_w, *alpha_b, *rgb_w, *rgb_b;
    float *packed;
};

// packed weight of layer L: [wave 4][chunk][feature tile FT][lane 64][k-step 8]
__global__ __launch_bounds__(256) void nerf_pack_kernel(PackArgs a, int L, int fast) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (L == N_MM) {  // biases and the two heads
        if (idx < 256 * 9 + 128) {
            const int l = idx >> 8 < MM_VIEWS ? idx >> 8 : MM_VIEWS;
            a.packed[W_TOTAL + idx] = a.b[l][idx - 256 * l];
        }
        if (idx < 256) a.packed[OFF_ALPHA_W + idx] = a.alpha_w[idx];
        if (idx < 4) a.packed[OFF_ALPHA_B + idx] = idx == 0 ? a.alpha_b[0] : 0.f;
        if (idx < 384) a.packed[OFF_RGB_W + idx] = a.rgb_w[idx];
        if (idx < 4) a.packed[OFF_RGB_B + idx] = idx < 3 ? a.rgb_b[idx] : 0.f;
        return;
    }
    const int FT = mm_out(L) / 128, C = mm_c0(L) + mm_c1(L);
    if (idx >= mm_out(L) * mm_k(L)) return;
    const int e = idx & 7, lane = (idx >> 3) & 63;
    int rest = idx >> 9;
    const int ft = rest % FT;
    rest /= FT;
    const int c = rest % C, wv = rest / C;
    const int feature = (wv * FT + ft) * 32 + (lane & 31);
    // fp32: k-step e of the chunk, k = 2 e + lane half; fp16: element e of the chunk's one k-step, k = 8 * lane half + e
    const int kk = 16 * c + (fast ? 8 * (lane >> 5) + e : 2 * e + (lane >> 5));
    const int row = kk < 16 * mm_c0(L) ? mm_row0(L) + kk : mm_row1(L) + kk - 16 * mm_c0(L);
    const int col = mm_col(L, row);
    const float w = col < 0 ? 0.f : a.w[L][(size_t)feature * mm_in(L) + col];
    if (!fast) {
        a.packed[mm_w_off(L) + idx] = w;
        return;
    }
    _Float16 *dst = reinterpret_cast<_Float16 *>(a.packed + mm_w_off(L)) + (size_t)(idx >> 3) * 16 + e;  // [8 heads | 8 remainders] per lane
    const _Float16 h = (_Float16)w;
    dst[0] = h;
    dst[8] = (_Float16)(w - (float)h);
}

struct DecodeArgs {
    const float *packed, *ray_o, *ray_d, *z_vals;  // DENSITY: ray_o is the points [n_pts,3], ray_d and z_vals are not read
    long long n_pts;
    int S;
    float *raw;  // [n_pts, 4]; DENSITY: alpha [n_pts]
    float *tap;  // nerf_decode_kernel<true> only: [n_pts, NT_COLS]
};

// embedding column e of one 3-vector (embedder.py:26-36): x, then per frequency the three sines and the three cosines
__device__ __forceinline__ float embed_col(int e, const float (&x)[3], const double (&t)[3]) {
    if (e < 3) return e == 0 ? x[0] : (e == 1 ? x[1] : x[2]);
    const int f = (e - 3) / 6, rem = (e - 3) % 6, ax = rem % 3;
    const double ta = ax == 0 ? t[0] : (ax == 1 ? t[1] : t[2]);
    return sin_rev(ta * (double)(1 << f) + (rem >= 3 ? 0.25 : 0.0));
}

// The tile's sample (s, q) of the element-wise phases: the point and, unless DENSITY, the unit direction.  DENSITY reads the point as
// it is given (no ray, no depth) and has no direction: the trunk does not read one (nerf_mesh.py:45-54).
template <bool DENSITY>
__device__ __forceinline__ void sample_inputs(const DecodeArgs &a, long long pt, float (&p)[3], float (&v)[3]) {
    if constexpr (DENSITY) {
        p[0] = a.ray_o[pt * 3], p[1] = a.ray_o[pt * 3 + 1], p[2] = a.ray_o[pt * 3 + 2];
        v[0] = v[1] = v[2] = 0.f;
    } else {
        const long long ray = pt / a.S;
        const float z = a.z_vals[pt];
        const float dx = a.ray_d[ray * 3], dy = a.ray_d[ray * 3 + 1], dz = a.ray_d[ray * 3 + 2];
        p[0] = ray_point(a.ray_o[ray * 3], dx, z), p[1] = ray_point(a.ray_o[ray * 3 + 1], dy, z),
        p[2] = ray_point(a.ray_o[ray * 3 + 2], dz, z);
        const double dn = sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
        v[0] = (float)((double)dx / dn), v[1] = (float)((double)dy / dn), v[2] = (float)((double)dz / dn);
    }
}

// TAP: also write the sample's row of the activation tap (nb_nerf_mm.h), every value as the next layer reads it.  The arithmetic
// does not depend on TAP: a layer's D fragments go to the tap from the registers that publish() writes to the image.
// DENSITY (nb_nerf_density): the trunk alone.  The same image, layers 0..7 by the same mm_layer / publish, then alpha_linear's four
// chains on h7 and their sum: what raw[..., 3] goes through above, so the same bits.  No view rows, no feature_linear, no heads.
template <bool TAP, bool DENSITY = false>
__global__ __launch_bounds__(256) void nerf_decode_kernel(DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float act[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane, q = wave;  // the element-wise phases: thread (sample s, quarter q)
    const long long pt_raw = (long long)blockIdx.x * TILE + s;
    const bool live = pt_raw < a.n_pts;
    const long long pt = live ? pt_raw : a.n_pts - 1;  // a padding sample repeats the last point and stores nothing
    // the tap rows of the two samples whose D fragments this lane holds (sample tiles 0 and 1), NULL = padding
    float *tap0 = nullptr, *tap1 = nullptr;
    if constexpr (TAP) {
        const long long p0 = (long long)blockIdx.x * TILE + (lane & 31);
        if (p0 < a.n_pts) tap0 = a.tap + p0 * NT_COLS;
        if (p0 + 32 < a.n_pts) tap1 = a.tap + (p0 + 32) * NT_COLS;
    }
    {
        float p[3], v[3];
        sample_inputs<DENSITY>(a, pt, p, v);
        const double tp[3] = {(double)p[0] * NB_INV_2PI, (double)p[1] * NB_INV_2PI, (double)p[2] * NB_INV_2PI};
        for (int e = q; e < 64; e += 4) act[(ROW_PTS + e) * TILE + s] = e < N_PTS_EMB ? embed_col(e, p, tp) : 0.f;
        if constexpr (!DENSITY) {
            const double tv[3] = {(double)v[0] * NB_INV_2PI, (double)v[1] * NB_INV_2PI, (double)v[2] * NB_INV_2PI};
            for (int e = q; e < 32; e += 4) act[(ROW_VIEW + e) * TILE + s] = e < N_VIEW_EMB ? embed_col(e, v, tv) : 0.f;
        }
    }
    __syncthreads();
    if constexpr (TAP) {  // the embeddings: thread (s, q) copies columns [24 q, 24 q + 24) of its sample's 96, 16 bytes at a time
        if (live) {
            float *dst = a.tap + pt * NT_COLS + NT_PTS;
            for (int c = 24 * q; c < 24 * q + 24; c += 4) {
                f32x4 v;
                for (int i = 0; i < 4; ++i) v[i] = act[(ROW_PTS + c + i) * TILE + s];
                *reinterpret_cast<f32x4 *>(dst + c) = v;
            }
        }
    }

    const float *pk = a.packed;
    f32x16 acc[2][2];
    const auto alpha_partial = [&]() {  // thread (s, q): alpha_linear's chain over columns [64 q, 64 q + 64) of h7
        const float *aw = pk + OFF_ALPHA_W + 64 * q;
        float sum = 0.f;
        for (int k = 0; k < 64; ++k) sum = fmaf(aw[k], act[(64 * q + k) * TILE + s], sum);
        act[(ROW_ALPHA + q) * TILE + s] = sum;
    };
    const auto alpha_sum = [&]() {
        const float *pa = act + ROW_ALPHA * TILE + s;
        return __fadd_rn(__fadd_rn(__fadd_rn(pa[0], pa[TILE]), __fadd_rn(pa[2 * TILE], pa[3 * TILE])), pk[OFF_ALPHA_B]);
    };
#pragma unroll 1
    for (int L = 0; L < (DENSITY ? MM_FEATURE : MM_VIEWS); ++L) {  // pts_linears[0..7] with relu, then feature_linear without
        if (L == MM_FEATURE) alpha_partial();  // alpha_linear reads h before feature_linear's publish overwrites it
        mm_layer<2>(pk + mm_w_off(L) + wave * (mm_k(L) * 64), pk + mm_b_off(L) + 64 * wave, act, mm_row0(L), mm_c0(L), mm_row1(L),
                    mm_c1(L), acc, lane);
        if constexpr (TAP) {  // layer L's columns start at 256 L: NT_H + 256 L for h, NT_FEATURE = 256 MM_FEATURE
            const int c = 256 * L + 64 * wave;
            if (L == MM_FEATURE) store_rows<2, false>(acc, tap0 ? tap0 + c : nullptr, tap1 ? tap1 + c : nullptr, lane);
            else store_rows<2, true>(acc, tap0 ? tap0 + c : nullptr, tap1 ? tap1 + c : nullptr, lane);
        }
        if (L == MM_FEATURE) publish<2, false>(acc, act, 64 * wave, lane);
        else publish<2, true>(acc, act, 64 * wave, lane);
    }
    if constexpr (DENSITY) {  // h7 is published: the four chains, a barrier, one thread per sample adds them
        alpha_partial();
        __syncthreads();
        if (q == 0 && live) a.raw[pt] = alpha_sum();
        return;
    }
    {
        f32x16 accv[1][2];
        mm_layer<1>(pk + mm_w_off(MM_VIEWS) + wave * (mm_k(MM_VIEWS) * 32), pk + mm_b_off(MM_VIEWS) + 32 * wave, act,
                    mm_row0(MM_VIEWS), mm_c0(MM_VIEWS), mm_row1(MM_VIEWS), mm_c1(MM_VIEWS), accv, lane);
        if constexpr (TAP) {
            const int c = NT_V + 32 * wave;
            store_rows<1, true>(accv, tap0 ? tap0 + c : nullptr, tap1 ? tap1 + c : nullptr, lane);
        }
        publish<1, true>(accv, act, 32 * wave, lane);
    }
    float out;
    if (q < 3) {  // rgb_linear
        const float *rw = pk + OFF_RGB_W + 128 * q;
        out = pk[OFF_RGB_B + q];
        for (int k = 0; k < 128; ++k) out = fmaf(rw[k], act[k * TILE + s], out);
    } else {  // alpha_linear's four partial sums
        out = alpha_sum();
    }
    if (live) a.raw[pt * 4 + q] = out;
}

// ---------------------------------------------------------------- NB_PREC_F16X3
__device__ __forceinline__ void put16(_Float16 *act, int row, int s, float v) {
    const _Float16 h = (_Float16)v;
    act[s * STRIDE16 + row] = h;
    act[LO16 + s * STRIDE16 + row] = (_Float16)(v - (float)h);
}
__device__ __forceinline__ float get16(const _Float16 *act, int row, int s) {
    return (float)act[s * STRIDE16 + row] + (float)act[LO16 + s * STRIDE16 + row];
}

template <int FT>
__device__ __forceinline__ void mm_layer16(const float *__restrict__ wp, const float *__restrict__ bias, const _Float16 *act, int row0,
                                           int c0, int row1, int c1, f32x16 (&acc)[FT][2], int lane) {
    const int hi = lane >> 5, col = lane & 31;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b = bias[32 * ft + tile_row(r, hi)];
            acc[ft][0][r] = b;
            acc[ft][1][r] = b;
        }
    const f32x4 *wq = reinterpret_cast<const f32x4 *>(wp) + lane * 2;  // per lane: eight heads, eight remainders
    const int C = c0 + c1;
    f32x4 cur[FT][2], nxt[FT][2];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) cur[ft][0] = wq[ft * 128], cur[ft][1] = wq[ft * 128 + 1];
    for (int c = 0; c < C; ++c) {
        const int cn = c + 1 < C ? c + 1 : c;
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) nxt[ft][0] = wq[(cn * FT + ft) * 128], nxt[ft][1] = wq[(cn * FT + ft) * 128 + 1];
        const int row = c < c0 ? row0 + 16 * c : row1 + 16 * (c - c0);
        const _Float16 *b = act + col * STRIDE16 + row + 8 * hi;
        f16x8 bh[2], bl[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bh[st] = *reinterpret_cast<const f16x8 *>(b + st * 32 * STRIDE16);
            bl[st] = *reinterpret_cast<const f16x8 *>(b + LO16 + st * 32 * STRIDE16);
        }
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
            const f16x8 ah = __builtin_bit_cast(f16x8, cur[ft][0]), al = __builtin_bit_cast(f16x8, cur[ft][1]);
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                acc[ft][st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[st], acc[ft][st], 0, 0, 0);
                acc[ft][st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[st], acc[ft][st], 0, 0, 0);
                acc[ft][st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[st], acc[ft][st], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) cur[ft][0] = nxt[ft][0], cur[ft][1] = nxt[ft][1];
    }
}

template <int FT, bool RELU>
__device__ __forceinline__ void publish16(const f32x16 (&acc)[FT][2], _Float16 *act, int f0, int lane) {
    const int hi = lane >> 5, col = lane & 31;
    __syncthreads();
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // registers 4 g .. 4 g + 3: features 8 g + 4 hi .. + 3 of the tile
                f16x4 h, l;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = RELU ? fmaxf(acc[ft][st][4 * g + i], 0.f) : acc[ft][st][4 * g + i];
                    h[i] = (_Float16)v;
                    l[i] = (_Float16)(v - (float)h[i]);
                }
                _Float16 *dst = act + (32 * st + col) * STRIDE16 + f0 + 32 * ft + 8 * g + 4 * hi;
                *reinterpret_cast<f16x4 *>(dst) = h;
                *reinterpret_cast<f16x4 *>(dst + LO16) = l;
            }
    __syncthreads();
}

template <bool DENSITY = false>
__global__ __launch_bounds__(256) void nerf_decode16_kernel(DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float act[];
    _Float16 *act16 = reinterpret_cast<_Float16 *>(act);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane, q = wave;
    const long long pt_raw = (long long)blockIdx.x * TILE + s;
    const bool live = pt_raw < a.n_pts;
    const long long pt = live ? pt_raw : a.n_pts - 1;
    {
        float p[3], v[3];
        sample_inputs<DENSITY>(a, pt, p, v);
        const double tp[3] = {(double)p[0] * NB_INV_2PI, (double)p[1] * NB_INV_2PI, (double)p[2] * NB_INV_2PI};
        for (int e = q; e < 64; e += 4) put16(act16, ROW_PTS + e, s, e < N_PTS_EMB ? embed_col(e, p, tp) : 0.f);
        if constexpr (!DENSITY) {
            const double tv[3] = {(double)v[0] * NB_INV_2PI, (double)v[1] * NB_INV_2PI, (double)v[2] * NB_INV_2PI};
            for (int e = q; e < 32; e += 4) put16(act16, ROW_VIEW + e, s, e < N_VIEW_EMB ? embed_col(e, v, tv) : 0.f);
        }
    }
    __syncthreads();

    const float *pk = a.packed;
    f32x16 acc[2][2];
    const auto alpha_partial = [&]() {
        const float *aw = pk + OFF_ALPHA_W + 64 * q;
        float sum = 0.f;
        for (int k = 0; k < 64; ++k) sum = fmaf(aw[k], get16(act16, 64 * q + k, s), sum);
        act[ALPHA16 + q * TILE + s] = sum;
    };
    const auto alpha_sum = [&]() {
        const float *pa = act + ALPHA16 + s;
        return __fadd_rn(__fadd_rn(__fadd_rn(pa[0], pa[TILE]), __fadd_rn(pa[2 * TILE], pa[3 * TILE])), pk[OFF_ALPHA_B]);
    };
#pragma unroll 1
    for (int L = 0; L < (DENSITY ? MM_FEATURE : MM_VIEWS); ++L) {
        if (L == MM_FEATURE) alpha_partial();
        mm_layer16<2>(pk + mm_w_off(L) + wave * (mm_k(L) * 64), pk + mm_b_off(L) + 64 * wave, act16, mm_row0(L), mm_c0(L),
                      mm_row1(L), mm_c1(L), acc, lane);
        if (L == MM_FEATURE) publish16<2, false>(acc, act16, 64 * wave, lane);
        else publish16<2, true>(acc, act16, 64 * wave, lane);
    }
    if constexpr (DENSITY) {
        alpha_partial();
        __syncthreads();
        if (q == 0 && live) a.raw[pt] = alpha_sum();
        return;
    }
    {
        f32x16 accv[1][2];
        mm_layer16<1>(pk + mm_w_off(MM_VIEWS) + wave * (mm_k(MM_VIEWS) * 32), pk + mm_b_off(MM_VIEWS) + 32 * wave, act16,
                      mm_row0(MM_VIEWS), mm_c0(MM_VIEWS), mm_row1(MM_VIEWS), mm_c1(MM_VIEWS), accv, lane);
        publish16<1, true>(accv, act16, 32 * wave, lane);
    }
    float out;
    if (q < 3) {
        const float *rw = pk + OFF_RGB_W + 128 * q;
        out = pk[OFF_RGB_B + q];
        for (int k = 0; k < 128; ++k) out = fmaf(rw[k], get16(act16, k, s), out);
    } else {
        out = alpha_sum();
    }
    if (live) a.raw[pt * 4 + q] = out;
}

// d alpha / d p from the gradient by the 63 embedding columns (embedder.py:26-36): column a is the coordinate itself, columns
// 3 + 6 f + a and 3 + 6 f + 3 + a are sin(2^f x_a) and cos(2^f x_a), whose derivatives 2^f cos and -2^f sin are the forward's own stored
// columns.  One thread per point; every product of two fp32 is exact in float64, the sum runs in float64 in ascending f and is rounded
// once (as nb_ray_distortion does).
__global__ __launch_bounds__(256) void nerf_embed_grad_kernel(const float *__restrict__ emb, long long emb_stride,
                                                              const float *__restrict__ d_emb, long long d_stride, long long n,
                                                              float *__restrict__ grad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *e = emb + i * emb_stride, *d = d_emb + i * d_stride;
    for (int ax = 0; ax < 3; ++ax) {
        double g = (double)d[ax];
        for (int f = 0; f < 10; ++f) {
            const int c = 3 + 6 * f + ax;
            g += (double)(1 << f) * ((double)d[c] * (double)e[c + 3] - (double)d[c + 3] * (double)e[c]);
        }
        grad[i * 3 + ax] = (float)g;
    }
}

int nerf_precision(const char *who, int precision) {
    NB_REQUIRE(precision == NB_PREC_F32 || precision == NB_PREC_F16X3, "%s: precision = %d (NB_PREC_F32 = %d or NB_PREC_F16X3 = %d)", who,
               precision, NB_PREC_F32, NB_PREC_F16X3);
    return NB_OK;
}

}  // namespace

extern "C" int64_t nb_nerf_pack_size(int precision) { return precision == NB_PREC_F32 || precision == NB_PREC_F16X3 ? PACK_FLOATS : 0; }

extern "C" int nb_nerf_pack(const nb_nerf_params *params, float *packed, int precision, void *stream) {
    if (int rc = nerf_precision("nb_nerf_pack", precision)) return rc;
    NB_REQUIRE(params && packed, "nb_nerf_pack: NULL pointer");
    NB_REQUIRE(((uintptr_t)packed & 15) == 0, "nb_nerf_pack: packed must be 16-byte aligned");
    PackArgs a = {};
    for (int i = 0; i < 8; ++i) a.w[i] = params->pts_w[i], a.b[i] = params->pts_b[i];
    a.w[MM_FEATURE] = params->feature_w, a.b[MM_FEATURE] = params->feature_b;
    a.w[MM_VIEWS] = params->views_w, a.b[MM_VIEWS] = params->views_b;
    a.alpha_w = params->alpha_w, a.alpha_b = params->alpha_b, a.rgb_w = params->rgb_w, a.rgb_b = params->rgb_b;
    a.packed = packed;
    uintptr_t bits = (uintptr_t)a.alpha_w | (uintptr_t)a.alpha_b | (uintptr_t)a.rgb_w | (uintptr_t)a.rgb_b;
    for (int i = 0; i < N_MM; ++i) {
        NB_REQUIRE(a.w[i] && a.b[i], "nb_nerf_pack: NULL weight or bias (matrix %d)", i);
        bits |= (uintptr_t)a.w[i] | (uintptr_t)a.b[i];
    }
    NB_REQUIRE(a.alpha_w && a.alpha_b && a.rgb_w && a.rgb_b, "nb_nerf_pack: NULL alpha_linear / rgb_linear parameter");
    NB_REQUIRE((bits & 3) == 0, "nb_nerf_pack: every parameter must be 4-byte aligned");
    for (int L = 0; L <= N_MM; ++L) {
        const int n = L == N_MM ? 256 * 9 + 128 : mm_out(L) * mm_k(L);
        hipLaunchKernelGGL(nerf_pack_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, L,
                           precision == NB_PREC_F16X3 ? 1 : 0);
        NB_CHECK_LAUNCH("nb_nerf_pack");
    }
    return NB_OK;
}

// the checks nb_nerf_decode and nb_nerf_decode_tap share; tap NULL = no tap (f32 or f16x3), else the f32 kernel with the tap
static int nerf_decode_launch(const char *who, const float *packed, const float *ray_o, const float *ray_d, const float *z_vals,
                              int64_t n_rays, int32_t n_samples, float *raw, float *tap, bool want_tap, int precision, void *stream) {
    NB_REQUIRE(n_rays >= 0 && n_rays < (1ll << 31), "%s: n_rays = %lld (0..2^31 - 1)", who, (long long)n_rays);
    NB_REQUIRE(n_samples >= 1 && n_samples <= 512, "%s: n_samples = %d (1..512)", who, n_samples);
    if (n_rays == 0) return NB_OK;
    NB_REQUIRE(packed && ray_o && ray_d && z_vals && raw && (tap || !want_tap), "%s: NULL pointer", who);
    NB_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)tap & 15) == 0, "%s: packed%s must be 16-byte aligned", who,
               want_tap ? " and tap" : "");
    NB_REQUIRE((((uintptr_t)ray_o | (uintptr_t)ray_d | (uintptr_t)z_vals | (uintptr_t)raw) & 3) == 0,
               "%s: ray_o, ray_d, z_vals and raw must be 4-byte aligned", who);
    const long long n_pts = (long long)n_rays * n_samples;
    NB_REQUIRE(n_pts / TILE < (1ll << 31) - 1, "%s: n_rays * n_samples = %lld (< 2^37)", who, n_pts);
    // the attribute belongs to (function, device): set on every call, whichever device and thread this is (a host-side table write)
    const bool fast = precision == NB_PREC_F16X3;
    const void *fn = fast       ? reinterpret_cast<const void *>(nerf_decode16_kernel<false>)
                     : want_tap ? reinterpret_cast<const void *>(nerf_decode_kernel<true>)
                                : reinterpret_cast<const void *>(nerf_decode_kernel<false>);
    const int lds = fast ? LDS_BYTES16 : LDS_BYTES;
    NB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    DecodeArgs a = {packed, ray_o, ray_d, z_vals, n_pts, n_samples, raw, tap};
    const dim3 grid(nb_ceil_div(n_pts, TILE));
    if (fast) hipLaunchKernelGGL(nerf_decode16_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else if (want_tap) hipLaunchKernelGGL(nerf_decode_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(nerf_decode_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
    NB_CHECK_LAUNCH(who);
    return NB_OK;
}

extern "C" int nb_nerf_decode(const float *packed, const float *ray_o, const float *ray_d, const float *z_vals, int64_t n_rays,
                              int32_t n_samples, float *raw, int precision, void *stream) {
    if (int rc = nerf_precision("nb_nerf_decode", precision)) return rc;
    return nerf_decode_launch("nb_nerf_decode", packed, ray_o, ray_d, z_vals, n_rays, n_samples, raw, nullptr, false, precision, stream);
}

extern "C" int nb_nerf_decode_tap(const float *packed, const float *ray_o, const float *ray_d, const float *z_vals, int64_t n_rays,
                                  int32_t n_samples, float *raw, float *tap, void *stream) {
    return nerf_decode_launch("nb_nerf_decode_tap", packed, ray_o, ray_d, z_vals, n_rays, n_samples, raw, tap, true, NB_PREC_F32, stream);
}

extern "C" int nb_nerf_density(const float *packed, const float *pts, int64_t n, float *alpha, int precision, void *stream) {
    if (int rc = nerf_precision("nb_nerf_density", precision)) return rc;
    NB_REQUIRE(n >= 0 && n / TILE < (1ll << 31) - 1, "nb_nerf_density: n = %lld (0..2^37 - 1)", (long long)n);
    if (n == 0) return NB_OK;
    NB_REQUIRE(packed && pts && alpha, "nb_nerf_density: NULL pointer");
    NB_REQUIRE(((uintptr_t)packed & 15) == 0, "nb_nerf_density: packed must be 16-byte aligned");
    NB_REQUIRE((((uintptr_t)pts | (uintptr_t)alpha) & 3) == 0, "nb_nerf_density: pts and alpha must be 4-byte aligned");
    const bool fast = precision == NB_PREC_F16X3;
    const void *fn = fast ? reinterpret_cast<const void *>(nerf_decode16_kernel<true>)
                          : reinterpret_cast<const void *>(nerf_decode_kernel<false, true>);
    const int lds = fast ? LDS_BYTES16 : LDS_BYTES;
    NB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    DecodeArgs a = {packed, pts, nullptr, nullptr, (long long)n, 1, alpha, nullptr};
    const dim3 grid(nb_ceil_div(n, TILE));
    if (fast) hipLaunchKernelGGL(nerf_decode16_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((nerf_decode_kernel<false, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    NB_CHECK_LAUNCH("nb_nerf_density");
    return NB_OK;
}

extern "C" int nb_nerf_embed_grad(const float *emb, int64_t emb_stride, const float *d_emb, int64_t d_stride, int64_t n, float *grad,
                                  void *stream) {
    NB_REQUIRE(n >= 0 && n / 256 < (1ll << 31) - 1, "nb_nerf_embed_grad: n = %lld (0..2^39 - 1)", (long long)n);
    NB_REQUIRE(emb_stride >= N_PTS_EMB && d_stride >= N_PTS_EMB, "nb_nerf_embed_grad: emb_stride = %lld, d_stride = %lld (>= %d floats)",
               (long long)emb_stride, (long long)d_stride, N_PTS_EMB);
    if (n == 0) return NB_OK;
    NB_REQUIRE(emb && d_emb && grad, "nb_nerf_embed_grad: NULL pointer");
    NB_REQUIRE((((uintptr_t)emb | (uintptr_t)d_emb | (uintptr_t)grad) & 3) == 0, "nb_nerf_embed_grad: emb, d_emb and grad must be 4-byte aligned");
    hipLaunchKernelGGL(nerf_embed_grad_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, emb, (long long)emb_stride,
                       d_emb, (long long)d_stride, (long long)n, grad);
    NB_CHECK_LAUNCH("nb_nerf_embed_grad");
    return NB_OK;
}
