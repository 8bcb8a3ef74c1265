// nb_march_pack.hip — the packer of the f16f6 weight stream that nb_march_fold.hip's kernel reads (layout: nb_pack_layout.h), gfx950.
// Runs once per weight version, behind nb_pack_kernel (nb_march.hip), whose fp32 section it reads the merged feature / latent
// layer from: pure index arithmetic and the quantisers of the cross terms.
#include "nb_f6_ops.h"
#include "nb_pack_layout.h"

using namespace nbm;

namespace {

// ---------------------------------------------------------------- weight stream packing
// input column of the layer phase `ph` held by element e of half-block (b, kh) of LDS block b; -1 = zero padding
__device__ __forceinline__ int phase_col(int ph, int b, int kh, int e) {
    if (ph < 3) return col_hidden(32 * b + e, kh);
    return pe_slot_col(2 * b + kh, e);  // the encodings: the owner lane's part
}
__device__ __forceinline__ float phase_weight(const nb_mlp_params &p, const float *f32_blob, int ph, int row, int b, int kh, int e) {
    const int col = phase_col(ph, b, kh, e);
    if (col < 0) return 0.f;
    if (ph == 0) return p.fc1_w[row * 256 + col];
    if (ph == 1) return p.fc2_w[row * 256 + col];
    if (ph == 2) {
        // view_w[:, :256] . (latent_w[:, :256] . feature_w): the inner product comes from the fp32 section (formed in fp64
        // there, fragment order: element hidden_q(col) of half tile_hi(col)), the outer one is summed in fp64 here
        const int hi2 = tile_hi(col & 31), q2 = hidden_q(col);
        double s = 0.0;
        for (int m = 0; m < 256; ++m)
            s += (double)p.view_w[row * 346 + m] *
                 (double)f32_blob[OFF_L4 + (((m >> 5) * GH + (q2 >> 2)) * 64 + (hi2 * 32 + (m & 31))) * 4 + (q2 & 3)];
        return (float)s;
    }
    return p.view_w[row * 346 + col];
}

// fp4 e2m1 (sign, 2 exponent bits of bias 1, 1 mantissa bit: 0 0.5 1 1.5 2 3 4 6), round to nearest (ties to the even code)
__device__ __forceinline__ unsigned fp4_e2m1_bits(float v) {
    const unsigned sgn = v < 0.f ? 8u : 0u;
    const float a = fminf(fabsf(v), 6.f);
    constexpr float grid[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    unsigned code = 0;
    float best = a;
    for (unsigned c = 1; c < 8; ++c) {
        const float d = fabsf(a - grid[c]);
        if (d < best || (d == best && (c & 1u) == 0u)) {
            best = d;
            code = c;
        }
    }
    return sgn | code;
}

// one thread per (wave, piece, lane): the lane's 16 bytes (+, for a four-bit fragment, its scale byte in the block's scale dword)
__global__ void nb_pack_fold_kernel(nb_mlp_params p, const float *__restrict__ f32_blob, unsigned *__restrict__ out, int *__restrict__ stats) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * P_TOTAL * 64) return;
    const int lane = t & 63, piece = (t >> 6) % P_TOTAL, w = (t >> 6) / P_TOTAL;
    const int i = lane & 31, kg = lane >> 5;
    int ph = 0, p0 = 0;
    for (int q = 0; q < N_PH; ++q) {
        const int n = phase_pieces(PH_NB[q], PH_MT[q]);
        if (piece < p0 + n) {
            ph = q;
            break;
        }
        p0 += n;
    }
    const int mt = PH_MT[ph], ppb = block_pieces(mt);
    const int rel = piece - p0, b = rel / ppb, r = rel % ppb;
    // the LDS block whose columns step block b multiplies: wave w walks the published blocks from its own one (layer_s, OWN)
    const int bl = ph < 3 ? (b + w) & 3 : b;
    unsigned w32[4] = {0u, 0u, 0u, 0u};
    if (r < 4 * mt) {  // A16 of chunk j, tile m
        const int j = r / mt, m = r % mt;
        const int row = (mt == 2 ? 64 * w + 32 * m : 32 * w) + i;
        for (int q = 0; q < 8; q += 2) {
            const f16x2 hp = {(_Float16)phase_weight(p, f32_blob, ph, row, bl, kg, 8 * j + q),
                              (_Float16)phase_weight(p, f32_blob, ph, row, bl, kg, 8 * j + q + 1)};
            w32[q / 2] = __builtin_bit_cast(unsigned, hp);
        }
    } else {  // a cross fragment: k = 0 W_h (multiplies the interleaved remainder operand), k = 1 W_l (natural order) — or the block's hole
        int r6 = r - 4 * mt, k = -1, m = 0, half = 0;
        for (int slot = 0; slot < 2; ++slot) {
            const int kk = TERM_ORDER[slot], width = mt * term_pieces(kk);
            if (r6 < width) {
                k = kk;
                m = r6 / term_pieces(kk);
                half = r6 % term_pieces(kk);
                break;
            }
            r6 -= width;
        }
        if (k >= 0) {
            const bool four = FP4_K[k];
            const float top = four ? 6.f : 7.5f;  // largest magnitude of the format
            const int row = (mt == 2 ? 64 * w + 32 * m : 32 * w) + i;
            float wv[32], amax = 0.f;
            for (int e = 0; e < 32; ++e) {
                const int n = k ? e : 16 * (e & 1) + (e >> 1);
                const float wt = phase_weight(p, f32_blob, ph, row, bl, kg, n);
                const float h = (float)(_Float16)wt;
                wv[e] = k ? wt - h : h;
                amax = fmaxf(amax, fabsf(wv[e]));
            }
            int ex = 0;
            if (amax > 0.f && amax < 3.0e38f) {
                ex = ilogbf(amax / top);
                if (ldexpf(top, ex) < amax) ++ex;  // the smallest power of two with max / 2^ex <= top
                ex = min(max(ex, -120), 120);
            }
            if (four) {
                for (int e = 0; e < 32; ++e) w32[e >> 3] |= fp4_e2m1_bits(ldexpf(wv[e], -ex)) << (4 * (e & 7));
                unsigned char *sc = reinterpret_cast<unsigned char *>(out) + (size_t)w * WAVE_STREAM + (size_t)P_TOTAL * 1024 +
                                    (size_t)(phase_s0(ph) + b) * 256 + lane * 4 + (k * mt + m);
                *sc = (unsigned char)(127 + ex);
            } else {
                unsigned w8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                for (int e = 0; e < 32; ++e) {
                    const unsigned code = fp6_e2m3_bits(ldexpf(wv[e], -ex));
                    const int bit = 6 * e;
                    w8[bit >> 5] |= code << (bit & 31);
                    if ((bit & 31) > 26) w8[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
                }
                w8[6] = (unsigned)(127 + ex);
                for (int q = 0; q < 4; ++q) w32[q] = w8[4 * half + q];
            }
            // statistic behind nb_mlp_six_bit_stats_offset(): how many non-zero head weights sit below 1/8 of their block's
            // maximum, i.e. where e2m3 keeps fewer than 3 bits and e2m1 none (per layer: small, non-zero)
            if (k == 0 && half == 0) {
                int small = 0, nz = 0;
                for (int e = 0; e < 32; ++e) {
                    nz += wv[e] != 0.f;
                    small += wv[e] != 0.f && fabsf(wv[e]) < 0.125f * amax;
                }
                const int layer = ph < 2 ? ph : 2;  // fc_1, fc_2, the folded colour head (both of its K phases)
                atomicAdd(&stats[2 * layer], small);
                atomicAdd(&stats[2 * layer + 1], nz);
            }
        }
    }
    unsigned *dst = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(out) + (size_t)w * WAVE_STREAM) + ((size_t)piece * 64 + lane) * 4;
    for (int q = 0; q < 4; ++q) dst[q] = w32[q];
}

}  // namespace

namespace nbm {

int pack_fold_stream(const nb_mlp_params *p, float *packed, hipStream_t st) {
    const long long n = (long long)4 * P_TOTAL * 64;
    int *stats = reinterpret_cast<int *>(packed + STATS_OFF);
    NB_REQUIRE(hipMemsetAsync(stats, 0, STATS_FLOATS * sizeof(int), st) == hipSuccess, "pack_fold_stream: hipMemsetAsync failed");
    hipLaunchKernelGGL(nb_pack_fold_kernel, dim3(nb_ceil_div(n, 256)), dim3(256), 0, st, *p, packed,
                       reinterpret_cast<unsigned *>(packed + STREAM_OFF), stats);
    NB_CHECK_LAUNCH("nb_pack_fold_kernel");
    return NB_OK;
}

}  // namespace nbm
