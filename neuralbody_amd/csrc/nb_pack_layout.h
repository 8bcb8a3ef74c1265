// nb_pack_layout.h — the ONE description of the packed weight blob (nb_mlp_pack): the fp32 section of MFMA fragments, the
// f16f6 weight stream behind it and the six-bit statistic behind that.  Plain constexpr C++17 with no HIP in it: every kernel
// that writes or reads the blob (nb_march.hip, nb_march_fold.hip, nb_march_fixup.hip, nb_march_pack.hip) includes it, and a host
// compiler can compile it on its own (tests/test_abi.py checks its numbers against tests/fold_stream_ref.py that way).
#pragma once

#if defined(__HIPCC__)
#define NB_LAYOUT_FN __host__ __device__ constexpr
#else
#define NB_LAYOUT_FN constexpr
#endif

namespace nbm {

// ---------------------------------------------------------------- fp32 section (written by nb_pack_kernel, nb_march.hip): offsets in floats
constexpr int G0 = 44;  // fc_0: 352 inputs = 176 K=2 chunks = 44 groups of 4 chunks
constexpr int GH = 32;  // hidden 256 inputs = 128 chunks = 32 groups
constexpr int GV = 44;  // view_fc: 128 chunks (latent_fc out) + 45 PE chunks + 3 zero chunks
constexpr int OFF_L0 = 0;
constexpr int OFF_B0 = OFF_L0 + 8 * G0 * 256;
constexpr int OFF_L1 = OFF_B0 + 256;
constexpr int OFF_B1 = OFF_L1 + 8 * GH * 256;
constexpr int OFF_L2 = OFF_B1 + 256;
constexpr int OFF_B2 = OFF_L2 + 8 * GH * 256;
constexpr int OFF_AW = OFF_B2 + 256;  // alpha_fc weights [2][128]
constexpr int OFF_AB = OFF_AW + 256;  // alpha_fc bias (4 floats, 1 used)
constexpr int OFF_L4 = OFF_AB + 4;    // merged latent_fc[:, :256] @ feature_fc
constexpr int OFF_LV = OFF_L4 + 8 * GH * 256;
constexpr int OFF_BV = OFF_LV + 4 * GV * 256;
constexpr int OFF_RW = OFF_BV + 128;  // rgb_fc weights [3][2][64]
constexpr int OFF_RB = OFF_RW + 384;  // rgb_fc bias (4 floats, 3 used)
constexpr int PACK_SIZE = OFF_RB + 4;

// ---------------------------------------------------------------- f16f6 weight stream (per wave), in 1-KiB pieces
// phase = NB K blocks x MT output tiles of this wave (wave w's b-th block of a phase over published activations is LDS block
// (b + w) & 3: it starts with the block it has published itself, layer_s); per block: for each of its 4 chunks, for each tile:
// A16 (1 piece: the fp16 heads, the main product); then its two CROSS TERMS in execution order, for each tile one fragment: k = 0 W_h (multiplies the
// remainder operand), k = 1 W_l (multiplies the head operand).  A cross fragment is fp6 e2m3 — 24 bytes of data + its E8M0 scale
// in the lane's seventh dword, 2 pieces — or, for the terms in NB_FP4_TERMS (bit k), fp4 e2m1 — 16 bytes of data, 1 piece, its
// scale one byte of the block's SCALE DWORD (byte k MT + m; one 256-byte load per block from behind the pieces).  The cross
// terms are 2^-11 of the main term, so their weight operand needs few bits: fp4 takes the stream from 176 to 132 pieces per wave
// and depth step — the stream (L2 -> L1, 64 B/clk/CU) is what the MFMA phases wait for (profiles/r06_march_premises.log) — for
// 2^-13 instead of 2^-15 relative error per term (profiles/r06_precision_fp4.md).
#ifndef NB_FP4_TERMS
#define NB_FP4_TERMS 3
#endif
constexpr bool FP4_K[2] = {(NB_FP4_TERMS & 1) != 0, (NB_FP4_TERMS & 2) != 0};
// six-bit fragments are two pieces = one (even-aligned) ring entry: when only W_h is four-bit its fragment goes second
constexpr int TERM_ORDER[2] = {(FP4_K[0] && !FP4_K[1]) ? 1 : 0, (FP4_K[0] && !FP4_K[1]) ? 0 : 1};
NB_LAYOUT_FN int term_pieces(int k) { return FP4_K[k] ? 1 : 2; }
// pieces per block (rounded to even: the next block's six-bit fragments stay even-aligned; an odd count leaves one hole)
NB_LAYOUT_FN int block_pieces(int mt) { return (4 * mt + mt * term_pieces(0) + mt * term_pieces(1) + 1) & ~1; }
// first piece (inside its block) of the fragment of the cross term executed `slot`-th (0 / 1), tile m
NB_LAYOUT_FN int cross_piece(int mt, int slot, int m) {
    return 4 * mt + (slot == 0 ? 0 : mt * term_pieces(TERM_ORDER[0])) + m * term_pieces(TERM_ORDER[slot]);
}
NB_LAYOUT_FN int phase_pieces(int nb, int mt) { return nb * block_pieces(mt); }
constexpr int N_PH = 4;
// fc_1, fc_2, the folded colour head over fc_2's outputs (one tile per wave), view_fc over the positional encodings
constexpr int PH_NB[N_PH] = {4, 4, 4, 2};
constexpr int PH_MT[N_PH] = {2, 2, 1, 1};
NB_LAYOUT_FN int phase_p0(int ph) {
    int p = 0;
    for (int i = 0; i < ph; ++i) p += phase_pieces(PH_NB[i], PH_MT[i]);
    return p;
}
NB_LAYOUT_FN int phase_s0(int ph) {  // first scale dword of the phase (one per block)
    int n = 0;
    for (int i = 0; i < ph; ++i) n += PH_NB[i];
    return n;
}
constexpr int P_L1 = phase_p0(0), P_L2 = phase_p0(1), P_VG = phase_p0(2), P_VP = phase_p0(3), P_TOTAL = phase_p0(4);
constexpr int N_SCALE = phase_s0(4);                        // 14 scale dwords (256 bytes each) behind the pieces
constexpr int WAVE_STREAM = P_TOTAL * 1024 + ((N_SCALE * 256 + 1023) & ~1023);  // bytes of one wave's share of the stream
static_assert(P_TOTAL == (NB_FP4_TERMS == 3 ? 132 : (NB_FP4_TERMS == 0 ? 176 : 160)), "pieces per wave per depth step");
static_assert(P_L1 % 2 == 0 && P_L2 % 2 == 0 && P_VG % 2 == 0 && P_VP % 2 == 0, "six-bit fragments on even pieces");
NB_LAYOUT_FN int phase_of_p0(int p0) { return p0 == P_L1 ? 0 : (p0 == P_L2 ? 1 : (p0 == P_VG ? 2 : 3)); }

// ---------------------------------------------------------------- the whole blob, in floats
constexpr long long STREAM_OFF = PACK_SIZE;                            // the four waves' shares of the stream
constexpr long long STREAM_FLOATS = (long long)4 * WAVE_STREAM / 4;
constexpr long long STATS_OFF = STREAM_OFF + STREAM_FLOATS;            // the six-bit statistic: 6 ints, 2 pad
constexpr long long STATS_FLOATS = 8;
constexpr long long BLOB_FLOATS = STATS_OFF + STATS_FLOATS;            // nb_mlp_pack_size()
static_assert(NB_FP4_TERMS != 3 || BLOB_FLOATS == 333320 + 4 * (132 * 1024 + 4096) / 4 + 8, "the size tests/test_abi.py pins");

}  // namespace nbm
