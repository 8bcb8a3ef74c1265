"""A numpy decoder of the f16f6 weight stream (nb_pack_fold_kernel, csrc/nb_march_pack.hip; layout: csrc/nb_pack_layout.h) and the
reference quantisers of its cross terms.  CPU only; nothing here touches the library.

The stream is what the march's four waves read per depth step: per wave 132 one-KiB pieces (64 lanes x 16 bytes) and, behind them,
14 scale dwords per lane.  A phase (fc_1, fc_2, the folded colour head over the hidden units, the colour head over the encodings) is
PH_NB K blocks of 64 input columns x PH_MT 32-row output tiles of the wave; a block is, in this order, its A16 pieces (chunk j = 8 of
each half-block's 32 elements, tile m: the fp16 heads), then the cross fragments in TERM_ORDER: W_h (the heads again, fp4 e2m1, element
order interleaved) and W_l (w - head, fp4 e2m1), each with one E8M0 scale byte per (row, half-block) in the block's scale dword.  Wave w
walks the blocks of phases 0-2 from its own one: step block b holds the columns of block (b + w) & 3.

It decodes the SHIPPED configuration (both cross terms four-bit) and is guarded by the pack size that tests/test_abi.py pins.

What this pins and what it does not: the decoder restates the packer's index arithmetic (which piece, lane and element hold which
(row, input column)).  Tests built on it therefore pin the stream's ARITHMETIC - heads, remainders, block exponents, rounding, the
statistic - and that every weight has exactly one place, but not the layout against the march kernel that consumes it.  That is
tests/test_gpu_publish_order.py::test_rotation_and_pack_agree, which renders through the march with one K block live at a time.
"""
import math

import numpy as np

N_WAVES = 4
PIECE = 1024  # bytes: 64 lanes x 16
PH_NB = (4, 4, 4, 2)  # K blocks per phase
PH_MT = (2, 2, 1, 1)  # output tiles per wave
PH_ROWS = (256, 256, 128, 128)
PH_WIDTH = (256, 256, 256, 346)  # width of the phase's natural weight matrix (phase 3: view_fc's, columns 256.. are the encodings)
TERM_ORDER = (0, 1)  # cross term executed first / second: 0 = W_h, 1 = W_l
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M3_GRID = tuple(m / 8.0 for m in range(8)) + tuple(2.0 ** e * (1.0 + m / 8.0) for e in range(3) for m in range(8))
E2M1_TOP, E2M3_TOP = 6.0, 7.5


def block_pieces(mt):
    """Pieces of one block: 4 chunks x mt A16 pieces, mt W_h and mt W_l fragments, rounded up to even."""
    return (4 * mt + mt + mt + 1) & ~1


PHASE_P0 = tuple(sum(PH_NB[i] * block_pieces(PH_MT[i]) for i in range(ph)) for ph in range(5))
PHASE_S0 = tuple(sum(PH_NB[:ph]) for ph in range(5))
P_TOTAL = PHASE_P0[4]
N_SCALE = PHASE_S0[4]
WAVE_STREAM = P_TOTAL * PIECE + ((N_SCALE * 256 + 1023) & ~1023)
PACK_F32 = 8 * 44 * 256 + 256 + 2 * (8 * 32 * 256 + 256) + 256 + 4 + 8 * 32 * 256 + 4 * 44 * 256 + 128 + 384 + 4  # floats
STREAM_FLOATS = N_WAVES * WAVE_STREAM // 4
PACK_SIZE = PACK_F32 + STREAM_FLOATS + 8
ABI_PACK_SIZE = 333320 + 4 * (132 * 1024 + 4096) // 4 + 8  # tests/test_abi.py::test_sizes_and_struct_layout


def check_pack_size(pack_size):
    """The decoder knows one stream layout: 132 pieces + 14 scale dwords per wave behind a 333320-float fp32 section."""
    if not (int(pack_size) == ABI_PACK_SIZE == PACK_SIZE and P_TOTAL == 132 and N_SCALE == 14):
        raise AssertionError("tests/fold_stream_ref.py decodes the stream of a %d-float blob (both cross terms fp4 e2m1, 132 pieces "
                             "per wave); the library packs %d floats: the stream layout changed, update the decoder"
                             % (PACK_SIZE, int(pack_size)))


# ------------------------------------------------------------------------------------------------------------------ columns
def tile_row(r, hi):
    return (r & 3) + 8 * (r >> 2) + 4 * hi


def col_hidden(q, hi):
    return 32 * (q >> 4) + tile_row(q & 15, hi)


def pe_slot_col(a, slot):
    """view_fc column of encoding slot 0..31 of axis a: x, (sin, cos)(x 2^k) k < 10, v, (sin, cos)(v 2^k) k < 4, two pads; -1 = pad."""
    if a >= 3 or slot >= 30:
        return -1
    if slot == 0:
        return 256 + 27 + a
    if slot <= 20:
        k, is_cos = (slot - 1) >> 1, (slot - 1) & 1
        return 256 + 27 + 3 + 6 * k + 3 * is_cos + a
    if slot == 21:
        return 256 + a
    k, is_cos = (slot - 22) >> 1, (slot - 22) & 1
    return 256 + 3 + 6 * k + 3 * is_cos + a


def phase_cols(ph):
    """int [PH_NB, 2, 32]: the natural input column of element e of half-block (block, kh); -1 = zero padding."""
    out = np.empty((PH_NB[ph], 2, 32), np.int64)
    for b in range(PH_NB[ph]):
        for kh in range(2):
            for e in range(32):
                out[b, kh, e] = col_hidden(32 * b + e, kh) if ph < 3 else pe_slot_col(2 * b + kh, e)
    return out


# --------------------------------------------------------------------------------------------------------------- quantisers
def _nearest_code(x, grid, top):
    """Code of the grid point nearest to |x| (saturated at top), by brute force in float64; a tie goes to the even code; bit
    len(grid) is the sign, set for every x < 0 (a negative value that rounds to zero keeps it: -0)."""
    x = np.asarray(x, np.float64)
    g = np.asarray(grid, np.float64)
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.abs(x), top)
        d = np.abs(a[..., None] - g)
        near = d == d.min(-1, keepdims=True)
    even = (np.arange(len(grid)) & 1) == 0
    pick_even = near & even
    code = np.where(pick_even.any(-1), pick_even.argmax(-1), near.argmax(-1))
    return (code + len(grid) * (x < 0)).astype(np.uint8)


def e2m1_code(x):
    """fp4 e2m1: sign, two exponent bits of bias 1, one mantissa bit (0 0.5 1 1.5 2 3 4 6)."""
    return _nearest_code(x, E2M1_GRID, E2M1_TOP)


def e2m3_code(x):
    """fp6 e2m3: sign, two exponent bits of bias 1, three mantissa bits (0 .. 0.875 by eighths, 1 .. 7.5)."""
    return _nearest_code(x, E2M3_GRID, E2M3_TOP)


def e2m1_value(code):
    code = np.asarray(code)
    return np.where(code & 8, -1.0, 1.0) * np.asarray(E2M1_GRID)[code & 7]


def block_exponent(amax, top):
    """The smallest ex with amax 2^-ex <= top, clamped to +-120; 0 for amax == 0 and for amax >= 3e38 (inf included)."""
    amax = float(amax)
    if not (amax > 0.0) or amax >= 3.0e38:  # (no fp32 number lies between 3e38 and its fp32 rounding: the same set of fp32 inputs)
        return 0
    ex = math.frexp(amax)[1]
    while math.ldexp(top, ex) < amax:  # exact: top 2^ex is a float64
        ex += 1
    while math.ldexp(top, ex - 1) >= amax:
        ex -= 1
    return min(max(ex, -120), 120)


def block_exponents(amax, top):
    return np.vectorize(lambda a: block_exponent(a, top), otypes=[np.int64])(amax)


# ------------------------------------------------------------------------------------------------------------------- layout
def _fragments():
    """Every fragment of one wave's share, wave-independent part: (phase, step block b, kind, j, m, piece, scale byte or None);
    kind 'a16' (chunk j, tile m) or 'x' (cross term k = j, tile m; scale byte = index inside the lane's scale dword)."""
    for ph in range(4):
        mt, ppb = PH_MT[ph], block_pieces(PH_MT[ph])
        for b in range(PH_NB[ph]):
            base = PHASE_P0[ph] + b * ppb
            for j in range(4):
                for m in range(mt):
                    yield ph, b, "a16", j, m, base + j * mt + m, None
            for slot in range(2):
                k = TERM_ORDER[slot]
                for m in range(mt):
                    yield ph, b, "x", k, m, base + 4 * mt + slot * mt + m, k * mt + m


def attribution():
    """int [3, WAVE_STREAM]: how often each byte of a wave's share is claimed as piece data (0), a scale byte (1), padding (2: the
    holes of a block, the unused bytes of the scale dwords, the tail of the scale area)."""
    n = np.zeros((3, WAVE_STREAM), np.int64)
    lanes = np.arange(64)
    for ph, b, kind, j, m, piece, sbyte in _fragments():
        n[0, piece * PIECE:(piece + 1) * PIECE] += 1
        if sbyte is not None:
            n[1, P_TOTAL * PIECE + (PHASE_S0[ph] + b) * 256 + lanes * 4 + sbyte] += 1
    n[2] = (n[0] + n[1]) == 0
    return n


def _row0(w, mt, m):
    return 64 * w + 32 * m if mt == 2 else 32 * w


def decode(stream):
    """stream: the uint8 [4 * WAVE_STREAM] stream section of a packed blob.  Returns one dict per phase, natural (row, column) order:
       heads   uint16 [R, W]      the fp16 head of every weight (W = 256, or view_fc's 346 columns of which 256.. are decoded)
       code    uint8 [2, R, W]    the four-bit codes of W_h (0) and W_l (1)
       ex      int   [2, R, NB, 2] the block exponent (scale byte - 127) of term k, row r, half-block (block, kh)
       seen_h, seen_c, seen_e     how often each of those was found in the stream (all must be 1 at the decoded places)
       pad_nonzero                non-zero heads or codes found at padding elements (column -1)
    and `unattributed`: the bytes of the stream no piece or scale byte accounts for, concatenated."""
    stream = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    assert stream.size == N_WAVES * WAVE_STREAM, stream.size
    cols = [phase_cols(ph) for ph in range(4)]
    out = []
    for ph in range(4):
        R, W = PH_ROWS[ph], PH_WIDTH[ph]
        out.append(dict(heads=np.zeros((R, W), np.uint16), code=np.zeros((2, R, W), np.uint8),
                        ex=np.full((2, R, PH_NB[ph], 2), -999, np.int64), seen_h=np.zeros((R, W), np.int64),
                        seen_c=np.zeros((2, R, W), np.int64), seen_e=np.zeros((2, R, PH_NB[ph], 2), np.int64), pad_nonzero=0))
    i32 = np.arange(32)
    for w in range(N_WAVES):
        wave = stream[w * WAVE_STREAM:(w + 1) * WAVE_STREAM]
        for ph, b, kind, j, m, piece, sbyte in _fragments():
            o = out[ph]
            bl = (b + w) & 3 if ph < 3 else b
            rows = _row0(w, PH_MT[ph], m) + i32
            data = wave[piece * PIECE:(piece + 1) * PIECE]
            for kh in range(2):
                if kind == "a16":
                    d = data.view(np.uint16).reshape(64, 8)[32 * kh:32 * kh + 32]
                    c = cols[ph][bl, kh, 8 * j:8 * j + 8]
                    ok = c >= 0
                    o["heads"][np.ix_(rows, c[ok])] = d[:, ok]
                    o["seen_h"][np.ix_(rows, c[ok])] += 1
                    o["pad_nonzero"] += int(np.count_nonzero(d[:, ~ok]))
                else:
                    k = j
                    byt = data.reshape(64, 16)[32 * kh:32 * kh + 32]
                    nib = np.empty((32, 32), np.uint8)
                    nib[:, 0::2], nib[:, 1::2] = byt & 15, byt >> 4
                    src = i32 if k == 1 else 16 * (i32 & 1) + (i32 >> 1)  # element of the half-block held by nibble e
                    c = cols[ph][bl, kh, src]
                    ok = c >= 0
                    o["code"][k][np.ix_(rows, c[ok])] = nib[:, ok]
                    o["seen_c"][k][np.ix_(rows, c[ok])] += 1
                    o["pad_nonzero"] += int(np.count_nonzero(nib[:, ~ok]))
                    sc = wave[P_TOTAL * PIECE + (PHASE_S0[ph] + b) * 256 + (32 * kh + i32) * 4 + sbyte]
                    o["ex"][k, rows, bl, kh] = sc.astype(np.int64) - 127
                    o["seen_e"][k, rows, bl, kh] += 1
    free = attribution()[2].astype(bool)
    unattributed = np.concatenate([stream[w * WAVE_STREAM:(w + 1) * WAVE_STREAM][free] for w in range(N_WAVES)])
    return out, unattributed


# ---------------------------------------------------------------------------------------------------------------- reference
def _ordered_product(a, b):
    """a @ b in float64, summed over the inner index in rising order (every product of two fp32 numbers is exact in float64, so the
    order of the sum is all that an implementation can differ in)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.zeros((a.shape[0], b.shape[1]))
    for m in range(a.shape[1]):
        s += a[:, m:m + 1] * b[m:m + 1, :]
    return s


def merged_colour_head(view_w, latent_w, feature_w):
    """view_w[:, :256] . (latent_w[:, :256] . feature_w), each product summed in float64 and rounded to fp32: float32 [128, 256]."""
    inner = _ordered_product(latent_w[:, :256], feature_w).astype(np.float32)
    return _ordered_product(view_w[:, :256], inner).astype(np.float32)


def phase_weights(p):
    """The natural fp32 weight matrix of each phase from a parameter dict (fc1_w, fc2_w, view_w, latent_w, feature_w)."""
    return [np.asarray(p["fc1_w"], np.float32), np.asarray(p["fc2_w"], np.float32),
            merged_colour_head(p["view_w"], p["latent_w"], p["feature_w"]), np.asarray(p["view_w"], np.float32)]


def expected(weights):
    """What the stream must hold for the four natural weight matrices: per phase heads uint16 [R, W] (decoded columns only), code
    [2, R, W], ex [2, R, NB, 2], and the statistic's counts small / nonzero [R, NB, 2] (non-zero heads below 1/8 of their block's
    largest head / non-zero heads)."""
    out = []
    for ph in range(4):
        w = np.asarray(weights[ph], np.float32)
        R, W = PH_ROWS[ph], PH_WIDTH[ph]
        assert w.shape == (R, W), (ph, w.shape)
        pc = phase_cols(ph)
        o = dict(heads=np.zeros((R, W), np.uint16), code=np.zeros((2, R, W), np.uint8), ex=np.zeros((2, R, PH_NB[ph], 2), np.int64),
                 small=np.zeros((R, PH_NB[ph], 2), np.int64), nonzero=np.zeros((R, PH_NB[ph], 2), np.int64),
                 valid=np.zeros((R, W), bool))
        with np.errstate(over="ignore", invalid="ignore"):
            for b in range(PH_NB[ph]):
                for kh in range(2):
                    c = pc[b, kh]
                    ok = c >= 0
                    v = np.zeros((R, 32), np.float32)
                    v[:, ok] = w[:, c[ok]]
                    h16 = v.astype(np.float16)
                    h = h16.astype(np.float32)
                    terms = (h, v - h)  # fp32 - fp32: exact, the head is v rounded to 11 bits
                    o["heads"][:, c[ok]] = h16.view(np.uint16)[:, ok]
                    o["valid"][:, c[ok]] = True
                    for k in range(2):
                        amax = np.fmax.reduce(np.abs(terms[k]), axis=1, initial=0.0)  # fmax: a NaN element does not count
                        ex = block_exponents(amax, E2M1_TOP)
                        o["ex"][k, :, b, kh] = ex
                        o["code"][k][:, c[ok]] = e2m1_code(np.ldexp(terms[k].astype(np.float64), -ex[:, None]))[:, ok]
                    amax_h = np.fmax.reduce(np.abs(h), axis=1, initial=0.0)
                    o["nonzero"][:, b, kh] = (h != 0).sum(1)
                    o["small"][:, b, kh] = ((h != 0) & (np.abs(h) < np.float32(0.125) * amax_h[:, None])).sum(1)
        out.append(o)
    return out


def expected_stats(exp):
    """The six integers of the statistic: (small, non-zero) of fc_1, fc_2 and the two colour-head phases together."""
    s = [(int(o["small"].sum()), int(o["nonzero"].sum())) for o in exp]
    return [s[0][0], s[0][1], s[1][0], s[1][1], s[2][0] + s[3][0], s[2][1] + s[3][1]]
