"""Inputs and float64 references for the tests of the kernels that prepare the f16f6 march's operands (tests/test_march_operands_host.py,
tests/test_gpu_march_operands.py): nb_fold_build, the fp32 section of nb_mlp_pack_sections, nb_mlp_latent_bias and, with
tests/fold_stream_ref.py, the f16f6 weight stream.  CPU only; nothing here touches the library.

nb_fold_build.  LATTICE inputs make the answer exact: V holds integers in [-8, 8] (half of them zero, as behind a ReLU), fc_0
multiples of 2^-6 in [-1, 1]; every partial sum of u = fc_0 . V is a multiple of 2^-6 below 2^11 (at most 128 terms of at most 8), an
fp32 number in any order, so head = fp16(u) and rem = fp16(u - head) are determined bit for bit.  Scaling fc_0 by a power of two keeps
that: 2^-14 turns the heads into fp16 subnormals, 2^7 (with a few large rows) takes products past +-65504.  REALISTIC inputs are held to
    |head + rem - u64| <= 2^-22 |u64| + 2^-25 + C_l 2^-24 sum_k |v_k w_k|
(two fp16 roundings of 2^-11 each, the fp16 subnormal quantum 2^-24 halved, an fp32 chain of C_l terms).

FOLD_CASES gives every level every row-count class: the workgroups hold 128 / 128 / 64 / 64 rows in 32-row tiles, and a workgroup's level
comes from the capacities, so the four levels of one case carry different capacities and the classes rotate through the levels.
"""
import numpy as np

from tests import fold_stream_ref as S

LEVEL_C = (32, 64, 128, 128)
LEVEL_BASE = (0, 32, 96, 224)
ROWS_WG = (128, 128, 64, 64)
SENTINEL16 = 0xBEEF  # what the planes hold before the call
POISON = 12345.0     # what the voxels and rows that must not be read hold
SLACK_ROWS = 4       # sentinel rows behind the zero row
# fc_0 scales of the exact cases: 2^-14 makes the heads fp16 subnormals (its remainders, multiples of 2^-20, are still fp16 numbers);
# 2^-20 (unit 2^-26) puts remainders at and below 2^-25, half the fp16 subnormal quantum, where they round to 0 or 2^-24
LATTICE_SCALES = (0, -14, -20)


# --------------------------------------------------------------------------------------------------------- nb_fold_build: shapes
def level_classes(wg):
    """(n_rows on the device, n_rows_max) of the ten row-count classes of a level whose workgroups hold wg rows."""
    return ((0, 1),                      # nothing active
            (1, 1),                      # one row, capacity = count
            (31, 31 + wg + 5),           # a tile less one row; the capacity spans a second workgroup that has no row
            (32, 32),                    # one tile
            (33, 40),                    # a tile and a row
            (wg - 1, wg - 1),            # a workgroup less one row
            (wg, 2 * wg + 3),            # a whole workgroup; two more workgroups without a row
            (wg + 1, wg + 1),            # a workgroup and a row
            (2 * wg + 1, 2 * wg + 1),    # two workgroups and a row
            (2 * wg + 9, wg + 2))        # the device count exceeds the capacity: clamped to it


CLASS_SHIFT = (0, 3, 5, 8)  # case c gives level l class (c + CLASS_SHIFT[l]) % 10: no two levels of a case share a class or a capacity
FOLD_CASES = tuple(tuple(level_classes(ROWS_WG[l])[(c + CLASS_SHIFT[l]) % 10] for l in range(4)) for c in range(10))
# the value cases (subnormal, saturating, realistic) run on one shape with several workgroups, a partial tile and spare capacity a level
VALUE_CASE = ((129, 140), (33, 33), (65, 130), (64, 64))


def live_rows(case):
    return [min(n, cap) for n, cap in case]


def row_bases(case):
    """First plane row of each level, and the zero row: the capacities' running sum."""
    base = np.concatenate([[0], np.cumsum([cap for _, cap in case])])
    return [int(b) for b in base[:4]], int(base[4])


# --------------------------------------------------------------------------------------------------------- nb_fold_build: values
def lattice_fc0(seed, scale_log2=0):
    """fc_0.weight [256, 352]: multiples of 2^-6 in [-1, 1], times 2^scale_log2."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-64, 65, size=(256, 352)).astype(np.float32) * np.float32(2.0 ** (scale_log2 - 6)))


def lattice_rows(case, seed):
    """Per level [cap, C] fp32: integers in [-8, 8], about half zero, in the live rows; POISON in the rows behind them."""
    rs = np.random.RandomState(seed)
    rows = []
    for l, (n, cap) in enumerate(case):
        v = np.full((cap, LEVEL_C[l]), POISON, np.float32)
        k = min(n, cap)
        v[:k] = rs.randint(-8, 9, size=(k, LEVEL_C[l])) * (rs.rand(k, LEVEL_C[l]) < 0.5)
        rows.append(v)
    return rows


def realistic_fc0(seed):
    return (np.random.RandomState(seed).standard_normal((256, 352)) / np.sqrt(352.0)).astype(np.float32)


def realistic_rows(case, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for l, (n, cap) in enumerate(case):
        v = np.full((cap, LEVEL_C[l]), POISON, np.float32)
        k = min(n, cap)
        v[:k] = np.maximum(rs.standard_normal((k, LEVEL_C[l])), 0.0)
        rows.append(v)
    return rows


def saturating_rows(case, seed, fc0):
    """The lattice rows with, per level, row 0 = 64 sign(fc_0 row 5) (u[0, 5] = 64 sum |w| and many of its neighbours leave the fp16
    range), row 1 its negative, and on level 1 a +inf in row 2 and a NaN in row 3 (with at least 4 live rows there)."""
    rows = lattice_rows(case, seed)
    live = live_rows(case)
    for l in range(4):
        if live[l] >= 2:
            sgn = np.sign(fc0[5, LEVEL_BASE[l]:LEVEL_BASE[l] + LEVEL_C[l]]).astype(np.float32)
            rows[l][0] = 64.0 * sgn
            rows[l][1] = -64.0 * sgn
    assert live[1] >= 4
    rows[1][2, 7] = np.inf
    rows[1][3, 11] = np.nan
    return rows


LONE_OFFENDER = (2, 37, 101)  # (level, row, feature) of the one product of single_offender that leaves the range


def single_offender(case, seed):
    """(fc_0, rows) of the lattice (fc_0 scaled by 2^7) in which exactly ONE product leaves the fp16 range: feature 101 of fc_0 is 128
    throughout and row 37 of level 2 is 8 throughout, u = 8 . 128 . 128 = 2^17.  Neither the row (37 = tile 1, row 5: the upper half
    of an accumulator tile) nor the feature (101 = wave 1, second column tile, column 5) is the first of anything."""
    l, r, f = LONE_OFFENDER
    fc0 = lattice_fc0(seed, 7)
    fc0[f] = 128.0
    rows = lattice_rows(case, seed + 1)
    assert live_rows(case)[l] > r
    rows[l][r] = 8.0
    return fc0, rows


def scatter_rows(rows, case, seed):
    """The same rows scattered into dense channels-last volumes: per level (volume [nvox, C] full of POISON but for the live rows,
    rows_lin [cap] int32): a shuffled choice of voxels no two of which are neighbours in memory; the entries of rows_lin behind the live
    rows point at poisoned voxels."""
    rs = np.random.RandomState(seed)
    out = []
    for l, (n, cap) in enumerate(case):
        nvox = 2 * cap + 3
        lin = (2 * rs.permutation(cap) + 1).astype(np.int32)  # odd voxels, shuffled: every even voxel is poison
        vol = np.full((nvox, LEVEL_C[l]), POISON, np.float32)
        k = min(n, cap)
        vol[lin[:k]] = rows[l][:k]
        out.append((vol, lin))
    return out


def fold_u64(rows, case, fc0):
    """Per level the float64 products u [live rows, 256] = V . fc_0[:, channels of the level]^T (IEEE: 0 . inf = NaN)."""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l, k in enumerate(live_rows(case)):
            w = fc0[:, LEVEL_BASE[l]:LEVEL_BASE[l] + LEVEL_C[l]].astype(np.float64)
            v = rows[l][:k].astype(np.float64)
            u = np.where(np.isfinite(v), v, 0.0) @ w.T
            for r in np.nonzero(~np.isfinite(v).all(1))[0]:  # term by term: a matrix product need not form 0 . inf
                u[r] = (v[r][None, :] * w).sum(1)
            out.append(u)
    return out


def fold_abs64(rows, case, fc0):
    """Per level sum_k |v_k w_k| in float64."""
    return [np.abs(rows[l][:k].astype(np.float64)) @ np.abs(fc0[:, LEVEL_BASE[l]:LEVEL_BASE[l] + LEVEL_C[l]].astype(np.float64)).T
            for l, k in enumerate(live_rows(case))]


def split_planes(u64):
    """head = fp16(fp32(u)) and rem = fp16(fp32(u) - fp32(head)) of an exactly representable u, products beyond +-65504 clamped first (a
    NaN stays one): uint16 [n, 512] = heads | remainders, and the mask of the products that left the range or are not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = u64.astype(np.float32)
        off = ~(np.abs(u) <= np.float32(65504.0))
        v = np.where(np.isnan(u), u, np.clip(u, np.float32(-65504.0), np.float32(65504.0))).astype(np.float32)
        h = v.astype(np.float16)
        r = (v - h.astype(np.float32)).astype(np.float16)
    return np.concatenate([h.view(np.uint16), r.view(np.uint16)], 1), off


def expected_planes(u64_levels, case):
    """uint16 [zero row + 1 + SLACK_ROWS, 512]: the planes after the call on a SENTINEL16-filled buffer, the mask of the entries whose
    product is NaN (their bits are not pinned), and the number of products of live rows that left the range."""
    bases, zero_row = row_bases(case)
    want = np.full((zero_row + 1 + SLACK_ROWS, 512), SENTINEL16, np.uint16)
    nan = np.zeros(want.shape, bool)
    n_off = 0
    for l, u in enumerate(u64_levels):
        planes, off = split_planes(u)
        want[bases[l]:bases[l] + u.shape[0]] = planes
        nan[bases[l]:bases[l] + u.shape[0]] = np.concatenate([np.isnan(u), np.isnan(u)], 1)
        n_off += int(off.sum())
    want[zero_row] = 0
    return want, nan, n_off


def planes_value(planes16):
    """head + rem of uint16 [n, 512] planes in float64."""
    f = planes16.view(np.float16).astype(np.float64)
    return f[:, :256] + f[:, 256:]


# ------------------------------------------------------------------------------------------------------------ decoder weights
MLP_SHAPES = {"fc0": (256, 352), "fc1": (256, 256), "fc2": (256, 256), "alpha": (1, 256), "feature": (256, 256),
              "latent": (256, 384), "view": (128, 346), "rgb": (3, 128)}


def zero_params():
    p = {}
    for name, (o, i) in MLP_SHAPES.items():
        p[name + "_w"] = np.zeros((o, i), np.float32)
        p[name + "_b"] = np.zeros(o, np.float32)
    return p


def normal_params(seed):
    """Every tensor normal with the standard deviation 1 / sqrt(fan_in) of nn.Conv1d's initialisation."""
    rs = np.random.RandomState(seed)
    p = {}
    for name, (o, i) in MLP_SHAPES.items():
        p[name + "_w"] = (rs.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
        p[name + "_b"] = (rs.standard_normal(o) / np.sqrt(i)).astype(np.float32)
    return p


def distinct_integers(shape, seed):
    """1 .. n shuffled: exact in fp32 (n <= 2^24), all different, none zero."""
    n = int(np.prod(shape))
    assert n <= 1 << 24
    return (np.random.RandomState(seed).permutation(n) + 1).astype(np.float32).reshape(shape)


def _ld(x):
    return np.asarray(x, np.longdouble)


def latent_bias_ref(p, code):
    """(reference, sum of |terms|) of out[:256] = latent_b + latent_w[:, :256] . feature_b + latent_w[:, 256:] . code, natural order, in
    extended precision (every product of two fp32 numbers is exact there; the sum carries 64 bits where the platform has them)."""
    lw, x = _ld(p["latent_w"]), np.concatenate([_ld(p["feature_b"]), _ld(code)])
    terms = lw * x[None, :]
    return _ld(p["latent_b"]) + terms.sum(1), np.abs(_ld(p["latent_b"])) + np.abs(terms).sum(1)


def view_bias_ref(p, code):
    """(reference, sum of |terms|) of out[256:] = view_b + view_w[:, :256] . (the merged layer's bias): the terms are those of the
    expanded double sum, so the second figure is |view_b| + |view_w[:, :256]| . (the first sum of |terms|)."""
    lb, lb_abs = latent_bias_ref(p, code)
    vw = _ld(p["view_w"][:, :256])
    return _ld(p["view_b"]) + (vw * lb[None, :]).sum(1), np.abs(_ld(p["view_b"])) + (np.abs(vw) * lb_abs[None, :]).sum(1)


def merged_ref(p):
    """(reference, sum of |terms|) of the merged layer latent_w[:, :256] . feature_w, [256, 256]."""
    a, b = _ld(p["latent_w"][:, :256]), _ld(p["feature_w"])
    ref, tot = np.zeros((256, 256), np.longdouble), np.zeros((256, 256), np.longdouble)
    for m in range(256):
        t = a[:, m:m + 1] * b[m:m + 1, :]
        ref += t
        tot += np.abs(t)
    return ref, tot


def fp64_sum_bound(ref, abs_terms):
    """|got - ref| <= 2^-24 |ref| + 2^-50 sum |terms|: one fp32 rounding of a sum formed in fp64, and the order of that sum."""
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -50 * abs_terms


def cancelling_params(seed, code):
    """normal_params with a latent_b that cancels the rest of the merged layer's bias to the last fp32 bit: the sum is then ~2^-25 of
    its terms, which an fp32 accumulation loses entirely."""
    p = normal_params(seed)
    p["latent_b"] = np.zeros(256, np.float32)
    rest, _ = latent_bias_ref(p, code)
    p["latent_b"] = (-rest).astype(np.float32)
    return p


# ------------------------------------------------------------------------------------------------------------ the f16f6 stream
def place_params(by_row):
    """Every weight of the four phases an integer exact in fp16 that names its column (1 + c) or its row (1 + r); the folded colour head
    is feature_w itself through latent_w[:, :256] = I and view_w[:, :256] = [I | 0]."""
    p = zero_params()

    def pattern(rows, cols, c0=0):
        r, c = np.meshgrid(np.arange(rows), np.arange(c0, c0 + cols), indexing="ij")
        return (1 + (r if by_row else c)).astype(np.float32)

    p["fc1_w"], p["fc2_w"], p["feature_w"] = pattern(256, 256), pattern(256, 256), pattern(256, 256)
    p["latent_w"][:, :256] = np.eye(256, dtype=np.float32)
    p["view_w"][:, :128] = np.eye(128, dtype=np.float32)
    p["view_w"][:, 256:] = pattern(128, 90, 256)
    return p


MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
MIDPOINT_CODES = (0, 2, 2, 4, 4, 6, 6)  # the even neighbour: 0 | 1.0 | 1.0 | 2.0 | 2.0 | 4.0 | 4.0
EDGE_ELEMENTS = np.array([6.0, -6.0] + [s * m for m in MIDPOINTS for s in (1.0, -1.0)], np.float64)  # 16 of a block's 32 elements
EDGE_CODES = np.array([7, 15] + [c + 8 * neg for c in MIDPOINT_CODES for neg in (0, 1)], np.uint8)
# (row, half-block (block, kh)) of fc_1 that each edge case occupies
EDGE_BLOCKS = {"head_midpoints": (3, (0, 0)), "rem_midpoints": (70, (1, 1)), "amax_6": (131, (2, 0)), "amax_6_up": (131, (2, 1)),
               "amax_6_small": (200, (3, 0)), "amax_6_small_up": (200, (3, 1)), "zero": (17, (2, 1)), "single": (254, (0, 1)),
               "huge": (100, (3, 1))}


def edge_params(seed):
    """normal_params whose fc_1 carries, in the blocks of EDGE_BLOCKS:
       head_midpoints   heads +-6 and every e2m1 midpoint with both signs (block exponent 0: the W_h codes are EDGE_CODES)
       rem_midpoints    1 + g 2^-15 for the same g: head 1, remainders on the midpoints of block exponent -15 (W_l codes = EDGE_CODES)
       amax_6(_small)   the largest head 6 2^e exactly (e = 3, -9): exponent e; (_up) one fp16 ulp above: exponent e + 1
       zero             an all-zero block: scale bytes 127, codes 0
       single           one non-zero element
       huge             3.2e38 (head inf, remainder -inf) and inf (remainder NaN): both exponents 0, the codes saturate."""
    p = normal_params(seed)
    pc = S.phase_cols(0)
    w = p["fc1_w"]

    def block(name):
        r, (b, kh) = EDGE_BLOCKS[name]
        return r, pc[b, kh]

    r, c = block("head_midpoints")
    w[r, c] = 0.0
    w[r, c[:16]] = EDGE_ELEMENTS
    r, c = block("rem_midpoints")
    w[r, c] = 1.0
    w[r, c[:16]] = 1.0 + EDGE_ELEMENTS * 2.0 ** -15
    for name, e in (("amax_6", 3), ("amax_6_small", -9)):
        r, c = block(name)
        w[r, c[5]] = -6.0 * 2.0 ** e
        w[r, c] = np.clip(w[r, c], -6.0 * 2.0 ** e, 6.0 * 2.0 ** e)
        r, c = block(name + "_up")
        w[r, c] = np.clip(w[r, c], -2.0 ** e, 2.0 ** e)
        w[r, c[9]] = (6.0 + 2.0 ** -8) * 2.0 ** e  # the fp16 numbers of [4, 8) are 2^-8 apart
    r, c = block("zero")
    w[r, c] = 0.0
    r, c = block("single")
    w[r, c] = 0.0
    w[r, c[13]] = -0.3
    r, c = block("huge")
    w[r, c[4]] = 3.2e38
    w[r, c[20]] = np.inf
    return p


def fraction_params():
    """Every block of every phase [1, 1/16, 1/16, ...]: 31 of a block's 32 non-zero heads are below 1/8 of its largest (29 of 30 in a
    block of the encodings, whose last two elements are padding)."""
    p = zero_params()
    for ph, name in ((0, "fc1_w"), (1, "fc2_w"), (2, "feature_w"), (3, "view_w")):
        pc = S.phase_cols(ph)
        w = p[name]
        for b in range(S.PH_NB[ph]):
            for kh in range(2):
                c = pc[b, kh]
                c = c[c >= 0]
                if c.size:
                    w[:, c] = 1.0 / 16.0
                    w[:, c[0]] = 1.0
    p["latent_w"][:, :256] = np.eye(256, dtype=np.float32)
    p["view_w"][:, :256] = 0.0
    p["view_w"][:, :128] = np.eye(128, dtype=np.float32)
    return p


FRACTION_COUNTS = [256 * 8 * 31, 256 * 8 * 32, 256 * 8 * 31, 256 * 8 * 32, 128 * (8 * 31 + 3 * 29), 128 * (8 * 32 + 3 * 30)]
