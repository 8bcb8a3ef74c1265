"""Inputs that drive known activations into each f16f6 layer phase of the march (tests/test_f16f6_model_host.py,
tests/test_gpu_f16f6_phases.py) and make its outputs readable through the product ABI.  CPU only; nothing here touches the library.

The scene.  Pose R = I, Th = 0, bounds_min = 0, voxel size 2^-5 (2^-2 for the encodings' cases), out_sh = 8 and a level-0 volume of
9^3 voxels: a point (x, y, z) 2^-5 with integer x, y, z lands on voxel (z, y, x) of level 0 with trilinear weights 1, 0, 0 ...,
every step of grid_coords / unnorm_s exact.  fc_0 is a SELECTION: feature f reads level-0 channel f % 32 with a power-of-two gain
2^gexp[f] (or 0) and nothing of the other levels, so the first layer's output is H1[f, s] = 2^gexp[f] V[voxel of s, f % 32]: chosen per
point, different for every sample of a 64-point group.  The 64 points of a group are a 4 x 4 x 4 block of voxels: with the
neighbours the trilinear footprint reaches, the group's voxel list is 5^3 + 3 x 2^3 = 149 entries, marched in two passes of the list.

The chain.  The tested phase carries the case's weights; fc_1 / fc_2 ahead of it are the identity (a lattice activation passes
unchanged: its bf6 remainder is lossless); layers behind it are the identity too and are modelled like any other (tests/f16f6_model).
The colour head is feature_w alone (latent_w[:, :256] = I, view_w[:, :128] = I).  Observation: alpha_fc one-hot on row r reads row r of
relu(fc_2's accumulators) in fp32 (density-only mode: straight from fc_2's registers); rgb_fc one-hot on rows 3 g .. 3 g + 2 reads the
colour head's accumulators.  `observe()` makes the parameter set of one such read-out.

EXACT cases (zero tolerance): activations X_h in {4, 5, 6, 7} 2^e (some halved), X_l in {1, 2, 3} 2^(e-13) > 0; weights
W_h in +-{1, 1.5, 2, 3, 4, 6} 2^f, W_l in {0.5, 0.75, 1, 1.5} 2^(f-12) with the head's sign, 8 per row — one in each of the row's eight
(row, half-block) scale blocks, every column hit.  The column's gain exponent is taken out of the weight (f = c_row - gexp[column]), so
all products of a (row, sample) lie on one grid, 2^(e + c_row - 15), and their sum stays below 2^24 units (at most 8 x 7 x 6 x 2^15 =
2^23.4): every partial sum in any order is an fp32 number, and heads, both four-bit terms and both bf6 forms are lossless
(test_f16f6_model_host.py checks all of this from the model).  The exponents differ per sample (e), per half-block (gexp), per row
(c_row) and per term, so every scale byte of a (row, half-block, term) and every block exponent of a (sample, half-block) has a value
of its own among its neighbours.
"""
import numpy as np

from tests import f16f6_model as M
from tests import fold_stream_ref as S
from tests import march_operand_cases as K

N0 = 9  # level-0 volume: 9^3 voxels
OUT_SH = (8, 8, 8)
LEVEL_SHAPES = ((N0, N0, N0), (2, 2, 2), (2, 2, 2), (2, 2, 2))
VS_HIDDEN, VS_PE = 2.0 ** -5, 2.0 ** -2
# gain exponent of the half-blocks (block, kh) = (0, 0), (0, 1), (1, 0) ...: three apart, because a weight block's exponent moves by up
# to two with its mantissa (6 2^f and 1 2^f: f and f - 2) and no two scale bytes of a row may coincide
GAIN_HB = (-10, 11, -7, 8, -1, 2, -4, 5)
W_MANT = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
WL_MANT = (0.5, 0.75, 1.0, 1.5)
PHASE_NAME = ("fc_1", "fc_2", "colour head over the hidden units", "colour head over the encodings")


def half_block_of(f):
    """(block, kh) index 2 block + kh of hidden column f (fold_stream_ref.col_hidden)."""
    f = np.asarray(f)
    return 2 * (f // 64) + ((f >> 2) & 1)


def group_voxels(n):
    """Integer (x, y, z) of n points: group g of 64 is the 4 x 4 x 4 block of voxels at 4 (g & 1, (g >> 1) & 1, (g >> 2) & 1)."""
    assert n <= 512
    i = np.arange(n)
    g, j = i // 64, i % 64
    return np.stack([4 * (g & 1) + (j & 3), 4 * ((g >> 1) & 1) + ((j >> 2) & 3), 4 * ((g >> 2) & 1) + (j >> 4)], 1)


def weight_columns(r):
    """The eight columns of row r's non-zeros: one per 32-column group j, alternating half (kh) from group to group, so that the row
    has one weight in each of its eight scale blocks; over the rows every column is hit (8 times for 256 rows)."""
    j = np.arange(8)
    return 32 * j + (r + 4 * j) % 32


class Case(object):
    """name, phase (0..3), kind ('exact' | 'bounded'), params (numpy, alpha_w / rgb_w zero), volumes (four [D, H, W, C] fp32), voxel
    size, pts / viewdir [N, 3] fp32, h1 [256, N] (the first layer's output the scene produces), rows (the observed output rows)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def pe(self):
        return M.positional_encoding(self.pts, self.viewdir)

    def model(self, density_only=False, drop=None):
        return M.decode(self.params, np.zeros(384, np.float32), self.h1, None if density_only else self.pe(), density_only, drop)

    def tested(self, m):
        """(y, abs) of the tested phase from a model() result: [R, N] each."""
        if self.phase < 2:
            return m["phases"][self.phase]["y"], m["phases"][self.phase]["abs"]
        return m["y_colour"], m["abs_colour"]

    def expected(self, m):
        """What the read-outs show, [R, N] float64: relu of fc_2's fp32 accumulators (phases 0, 1) or of the colour head's."""
        return (m["h3"] if self.phase < 2 else m["view"]).astype(np.float64)


def base_params():
    p = K.zero_params()
    p["fc1_w"] = np.eye(256, dtype=np.float32)
    p["fc2_w"] = np.eye(256, dtype=np.float32)
    p["latent_w"][:, :256] = np.eye(256, dtype=np.float32)
    p["view_w"][:, :128] = np.eye(128, dtype=np.float32)
    return p


def observe(params, phase, row):
    """The parameter set of one read-out: phases 0, 1 — alpha_fc one-hot on `row`; phases 2, 3 — rgb_fc one-hot on row, row + 1,
    row + 2 (rows beyond 127 dropped).  The other head is zero."""
    p = dict(params)
    if phase < 2:
        p["alpha_w"] = np.zeros((1, 256), np.float32)
        p["alpha_w"][0, row] = 1.0
    else:
        p["rgb_w"] = np.zeros((3, 128), np.float32)
        for ch in range(3):
            if row + ch < 128:
                p["rgb_w"][ch, row + ch] = 1.0
    return p


def readout_rows(phase, rows):
    """The `row` arguments of observe() that cover `rows`, and per read-out the (output column, row) pairs it yields."""
    if phase < 2:
        return [(r, [(3, r)]) for r in rows]
    starts = sorted(set(3 * (r // 3) for r in rows))
    return [(s, [(ch, s + ch) for ch in range(3) if s + ch < 128 and s + ch in set(rows)]) for s in starts]


def _scene(case_kw, gexp, gain_on, chan_vals, n, vs):
    """fc_0, the volumes, the points and H1 of n samples whose level-0 channels are chan_vals [n, 32] (fp32)."""
    fc0 = np.zeros((256, 352), np.float32)
    f = np.arange(256)
    fc0[f, f % 32] = np.where(gain_on, np.ldexp(1.0, gexp), 0.0)
    vox = group_voxels(n)
    vols = [np.zeros(s + (c,), np.float32) for s, c in zip(LEVEL_SHAPES, K.LEVEL_C)]
    vols[0][vox[:, 2], vox[:, 1], vox[:, 0]] = chan_vals
    case_kw["params"]["fc0_w"] = fc0
    case_kw.update(volumes=vols, voxel_size=vs, pts=(vox * vs).astype(np.float32),
                   h1=(fc0[f, f % 32][:, None] * chan_vals[:, f % 32].T).astype(np.float32))


# --------------------------------------------------------------------------------------------------------------------- EXACT
EXACT_VARIANTS = ("full", "wl0", "xl0", "cancel", "edge", "ties")


def exact_case(phase, variant, n=64, seed=0, rows=None):
    """An EXACT case of a hidden-input phase (0: fc_1, 1: fc_2, 2: the colour head over the hidden units).
       full    the recipe of the module docstring
       wl0     W_l = 0, X_l != 0          xl0   X_l = 0, W_l != 0
       cancel  X_h the same for every column of a sample and the heads of a row +-pairs: the main products cancel, the cross terms
               are the whole output
       edge    half-block (1, 1) all zero (gain 0); every fourth sample's heads all 4 2^e or 2 2^e (the block maximum a power of
               two); channels 2 and 5 of block 2 carry 4 2^(e-7): 2^7 below the block maximum, bf6 subnormals
       ties    heads on the bf6 midpoints 9, 11, 13, 15 (x 2^(t-127)) and, where the tested phase reads H1 itself (phase 0),
               remainders on the midpoints 1.125, 1.375: ties to even give 8, 12, 12, 16 and 1.0, 1.5.  (Behind an identity layer a
               remainder has been through bf6 once and lies on its grid: phases 1 and 2 see the head ties only.  publish_s converts
               every hidden layer's input with the same code; the encodings' own conversion gets both kinds in exact_pe_case.)"""
    assert phase in (0, 1, 2) and variant in EXACT_VARIANTS
    rs = np.random.RandomState(1000 * phase + 17 * EXACT_VARIANTS.index(variant) + seed)
    R = S.PH_ROWS[phase]
    f = np.arange(256)
    hb = half_block_of(f)
    gexp = np.asarray(GAIN_HB)[hb]
    gain_on = np.ones(256, bool)
    mh = rs.choice([4.0, 5.0, 6.0, 7.0], size=(n, 32))
    mh = np.where(rs.rand(n, 32) < 0.25, mh / 2, mh)
    ml = rs.choice([1.0, 2.0, 3.0], size=(n, 32))
    e_s = rs.randint(-1, 2, size=n)
    if variant == "xl0":
        ml[:] = 0.0
    if variant == "cancel":
        mh = np.repeat(rs.choice([4.0, 5.0, 6.0, 7.0], size=(n, 1)), 32, 1)
    if variant == "edge":
        gain_on[hb == 3] = False
        mh[1::4] = np.where(rs.rand(*mh[1::4].shape) < 0.5, 4.0, 2.0)
        mh[1::4, ::4] = 4.0  # every half of the channels holds one
        sub = (f // 64 == 2) & np.isin(f % 32, (2, 5))
        gexp = np.where(sub, gexp - 7, gexp)
        mh[:, (2, 5)] = 4.0
        ml[:, (2, 5)] = 0.0
    if variant == "ties":
        tie = rs.rand(n, 32) < 0.5
        mh = np.where(tie, rs.choice([4.5, 5.5, 6.5, 7.5], size=(n, 32)), rs.choice([4.0, 6.0], size=(n, 32)))
        ml = np.where(rs.rand(n, 32) < 0.5, rs.choice([2.25, 2.75], size=(n, 32)), rs.choice([0.0, 1.0, 2.0], size=(n, 32)))
        mh[:, ::4] = np.maximum(mh[:, ::4], 4.0)
    chan = ((mh + ml * 2.0 ** -13) * np.ldexp(1.0, e_s)[:, None]).astype(np.float32)
    # weights
    c_row = rs.randint(-1, 2, size=R)
    W = np.zeros((R, 256), np.float64)
    for r in range(R):
        cols = weight_columns(r)
        m = rs.choice(W_MANT, size=8)
        l = rs.choice(WL_MANT, size=8)
        sgn = np.where(rs.rand(8) < 0.25, -1.0, 1.0)
        if variant == "wl0":
            l[:] = 0.0
        if variant == "cancel":
            m[1::2] = m[0::2]
            sgn[0::2] = np.where(rs.rand(4) < 0.5, -1.0, 1.0)
            sgn[1::2] = -sgn[0::2]
        W[r, cols] = sgn * (m + l * 2.0 ** -12) * np.ldexp(1.0, c_row[r] - gexp[cols])
    W32 = W.astype(np.float32)
    assert (W32.astype(np.float64) == W).all()
    p = base_params()
    if phase == 2:
        p["feature_w"] = np.zeros((256, 256), np.float32)
        p["feature_w"][:128] = W32
    else:
        p[("fc1_w", "fc2_w")[phase]] = W32
    kw = dict(name="%s-%s" % (("fc1", "fc2", "colour")[phase], variant), phase=phase, kind="exact", variant=variant, params=p,
              rows=list(range(R)) if rows is None else list(rows), viewdir=np.tile(np.float32([0, 0, 1]), (n, 1)))
    _scene(kw, gexp, gain_on, chan, n, VS_HIDDEN)
    return Case(**kw)


PE_VARIANTS = ("full", "wl0", "xl0", "ties")
PE_X_COL = tuple(S.pe_slot_col(a, 0) for a in range(3))   # view_fc columns of x_a
PE_V_COL = tuple(S.pe_slot_col(a, 21) for a in range(3))  # ... and of v_a


def _pe_scene(kw, x, v, n):
    p = kw["params"]
    p["fc0_w"] = np.zeros((256, 352), np.float32)
    vols = [np.zeros(s + (c,), np.float32) for s, c in zip(LEVEL_SHAPES, K.LEVEL_C)]
    kw.update(volumes=vols, voxel_size=VS_PE, pts=x.astype(np.float32), viewdir=v.astype(np.float32), h1=np.zeros((256, n), np.float32))


def exact_pe_case(variant="full", n=64, seed=0, rows=None):
    """The colour head over the encodings: only the x and v slots (0 and 21 of each axis' half-block) have weights; point coordinates
    and view direction components in [1, 2) on the lattice {4 .. 7} 2^-2 + {1, 2, 3} 2^-15 (the sines and cosines stay below them, so
    the half-block maximum is x_a or v_a); the hidden units are zero (fc_0 = 0) and so is feature_w.  'ties': heads and remainders
    on bf6 midpoints, as in exact_case."""
    assert variant in PE_VARIANTS
    rs = np.random.RandomState(3000 + 17 * EXACT_VARIANTS.index(variant) + seed)
    ml = rs.choice([1.0, 2.0, 3.0], size=(2, n, 3)) * (variant != "xl0")
    mh = rs.choice([4.0, 5.0, 6.0, 7.0], size=(2, n, 3))
    if variant == "ties":  # x 2^-2 / 2^-3: the heads 9, 11, 13, 15 and the remainders 1.125, 1.375 of exact_case's ties
        mh = np.where(rs.rand(2, n, 3) < 0.5, rs.choice([4.5, 5.5, 6.5, 7.5], size=(2, n, 3)), rs.choice([4.0, 6.0], size=(2, n, 3)))
        ml = np.where(rs.rand(2, n, 3) < 0.5, rs.choice([2.25, 2.75], size=(2, n, 3)), rs.choice([0.0, 1.0, 2.0], size=(2, n, 3)))
    xv = (mh + ml * 2.0 ** -13) * 0.25
    c_row = rs.randint(-1, 2, size=128)
    p = base_params()
    for r in range(128):
        m, l = rs.choice(W_MANT, size=6), rs.choice(WL_MANT, size=6) * (variant != "wl0")
        sgn = np.where(rs.rand(6) < 0.2, -1.0, 1.0)
        p["view_w"][r, list(PE_X_COL + PE_V_COL)] = sgn * (m + l * 2.0 ** -12) * 2.0 ** c_row[r]
    kw = dict(name="pe-%s" % variant, phase=3, kind="exact", variant=variant, params=p, rows=list(range(128)) if rows is None else list(rows))
    _pe_scene(kw, xv[0], xv[1], n)
    return Case(**kw)


# ------------------------------------------------------------------------------------------------------------------- BOUNDED
# |got - model| <= BOUNDED_FACTOR 2^-24 sum |terms|.  BOUNDED_MEASURED is the largest ratio |got - model| / (2^-24 sum |terms|) of the
# unmutated kernel on the MI355X over the three BOUNDED cases (tests/test_gpu_f16f6_phases.py prints it per case); the factor is four
# times that: the margin is for other summation orders on other inputs.  Two conditions hold whatever was measured
# (test_f16f6_model_host.py): the factor stays below 2^8 (2^-16 sum |terms|: 256 worst-case roundings) and the tolerance below one
# eighth of the shift the model shows when either cross term of the tested phase is removed (the median over the case's read-outs: a
# single read-out's shift can be anything down to zero, its cross products cancelling by chance).
# Measured: fc_2 2.44, colour head over the hidden units 0.79, over the encodings 1.08.
BOUNDED_MEASURED = 2.44
BOUNDED_FACTOR = 4.0 * BOUNDED_MEASURED
BOUNDED_ROWS = {1: tuple(range(7, 256, 16)), 2: (0, 1, 2, 33, 34, 35, 66, 67, 68, 99, 100, 101), 3: (0, 1, 2, 33, 34, 35, 66, 67, 68, 99, 100, 101)}


def _head_plus_remainder(rs, shape, lo, hi):
    """fp32 values head + rem: head an fp16 number with lo <= head < hi whose lowest mantissa bit is set (a number of 11 significant
    bits is no midpoint of a three-bit grid, and below the block's subnormal step its odd unit is finer than any midpoint), rem > 0
    between 0.05 and 0.45 of half an fp16 ulp of the head (the head is what fp16 rounding returns, the remainder has one sign; passed
    through an identity layer it becomes a bf6 number of the same block exponent: on the grid, not between two of its points — and
    still below half an ulp: bf6 rounds a normal up by at most 1/8 and an element 2^5 .. 2^7 below the block's largest by at most
    half the subnormal step, a quarter to one ulp-half of such an element)."""
    head = (rs.uniform(lo, hi, size=shape).astype(np.float16).view(np.uint16) | 1).view(np.float16).astype(np.float64)  # 11 bits used
    ulp = np.ldexp(1.0, np.floor(np.log2(head)).astype(np.int64) - 10)
    x = (head + rs.uniform(0.05, 0.45, size=shape) * ulp / 2).astype(np.float32)
    assert (x.astype(np.float16).astype(np.float64) == head).all() and (x.astype(np.float64) > head).all()
    return x


def _no_midpoints(split, cols):
    s = split
    return not (M.is_e3m2_midpoint(s["xx_scaled"][cols]).any() or M.is_e3m2_midpoint(s["xl_scaled"][cols]).any())


def tested_input_split(case, m=None):
    """The activation split the TESTED phase of a case sees (from the model)."""
    m = m or case.model()
    return m["phases"][case.phase]["split"]


def bounded_case(phase, n=64, seed=0):
    """Realistic magnitudes: the tested phase's weights from normal_params (256 non-zeros per row; phase 3: the six x / v columns),
    its inputs constructed as head + one-signed remainder with none on a bf6 midpoint (seeds are advanced until the model says so).
    Only phases whose accumulators a VALU head reads in fp32: fc_2 (1) and the two colour-head phases (2, 3)."""
    assert phase in (1, 2, 3)
    for attempt in range(50):
        rs = np.random.RandomState(5000 + 100 * phase + seed + 1000 * attempt)
        q = K.normal_params(77 + phase + seed)
        p = base_params()
        kw = dict(name="bounded-%s" % ("fc1", "fc2", "colour", "pe")[phase], phase=phase, kind="bounded", variant="bounded", params=p,
                  rows=list(BOUNDED_ROWS[phase]))
        if phase == 3:
            live = list(PE_X_COL + PE_V_COL)
            p["view_w"][:, live] = q["view_w"][:, live]
            _pe_scene(kw, _head_plus_remainder(rs, (n, 3), 1.0, 2.0), _head_plus_remainder(rs, (n, 3), 1.0, 2.0), n)
        else:
            if phase == 1:
                p["fc2_w"] = q["fc2_w"]
            else:
                p["feature_w"] = q["feature_w"]
            kw["viewdir"] = np.tile(np.float32([0, 0, 1]), (n, 1))
            gexp = rs.randint(-1, 2, size=256)
            _scene(kw, gexp, np.ones(256, bool), _head_plus_remainder(rs, (n, 32), 0.05, 2.0), n, VS_HIDDEN)
        case = Case(**kw)
        cols = np.arange(256) if phase < 3 else np.asarray(PE_X_COL + PE_V_COL)
        if _no_midpoints(tested_input_split(case), cols):
            return case
    raise AssertionError("no midpoint-free input found")


# --------------------------------------------------------------------------------------------------------- the folded first layer
def fold_case(kind, n=64, seed=0):
    """The folded first layer's three products U_h . Wt_h + U_h . Wt_l + U_l . Wt_h, observed through identity layers (alpha_fc
    one-hot).  Every point is offset from its voxel along ONE axis (sample s: axis s % 3), so its two non-zero trilinear weights are
    exact products (1 - t) . 1 . 1 and t . 1 . 1:
       'u_rem'   U with a remainder (the EXACT lattice), dyadic weights t in {1/4, 1/2, 3/4}
       'wt_rem'  t = 1/2 + 2^-13 (head 1/2, remainder 2^-13; 1 - t: head 1/2, remainder -2^-13), U head-only.
    H1 = (1 - t) U[voxel] + t U[voxel + 1 along the axis]; the neighbour voxels along x, y, z of a sample are other samples' voxels or
    carry values of their own (group 0's neighbours at index 4 are filled as well).  All sums exact in fp32."""
    assert kind in ("u_rem", "wt_rem")
    rs = np.random.RandomState(7000 + seed + (kind == "wt_rem"))
    f = np.arange(256)
    gexp = np.asarray(GAIN_HB)[half_block_of(f)]
    # the volume: every voxel of [0, 5)^3 filled (the 4^3 block and its upper neighbours)
    mh = rs.choice([4.0, 5.0, 6.0, 7.0], size=(5, 5, 5, 32))
    ml = rs.choice([1.0, 2.0, 3.0], size=(5, 5, 5, 32)) * (kind == "u_rem")
    vol0 = np.zeros((N0, N0, N0, 32), np.float32)
    vol0[:5, :5, :5] = (mh + ml * 2.0 ** -13).astype(np.float32)
    vox = group_voxels(n)
    assert n <= 64
    axis = np.arange(n) % 3
    t = rs.choice([0.25, 0.5, 0.75], size=n) if kind == "u_rem" else np.full(n, 0.5 + 2.0 ** -13)
    off = np.zeros((n, 3))
    off[np.arange(n), axis] = t
    nb = vox.copy()
    nb[np.arange(n), axis] += 1
    v0 = vol0[vox[:, 2], vox[:, 1], vox[:, 0]].astype(np.float64)
    v1 = vol0[nb[:, 2], nb[:, 1], nb[:, 0]].astype(np.float64)
    chan = (1.0 - t)[:, None] * v0 + t[:, None] * v1
    p = base_params()
    fc0 = np.zeros((256, 352), np.float32)
    fc0[f, f % 32] = np.ldexp(1.0, gexp)
    p["fc0_w"] = fc0
    h1 = fc0[f, f % 32].astype(np.float64)[:, None] * chan[:, f % 32].T
    h32 = h1.astype(np.float32)
    assert (h32.astype(np.float64) == h1).all()
    vols = [vol0] + [np.zeros(s + (c,), np.float32) for s, c in zip(LEVEL_SHAPES[1:], K.LEVEL_C[1:])]
    pts = ((vox + off) * VS_HIDDEN).astype(np.float32)
    assert (pts.astype(np.float64) == (vox + off) * VS_HIDDEN).all()
    return Case(name="fold-%s" % kind, phase=1, kind="exact", variant=kind, params=p, volumes=vols, voxel_size=VS_HIDDEN, pts=pts,
                viewdir=np.tile(np.float32([0, 0, 1]), (n, 1)), h1=h32, rows=list(range(5, 256, 8)), t=t)


# ------------------------------------------------------------------------------------------------------------------ the lists
_CACHE = {}


def get(key):
    """Cases by key, built once: ('exact', phase, variant) | ('bounded', phase) | ('fold', kind) | ('core', phase)."""
    if key not in _CACHE:
        if key[0] == "exact":
            _CACHE[key] = exact_pe_case(key[2]) if key[1] == 3 else exact_case(key[1], key[2], n=128 if key[2] == "full" else 64,
                                                                                rows=None if key[2] == "full" else VARIANT_ROWS[key[1]])
        elif key[0] == "bounded":
            _CACHE[key] = bounded_case(key[1])
        elif key[0] == "fold":
            _CACHE[key] = fold_case(key[1])
        elif key[0] == "core":  # the small core every instantiation of the kernel runs: fc_1 then fc_2 read through 16 rows
            _CACHE[key] = exact_case(key[1], "full", n=64, seed=5, rows=VARIANT_ROWS[key[1]])
    return _CACHE[key]


# the variants read 16 (colour head: 12) rows: every wave, both tiles of a wave, both halves of a tile, accumulator registers 0..15
VARIANT_ROWS = {0: tuple(16 * i + (5 * i) % 16 for i in range(16)), 1: tuple(16 * i + (5 * i + 3) % 16 for i in range(16)),
                2: (0, 1, 2, 39, 40, 41, 78, 79, 80, 117, 118, 119)}
EXACT_KEYS = tuple(("exact", ph, v) for ph in (0, 1, 2) for v in EXACT_VARIANTS) + tuple(("exact", 3, v) for v in PE_VARIANTS)
BOUNDED_KEYS = tuple(("bounded", ph) for ph in (1, 2, 3))
FOLD_KEYS = (("fold", "u_rem"), ("fold", "wt_rem"))
CORE_KEYS = (("core", 0), ("core", 1), ("core", 2))
