"""Inputs and float64 references for the per-kernel tests of the sparse 3x3x3 convolutions (tests/test_encoder_kernel_cases_host.py,
tests/test_gpu_encoder_kernels.py).  CPU only; nothing here touches the library.

LATTICE inputs make the answer exact.  The 16-bit kernels compute a_h w_h + a_h w_l + a_l w_h per product (the remainder x remainder
term is dropped by design) and accumulate in fp32.  With every operand drawn from {0, +-1, +-1 +- 2^-12} (a non-zero remainder only
beside a non-zero head) the products are +-1 and +-2^-12, and while  sum |a| |w| < 2^24 units of 2^-12  every partial sum in any
order is an fp32 number: a correct kernel equals the float64 reference bit for bit.  The fp32 kernels get integers in -3 .. 3 (unit 1).
`assert_lattice(S, unit)` is that precondition, a condition on the inputs taken from the float64 reference.

REALISTIC inputs (relu of normals, N(0, 1 / (27 Cin)) weights, gradients over 2^-20 .. 2^4) are compared element by element with the
float64 product of the UNSPLIT values within  c * S,  S = sum |a| |w|  of that element; the worst-case c of each arithmetic:
  fp16 pairs   2^-20 + (81 Cin / 16 + 8) 2^-24   (two operands at 2^-22 each and the dropped term 2^-22, rounded up to 2^-20; one
               fp32 rounding per MFMA = 27 offsets x Cin / 16 chunks x 3 products, and the 8 partial tiles of the offset-split kernel)
  bf16 pairs   2^-15 + the same accumulation term   (16 mantissa bits a pair)
  fp32         27 Cin 2^-23   (two roundings per term)
and for the weight gradient, whose reduction runs over the n live rows:
  bf16 pairs   2^-15 + (3 ceil(n / 16) + ceil(n / 1024) + 8) 2^-24   (three MFMAs per 16 rows, one atomic per 1024-row workgroup)
  fp32         max(n, 1) 2^-23
"""
import functools
import math

import numpy as np
import torch

from oracle.spconv_rulebook import apply_rulebook, sparse_rulebook, subm_rulebook

GRID = (9, 10, 11)
BIG_GRID = (12, 12, 15)
REM = 2.0 ** -12  # the lattice's remainder = its unit
ISOLATED = (4, 7, 8)

# the (Cin, Cout) pairs of NB_FOR_CONV_SHAPES; those the 16-bit kernels take (both sides >= 32), forward and as backward-input products
ALL_PAIRS = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))
PAIRS16 = tuple(p for p in ALL_PAIRS if min(p) >= 32)
REVERSED16 = ((64, 32), (128, 64))
# the three capacity classes of the 16-bit forward tests: None = the live row count (offset-split kernel), two beyond its 4096-row limit
CAPACITIES = (None, 4224, 65536)


# ----------------------------------------------------------------------------------------------------------------- active sets
def _sorted_unique(coord, dhw):
    lin = np.unique(np.ravel_multi_index(np.asarray(coord, np.int64).T, dhw))
    return np.stack(np.unravel_index(lin, dhw), 1).astype(np.int32)


def active_set():
    """int32 [N, 3] (z, y, x) on GRID in linear order, N ~ 300: the eight corners, one ISOLATED voxel (only the centre offset is live),
    a dense 4 x 4 x 4 block (all 27 offsets live inside), a line of 9 voxels along z, and a seeded scatter."""
    D, H, W = GRID
    pts = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    pts += [ISOLATED]
    pts += [(z, y, x) for z in range(2, 6) for y in range(1, 5) for x in range(1, 5)]
    pts += [(z, 7, 2) for z in range(D)]
    fixed = set(pts)
    near_isolated = {(ISOLATED[0] + a, ISOLATED[1] + b, ISOLATED[2] + c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)}
    free = [c for c in np.ndindex(*GRID) if c not in fixed and c not in near_isolated]
    rs = np.random.RandomState(11)
    pts += [free[i] for i in rs.choice(len(free), 300 - len(fixed), replace=False)]
    return _sorted_unique(pts, GRID)


def bigger_active_set():
    """2049 of the 2160 voxels of BIG_GRID, in linear order: past 256 rows per wave and 1024 rows per workgroup of the weight gradient,
    with a lone last row."""
    rs = np.random.RandomState(12)
    lin = np.sort(rs.choice(int(np.prod(BIG_GRID)), 2049, replace=False))
    return np.stack(np.unravel_index(lin, BIG_GRID), 1).astype(np.int32)


class Geometry:
    """One (active set, stride): the input rows' linear indices, the output rows' (linear order, the order of the device's index
    sets), and the rulebook pairs per kernel offset as int64 [n_o, 2] = (input row, output row)."""

    def __init__(self, coord, dhw, stride):
        self.in_dhw, self.stride = tuple(int(s) for s in dhw), stride
        self.n_in = len(coord)
        self.in_lin = np.ravel_multi_index(coord.astype(np.int64).T, dhw).astype(np.int32)
        assert np.all(np.diff(self.in_lin) > 0), "rows in linear order, no duplicates"
        idx = np.concatenate([np.zeros((len(coord), 1), np.int64), coord.astype(np.int64)], 1)
        if stride == 1:
            keys, pairs = subm_rulebook(idx, dhw)
            self.out_dhw = self.in_dhw
        else:
            keys, out_shape, pairs = sparse_rulebook(idx, dhw)
            self.out_dhw = tuple(int(s) for s in out_shape)
        lin = np.ravel_multi_index(keys[:, 1:].T, self.out_dhw)
        order = np.argsort(lin)  # the rulebook numbers output voxels as it meets them, the device in linear order
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        self.out_lin = lin[order].astype(np.int32)
        self.n_out = len(lin)
        self.pairs = [np.stack([p[:, 0], rank[p[:, 1]]], 1) if len(p) else p for p in pairs]

    def in_grid(self):
        g = np.full(int(np.prod(self.in_dhw)), -1, np.int32)
        g[self.in_lin] = np.arange(self.n_in, dtype=np.int32)
        return g.reshape(self.in_dhw)

    def out_grid(self):
        g = np.full(int(np.prod(self.out_dhw)), -1, np.int32)
        g[self.out_lin] = np.arange(self.n_out, dtype=np.int32)
        return g.reshape(self.out_dhw)

    def swapped_pairs(self):
        return [p[:, ::-1] if len(p) else p for p in self.pairs]


@functools.lru_cache(maxsize=None)
def geometry(which, stride):
    """which: "small" (active_set on GRID) or "big" (bigger_active_set on BIG_GRID)."""
    return Geometry(active_set(), GRID, stride) if which == "small" else Geometry(bigger_active_set(), BIG_GRID, stride)


def pad_lin(lin, cap):
    """`lin` extended to `cap` entries with repeats of its own (valid) voxels: rows beyond the live count must not be computed, and if
    a kernel did compute one it still reads nothing out of range."""
    lin = np.asarray(lin, np.int32)
    return lin[np.arange(max(int(cap), len(lin))) % len(lin)].copy()


def row_counts(n_all, counts=(0, 1, 31, 32, 33, 127, 128, 129)):
    """the live row counts a test loops over: tile edges, and all rows (counts beyond the set are left out, `n_all` is always there)"""
    return [n for n in counts if n < n_all] + [n_all]


# ----------------------------------------------------------------------------------------------------------------- generators
def lattice16(rs, shape):
    """fp32 values in {0, +-1, +-1 +- 2^-12}: a quarter zeros; a remainder only beside a head"""
    head = rs.choice([-1.0, 1.0], size=shape) * (rs.uniform(size=shape) >= 0.25)
    rem = rs.choice([-REM, 0.0, REM], size=shape) * (head != 0)
    return (head + rem).astype(np.float32)


def lattice32(rs, shape):
    return rs.randint(-3, 4, size=shape).astype(np.float32)


def realistic_rows(rs, shape):
    return np.maximum(rs.standard_normal(shape), 0.0).astype(np.float32)


def realistic_weight(rs, cin, cout):
    return (rs.standard_normal((3, 3, 3, cin, cout)) / math.sqrt(27 * cin)).astype(np.float32)


def wide_gradients(rs, shape):
    """magnitudes over 2^-20 .. 2^4, random signs"""
    return (rs.choice([-1.0, 1.0], size=shape) * np.exp2(rs.uniform(-20.0, 4.0, size=shape))).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- splits
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def split(x, kind):
    """torch's own rounding on the CPU: head = x.to(dtype), remainder = (x - head).to(dtype) -> two float64 arrays"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    h = x.to(DTYPES[kind])
    l = (x - h.float()).to(DTYPES[kind])
    return h.double().numpy(), l.double().numpy()


def split_planes(x, kind, cap=None):
    """int16 [2, cap, C]: the bits of the head and remainder planes of rows x [n, C]; rows beyond n hold NaNs (nothing may read them)"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    n, c = x.shape
    cap = n if cap is None else int(cap)
    planes = torch.full((2, max(cap, 1), c), float("nan"), dtype=DTYPES[kind])
    planes[0, :n] = x.to(DTYPES[kind])
    planes[1, :n] = (x - planes[0, :n].float()).to(DTYPES[kind])
    return planes.view(torch.int16)


def planes_to_float(planes, kind):
    """int16 planes [2, n, C] -> (heads, remainders) as fp32 tensors"""
    p = planes.view(DTYPES[kind]).float()
    return p[0], p[1]


# ----------------------------------------------------------------------------------------------------------------- references
def _w27(w):
    return np.asarray(w, np.float64).reshape(3, 3, 3, w.shape[-2], w.shape[-1])


def conv_ref(geo, a, w, n=None):
    """float64 forward convolution, output rows [:n]"""
    out = apply_rulebook(np.asarray(a, np.float64), _w27(w), geo.n_out, geo.pairs)
    return out[:geo.n_out if n is None else n]


def bwd_input_ref(geo, dx, w, n=None):
    """float64 backward-input product: the scatter-add of dx @ W[o]^T over the forward pairs, input rows [:n]"""
    wt = np.swapaxes(_w27(w), 3, 4)
    out = apply_rulebook(np.asarray(dx, np.float64), wt, geo.n_in, geo.swapped_pairs())
    return out[:geo.n_in if n is None else n]


def bwd_weight_ref(geo, a, dx, n=None, rows=None):
    """float64 weight gradient sum_pairs in^T (x) dx over the output rows [:n] (or rows[0] .. rows[1] - 1) -> [3, 3, 3, Cin, Cout]"""
    a, dx = np.asarray(a, np.float64), np.asarray(dx, np.float64)
    lo, hi = rows if rows is not None else (0, geo.n_out if n is None else n)
    dw = np.zeros((27, a.shape[1], dx.shape[1]))
    for o, p in enumerate(geo.pairs):
        if len(p):
            p = p[(p[:, 1] >= lo) & (p[:, 1] < hi)]
            dw[o] = a[p[:, 0]].T @ dx[p[:, 1]]
    return dw.reshape(3, 3, 3, a.shape[1], dx.shape[1])


def three_products(ref, a_parts, b_parts):
    """what the matrix-pipe kernels compute: ref(a_h, b_h) + ref(a_h, b_l) + ref(a_l, b_h) — not ref(a_h + a_l, b_h + b_l)"""
    (ah, al), (bh, bl) = a_parts, b_parts
    return ref(ah, bh) + ref(ah, bl) + ref(al, bh)


def assert_lattice(S, unit):
    """the precondition of the exact comparison: every partial sum, in any order, is an fp32 number"""
    m = float(np.max(S, initial=0.0)) / unit
    assert m < 2 ** 24, "lattice precondition: sum |a| |w| = %.0f units" % m


# ----------------------------------------------------------------------------------------------------------------- bounds
def c_pairs16(kind, cin):
    return (2.0 ** -20 if kind == "fp16" else 2.0 ** -15) + (81 * cin / 16 + 8) * 2.0 ** -24


def c_fp32(cin):
    return 27 * cin * 2.0 ** -23


def c_weight16(n):
    return 2.0 ** -15 + (3 * math.ceil(n / 16) + math.ceil(n / 1024) + 8) * 2.0 ** -24


def c_weight32(n):
    return max(n, 1) * 2.0 ** -23


def worst_ratio(got, ref, S):
    """max |got - ref| / S over the elements with S > 0; where S == 0 the result must be exactly zero"""
    got, ref, S = (np.asarray(v, np.float64) for v in (got, ref, S))
    assert np.all(got[S == 0] == 0), "a non-zero result where no term contributes"
    live = S > 0
    return float(np.max(np.abs(got[live] - ref[live]) / S[live], initial=0.0))


# ----------------------------------------------------------------------------------------------------------------- the GPU cases
# 16-bit forward: (Cin, Cout, stride) — every pair at stride 1, the pairs of the strided layers at stride 2 as well
FORWARD16 = tuple((ci, co, 1) for ci, co in PAIRS16) + ((32, 64, 2), (64, 128, 2), (128, 128, 2))
# 16-bit backward-input: the LAYER's (Cin, Cout, stride); the packed convolution runs Cout -> Cin, a strided layer with stride = -2
BWD_INPUT16 = ((32, 32, 1), (64, 64, 1), (128, 128, 1), (32, 64, 2), (64, 128, 2), (128, 128, 2))
# the kernel nb_enc_conv16 runs per (Cin, Cout) of the convolution it is given, for the three CAPACITIES
VARIANTS = {
    (32, 32): ("KS", "WAVE_ALL_TILES", "WAVE_ALL_TILES"),
    (32, 64): ("KS", "WAVE_ONE_TILE", "WAVE_ALL_TILES"),
    (64, 64): ("KS", "LDS_ALL_TILES", "LDS_ALL_TILES"),
    (64, 128): ("KS", "LDS_TWO_TILES", "LDS_ALL_TILES"),
    (128, 128): ("KS", "LDS_TWO_TILES", "LDS_ALL_TILES"),  # 4224: the row stage; 65536: four tiles per wave, rows into registers
    (64, 32): ("KS", "LDS_ALL_TILES", "LDS_ALL_TILES"),
    (128, 64): ("KS", "LDS_ALL_TILES", "LDS_ALL_TILES"),
}


def capacity(cls, live):
    return int(live) if cls is None else cls
