"""Inputs and float64 references for the per-kernel tests of the decoder's backward (tests/test_bwd_kernel_cases_host.py,
tests/test_gpu_backward_kernels.py): the GEMM kernels behind nb_gemm_fused, nb_colsum, nb_relu_bwd, nb_trilinear_bwd.  CPU only;
the generators and the references of tests/spconv_cases.py are reused, not restated.

GEMM LATTICES (each makes the answer an fp32 number in any summation order, so a correct kernel equals the float64 reference bit
for bit; `assert_lattice` on  alpha sum |a| |b| + |C0|  is the precondition, asserted for every case on the CPU first):
  "int"     integers -3 .. 3 (spconv_cases.lattice32), unit 1: exact on every kernel, fp32 and bf16 pairs alike (a head, no remainder);
  "dense"   {0, +-1, +-1 +- 2^-12} (spconv_cases.lattice16), unit 2^-12, for the bf16-pair kernels: the reference is
            three_products of the bf16 splits (a_h b_h + a_h b_l + a_l b_h), NOT the full product;
  "sparse"  {0, +-(1 + 2^-9)}, unit 2^-18: bf16 head 1, remainder 2^-9, so the full product of two values is 1 + 2^-8 + 2^-18 and the
            pair kernels give 1 + 2^-8.  The second operand is zero except on at most KEEP positions of the reduction axis
            (`keep_positions`), so sum |a| |b| <= 40 (1 + 2^-9)^2 < 64 = 2^24 units whatever the reduction length.  Exact on both
            arithmetics with different answers: a case on this lattice also proves which arithmetic ran.
alpha is a power of two (1, 2, 0.5: the unit of the result is alpha x the lattice's), C0 holds integers.

COLUMN SUMS: where sum_rows |C| < 2^24 units the fp32 sum is exact in any order (compared bit for bit: the integer lattice); elsewhere
every one of the at most n_rows additions into a column rounds once, each by at most 2^-24 of a partial sum that sum_rows |C| bounds:
|got - ref| <= n_rows 2^-24 sum_rows |C|  per column.

TRILINEAR: `trilinear_scatter` restates grid_sample's backward (align_corners=True, zeros padding) in float64 and keeps the rows of
the active voxels.  The LATTICE scene (R = I, Th = 0, bounds_min = 0, voxel size and out_sh powers of two, every level's size - 1 a
power of two, points on quarter voxels of the finest level, integer dF) makes every index coordinate, weight and partial sum an fp32
number: bit for bit.  The REALISTIC scene is compared within  c sum |w| |dF|  per element,  c = (6 + 2 K) 2^-24,  K = the largest
number of points that reach one row: a weight is three factors of one rounding each and two multiplications (5 roundings, 6 with
their second-order terms), and every contribution enters a run's register sum by one fma and leaves in at most one atomic addition
(2 K roundings of partial sums that sum |w| |dF| bounds).  Its index coordinates are computed in fp32 by the operations of the kernel
(`fp32_grid`, `unnormalize` with dtype float32, as grid_sample itself does in fp32); weights and sums are float64.
"""
import functools

import numpy as np
import torch

from tests import spconv_cases as sc

VARIANTS = ("SCALE_ONLY", "TN", "TN16", "ROWS", "ROWS_FAST", "ROWS_FAST_T", "ROWS16")
SPARSE = 1.0 + 2.0 ** -9
UNIT = {"int": 1.0, "dense": sc.REM, "sparse": 2.0 ** -18}
KEEP = 40  # live positions of the reduction axis on the sparse lattice
SPECIALS = (0.0, -0.0, float("nan"), 2.0 ** -126, 2.0 ** -140, float("inf"), float("-inf"))  # the values a ReLU mask must decide
GUARD = -7.25  # what the columns beside a destination slice hold


# ----------------------------------------------------------------------------------------------------------------- the GEMM cases
# (variant, trans_a, trans_b, m, k, n, layout): layout = (column offset of A, of B) in floats inside their wider matrices; the row
# strides are multiples of 4 floats unless the offset is odd (then the stride is 2 mod 4 as well)
EPILOGUES = ("none", "mask", "colsum", "mask+colsum+beta")


def rows_cases():
    """(a) the general kernel: K no multiple of 16, or an operand off the 16-byte grid by 4 (A) or 8 (B) bytes"""
    out = []
    for tb in (False, True):
        for m, k, n in ((1, 1, 1), (33, 3, 31), (257, 129, 45)):
            out.append(("ROWS", False, tb, m, k, n, (2, 1)))
        out.append(("ROWS", False, tb, 64, 16, 352, (1, 4)))
        out.append(("ROWS", False, tb, 64, 16, 352, (4, 2)))
    return out


FAST_K = (16, 48, 272)
FAST_N = (1, 127, 128, 130, 352)
FAST_M = {False: (1, 31, 128, 129, 1023), True: (1, 129, 1023, 2050)}


def fast_cases(trans_b, m):
    """(b) the aligned fp32 kernels; K % 32 == 16 keeps op(B) = B off the 16-bit kernel at any m"""
    name = "ROWS_FAST_T" if trans_b else "ROWS_FAST"
    return [(name, False, trans_b, m, k, n, (4, 4)) for k in FAST_K for n in FAST_N]


ROWS16_M = (1024, 1025, 2050)
ROWS16_K = (32, 96, 384)
ROWS16_N = (4, 127, 260, 352)


def rows16_cases(m):
    return [("ROWS16", False, False, m, k, n, (4, 4)) for k in ROWS16_K for n in ROWS16_N]


TN_K = (1, 255, 256, 257, 1023, 2049)
TN_MN = (1, 31, 33, 70)


def tn_cases(k):
    """(d) split-K fp32: fewer than 1024 rows with aligned operands; 2049 rows with A off the 16-byte grid by 4 bytes"""
    return [("TN", True, False, m, k, n, (1, 4) if k >= 1024 else (4, 4)) for m in TN_MN for n in TN_MN]


TN16_K = (1024, 1056, 2049, 3103)
TN16_MN = ((32, 32), (346, 256), (129, 33), (256, 128))


def tn16_cases(k):
    return [("TN16", True, False, m, k, n, (8, 4)) for m, n in TN16_MN]


def split_off_cases():
    """(g) NB_BWD_SPLIT=0: the large shapes of (c) and (e) on the fp32 kernels"""
    return [("ROWS_FAST", False, False, 2050, k, n, (4, 4)) for k in ROWS16_K for n in (260, 352)] + \
           [("TN", True, False, m, k, n, (8, 4)) for k in (2049, 3103) for m, n in TN16_MN]


def all_default_cases():
    out = rows_cases()
    for tb in (False, True):
        for m in FAST_M[tb]:
            out += fast_cases(tb, m)
    for m in ROWS16_M:
        out += rows16_cases(m)
    for k in TN_K:
        out += tn_cases(k)
    for k in TN16_K:
        out += tn16_cases(k)
    return out


def stored_shapes(case):
    """the shapes A and B are stored in"""
    _, ta, tb, m, k, n, _ = case
    return ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))


def wide_width(cols, off):
    """the row stride of `widen`: a multiple of 4 floats for an even offset, 2 mod 4 for an odd one"""
    width = off + cols + 3
    return width + (-width) % 4 + (2 if off % 2 else 0)


def widen(x, off, fill=0.0):
    """x as the column slice [off, off + cols) of a wider fp32 matrix filled with `fill` (`off` = 1: an operand off the 16-byte grid
    by 4 bytes with a row stride no aligned kernel takes; 2: off by 8 bytes with an aligned stride)"""
    rows, cols = x.shape
    wide = np.full((rows, wide_width(cols, off)), fill, np.float32)
    wide[:, off:off + cols] = x
    return wide


def host_view(shape, off):
    """a host tensor with the strides and the alignment that `widen`'s slice has on the device (torch's allocations start on a 64-byte
    boundary on either side)"""
    wide = torch.zeros((max(shape[0], 1), wide_width(shape[1], off)), dtype=torch.float32)
    assert wide.data_ptr() % 64 == 0
    return wide[:shape[0], off:off + shape[1]]


# ----------------------------------------------------------------------------------------------------------------- generators
def keep_positions(k):
    """at most KEEP positions of a reduction axis of length k: the first, the last, and KEEP - 2 spread evenly over its 32-wide chunks
    with position % 32 = 13 j % 32 running through every residue (every slot of a K chunk; every chunk of a short axis, every
    256-row and 1024-row block of a long one; tests/test_bwd_kernel_cases_host.py asserts that for the lengths in use)"""
    if k <= KEEP:
        return np.arange(k)
    j = np.arange(KEEP - 2)
    pos = 32 * ((j * ((k + 31) // 32)) // (KEEP - 2)) + (13 * j) % 32
    return np.unique(np.concatenate([[0, k - 1], np.where(pos < k, pos, pos - 32)]))


def sparse_values(rs, shape):
    """{0, +-(1 + 2^-9)}, a quarter zeros"""
    return (rs.choice([-SPARSE, SPARSE], size=shape) * (rs.uniform(size=shape) >= 0.25)).astype(np.float32)


class Operand:
    """a matrix as stored (x, fp32) with its bf16 head and remainder by spconv_cases.split (h, l: float64)"""

    def __init__(self, x, h, l):
        self.x, self.h, self.l = x, h, l

    def heads_only(self):
        return Operand(self.h.astype(np.float32), self.h, np.zeros_like(self.l))

    def times(self, live):
        return Operand((self.x * live).astype(np.float32), self.h * live, self.l * live)


POOL = (3300, 420)  # every operand of a two-part lattice is a window of one matrix, generated and split once (the split is the slow part)


@functools.lru_cache(maxsize=None)
def _pool(lattice):
    rs = np.random.RandomState({"dense": 41, "sparse": 42}[lattice])
    x = sc.lattice16(rs, POOL) if lattice == "dense" else sparse_values(rs, POOL)
    return (x,) + sc.split(x, "bf16")


def _window(lattice, rs, shape):
    x, h, l = _pool(lattice)
    r0, c0 = rs.randint(0, POOL[0] - shape[0] + 1), rs.randint(0, POOL[1] - shape[1] + 1)
    w = (slice(r0, r0 + shape[0]), slice(c0, c0 + shape[1]))
    return Operand(x[w], h[w], l[w])


def operands(case, lattice, rs, remainders="both"):
    """(A, B) as stored: two Operands.  remainders ("dense" only): "both", "a" or "b" — which operand keeps its 2^-12 remainders."""
    _, ta, tb, m, k, n, _ = case
    sa, sb = stored_shapes(case)
    if lattice == "int":  # integers -3 .. 3 are bf16 numbers: a head, no remainder (the host test checks that on the split)
        a, b = sc.lattice32(rs, sa), sc.lattice32(rs, sb)
        return Operand(a, a.astype(np.float64), np.zeros(sa)), Operand(b, b.astype(np.float64), np.zeros(sb))
    a, b = _window(lattice, rs, sa), _window(lattice, rs, sb)
    if lattice == "dense":
        return (a if remainders in ("both", "a") else a.heads_only()), (b if remainders in ("both", "b") else b.heads_only())
    assert lattice == "sparse"
    live = np.zeros(k, bool)
    live[keep_positions(k)] = True
    return a, b.times(live[None, :] if tb else live[:, None])


def mask_values(rs, shape):
    """post-activation values for the ReLU mask: normals, with the SPECIALS strewn in (about one in eight)"""
    y = rs.standard_normal(shape).astype(np.float32)
    pick = rs.randint(0, 8 * len(SPECIALS), size=shape)
    for i, v in enumerate(SPECIALS):
        y[pick == i] = np.float32(v)
    return y


# ----------------------------------------------------------------------------------------------------------------- references
def _op(x, trans):
    return x.T if trans else x


def product(case, a, b, arithmetic):
    """float64 (op(A) op(B), sum |op(A)| |op(B)|) of two Operands (or plain arrays, split here); arithmetic "fp32": the full product;
    "pairs": what the bf16-pair kernels compute (spconv_cases.three_products of the splits)"""
    _, ta, tb = case[:3]
    mm = lambda p, q: _op(np.asarray(p, np.float64), ta) @ _op(np.asarray(q, np.float64), tb)
    xa, xb = (v.x if isinstance(v, Operand) else np.asarray(v) for v in (a, b))
    S = mm(np.abs(xa), np.abs(xb))
    if arithmetic == "fp32":
        return mm(xa, xb), S
    assert arithmetic == "pairs"
    parts = [(v.h, v.l) if isinstance(v, Operand) else sc.split(v, "bf16") for v in (a, b)]
    return sc.three_products(mm, parts[0], parts[1]), S


def arithmetic_of(variant):
    return "pairs" if variant in ("TN16", "ROWS16") else "fp32"


def epilogue(prod, S, alpha, beta, c0, y):
    """(C, column sums, sum |.| per element) of  C = alpha prod + beta C0,  zeroed where not y > 0"""
    C = alpha * prod + (beta * np.asarray(c0, np.float64) if beta else 0.0)
    Sout = alpha * S + (np.abs(np.asarray(c0, np.float64)) if beta else 0.0)
    if y is not None:
        with np.errstate(invalid="ignore"):
            on = np.asarray(y) > 0
        C, Sout = np.where(on, C, 0.0), np.where(on, Sout, 0.0)
    return C, C.sum(0), Sout


def assert_case_lattice(S, Sout, lattice, alpha):
    sc.assert_lattice(S, UNIT[lattice])                  # the accumulators
    sc.assert_lattice(Sout, UNIT[lattice] * alpha)       # the stored / atomically accumulated result (alpha unit divides the integers)
    assert alpha in (1.0, 2.0, 0.5)


def colsum_exact(C, unit):
    """may the column sums of C be compared bit for bit?"""
    return float(np.max(np.abs(C).sum(0), initial=0.0)) / unit < 2 ** 24


def colsum_bound(C):
    """per column: n_rows 2^-24 sum_rows |C|"""
    return C.shape[0] * 2.0 ** -24 * np.abs(C).sum(0)


def epilogue_args(name):
    """(with mask, with colsum, alpha, beta)"""
    return {"none": (False, False, 1.0, 0.0), "mask": (True, False, 2.0, 0.0), "colsum": (False, True, 0.5, 0.0),
            "mask+colsum+beta": (True, True, 1.0, 1.0)}[name]


# ----------------------------------------------------------------------------------------------------------------- colsum / relu
COLSUM_ROWS = (1, 4095, 4096, 4097, 9000)
COLSUM_COLS = (1, 63, 64, 65, 83)
RELU_N = (0, 1, 3, 4, 5, 1023, 1024, 1025)


def colsum_slabs(n_rows):
    """the row slabs nb_colsum splits into (one fp32 atomic per column and slab)"""
    return 1 if n_rows < 4096 else min(n_rows // 1024, 256)


def relu_values(rs, n):
    """y with every one of SPECIALS where n allows, spread from the front (the vector body), and three of them as the last elements"""
    y = rs.standard_normal(n).astype(np.float32)
    sp = np.array(SPECIALS, np.float32)
    idx = (np.arange(len(sp)) * max(n // len(sp), 1)) % max(n, 1)
    y[idx[:n]] = sp[:n]
    if n >= 16:  # ... and at the very end: the scalar tail of a length that is no multiple of 4
        y[n - 3:] = np.array([2.0 ** -140, -0.0, float("nan")], np.float32)
    return y


# ----------------------------------------------------------------------------------------------------------------- trilinear
LEVEL_CHANNELS = (32, 64, 128, 128)
CHAN_BASE = (0, 32, 96, 224)


def unnormalize(g, size, dtype=np.float64):
    """grid_sampler_unnormalize, align_corners=True: ((g + 1) / 2) (size - 1), every operation rounded to `dtype`"""
    g = np.asarray(g, dtype)
    return ((g + dtype(1)) / dtype(2)) * dtype(size - 1)


def fp32_grid(pts, bounds_min, voxel_size, out_sh):
    """normalised coordinates [n, 3] in grid_sample's (x, y, z) = (W, H, D) order of world points under R = I, Th = 0, in fp32 with the
    reference's operations (dhw = xyz[[2, 1, 0]] - min, / voxel_size, / out_sh, * 2 - 1); voxel_size and out_sh in (d, h, w) order"""
    p = np.asarray(pts, np.float32)
    cols = []
    for axis in (0, 1, 2):  # x -> W (index 2 of dhw), y -> H, z -> D
        d = 2 - axis
        v = (p[:, axis] - np.float32(bounds_min[axis])) / np.float32(voxel_size[d]) / np.float32(out_sh[d])
        cols.append(v * np.float32(2) - np.float32(1))
    return np.stack(cols, 1).astype(np.float32)


def trilinear_scatter(g, d_feat, grids, index_dtype=np.float64):
    """float64 backward of the four-level lookup  feat[:, level channels] = grid_sample(volume_l, g, align_corners=True, zeros)  with
    respect to the rows of the active voxels.  g [n, 3] (x, y, z); d_feat [n, 352]; grids[l] int [D, H, W] = row id or -1.
    -> (drows[l] [n_rows_l, C_l], S[l] = the same sum of |w| |dF|, K[l] = points reaching each row)"""
    d_feat = np.asarray(d_feat, np.float64)
    out = []
    for l, grid in enumerate(grids):
        grid = np.asarray(grid)
        D, H, W = grid.shape
        C = LEVEL_CHANNELS[l]
        n_rows = int(grid.max()) + 1
        dF = d_feat[:, CHAN_BASE[l]:CHAN_BASE[l] + C]
        drows, S, K = np.zeros((n_rows, C)), np.zeros((n_rows, C)), np.zeros(n_rows, np.int64)
        ix, iy, iz = (unnormalize(g[:, a], s, index_dtype).astype(np.float64) for a, s in ((0, W), (1, H), (2, D)))
        x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
            xx, yy, zz = x0 + dx, y0 + dy, z0 + dz
            w = (1 - np.abs(ix - xx)) * (1 - np.abs(iy - yy)) * (1 - np.abs(iz - zz))
            inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
            row = np.full(len(g), -1, np.int64)
            row[inb] = grid[zz[inb].astype(np.int64), yy[inb].astype(np.int64), xx[inb].astype(np.int64)]
            ok = row >= 0
            np.add.at(drows, row[ok], w[ok, None] * dF[ok])
            np.add.at(S, row[ok], np.abs(w[ok, None] * dF[ok]))
            np.add.at(K, row[ok], 1)
        out.append((drows, S, K))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def c_trilinear(K):
    return (6 + 2 * int(K)) * 2.0 ** -24


# the lattice scene: level shapes (D, H, W) with size - 1 a power of two, different per axis and per level
TRI_SHAPES = ((17, 9, 33), (9, 5, 17), (5, 3, 9), (3, 3, 5))
TRI_OUT_SH = (16, 8, 32)          # (d, h, w): level 0 has one voxel per unit of out_sh
TRI_VOXEL = (2.0 ** -5,) * 3      # metres, (d, h, w)
TRI_RUNS = (1, 2, 7, 64)          # and n, n + 5 (the test adds them)


def tri_weight_denominator(l):
    """the weights of level l are multiples of 1 / this: a quarter voxel of level 0 is 1 / (4 out_sh / (size - 1)) of a voxel per axis"""
    return int(np.prod([4 * o // (s - 1) for o, s in zip(TRI_OUT_SH, TRI_SHAPES[l])]))


@functools.lru_cache(maxsize=None)
def tri_lattice_scene():
    """-> dict(pts [n, 3] world xyz fp32, d_feat [n, 352], grids [4] int32 [D, H, W], n_rows [4]).  The points, in order (a run of
    consecutive points is one ray): a diagonal walk in quarter-voxel steps that shares its base voxel on the coarse levels and not on
    the fine ones; the volume's corners, edge and face centres; points a quarter and three quarters of a voxel outside every face
    (index in (-1, 0) and (size - 1, size)); points far outside (the clamp; every corner out of bounds); a seeded scatter."""
    rs = np.random.RandomState(31)
    vs = TRI_VOXEL[0]
    ext = np.array([TRI_OUT_SH[2], TRI_OUT_SH[1], TRI_OUT_SH[0]], np.float64)  # extent in level-0 voxels, xyz order
    q = []  # in quarter voxels of level 0, xyz
    q += [(5 + 3 * i, 3 + i, 2 + 2 * i) for i in range(20)]                                       # the walk: strictly inside
    q += [(4 * ext[0] * a, 4 * ext[1] * b, 4 * ext[2] * c) for a in (0, 0.5, 1) for b in (0, 0.5, 1) for c in (0, 0.5, 1)]  # faces, edges, corners, centre
    for axis in range(3):
        for off in (-1, -3, 4 * ext[axis] + 1, 4 * ext[axis] + 3):                                 # just outside each side
            p = [9, 6, 11]
            p[axis] = off
            q.append(tuple(p))
            p2 = [4 * ext[0], 0, 4 * ext[2]]                                                        # ... and from a corner
            p2[axis] = off
            q.append(tuple(p2))
    for axis in range(3):
        for off in (-4 * 40, 4 * (ext[axis] + 40), -4 * 3, 4 * (ext[axis] + 2)):                   # far outside; beyond -2 / size + 1
            p = [10, 7, 13]
            p[axis] = off
            q.append(tuple(p))
    q += [tuple(v) for v in rs.randint(0, (4 * ext + 1).astype(np.int64), size=(40, 3))]                              # scatter on the lattice
    pts = (np.asarray(q, np.float64) * (vs / 4)).astype(np.float32)
    n = len(pts)
    d_feat = rs.randint(-3, 4, size=(n, 352)).astype(np.float32)
    # 4-channel groups that are all zero for some levels only
    d_feat[3, 0:4] = 0
    d_feat[3, 32:40] = 0
    d_feat[7, 96:224] = 0
    d_feat[21, 224:352] = 0
    d_feat[40:44, 0:32] = 0
    grids, n_rows = [], []
    for l, shape in enumerate(TRI_SHAPES):
        act = rs.uniform(size=shape) < 0.7          # inactive voxels among the corners
        act[0, 0, 0] = act[-1, -1, -1] = True
        act[0, -1, 0] = False                       # an inactive corner of the volume
        idx = np.cumsum(act.reshape(-1)) - 1
        grids.append(np.where(act.reshape(-1), idx, -1).astype(np.int32).reshape(shape))
        n_rows.append(int(act.sum()))
    return {"pts": pts, "d_feat": d_feat, "grids": grids, "n_rows": n_rows}


def tri_lattice_grid(scene):
    return fp32_grid(scene["pts"], (0.0, 0.0, 0.0), TRI_VOXEL, TRI_OUT_SH)


def assert_tri_lattice(S):
    """the precondition of the bit-for-bit comparison: per row element, sum |w| |dF| in units of the level's weight denominator < 2^24"""
    for l, s in enumerate(S):
        sc.assert_lattice(s, 1.0 / tri_weight_denominator(l))


def random_tri_scene(seed=5, n=300):
    """a random scene for the host check against autograd: normalised coordinates over [-1.3, 1.3], normal dF, random active sets"""
    rs = np.random.RandomState(seed)
    g = rs.uniform(-1.3, 1.3, size=(n, 3))
    d_feat = rs.standard_normal((n, 352))
    grids = []
    for shape in ((6, 7, 5), (4, 5, 6), (3, 4, 2), (2, 3, 3)):
        act = rs.uniform(size=shape) < 0.6
        idx = np.cumsum(act.reshape(-1)) - 1
        grids.append(np.where(act.reshape(-1), idx, -1).astype(np.int32).reshape(shape))
    return g, d_feat, grids


def autograd_scatter(g, d_feat, grids):
    """the same gradients by float64 autograd through F.grid_sample on dense volumes, rows of the active voxels"""
    gt = torch.from_numpy(np.asarray(g, np.float64))[None, None, None]  # [1, 1, 1, n, 3]
    dF = torch.from_numpy(np.asarray(d_feat, np.float64))
    out = []
    for l, grid in enumerate(grids):
        C = LEVEL_CHANNELS[l]
        vol = torch.zeros((1, C) + tuple(grid.shape), dtype=torch.float64, requires_grad=True)
        feat = torch.nn.functional.grid_sample(vol, gt, padding_mode="zeros", align_corners=True)[0, :, 0, 0].t()  # [n, C]
        (feat * dF[:, CHAN_BASE[l]:CHAN_BASE[l] + C]).sum().backward()
        dense = vol.grad[0].permute(1, 2, 3, 0).numpy()
        out.append(dense[np.asarray(grid) >= 0])
    return out


@functools.lru_cache(maxsize=None)
def tri_realistic_scene():
    """the synthetic body (R = I, Th = 0) seen by a 24 x 24 camera, 32 samples a ray: world points fp32 [n, 3] in ray order, normal dF,
    the active sets of the four dense levels (the body's voxels at strides 2, 4, 8, 16) -> dict like tri_lattice_scene's, with
    bounds_min (xyz), voxel_size, out_sh (dhw) and run = samples per ray"""
    from tests import synthetic as syn

    body = syn.make_body(seed=0, box=(0.3, 0.5, 0.2))
    assert np.array_equal(body["R"], np.eye(3, dtype=np.float32)) and not body["Th"].any()
    K, R, T = syn.make_camera(body, 24, 24, focal_factor=2.5, distance=1.5)
    ro, rd, near, far, _ = syn.host_image_rays(24, 24, K, R, T, body["can_bounds"])
    S = 32
    t = np.linspace(0.0, 1.0, S, dtype=np.float32)
    z = near[:, None] * (1 - t) + far[:, None] * t
    pts = (ro[:, None] + rd[:, None] * z[..., None]).reshape(-1, 3).astype(np.float32)
    rs = np.random.RandomState(6)
    d_feat = rs.standard_normal((len(pts), 352)).astype(np.float32)
    out_sh = [int(v) for v in body["out_sh"]]
    grids, n_rows = [], []
    for l in range(4):
        shape = tuple(o >> (l + 1) for o in out_sh)
        act = np.zeros(shape, bool)
        c = body["coord"] >> (l + 1)
        act[c[:, 0], c[:, 1], c[:, 2]] = True
        idx = np.cumsum(act.reshape(-1)) - 1
        grids.append(np.where(act.reshape(-1), idx, -1).astype(np.int32).reshape(shape))
        n_rows.append(int(act.sum()))
    return {"pts": pts, "d_feat": d_feat, "grids": grids, "n_rows": n_rows, "bounds_min": body["bounds"][0], "voxel_size": (0.005,) * 3,
            "out_sh": out_sh, "run": S}
