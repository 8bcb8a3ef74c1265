"""Inputs, float64 references, path predicates and bounds for the tests of the exact fp32 point decoder (nb_points_kernel<DENSITY_ONLY,
DBG> with the decode<> body it shares with nb_march_kernel) and of nb_composite_kernel: tests/test_decode_f32_host.py (CPU) and
tests/test_gpu_decode_f32.py.  CPU only; nothing here touches the library.  The geometry, generators and references of
tests/bwd_cases.py, spconv_cases.py, march_operand_cases.py and march_ray_cases.py are imported, not restated.

A. THE GATHER.  The lattice scene of bwd_cases (TRI_SHAPES, TRI_OUT_SH, TRI_VOXEL, points on quarter voxels of level 0; below a
point is given in those quarter voxels, `q`, in canonical x, y, z).  The volumes hold integers in -255 .. 255, no two of the eight
corners of any cell and no two neighbouring channels equal (`distinct_volumes`).  The weights of level l are multiples of
1 / tri_weight_denominator(l), so every partial sum of the eight-term fma chain is an fp32 number (255 x 16384 < 2^23): `gather_f64`,
the float64 forward twin of bwd_cases.trilinear_scatter, is the answer bit for bit.  A second run replaces every voxel that no point of
the case reads with a non-zero weight by POISON: the clamped reads of out-of-bounds corners and whatever else the tile fill fetches
must not reach the result, whatever those voxels hold.
   `coop_fits` restates the box arithmetic of gather_level_coop; A_CASES names, per wave of 32 consecutive points, the path every
level is to take ('T' the LDS tile, 'P' the per-lane gather), and the host test holds the predicate to it.  The largest tile holds 128 /
64 / 32 / 32 voxels; on level 3, whose volume is 5 x 3 x 3, no box has exactly 32 voxels: 5 x 2 x 3 = 30 is the largest that fits and
5 x 3 x 3 = 45 exceeds it by one plane (the 1024-piece threshold itself is met exactly on levels 0 - 2: 128 x 8, 64 x 16, 32 x 32).
   POSES: the identity, and a signed axis permutation with power-of-two Th and dyadic bounds_min, under which every operation of
grid_coords stays exact: the same normalised coordinates from other world points, other R / Th / bounds_min entries.
   REALISTIC: the samples of bwd_cases.tri_realistic_scene() under a real rotation; `grid_coords32` restates grid_coords in fp32 in
the kernel's order (march_ray_cases._fma32), the index coordinates are fp32 (bwd_cases.unnormalize), weights and sums float64:
|got - ref| <= GATHER_C sum |w| |v| per element, GATHER_C = (6 + 8) 2^-24 (a weight counted as bwd_cases.c_trilinear counts it, then
eight fused additions).

B. THE LAYERS.  Exact: points on voxel centres of every level (F = the voxel's own integers, |v| <= 7), sparse integer weights
(`exact_params`), so that h1, h2, h3, sigma, G, V and rgb are integers (multiples of 2^-3 behind the raw encoding columns) below 2^24
units at every stage: one float64 chain, `layer_chain`, is the answer bit for bit.  The 84 sines and cosines are tied to the PE tap by
`pe_tie_params` (V[:, r] = relu(+-PE[:, r])), rgb_fc to the V tap by `rgb_tie`.  Realistic: normal_params scaled like
tests/synthetic.make_weights; each stage against the float64 product of the kernel's own tapped input within
(K + 2) 2^-24 (|b| + sum |w| |x|), K the reduction length: it holds for K fused or unfused additions in any order.

C. THE ENCODINGS.  |PE - sin / cos in float64 of the fp32 argument x 2^k| <= PE_TOL = 4e-7, the figure the comment above sin_rev
states; `pe_points` holds the arguments named in the docstring of that function.

D. nb_composite.  `composite_inputs` shapes its rays as test_composite_bwd_edges does; march_ray_cases.composite_f64 /
integrator_ratios / tol(S) judge the result.  tol(S) = (8 + S/2) 2^-24 was derived for about S roundings along a ray; the scan
multiplies the same factors in a tree (6 doubling steps per 64 samples and one carried product per trip), so fewer roundings lie on
any path.  `composite_scan_f32` restates the scan's order in numpy float32.
MEASURED_RATIO: the largest |error| / tolerance of the unmutated nb_composite on the MI355X over COMPOSITE_S x COMPOSITE_N x both
backgrounds (the test prints them per case).  The bound was not touched.
"""
import functools
import itertools

import numpy as np

from tests import bwd_cases as bc
from tests import fold_stream_ref as FS
from tests import march_operand_cases as K
from tests import march_ray_cases as R
from tests import spconv_cases as sc

F32 = np.float32
U24 = 2.0 ** -24
POISON = K.POISON
SENTINEL = -7777.0
MEASURED_RATIO = {"weights": 0.075, "rgb": 0.126, "acc": 0.050, "depth": 0.085, "acc_sum": 0.044, "disp": 0.319}
MEASURED_PE_MAX = 1.61e-7        # the largest |PE - float64| on the MI355X over pe_points (PE_TOL below is the claim it is held to)
MEASURED_GATHER_RATIO = 0.401    # realistic gather, worst level; per level 0.333, 0.303, 0.369, 0.401
MEASURED_LAYER_RATIO = 0.021     # realistic layers, worst stage (G); h1 0.016, h2 0.018, h3 0.019, sigma 0.008, V 0.015, rgb 0.016

SHAPES = bc.TRI_SHAPES
OUT_SH = bc.TRI_OUT_SH
VOXEL = bc.TRI_VOXEL
LEVEL_C = bc.LEVEL_CHANNELS
CHAN_BASE = bc.CHAN_BASE
EXT_Q = np.array([4 * OUT_SH[2], 4 * OUT_SH[1], 4 * OUT_SH[0]], np.int64)  # the volume's extent in quarter voxels of level 0, xyz
TILE_PIECES = 1024   # 16-byte pieces a wave's LDS tile holds
MAX_TILE_VOXELS = tuple(4 * TILE_PIECES // c for c in LEVEL_C)
FAR = 2.0 ** 107     # quarter voxels: 2^100 m (about 1e30) away
GATHER_C = (6 + 8) * U24
PE_TOL = 4e-7


def cell_q(l):
    """the size of a voxel of level l in quarter voxels of level 0, xyz"""
    D, H, W = SHAPES[l]
    return np.array([4 * OUT_SH[2] // (W - 1), 4 * OUT_SH[1] // (H - 1), 4 * OUT_SH[0] // (D - 1)], np.int64)


# ------------------------------------------------------------------------------------------------------------------------ poses
POSES = {
    "identity": dict(R=np.eye(3, dtype=F32), Th=np.zeros(3, F32), bmin=np.zeros(3, F32)),
    # canonical = (world - Th) @ R:  world x -> -z, y -> x, z -> -y  (a proper rotation)
    "permuted": dict(R=np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0]], F32), Th=np.array([2.0, -0.5, 4.0], F32),
                     bmin=np.array([0.5, -0.25, 1.0], F32)),
}


def signed_permutations():
    """all 48 signed axis permutations as 3 x 3 float32 matrices"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3), F32)
            for i in range(3):
                m[i, perm[i]] = signs[i]
            out.append(m)
    return out


def world_points(q, pose):
    """fp32 world points whose canonical coordinates minus bounds_min are q (quarter voxels of level 0): (c + bmin) @ R^T + Th.  Only
    the non-zero entries of R take part (0 x inf has no place here); exact for every finite lattice point, asserted."""
    c = np.asarray(q, np.float64) * (VOXEL[0] / 4) + pose["bmin"].astype(np.float64)[None, :]
    Rm = pose["R"].astype(np.float64)
    w = np.zeros_like(c)
    for i in range(3):
        for j in range(3):
            if Rm[i, j] != 0:
                w[:, i] += c[:, j] * Rm[i, j]
    w += pose["Th"].astype(np.float64)[None, :]
    w32 = w.astype(F32)
    small = np.isfinite(w) & (np.abs(w) < 1e6)
    assert np.array_equal(w32[small].astype(np.float64), w[small]), "a lattice point is no fp32 number under this pose"
    return w32


def _b(x, like):
    return np.full(like.shape, x, F32)


def grid_coords32(pts, Rm, Th, bmin, voxel=VOXEL, out_sh=OUT_SH):
    """grid_coords restated in fp32 in the kernel's order: q = p - Th; c_j = fma(q_z, R[2][j], fma(q_y, R[1][j], q_x R[0][j]));
    (c - bmin) / voxel / out_sh * 2 - 1 per axis -> [n, 3] normalised (x, y, z) = (W, H, D); voxel and out_sh in (d, h, w) order."""
    p = np.asarray(pts, F32)
    Rm, Th, bmin = np.asarray(Rm, F32).reshape(3, 3), np.asarray(Th, F32), np.asarray(bmin, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = [p[:, a] - Th[a] for a in range(3)]
        cols = []
        for j in range(3):
            c = R._fma32(q[2], _b(Rm[2, j], q[2]), R._fma32(q[1], _b(Rm[1, j], q[1]), q[0] * Rm[0, j]))
            d = 2 - j
            v = (c - bmin[j]) / F32(voxel[d]) / F32(out_sh[d])
            cols.append(v * F32(2) - F32(1))
    g = np.stack(cols, 1)
    assert g.dtype == F32
    return g


def grid_coords64(pts, Rm, Th, bmin, voxel=VOXEL, out_sh=OUT_SH, bmin_order=(0, 1, 2)):
    """the same in float64 from the fp32 inputs: (p - Th) @ R, then the normalisation.  bmin_order: the entry of bounds_min each
    canonical axis subtracts (the kernel: x, y, z)"""
    p = np.asarray(pts, F32).astype(np.float64)
    c = (p - np.asarray(Th, np.float64)[None, :]) @ np.asarray(Rm, np.float64).reshape(3, 3)
    b = np.asarray(bmin, np.float64)[list(bmin_order)]
    vs = np.array([voxel[2], voxel[1], voxel[0]], np.float64)
    osh = np.array([out_sh[2], out_sh[1], out_sh[0]], np.float64)
    return (c - b[None, :]) / vs / osh * 2.0 - 1.0


# ------------------------------------------------------------------------------------------------------------- the path predicate
def unnorm_clamped32(g, size):
    """unnorm_clamped: ((g + 1) / 2) (size - 1) in fp32, then fmaxf(., -2), fminf(., size + 1) (which drop a NaN)"""
    with np.errstate(invalid="ignore", over="ignore"):
        i = bc.unnormalize(g, size, F32)
        return np.fmin(np.fmax(i, F32(-2)), F32(size + 1))


def wave_box(level, wave_points, shapes=SHAPES):
    """(lo, hi) voxel box (x, y, z) of gather_level_coop for one wave: wave_points = the fp32 normalised coordinates [<= 32, 3] of
    its live points (the padding lanes repeat the last one)."""
    g = np.asarray(wave_points, F32)
    assert 1 <= len(g) <= 32
    D, H, W = shapes[level]
    with np.errstate(invalid="ignore"):
        gmin, gmax = np.fmin.reduce(g, 0), np.fmax.reduce(g, 0)
    lo, hi = [], []
    for a, size in enumerate((W, H, D)):
        lo.append(min(max(int(np.floor(unnorm_clamped32(gmin[a], size))), 0), size - 1))
        hi.append(min(max(int(np.floor(unnorm_clamped32(gmax[a], size))) + 1, 0), size - 1))
    return np.array(lo), np.array(hi)


def coop_fits(level, wave_points, shapes=SHAPES):
    """does the wave's box fit its LDS tile on this level?  nx ny nz C / 4 <= 1024"""
    lo, hi = wave_box(level, wave_points, shapes)
    return int(np.prod(hi - lo + 1)) * LEVEL_C[level] // 4 <= TILE_PIECES


def wave_paths(g, n=None, shapes=SHAPES):
    """per wave of the first n points a string of four letters, 'T' (tile) or 'P' (per lane), and the boxes [waves, 4, 2, 3]"""
    n = len(g) if n is None else n
    paths, boxes = [], []
    for w0 in range(0, n, 32):
        wp = g[w0:min(w0 + 32, n)]
        paths.append("".join("T" if coop_fits(l, wp, shapes) else "P" for l in range(4)))
        boxes.append([wave_box(l, wp, shapes) for l in range(4)])
    return paths, np.array(boxes)


# ---------------------------------------------------------------------------------------------------------------- A: the volumes
def _violations(v):
    """elements equal to a neighbour inside a 2 x 2 x 2 cell (13 offsets) or to the channel before them"""
    bad = np.zeros(v.shape, bool)
    D, H, W, _ = v.shape
    for dz, dy, dx in itertools.product((0, 1), (-1, 0, 1), (-1, 0, 1)):
        if (dz, dy, dx) <= (0, 0, 0):
            continue
        ys, yo = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
        xs, xo = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
        bad[dz:, ys, xs] |= v[dz:, ys, xs] == v[:D - dz, yo, xo]
    bad[..., 1:] |= v[..., 1:] == v[..., :-1]
    return bad


@functools.lru_cache(maxsize=None)
def distinct_volumes(seed=3, shapes=SHAPES):
    """four channels-last volumes of integers in -255 .. 255; elements that agree with a neighbour are drawn again until none does"""
    rs = np.random.RandomState(seed)
    out = []
    for shape, c in zip(shapes, LEVEL_C):
        v = rs.randint(-255, 256, size=tuple(shape) + (c,))
        for _ in range(100):
            bad = _violations(v)
            if not bad.any():
                break
            v[bad] = rs.randint(-255, 256, size=int(bad.sum()))
        assert not _violations(v).any()
        v = v.astype(F32)
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def poisoned(vols, touched):
    """the volumes with POISON in every voxel that is not `touched`"""
    return [np.where(t[..., None], v, F32(POISON)).astype(F32) for v, t in zip(vols, touched)]


# -------------------------------------------------------------------------------------------------------------- A: the reference
A_MUTANTS = ("drop_corner", "clamp_last_plane", "box_short", "tile_shift", "swap_levels_23", "swap_halves")


def gather_f64(g, vols, index_dtype=np.float64, mutate=None, boxes=None, paths=None):
    """The float64 forward twin of bwd_cases.trilinear_scatter: feat[:, level channels] = grid_sample(volume_l, g, align_corners=True,
    zeros padding) with the kernel's corner order.  g [n, 3] normalised (x, y, z); vols: channels-last [D, H, W, C]; index_dtype: the
    arithmetic of the index coordinates (weights and sums are float64).  A coordinate beyond [-2, size + 1] is clamped as the kernel
    clamps it (every corner is out of bounds either way) and a NaN goes to -2.
    -> (F [n, 352], S = sum |w| |v| [n, 352], touched[l] bool [D, H, W]: read with a non-zero weight).
    mutate: one of A_MUTANTS; 'box_short' and 'tile_shift' act on the waves that take the tile (boxes, paths of wave_paths)."""
    g = np.asarray(g)
    n = len(g)
    F, S, touched = np.zeros((n, 352)), np.zeros((n, 352)), []
    wave = np.arange(n) // 32
    for l, vol in enumerate(vols):
        D, H, W, C = vol.shape
        v64 = np.asarray(vol, np.float64)
        idx = []
        with np.errstate(invalid="ignore", over="ignore"):
            for a, s in ((0, W), (1, H), (2, D)):
                i = bc.unnormalize(g[:, a], s, index_dtype).astype(np.float64)
                idx.append(np.fmin(np.fmax(i, -2.0), s + 1.0))
        ix, iy, iz = idx
        x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
        t = np.zeros((D, H, W), bool)
        out, tot = np.zeros((n, C)), np.zeros((n, C))
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
            xx, yy, zz = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64), (z0 + dz).astype(np.int64)
            w = (1 - np.abs(ix - xx)) * (1 - np.abs(iy - yy)) * (1 - np.abs(iz - zz))
            inx = (xx >= 0) & (xx < W)
            if mutate == "clamp_last_plane":
                inx |= xx == W
            inb = inx & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
            if mutate == "drop_corner" and corner == 6:
                inb = np.zeros(n, bool)
            w = np.where(inb, w, 0.0)
            xc, yc, zc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1), np.clip(zz, 0, D - 1)
            if mutate in ("box_short", "tile_shift"):
                tile = np.array([p[l] == "T" for p in paths])[wave]
                lo, hi = boxes[wave, l, 0], boxes[wave, l, 1]
                if mutate == "box_short":  # the box one voxel short in x: its last column repeats the one before
                    xc = np.where(tile & (hi[:, 0] > lo[:, 0]), np.minimum(xc, hi[:, 0] - 1), xc)
                else:                      # the first voxel of the tile holds its x neighbour
                    first = tile & (xc == lo[:, 0]) & (yc == lo[:, 1]) & (zc == lo[:, 2]) & (hi[:, 0] > lo[:, 0])
                    xc = np.where(first, xc + 1, xc)
            val = v64[zc, yc, xc]
            out += w[:, None] * val
            tot += np.abs(w[:, None] * val)
            live = w != 0
            t[zc[live], yc[live], xc[live]] = True
        if mutate == "swap_halves" and l == 2:
            out = np.concatenate([out[:, C // 2:], out[:, :C // 2]], 1)
        F[:, CHAN_BASE[l]:CHAN_BASE[l] + C], S[:, CHAN_BASE[l]:CHAN_BASE[l] + C] = out, tot
        touched.append(t)
    if mutate == "swap_levels_23":
        F = np.concatenate([F[:, :96], F[:, 224:352], F[:, 96:224]], 1)
    return F, S, touched


def assert_gather_lattice(S):
    """the precondition of the bit-for-bit comparison, per level"""
    for l in range(4):
        sc.assert_lattice(S[:, CHAN_BASE[l]:CHAN_BASE[l] + LEVEL_C[l]], 1.0 / bc.tri_weight_denominator(l))


# ------------------------------------------------------------------------------------------------------------------ A: the waves
def _spread(rs, lo, hi, n=32):
    """n points with integer quarter-voxel coordinates in [lo, hi] per axis; the first two are the corners lo and hi themselves"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    p = np.stack([rs.randint(lo[a], hi[a] + 1, size=n) for a in range(3)], 1)
    p[0], p[1] = lo, hi
    return p.astype(np.float64)


def box_wave(rs, level, lo_vox, dims):
    """a wave whose box on `level` is dims = (nx, ny, nz) voxels from voxel lo_vox: floors lo .. lo + n - 2 per axis; n = 1 puts the
    axis on the level's last plane (index exactly size - 1, whose upper neighbour is clamped away)"""
    c = cell_q(level)
    D, H, W = SHAPES[level]
    lo, hi = [], []
    for a, size in enumerate((W, H, D)):
        if dims[a] == 1:
            lo.append((size - 1) * c[a])
            hi.append((size - 1) * c[a])
        else:
            assert lo_vox[a] + dims[a] - 1 <= size - 1
            lo.append(lo_vox[a] * c[a])
            hi.append((lo_vox[a] + dims[a] - 2) * c[a] + c[a] - 1)
    return _spread(rs, lo, hi)


def cell_wave(rs, vox):
    """32 different points inside voxel `vox` of level 0 (offsets 0 .. 3 quarter voxels per axis, the two extremes included)"""
    offs = np.array(list(itertools.product(range(4), repeat=3)))
    pick = np.concatenate([[0, 63], 1 + rs.choice(62, 30, replace=False)])
    return (4 * np.asarray(vox)[None, :] + offs[pick]).astype(np.float64)


def _edge_wave(rs, high):
    """a wave clustered in the first (last) cell of the volume with, per axis, the index exactly 0 (size - 1), a quarter and three
    quarters of a voxel outside, beyond -2 (size + 1) and 2^100 m away; the volume's corner and a point outside all three faces"""
    base = (EXT_Q - 4) if high else np.zeros(3, np.int64)
    inner = base + np.array([1, 2, 3])
    pts = []
    for a in range(3):
        specials = (EXT_Q[a], EXT_Q[a] + 1, EXT_Q[a] + 3, EXT_Q[a] + 9, FAR) if high else (0, -1, -3, -9, -FAR)
        for s in specials:
            p = inner.astype(np.float64)
            p[a] = s
            pts.append(p)
    corner = EXT_Q.astype(np.float64) if high else np.zeros(3)
    pts += [corner, corner + (1.0 if high else -1.0), corner + (np.array([3.0, 9.0, 1.0]) if high else -np.array([3.0, 9.0, 1.0]))]
    fill = base[None, :] + rs.randint(0, 4, size=(32 - len(pts), 3))
    return np.concatenate([np.asarray(pts), fill.astype(np.float64)], 0)


def _scatter(rs, n):
    """n points over the whole volume, the first two its opposite corners"""
    p = _spread(rs, np.zeros(3, np.int64), EXT_Q, n)
    return p


def _tri_scene_q():
    q = bc.tri_lattice_scene()["pts"].astype(np.float64) / (VOXEL[0] / 4)
    assert np.array_equal(q, np.round(q))
    return q


class ACase:
    """name; q [n, 3] canonical quarter-voxel coordinates (wave by wave); paths: per wave the letters of the four levels; dims:
    {(wave, level): (nx, ny, nz)} the boxes the case is about"""

    def __init__(self, name, waves, paths, dims=None):
        self.name, self.q, self.paths, self.dims = name, np.concatenate(waves, 0), tuple(paths.split()), dims or {}
        self.q.setflags(write=False)

    def __repr__(self):
        return self.name


# per level: (the largest box that fits, lo voxel), (one voxel plane more)
FIT_BOXES = (((4, 4, 8), (4, 4, 9), (3, 2, 5)), ((4, 4, 4), (4, 4, 5), (2, 0, 3)), ((4, 2, 4), (5, 2, 4), (1, 0, 0)),
             ((5, 2, 3), (5, 3, 3), (0, 0, 0)))
DIVISOR_BOXES = (((3, 2, 3), (10, 3, 6)), ((5, 3, 2), (20, 1, 9)), ((6, 2, 2), (2, 5, 12)), ((7, 1, 3), (14, 0, 3)),
                 ((5, 1, 4), (25, 0, 1)), ((3, 1, 5), (7, 0, 10)))


@functools.lru_cache(maxsize=None)
def a_cases():
    rs = np.random.RandomState(2024)
    cases = []
    cell_a, cell_b, cell_c = cell_wave(rs, (8, 2, 4)), cell_wave(rs, (17, 5, 9)), cell_wave(rs, (24, 1, 13))
    cases.append(ACase("cell", [cell_a], "TTTT", {(0, l): (2, 2, 2) for l in range(4)}))
    for l, (fit, over, lo) in enumerate(FIT_BOXES):
        cases.append(ACase("fit-L%d" % l, [box_wave(rs, l, lo, fit), box_wave(rs, l, lo, over)],
                           {0: "TTTT PTPT", 1: "PTTT PPPT", 2: "PPTT PPPT", 3: "PPPT PPPP"}[l], {(0, l): fit, (1, l): over}))
    cases.append(ACase("divisors", [box_wave(rs, 0, lo, d) for d, lo in DIVISOR_BOXES], " ".join(["TTTT"] * len(DIVISOR_BOXES)),
                       {(w, 0): d for w, (d, _) in enumerate(DIVISOR_BOXES)}))
    # tile on levels 0 - 1, per lane on 2 - 3: every axis straddles a level-3 boundary by one quarter voxel
    fine_tile = _spread(rs, (31, 15, 31), (64, 16, 32))
    # per lane on 0 - 1, tile on 2 - 3: wide in level-0 voxels, inside 2 x 2 x 2 cells of level 2
    coarse_tile = _spread(rs, (1, 1, 1), (31, 31, 31))
    cases.append(ACase("mixed", [fine_tile, coarse_tile], "TTPP PPTT",
                       {(0, 0): (11, 3, 3), (0, 1): (7, 3, 3), (0, 2): (5, 3, 3), (0, 3): (4, 3, 3), (1, 1): (5, 5, 5), (1, 2): (3, 3, 3)}))
    cases.append(ACase("scattered", [_scatter(rs, 32), _scatter(rs, 32)], "PPPP PPPP"))
    # one workgroup of four different waves (private tiles), and its first two waves again in the next workgroup
    cases.append(ACase("workgroups", [cell_a, cell_b, box_wave(rs, 0, (10, 3, 6), (3, 2, 3)), cell_c, cell_a, cell_b],
                       "TTTT TTTT TTTT TTTT TTTT TTTT"))
    low, high = _edge_wave(rs, False), _edge_wave(rs, True)
    cases.append(ACase("edges-clustered", [low, high], "TTTT TTTT", {(w, l): (2, 2, 2) for w in (0, 1) for l in range(4)}))
    mix = np.concatenate([low, high, _scatter(rs, 64)], 0)
    mix = mix[np.concatenate([np.arange(k, 128, 4) for k in range(4)])]  # every wave gets a quarter of each part
    cases.append(ACase("edges-scattered", [mix], "PPPP PPPP PPPP PPPP"))
    cases.append(ACase("tri-scene", [_tri_scene_q()], "PPPP PPPP PPPP PPPP"))
    return tuple(cases)


def a_case(name):
    return next(c for c in a_cases() if c.name == name)


# the row-count case: 192 points; the waves that end behind points 0, 32 and 128 start with a point of one cell and go on scattered,
# so that with n = 1, 33, 129 the last wave's only live point has a 2 x 2 x 2 box the padding lanes must not widen
ROW_COUNTS = (1, 31, 32, 33, 127, 128, 129)
ROWS_LAST_WAVE = {1: "TTTT", 31: "PPPP", 32: "PPPP", 33: "TTTT", 127: "PPPP", 128: "PPPP", 129: "TTTT", 192: "PPPP"}


@functools.lru_cache(maxsize=None)
def rows_case():
    rs = np.random.RandomState(77)
    q = _scatter(rs, 192)
    cell = cell_wave(rs, (8, 2, 4))
    for w0 in (0, 32, 128):
        q[w0] = cell[5]
        q[w0 + 1], q[w0 + 2] = 0.0, EXT_Q  # the rest of the wave spans the volume
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def odd_case():
    """-> (q with the odd points, q without, their indices): a clustered wave with one NaN point and one whose x is +inf, and the same
    wave with two ordinary points in their place; a second, ordinary wave"""
    rs = np.random.RandomState(5)
    plain = np.concatenate([cell_wave(rs, (8, 2, 4)), cell_wave(rs, (17, 5, 9))], 0)
    odd = plain.copy()
    odd[5] = np.nan
    odd[17, 0] = np.inf
    return odd, plain, (5, 17)


def case_grid(q, pose_name):
    """(world points fp32, normalised coordinates fp32 by the kernel's operations) of canonical lattice points under a pose"""
    pose = POSES[pose_name]
    w = world_points(q, pose)
    return w, grid_coords32(w, pose["R"], pose["Th"], pose["bmin"])


# ------------------------------------------------------------------------------------------------------------------ A: realistic
def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def realistic_scene(n_rays=48):
    """The samples of bwd_cases.tri_realistic_scene() (every fifth ray, n_rays of them: a wave = the 32 samples of one ray), then
    a bundle of 32 neighbouring rays depth by depth (a wave = the rays at one depth), moved to a pose with a real rotation; normal volumes
    of the scene's four level shapes.  -> dict(pts world fp32, pose, g fp32 by grid_coords32, vols, shapes, voxel, out_sh)"""
    s = bc.tri_realistic_scene()
    run = s["run"]
    can = s["pts"].reshape(-1, run, 3)
    assert len(can) >= 5 * n_rays
    ray_major = can[np.arange(3, len(can), 5)[:n_rays]].reshape(-1, 3)
    side = can[len(can) // 2 - 16:len(can) // 2 + 16]  # 32 consecutive rays from the middle of the image
    depth_major = side.transpose(1, 0, 2).reshape(-1, 3)
    can = np.concatenate([ray_major, depth_major], 0).astype(np.float64)
    Rm = _rotation((1.0, 2.0, 3.0), 0.3).astype(F32)
    Th = np.array([0.3, -1.2, 0.7], F32)
    world = (can @ Rm.astype(np.float64).T + Th.astype(np.float64)[None, :]).astype(F32)  # canonical = (world - Th) @ R
    pose = dict(R=Rm, Th=Th, bmin=np.asarray(s["bounds_min"], F32))
    shapes = tuple(tuple(int(v) for v in g.shape) for g in s["grids"])
    rs = np.random.RandomState(12)
    vols = tuple(rs.standard_normal(sh + (c,)).astype(F32) for sh, c in zip(shapes, LEVEL_C))
    g = grid_coords32(world, Rm, Th, pose["bmin"], s["voxel_size"], s["out_sh"])
    return dict(pts=world, pose=pose, g=g, vols=vols, shapes=shapes, voxel=tuple(s["voxel_size"]), out_sh=tuple(s["out_sh"]))


def gather_ratios(got, ref, S):
    """per level the worst |got - ref| / (GATHER_C sum |w| |v|)"""
    return [sc.worst_ratio(got[:, CHAN_BASE[l]:CHAN_BASE[l] + LEVEL_C[l]], ref[:, CHAN_BASE[l]:CHAN_BASE[l] + LEVEL_C[l]],
                           S[:, CHAN_BASE[l]:CHAN_BASE[l] + LEVEL_C[l]]) / GATHER_C for l in range(4)]


# ------------------------------------------------------------------------------------------------------------------ B: the layout
N_PE = 45
G0, GH, GV, NB_PF = 44, 32, 44, 8   # groups of four K = 2 chunks per 32-row tile of fc_0 / a hidden layer / view_fc; the ring depth
RAW_COLS = (256, 257, 258, 283, 284, 285)  # view_fc's six raw encoding columns: the view direction, the point
STAGES = ("h1", "h2", "h3", "sigma", "G", "V", "rgb")
STAGE_K = {"h1": 352, "h2": 256, "h3": 256, "sigma": 256, "G": 256, "V": 346, "rgb": 128}


def col_feat(q, hi):
    """fc_0 input column of gather register q (0 .. 175) of half hi (nb_march_common.h)"""
    l = 0 if q < 16 else (1 if q < 48 else (2 if q < 112 else 3))
    return CHAN_BASE[l] + hi * (LEVEL_C[l] // 2) + (q - CHAN_BASE[l] // 2)


def col_pe(c, hi):
    """view_fc column of encoding slot c of half hi, -1 = padding (nb_march_common.h)"""
    if c < 12:
        return 256 + 3 + 6 * (c // 3) + 3 * hi + c % 3
    if c < 42:
        return 256 + 27 + 3 + 6 * ((c - 12) // 3) + 3 * hi + (c - 12) % 3
    if c < 45:
        return (256 + 27 + c - 42) if hi else (256 + c - 42)
    return -1


def col_view(q, hi):
    return FS.col_hidden(q, hi) if q < 128 else col_pe(q - 128, hi)


def fragment_cols(kind, g):
    """the eight input columns (i, hi) of weight fragment group g of a layer: kind 'feat', 'hidden' or 'view'"""
    f = {"feat": col_feat, "hidden": FS.col_hidden, "view": col_view}[kind]
    return [f(4 * g + i, hi) for i in range(4) for hi in range(2)]


# ----------------------------------------------------------------------------------------------------------------- B: exact case
def _sparse_int(rs, rows, cols, nnz):
    """[rows, cols]: nnz entries of {+-1, +-2} per row, placed so that rows x nnz consecutive slots of a shuffled column order are
    filled: every column is hit when rows x nnz >= cols"""
    w = np.zeros((rows, cols), F32)
    order = rs.permutation(cols)
    for r in range(rows):
        c = order[(r * nnz + np.arange(nnz)) % cols]
        w[r, c] = rs.choice([-2.0, -1.0, 1.0, 2.0], size=nnz)
    return w


def _distinct_bias(rs, n):
    """n different integers centred on zero"""
    return (rs.permutation(n) - n // 2).astype(F32)


EXACT_NNZ = {"fc0": 6, "fc1": 4, "fc2": 4, "latent": 4, "code": 2, "view": 4}


@functools.lru_cache(maxsize=None)
def exact_params(seed=11):
    """-> (params, latent code): integer weights throughout.  feature_fc is a signed permutation and latent_fc sparse, so the merged
    matrix the packer forms in double is integer as well; latent_fc[:, 256:] and the code reach the bias only."""
    rs = np.random.RandomState(seed)
    p = K.zero_params()
    p["fc0_w"], p["fc0_b"] = _sparse_int(rs, 256, 352, EXACT_NNZ["fc0"]), _distinct_bias(rs, 256)
    p["fc1_w"], p["fc1_b"] = _sparse_int(rs, 256, 256, EXACT_NNZ["fc1"]), _distinct_bias(rs, 256)
    p["fc2_w"], p["fc2_b"] = _sparse_int(rs, 256, 256, EXACT_NNZ["fc2"]), _distinct_bias(rs, 256)
    p["alpha_w"], p["alpha_b"] = rs.choice([-2.0, -1.0, 1.0, 2.0], size=(1, 256)).astype(F32), np.array([-3.0], F32)
    perm = rs.permutation(256)
    p["feature_w"][np.arange(256), perm] = rs.choice([-1.0, 1.0], size=256)
    p["feature_b"] = rs.randint(-8, 9, size=256).astype(F32)
    p["latent_w"][:, :256] = _sparse_int(rs, 256, 256, EXACT_NNZ["latent"])
    p["latent_w"][:, 256:] = _sparse_int(rs, 256, 128, EXACT_NNZ["code"])
    p["latent_b"] = _distinct_bias(rs, 256)
    p["view_w"][:, :256] = _sparse_int(rs, 128, 256, EXACT_NNZ["view"])
    raw = np.asarray(RAW_COLS)
    p["view_w"][np.arange(128), raw[np.arange(128) % 6]] = rs.choice([-2.0, -1.0, 1.0, 2.0], size=128)
    p["view_b"] = _distinct_bias(rs, 128)
    p["rgb_w"], p["rgb_b"] = rs.choice([-2.0, -1.0, 1.0, 2.0], size=(3, 128)).astype(F32), np.array([1.0, -2.0, 3.0], F32)
    code = rs.randint(-4, 5, size=128).astype(F32)
    return p, code


EXACT_UNIT = {"h1": 1.0, "h2": 1.0, "h3": 1.0, "sigma": 1.0, "G": 1.0, "V": 2.0 ** -3, "rgb": 2.0 ** -3}
B_POSE = "permuted"
B_N = 160


@functools.lru_cache(maxsize=None)
def exact_points():
    """-> (q [B_N, 3], view directions fp32 [B_N, 3], volumes): the 45 points that are voxel centres of EVERY level (the voxels of
    level 3), repeated in a shuffled order with different dyadic, unnormalised view directions; volumes of integers in -7 .. 7"""
    rs = np.random.RandomState(21)
    c3 = cell_q(3)
    D, H, W = SHAPES[3]
    centres = np.array([(x * c3[0], y * c3[1], z * c3[2]) for z in range(D) for y in range(H) for x in range(W)], np.float64)
    q = centres[np.concatenate([rs.permutation(len(centres)) for _ in range(4)])[:B_N]]
    v = rs.choice([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 2.0, -2.0], size=(B_N, 3)).astype(F32)
    vols = tuple(rs.randint(-7, 8, size=tuple(sh) + (c,)).astype(F32) for sh, c in zip(SHAPES, LEVEL_C))
    return q, v, vols


def view_input(G, pe90):
    """view_fc's input [n, 346] = [latent_fc output | encodings in column order]"""
    return np.concatenate([np.asarray(G, np.float64), np.asarray(pe90, np.float64)], 1)


def raw_encodings(x, v):
    """[n, 90] float64 with the six raw columns (the view direction, the point) and zeros for the 84 sines and cosines"""
    pe = np.zeros((len(x), 90))
    pe[:, 0:3], pe[:, 27:30] = np.asarray(v, np.float64), np.asarray(x, np.float64)
    return pe


def merged64(p):
    return np.asarray(K.merged_ref(p)[0], np.float64)


def latent_bias64(p, code):
    return np.asarray(K.latent_bias_ref(p, code)[0], np.float64)


B_MUTANTS = ("tile_bias", "swap_kchunks", "pf_tail", "drop_encoding_column", "swap_rgb", "no_relu_V")


def mutated_params(p, mutate):
    """the weights a kernel with the named mistake would in effect multiply by"""
    p = dict((k, v.copy()) for k, v in p.items())
    if mutate == "tile_bias":         # the bias fragment of tile 3 of fc_1 taken from tile 4
        p["fc1_b"][96:128] = p["fc1_b"][128:160]
    elif mutate == "swap_kchunks":    # K chunks 5 and 70 of fc_1 exchanged
        a, b = [FS.col_hidden(5, hi) for hi in (0, 1)], [FS.col_hidden(70, hi) for hi in (0, 1)]
        p["fc1_w"][:, a + b] = p["fc1_w"][:, b + a]
    elif mutate == "pf_tail":         # the last NB_PF fragments of fc_2 (tile 7, groups GH - 8 ..) replaced by the first (tile 0, groups 0 ..)
        src = p["fc2_w"].copy()
        for k in range(NB_PF):
            p["fc2_w"][224:256, fragment_cols("hidden", GH - NB_PF + k)] = src[0:32, fragment_cols("hidden", k)]
    elif mutate == "drop_encoding_column":
        p["view_w"][:, 284] = 0.0
    return p


def layer_chain(p, code, F, pe90, mutate=None, merged=None, lb=None, inputs=None):
    """The decoder in float64 -> {stage: (value [n, .], S = |b| + sum |w| |x|)} for STAGES; h1, h2, h3 and V behind their ReLU.
    F [n, 352]; pe90 [n, 90] the encodings in view_fc's column order.  merged / lb: the merged layer and its bias where they are not
    to be formed here (the fp32 ones read back from the pack).  inputs: {stage: the input to use instead of the chain's own}: the
    kernel's tapped activations, so that errors do not compound."""
    if mutate in B_MUTANTS:
        p = mutated_params(p, mutate)
    inputs = inputs or {}
    d = lambda a: np.asarray(a, np.float64)
    relu = lambda a: np.maximum(a, 0.0)
    out = {}

    def lin(x, w, b):
        return x @ d(w).T + d(b)[None, :], np.abs(x) @ np.abs(d(w)).T + np.abs(d(b))[None, :]

    x = d(F)
    for name, key in (("h1", "fc0"), ("h2", "fc1"), ("h3", "fc2")):
        x = d(inputs.get(name, x))
        y, S = lin(x, p[key + "_w"], p[key + "_b"])
        out[name] = (relu(y), S)
        x = out[name][0]
    h3 = d(inputs.get("sigma", x))
    out["sigma"] = lin(h3, p["alpha_w"], p["alpha_b"])
    h3 = d(inputs.get("G", x))
    out["G"] = lin(h3, merged64(p) if merged is None else merged, latent_bias64(p, code) if lb is None else lb)
    vin = view_input(inputs.get("V", out["G"][0]), pe90)
    y, S = lin(vin, p["view_w"], p["view_b"])
    out["V"] = (y if mutate == "no_relu_V" else relu(y), S)
    y, S = lin(d(inputs.get("rgb", out["V"][0])), p["rgb_w"], p["rgb_b"])
    out["rgb"] = (y[:, ::-1] if mutate == "swap_rgb" else y, S[:, ::-1] if mutate == "swap_rgb" else S)
    return out


def layer_bound(stage, S):
    """(K + 2) 2^-24 (|b| + sum |w| |x|): K additions in any order, fused or not, the half-wave addition and the bias of the VALU tails"""
    return (STAGE_K[stage] + 2) * U24 * S


def pe_tie_params(sign):
    """view_fc row r = sign on encoding column r (r < 90), everything else zero: V[:, r] = relu(sign PE[:, r])"""
    p = K.zero_params()
    p["view_w"][np.arange(90), 256 + np.arange(90)] = sign
    return p


def rgb_tie(p, t):
    """p with rgb_fc = one +-1 per channel on V columns 3 t, 3 t + 1, 3 t + 2 (mod 128), zero bias -> (params, columns, signs).
    view_fc's bias is raised by 1 so that every column of V is positive for some point of the realistic scene (the host test says so)"""
    p = dict((k, v.copy()) for k, v in p.items())
    p["view_b"] = p["view_b"] + F32(1.0)
    cols = (3 * t + np.arange(3)) % 128
    signs = np.where((t + np.arange(3)) % 2 == 0, 1.0, -1.0).astype(F32)
    p["rgb_w"] = np.zeros((3, 128), F32)
    p["rgb_w"][np.arange(3), cols] = signs
    p["rgb_b"] = np.zeros(3, F32)
    return p, cols, signs


def realistic_params(seed=4):
    """normal_params scaled like tests/synthetic.make_weights: the trunk x 2.5, alpha_fc x 20 with a bias of -3, rgb_fc x 8"""
    p = K.normal_params(seed)
    for name in ("fc0_w", "fc1_w", "fc2_w"):
        p[name] = p[name] * F32(2.5)
    p["alpha_w"] = p["alpha_w"] * F32(20.0)
    p["alpha_b"] = np.array([-3.0], F32)
    p["rgb_w"] = p["rgb_w"] * F32(8.0)
    code = np.random.RandomState(seed + 1).standard_normal(128).astype(F32)
    return p, code


# --------------------------------------------------------------------------------------------------------------- C: the encodings
INV_2PI = 0.15915494309189533576888376337251436


def encodings_f64(x, v, mutate=None):
    """[n, 90] in view_fc's column order: v, (sin, cos)(v 2^k) k < 4, x, (sin, cos)(x 2^k) k < 10, in float64 of the fp32 inputs.
    mutate: 'cos_for_sin' (frequency 3 of the point), 'next_frequency' (frequency k of the point taken as k + 1)"""
    out = []
    for a, freqs, is_x in ((np.asarray(v, F32).astype(np.float64), 4, False), (np.asarray(x, F32).astype(np.float64), 10, True)):
        out.append(a)
        for k in range(freqs):
            kk = k + 1 if (mutate == "next_frequency" and is_x) else k
            arg = a * 2.0 ** kk
            s, c = np.sin(arg), np.cos(arg)
            out += [c if (mutate == "cos_for_sin" and is_x and k == 3) else s, c]
    return np.concatenate(out, 1)


def _seam_arguments(frac, count, limit=2.0 ** 15):
    """fp32 arguments below `limit` whose revolutions x / 2 pi lie within 1e-7 of m + frac for an integer m"""
    m = np.arange(0, int(limit * INV_2PI) - 1, dtype=np.float64)
    x = ((m + frac) / INV_2PI).astype(F32)
    u = x.astype(np.float64) * INV_2PI
    hit = np.abs(u - (m + frac)) < 1e-7
    x = x[hit]
    pick = np.unique(np.round(np.linspace(0, len(x) - 1, count)).astype(np.int64))
    return x[pick]


@functools.lru_cache(maxsize=None)
def pe_points():
    """-> (points fp32 [n, 3], directions fp32 [n, 3]), the same list of arguments in both, rotated through the axes:
       0 and -0; +-2^-k, k <= 12; uniform in [-64, 64] and +-64 themselves (arguments up to 2^15 rad at frequency 9: the double
       reduction must hold); arguments x / 2^k, |.| <= 64, for which frequency k falls within 1e-7 of a half revolution (the
       u - rint(u) seam) or of a quarter / three quarters (the + 1/4 of the cosine); components exactly +-1 and 0; unnormalised
       directions."""
    rs = np.random.RandomState(8)
    vals = [0.0, -0.0, 1.0, -1.0, 64.0, -64.0, 3.0, -4.0, 12.0]
    vals += [s * 2.0 ** -k for k in range(1, 13) for s in (1.0, -1.0)]
    for frac in (0.5, 0.25, 0.75):
        for x in _seam_arguments(frac, 24):
            k = 0 if x <= 64 else int(np.ceil(np.log2(float(x) / 64.0)))
            vals += [float(x) / 2.0 ** k, -float(x) / 2.0 ** k]
    vals += list(rs.uniform(-64.0, 64.0, size=96))
    vals = np.asarray(vals, F32)
    n = len(vals)
    pts = np.stack([vals, np.roll(vals, 7), np.roll(vals, 19)], 1)
    dirs = np.stack([np.roll(vals, 3), np.roll(vals, 5), np.roll(vals, 11)], 1)
    return np.ascontiguousarray(pts), np.ascontiguousarray(dirs)


def seam_hits(x, freqs):
    """how many (argument, frequency) pairs lie within 1e-7 revolutions of a half and of a quarter / three-quarter revolution"""
    u = np.asarray(x, F32).astype(np.float64).reshape(-1, 1) * INV_2PI * 2.0 ** np.arange(freqs)[None, :]
    f = u - np.floor(u)
    big = np.abs(u) > 1.0  # beyond the first revolution: the reduction is in play
    return int(((np.abs(f - 0.5) < 1e-7) & big).sum()), int((((np.abs(f - 0.25) < 1e-7) | (np.abs(f - 0.75) < 1e-7)) & big).sum())


# ---------------------------------------------------------------------------------------------------------------- D: nb_composite
COMPOSITE_S = (1, 2, 63, 64, 65, 127, 128, 129, 200)
COMPOSITE_N = (1, 3, 4, 5, 9)
RAY_KINDS = ("no_density", "sigma_zero", "saturates_at_third", "saturated_from_first", "zero_direction", "logits_30", "equal_depths",
             "plain", "plain2")
D_MUTANTS = ("shifted_product", "no_carry", "last_interval_without_norm")


def composite_inputs(S, n):
    """raw [n, S, 4], z [n, S] strictly increasing (but for one ray's two equal depths), ray_d [n, 3] and the kind of every ray: ray
    r is kind (r + shift) mod 9; n = 9 holds every kind, the smaller n rotate through them with S"""
    rs = np.random.RandomState(1000 * S + n)
    shift = 0 if n >= len(RAY_KINDS) else 2 * COMPOSITE_S.index(S) if S in COMPOSITE_S else 0
    raw = (rs.standard_normal((n, S, 4)) * 2).astype(F32)
    z = (1.0 + np.cumsum(rs.uniform(0.2, 1.0, (n, S)) * (2.0 / S), axis=1)).astype(F32)
    assert S == 1 or np.all(np.diff(z, axis=1) > 0)
    d = rs.standard_normal((n, 3)).astype(F32)
    kinds = []
    for r in range(n):
        kind = RAY_KINDS[(r + shift) % len(RAY_KINDS)]
        kinds.append(kind)
        if kind == "no_density":
            raw[r, :, 3] = -np.abs(raw[r, :, 3]) - F32(0.01)
        elif kind == "sigma_zero":
            raw[r, :, 3] = 0.0
        elif kind == "saturates_at_third":
            raw[r, S // 3, 3] = 3e4
        elif kind == "saturated_from_first":
            raw[r, :, 3] = 1e3
        elif kind == "zero_direction":
            d[r] = 0.0
            raw[r, S - 1, 3] = abs(raw[r, S - 1, 3]) + F32(0.5)
        elif kind == "logits_30":
            raw[r, :, :3] = np.where(rs.rand(S, 3) < 0.5, F32(30.0), F32(-30.0))
        elif kind == "equal_depths" and S >= 2:
            z[r, S // 2] = z[r, S // 2 - 1]
    return raw, z, d, kinds


def composite_f64_mutant(raw, z, ray_d, white_bkgd=False, mutate=None):
    """march_ray_cases.composite_f64 restated (equal to it without a mutation: the host test says so), with one of D_MUTANTS"""
    raw, z = np.asarray(raw, np.float64), np.asarray(z, np.float64)
    n, S = z.shape
    dn = R.ray_norm_f32(ray_d).astype(np.float64)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10)], 1) * dn[:, None]
    if mutate == "last_interval_without_norm":
        dist[:, -1] = 1e10
    alpha = -np.expm1(-np.maximum(raw[..., 3], 0.0) * dist)
    f = 1.0 - alpha + 1e-10
    excl = lambda ff: np.cumprod(np.concatenate([np.ones((n, 1)), ff], 1), 1)[:, :-1]
    if mutate == "no_carry":  # every 64-sample trip starts from T = 1
        T = np.concatenate([excl(f[:, b:b + 64]) for b in range(0, S, 64)], 1)
    else:
        T = excl(f)
    if mutate == "shifted_product":  # the inclusive product
        T = T * f
    w = alpha * T
    rgb = (w[..., None] / (1.0 + np.exp(-raw[..., :3]))).sum(1)
    acc = w.sum(1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc)[:, None]
    return dict(weights=w, rgb=rgb, acc=acc, depth=(w * z).sum(1))


def composite_scan_f32(raw, z, ray_d, white_bkgd=False):
    """nb_composite_kernel's order in numpy float32 (expf correctly rounded): per trip of 64 samples an inclusive product scan of
    1 - alpha + 1e-10 in 6 doubling steps (lanes behind S hold 1), w = alpha (T excl), T carried as T x the trip's whole product, the
    five sums by a 6-step butterfly and added to the ray's running sums -> dict like composite_f64's plus disp"""
    raw, z = np.asarray(raw, F32), np.asarray(z, F32)
    n, S = z.shape
    dn = R.ray_norm_f32(ray_d)
    one = F32(1.0)
    T = np.ones(n, F32)
    sums = [np.zeros(n, F32) for _ in range(5)]
    w_out = np.zeros((n, S), F32)
    lanes = np.arange(64)
    for base in range(0, S, 64):
        m = min(64, S - base)
        zc, alpha = np.zeros((n, 64), F32), np.zeros((n, 64), F32)
        r = np.zeros((n, 64, 4), F32)
        zc[:, :m], r[:, :m] = z[:, base:base + m], raw[:, base:base + m]
        dist = np.full((n, m), 1e10, F32)
        k = min(m, S - 1 - base)
        dist[:, :k] = z[:, base + 1:base + 1 + k] - z[:, base:base + k]
        dist = dist * dn[:, None]
        alpha[:, :m] = one - R._exp32(-np.maximum(r[:, :m, 3], F32(0.0)) * dist)
        f = np.ones((n, 64), F32)
        f[:, :m] = (one - alpha[:, :m]) + F32(1e-10)
        p = f.copy()
        off = 1
        while off < 64:
            up = np.concatenate([np.ones((n, off), F32), p[:, :-off]], 1)
            p = np.where(lanes[None, :] >= off, p * up, p)
            off *= 2
        excl = np.concatenate([np.ones((n, 1), F32), p[:, :-1]], 1)
        w = alpha * (T[:, None] * excl)
        T = T * p[:, 63]
        w_out[:, base:base + m] = w[:, :m]
        parts = [w / (one + R._exp32(-r[:, :, ch])) for ch in range(3)] + [w * zc, w]
        for i, s in enumerate(parts):
            off = 32
            while off > 0:
                s = s + s[:, lanes ^ off]
                off //= 2
            sums[i] = sums[i] + s[:, 0]
        assert all(s.dtype == F32 for s in sums) and T.dtype == F32
    rgb, depth, acc = np.stack(sums[:3], 1), sums[3], sums[4]
    if white_bkgd:
        rgb = rgb + (one - acc)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = depth / acc
        disp = one / np.where(np.isnan(q), q, np.maximum(F32(1e-10), q))
    return dict(weights=w_out, rgb_map=rgb, acc_map=acc, depth_map=depth, disp_map=disp.astype(F32))
