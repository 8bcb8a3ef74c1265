"""Inputs, float64 references and numpy models for the tests of the field normals (csrc/nb_field_normal.hip, Network.
calculate_density_gradient, Renderer.render(normals=True), RendererMesh.extract_mesh(normals="field")): tests/test_field_normals_host.py
(CPU) and tests/test_gpu_field_normals.py.  CPU only; nothing here touches the library.  The geometry, generators and references of
tests/bwd_cases.py, decode_f32_cases.py and march_ray_cases.py are imported, not restated.

A. nb_trilinear_grad.  `grad_f64` is the coordinate twin of decode_f32_cases.gather_f64: per level the forward's cell (the floor of
the clamped index coordinate: at an integer coordinate the right-hand cell) and weight pairs, the three directional differences of
the blend, the level's scale (size - 1) / (voxel_size out_sh) and the rotation into world axes, all in float64 from the given
normalised coordinates.  It also returns A, per component the sum of the absolute values of every product that enters it.
   LATTICE: the lattice scene of bwd_cases (quarter-voxel points, TRI_SHAPES), its active sets (grid entry -1 = a constant zero), the
integer volumes of decode_f32_cases.distinct_volumes, d_feat with two small integers per level and point.  Weight pairs are
multiples of 2^-4 (level 0) to 2^-10 (level 3), scales are powers of two (32 to 4), so every term is a multiple of UNIT = 2^-7 and
A < 2^24 UNIT: every partial sum in any order is an fp32 number and grad_f64 is the answer bit for bit.  MUTANTS name four ways to get it wrong.
   REALISTIC: decode_f32_cases.realistic_scene() (a real rotation) with the active sets of bwd_cases.tri_realistic_scene(), normal
d_feat; index coordinates in fp32 as the kernel forms them, everything behind them float64: |got - ref| <= GRAD_C A.

B. The chain.  `chain_f64`: d_feat = (((w_alpha [h3 > 0]) W_2 [h2 > 0]) W_1 [h1 > 0]) W_0 in float64 with the masks of a tap.

C. End to end.  `e2e_reference(scene)`: float64 autograd of the oracle's calculate_density at the samples of rays 0:256:16, and the
points the comparison leaves out — computed from the reference alone: a float64 pre-activation of fc_0 / fc_1 / fc_2 within
PREACT_EXCLUDE of the layer's largest magnitude from zero (a ReLU that fp32 may decide the other way), or an index coordinate of any
level within INDEX_EXCLUDE of an integer (a cell that fp32 may assign the other way).

D. nb_normal_select / nb_normal_composite restated in numpy float32, one IEEE operation per step.
"""
import functools

import numpy as np

from tests import bwd_cases as bc
from tests import decode_f32_cases as dc
from tests import march_ray_cases as R

F32 = np.float32
U24 = 2.0 ** -24
POISON = dc.POISON
GRAD_C = (8 * 352 + 16) * U24  # 2816 summed products in any order; 16: the roundings of weights, scales and rotation
MEASURED_GRAD_RATIO = 0.0002   # the largest |got - ref| / (GRAD_C A) of the realistic case on the MI355X (the bound was not moved)
LATTICE_N = (1, 63, 64, 65, 257)
MUTANTS = ("drop_corner", "left_cell", "R_transposed", "level_scale")
CHAIN_N = (1, 1023, 1024, 1025)   # around the 1024-row switch of nb_gemm_fused to the bf16-pair kernel
CHAIN_TOL, CHUNK_TOL = 1e-4, 2e-5
E2E_SCENES = ("small", "small_dense")
E2E_RAYS = slice(0, 256, 16)
PREACT_EXCLUDE, INDEX_EXCLUDE, EXCLUDE_CAP = 1e-5, 1e-4, 0.10
E2E_TOL, E2E_SIN, E2E_SIN_FROM = 1e-4, 1e-2, 1e-2
W_MIN = 2.0 ** -8
VOXEL32 = (float(F32(0.005)),) * 3  # the voxel size of the golden scenes as the oracle and the kernels hold it: the fp32 number


# ------------------------------------------------------------------------------------------------------------------------ A
def level_scale(shape, voxel, out_sh):
    """d(index coordinate) / d(canonical coordinate) along x, y, z of a level of `shape` (D, H, W); voxel, out_sh in (d, h, w)"""
    D, H, W = shape
    v, o = [float(x) for x in voxel], [float(x) for x in out_sh]
    return np.array([(W - 1) / (v[2] * o[2]), (H - 1) / (v[1] * o[1]), (D - 1) / (v[0] * o[0])])


def grad_f64(g, d_feat, vols, voxel, out_sh, Rm, grids=None, index_dtype=np.float64, mutate=None):
    """g [n, 3] normalised (x, y, z); d_feat [n, 352]; vols channels-last [D, H, W, C]; grids[l] int [D, H, W] (entry < 0: the voxel
    counts as zero whatever the volume holds) or None; Rm [3, 3] with canonical = (p - Th) @ Rm.
    -> (grad [n, 3] world, A [n, 3], touched[l] bool [D, H, W]: the voxel is read with a non-zero weight pair)"""
    g = np.asarray(g)
    n = len(g)
    d_feat = np.asarray(d_feat, np.float64)
    gc, Ac, touched = np.zeros((n, 3)), np.zeros((n, 3)), []
    shapes = [v.shape[:3] for v in vols]
    for l, vol in enumerate(vols):
        D, H, W, C = vol.shape
        v64 = np.asarray(vol, np.float64)
        live = np.ones((D, H, W), bool) if grids is None else np.asarray(grids[l]) >= 0
        dF = d_feat[:, bc.CHAN_BASE[l]:bc.CHAN_BASE[l] + C]
        idx = []
        with np.errstate(invalid="ignore", over="ignore"):
            for a, s in ((0, W), (1, H), (2, D)):
                i = bc.unnormalize(g[:, a], s, index_dtype).astype(np.float64)
                idx.append(np.fmin(np.fmax(i, -2.0), s + 1.0))
        base = [np.floor(i) for i in idx]
        if mutate == "left_cell":  # the cell to the LEFT of an integer coordinate: the same blend, another derivative
            base = [np.ceil(i) - 1.0 for i in idx]
        w = [np.stack([b + 1.0 - i, i - b], 1) for i, b in zip(idx, base)]  # [n, 2] per axis
        t, At = np.zeros((n, 3)), np.zeros((n, 3))
        tch = np.zeros((D, H, W), bool)
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
            xx, yy, zz = (base[0] + dx).astype(np.int64), (base[1] + dy).astype(np.int64), (base[2] + dz).astype(np.int64)
            inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
            xc, yc, zc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1), np.clip(zz, 0, D - 1)
            ok = inb & live[zc, yc, xc]
            if mutate == "drop_corner" and corner == 6:
                ok = np.zeros(n, bool)
            val = np.where(ok[:, None], v64[zc, yc, xc], 0.0)
            p, pa = (dF * val).sum(1), np.abs(dF * val).sum(1)
            pair = (w[1][:, dy] * w[2][:, dz], w[0][:, dx] * w[2][:, dz], w[0][:, dx] * w[1][:, dy])
            for k, d in enumerate((dx, dy, dz)):
                t[:, k] += (p if d else -p) * pair[k]
                At[:, k] += pa * np.abs(pair[k])
            hit = ok & ((pair[0] != 0) | (pair[1] != 0) | (pair[2] != 0))
            tch[zc[hit], yc[hit], xc[hit]] = True
        sc = level_scale(shapes[(l + 1) % 4] if mutate == "level_scale" else shapes[l], voxel, out_sh)
        gc += t * sc[None, :]
        Ac += At * np.abs(sc)[None, :]
        touched.append(tch)
    Rm = np.asarray(Rm, np.float64).reshape(3, 3)
    if mutate == "R_transposed":
        Rm = Rm.T
    return gc @ Rm.T, Ac @ np.abs(Rm).T, touched


# pair weights of level l are multiples of this (the coarsest of the three axis pairs); terms are multiples of UNIT
UNIT = 2.0 ** -7


@functools.lru_cache(maxsize=None)
def lattice_q():
    """[>= 257, 3] quarter-voxel points: the lattice scene of bwd_cases (a walk, the volume's faces, edges and corners — points ON voxel
    planes —, the zero-padding rim on every side, far points beyond the clamp, a scatter), then the scattered row-count points of
    decode_f32_cases; the FIRST point is moved onto a voxel plane of every level so that n = 1 sees a right-hand derivative too"""
    q = bc.tri_lattice_scene()["pts"].astype(np.float64) / (dc.VOXEL[0] / 4)
    assert np.array_equal(q, np.round(q))
    q = np.concatenate([q, np.asarray(dc.rows_case(), np.float64)], 0)
    q[0] = (32.0, 16.0, 32.0)
    assert len(q) >= max(LATTICE_N)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def lattice_d_feat():
    """[len(lattice_q), 352]: per point and level two channels from {-2, -1, 1, 2}, the rest zero; a few points with a level left out"""
    rs = np.random.RandomState(41)
    n = len(lattice_q())
    d = np.zeros((n, 352), F32)
    for l, c in enumerate(bc.LEVEL_CHANNELS):
        for p in range(n):
            ch = rs.choice(c, 2, replace=False)
            d[p, bc.CHAN_BASE[l] + ch] = rs.choice([-2.0, -1.0, 1.0, 2.0], 2)
    d[5, 0:32] = 0
    d[9, 224:352] = 0
    d.setflags(write=False)
    return d


def lattice_grids():
    return bc.tri_lattice_scene()["grids"]


def rows_of(vols, grids, touched=None):
    """the compact active rows [n_rows_l, C_l] of every level in grid order (the grids number their active voxels in linear order);
    touched: rows of voxels outside it hold POISON"""
    out = []
    for l, (v, grid) in enumerate(zip(vols, grids)):
        act = np.asarray(grid) >= 0
        assert np.array_equal(np.asarray(grid)[act], np.arange(int(act.sum())))
        rows = np.array(v[act], F32)
        if touched is not None:
            rows[~touched[l][act]] = F32(POISON)
        out.append(rows)
    return out


def lattice_reference(pose_name, n, mutate=None):
    """-> (world points fp32 [n, 3], d_feat [n, 352], grad float64 [n, 3], A, touched) of the first n lattice points under a pose"""
    w, g = dc.case_grid(lattice_q()[:n], pose_name)
    d = lattice_d_feat()[:n]
    grad, A, touched = grad_f64(g.astype(np.float64), d, dc.distinct_volumes(), dc.VOXEL, dc.OUT_SH, dc.POSES[pose_name]["R"],
                                grids=lattice_grids(), mutate=mutate)
    return w, d, grad, A, touched


def assert_grad_lattice(grad, A):
    """the precondition of the bit-for-bit comparison: every term is a multiple of UNIT and their absolute sum stays below 2^24 units"""
    bc.sc.assert_lattice(A, UNIT)
    assert np.array_equal(grad / UNIT, np.round(grad / UNIT))


@functools.lru_cache(maxsize=None)
def realistic_case():
    """-> dict(pts, pose, g fp32, vols, grids, voxel, out_sh, d_feat fp32, grad float64, A)"""
    s = dict(dc.realistic_scene())
    s["grids"] = bc.tri_realistic_scene()["grids"]
    assert all(tuple(g.shape) == tuple(sh) for g, sh in zip(s["grids"], s["shapes"]))
    s["d_feat"] = np.random.RandomState(9).standard_normal((len(s["pts"]), 352)).astype(F32)
    s["grad"], s["A"], _ = grad_f64(s["g"], s["d_feat"], s["vols"], s["voxel"], s["out_sh"], s["pose"]["R"], grids=s["grids"],
                                    index_dtype=F32)
    return s


# ------------------------------------------------------------------------------------------------------------------------ B
def chain_f64(sd, h1, h2, h3):
    """d sigma / d F [n, 352] in float64 under the ReLU masks of a tap (h > 0)"""
    W = {k: np.asarray(sd[k + ".weight"], np.float64)[:, :, 0] for k in ("fc_0", "fc_1", "fc_2", "alpha_fc")}
    dh = W["alpha_fc"] * (np.asarray(h3) > 0)
    dh = (dh @ W["fc_2"]) * (np.asarray(h2) > 0)
    dh = (dh @ W["fc_1"]) * (np.asarray(h1) > 0)
    return dh @ W["fc_0"]


# ------------------------------------------------------------------------------------------------------------------------ C
@functools.lru_cache(maxsize=None)
def e2e_reference(name, voxel_size=None, first_ray=0):
    """`voxel_size` (dhw, None: the golden scenes' 5 mm cube): the scene's body voxelised, and the oracle's grid coordinates formed, at
    that size.  `first_ray`: the sixteen rays are first_ray + E2E_RAYS.
    -> dict(wpts fp32 [1024, 3], sigma64 [1024], g64 [1024, 3], keep bool [1024], vols: the oracle's fp32 volumes (NCDHW tensors),
    out_sh, recipe, sd, batch, h: the float64 activations h1, h2, h3 [1024, 256], gn: the float64 normalised coordinates) of a golden scene"""
    import torch

    from oracle import neuralbody_oracle as orc
    from tests import helpers as H
    from tests.golden import scenes

    r, sd, body, batch, cam, _ = scenes.build(name, voxel_size)
    sdt, vols, out_sh = H.oracle_volumes(sd, batch, r["mode"] == "train")
    S = 64
    rays = slice(E2E_RAYS.start + first_ray, E2E_RAYS.stop + first_ray, E2E_RAYS.step)
    t = np.linspace(0.0, 1.0, S, dtype=F32)
    z = R.z_vals_f32(batch["near"][0][rays], batch["far"][0][rays], t)
    wpts = R.sample_points_f32(batch["ray_o"][0][rays], batch["ray_d"][0][rays], z)[0].reshape(-1, 3)
    assert wpts.shape == (1024, 3)
    sd64 = orc.tensor_state_dict(sd, dtype=torch.float64)
    vols64 = [v.double() for v in vols]
    sp = {k: torch.from_numpy(np.asarray(batch[k])).double() for k in ("R", "Th", "bounds")}
    sp["out_sh"] = out_sh
    p = torch.from_numpy(wpts.astype(np.float64))[None].requires_grad_(True)
    gcoord = orc.get_grid_coords(orc.pts_to_can_pts(p, sp["R"], sp["Th"]), sp["bounds"], out_sh,
                                 (0.005,) * 3 if voxel_size is None else tuple(voxel_size))[:, None, None]
    x = orc.interpolate_features(gcoord, vols64)
    near_zero = torch.zeros(1024, dtype=torch.bool)
    hs = []
    for layer in ("fc_0", "fc_1", "fc_2"):
        pre = orc._conv1d(sd64, layer, x)  # [1, 256, n]
        near_zero |= (pre.detach().abs() <= PREACT_EXCLUDE * pre.detach().abs().max())[0].any(0)
        x = torch.relu(pre)
        hs.append(x.detach()[0].t().numpy())
    sigma = orc._conv1d(sd64, "alpha_fc", x)[0, 0]
    sigma.sum().backward()
    gn = gcoord.detach()[0, 0, 0].numpy()
    near_plane = np.zeros(1024, bool)
    for v in vols:
        D, H_, W = v.shape[2:]
        for a, s in ((0, W), (1, H_), (2, D)):
            i = bc.unnormalize(gn[:, a], s)
            near_plane |= np.abs(i - np.round(i)) <= INDEX_EXCLUDE
    keep = ~(near_zero.numpy() | near_plane)
    return dict(wpts=wpts, sigma64=sigma.detach().numpy(), g64=p.grad[0].numpy(), keep=keep, vols=vols, out_sh=out_sh, recipe=r, sd=sd,
                batch=batch, h=hs, gn=gn)


# ------------------------------------------------------------------------------------------------------------------------ D
def select_model(ray_o, ray_d, near, far, t_vals, t_rand, weights, w_min):
    """-> (idx int32 [m], wpts fp32 [m, 3]) of nb_normal_select"""
    weights = np.asarray(weights, F32)
    n, S = weights.shape
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(weights.reshape(-1) >= F32(w_min)).astype(np.int32)
    if n * S == 0:
        return idx, np.zeros((0, 3), F32)
    z = R.z_vals_f32(near, far, t_vals, t_rand)
    p = R.sample_points_f32(ray_o, ray_d, z)[0].reshape(-1, 3)
    return idx, p[idx]


def composite_model(idx, grad, weights):
    """-> (normal_map fp32 [n, 3], normal_acc fp32 [n]) of nb_normal_composite: float32, one operation per step, sample order"""
    weights = np.asarray(weights, F32)
    n, S = weights.shape
    grad = np.asarray(grad, F32).reshape(-1, 3)
    nm, na = np.zeros((n, 3), F32), np.zeros(n, F32)
    big = F32(3.4028234664e38)
    with np.errstate(all="ignore"):
        for k, i in enumerate(np.asarray(idx)):
            ray = int(i) // S
            w = weights.reshape(-1)[i]
            gx, gy, gz = grad[k]
            ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
            na[ray] = na[ray] + w
            if not (ln >= F32(1e-12)) or not (ln <= big):
                continue
            nm[ray] = nm[ray] + w * (-grad[k] / ln)
        ln = np.sqrt((nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2])
        unit = (ln >= F32(1e-6)) & (ln <= big)
        out = np.where(unit[:, None], nm / np.where(unit, ln, F32(1))[:, None], F32(0)).astype(F32)
    return out, na


SELECT_SHAPES = ((1, 1), (33, 31), (16, 64), (25, 41), (64, 65))  # n_rays x S = 1, 1023, 1024, 1025, 64 x 65


def select_inputs(n, S, seed=0):
    """rays with power-of-two origins and small-integer directions, integer weights 0..3 (about a third zero) with ray 0 — and one
    ray in the middle — all zero, jitter on a 1/8 lattice"""
    rs = np.random.RandomState(100 + seed + n * S)
    ray_o = rs.randint(-4, 5, (n, 3)).astype(F32)
    ray_d = rs.randint(-3, 4, (n, 3)).astype(F32)
    ray_d[~ray_d.any(1), 2] = 1.0
    near = rs.randint(1, 4, n).astype(F32)
    far = near + rs.randint(1, 5, n).astype(F32)
    t_vals = np.linspace(0.0, 1.0, S, dtype=F32) if S > 1 else np.zeros(1, F32)
    t_rand = (rs.randint(0, 8, (n, S)) / 8.0).astype(F32)
    weights = np.maximum(rs.randint(-2, 4, (n, S)), 0).astype(F32)
    if n > 1:
        weights[0] = 0
        weights[n // 2] = 0
    return ray_o, ray_d, near, far, t_vals, t_rand, weights


def integer_gradients(m, seed=0):
    """[m, 3] axis-aligned integer gradients (so that -g / |g| is a signed unit axis and every sum of integer weights is exact), some zero"""
    rs = np.random.RandomState(7 + seed + m)
    g = np.zeros((m, 3), F32)
    g[np.arange(m), rs.randint(0, 3, m)] = rs.choice([-4.0, -3.0, -1.0, 2.0, 5.0], m)
    g[rs.uniform(size=m) < 0.1] = 0
    return g
