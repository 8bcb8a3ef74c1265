"""A seeded synthetic SMPL-shaped body model and numpy restatements of SMPLlayer.forward (zju_smpl/smplmodel/body_model.py:89-153
over lbs.py:142-233, 280-378; return_verts=True, scale=1), written from the formulas:

    R_j      = I + sin(a) K + (1 - cos(a)) K^2,  a = |r_j + 1e-8|,  K = skew(r_j / a)        (batch_rodrigues, as written there)
    v_shaped = v_template + shapedirs . beta,    J = J_regressor . v_shaped
    v_posed  = v_shaped + (R_1..23 - I) . posedirs   (new_params only)
    G_j      = G_parent(j) . [R_j | J_j - J_parent(j)],   A_j = G_j - [0 | G_j . (J_j, 0)]
    v'       = (sum_j W[v,j] A_j) . (v_posed, 1),   world = v' . rot(Rh)^T + Th

`forward(model, ..., dtype)` evaluates them in float64 (the tests' reference) or float32 (the host frame tools/bench_smpl_pose.py
times).  The model arrays carry the reference pickle's names and shapes.

`voxelize_f32` restates nb_smpl_voxelize operation by operation (and names its mutants): see the section at the end."""
import numpy as np

SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
N_JOINTS, N_BETAS = 24, 10
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")


def random_tree(seed, n=N_JOINTS):
    """A valid kinematic tree: parents[0] = -1, parents[j] drawn from 0 .. j - 1."""
    rs = np.random.RandomState(seed)
    return [-1] + [int(rs.randint(0, j)) for j in range(1, n)]


def synthetic_smpl(seed, V, parents, box=(0.7, 1.8, 0.3)):
    """A body-sized model of V vertices: vertices uniform in a 0.7 x 1.8 x 0.3 m box (`box`), shapedirs sigma 0.01, posedirs sigma 0.003,
    every joint regressed from 12 vertices (convex weights), 4 non-zero skinning weights per vertex (convex, float64 normalised,
    rounded to float32 like everything else).  -> dict with the reference pickle's keys (posedirs [V,3,207], kintree_table [2,24])."""
    rs = np.random.RandomState(seed)
    v_template = (rs.uniform(-0.5, 0.5, (V, 3)) * np.array(box)).astype(np.float32)
    shapedirs = (0.01 * rs.standard_normal((V, 3, N_BETAS))).astype(np.float32)
    posedirs = (0.003 * rs.standard_normal((V, 3, 9 * (N_JOINTS - 1)))).astype(np.float32)
    J_regressor = np.zeros((N_JOINTS, V), np.float64)
    for j in range(N_JOINTS):
        idx = rs.choice(V, 12, replace=False)
        w = rs.uniform(0.2, 1.0, 12)
        J_regressor[j, idx] = w / w.sum()
    weights = np.zeros((V, N_JOINTS), np.float64)
    for v in range(V):
        idx = rs.choice(N_JOINTS, 4, replace=False)
        w = rs.uniform(0.05, 1.0, 4)
        weights[v, idx] = w / w.sum()
    kintree = np.stack([np.array(parents, np.int64), np.arange(N_JOINTS)])
    kintree[0, 0] = 2 ** 32 - 1  # the pickle's own root entry (uint32 -1); SMPLlayer overwrites it with -1
    return {"v_template": v_template, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": J_regressor.astype(np.float32),
            "weights": weights.astype(np.float32), "kintree_table": kintree, "f": np.zeros((1, 3), np.int64)}


def checksums(model):
    """float64 sum and sum of squares of every model array, in MODEL_KEYS order -> [5,2]."""
    return np.array([[np.sum(model[k], dtype=np.float64), np.sum(np.square(model[k], dtype=np.float64))] for k in MODEL_KEYS])


def parents_of(model):
    p = [int(v) for v in np.asarray(model["kintree_table"])[0]] if "kintree_table" in model else [int(v) for v in model["parents"]]
    p[0] = -1
    return p


def rodrigues_lbs(r, dtype):
    """batch_rodrigues for r [n,3] in `dtype` -> [n,3,3]."""
    r = np.asarray(r, dtype)
    shifted = r + dtype(1e-8)
    angle = np.sqrt(np.sum(shifted * shifted, axis=1, dtype=dtype), dtype=dtype)[:, None]
    d = r / angle
    K = np.zeros((r.shape[0], 3, 3), dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    s, c = np.sin(angle, dtype=dtype)[:, :, None], np.cos(angle, dtype=dtype)[:, :, None]
    return np.eye(3, dtype=dtype)[None] + s * K + (dtype(1) - c) * np.matmul(K, K)


def forward(model, poses, shapes, Rh, Th, new_params=False, dtype=np.float64, want_shaped=False):
    """One frame: poses [72], shapes [10], Rh [3], Th [3] -> world vertices [V,3] in `dtype` (and v_shaped with want_shaped)."""
    f = lambda a: np.asarray(a, np.float32).astype(dtype)  # noqa: E731 (the model and the parameters are float32 numbers)
    parents = parents_of(model)
    v_template, shapedirs, W, Jr = f(model["v_template"]), f(model["shapedirs"]), f(model["weights"]), f(model["J_regressor"])
    V = v_template.shape[0]
    v_shaped = v_template + np.matmul(shapedirs, f(shapes).reshape(N_BETAS))
    J = np.matmul(Jr, v_shaped)
    R = rodrigues_lbs(f(poses).reshape(N_JOINTS, 3), dtype)
    v_posed = v_shaped
    if new_params:
        posedirs = f(model["posedirs"]).reshape(3 * V, -1)
        feat = (R[1:] - np.eye(3, dtype=dtype)).reshape(-1)
        v_posed = np.matmul(posedirs, feat).reshape(V, 3) + v_shaped
    G = np.zeros((N_JOINTS, 4, 4), dtype)
    for j in range(N_JOINTS):
        L = np.eye(4, dtype=dtype)
        L[:3, :3] = R[j]
        L[:3, 3] = J[j] if parents[j] < 0 else J[j] - J[parents[j]]
        G[j] = L if parents[j] < 0 else np.matmul(G[parents[j]], L)
    A = G.copy()
    A[:, :3, 3] -= np.matmul(G[:, :3, :3], J[:, :, None])[:, :, 0]
    T = np.matmul(W, A.reshape(N_JOINTS, 16)).reshape(V, 4, 4)
    v = np.matmul(T[:, :3, :3], v_posed[:, :, None])[:, :, 0] + T[:, :3, 3]
    rot = rodrigues_lbs(f(Rh).reshape(1, 3), dtype)[0]
    world = np.matmul(v, rot.T) + f(Th).reshape(1, 3)
    return (world, v_shaped) if want_shaped else world


# ------------------------------------------------------------------------------------------- the fixture's cases
def draw_params(seed, zero_pose=False, sigma=0.4):
    """poses sigma 0.4 rad, shapes sigma 1, a non-zero Rh, Th within +-1 m (float32, as params/{i}.npy holds them)."""
    rs = np.random.RandomState(seed)
    poses = (sigma * rs.standard_normal(72)).astype(np.float32)
    shapes = rs.standard_normal(N_BETAS).astype(np.float32)
    Rh = rs.uniform(-1.5, 1.5, 3).astype(np.float32)
    Th = rs.uniform(-1.0, 1.0, 3).astype(np.float32)
    if zero_pose:
        poses[:] = 0
    return poses, shapes, Rh, Th


# name -> (model seed, V, tree, new_params, parameter seed, zero pose).  The parameter seeds are the first of 101 + 10 k, 102 + 10 k, ...
# whose vertices pass voxel_case_check below (make_golden_smpl.py asserts it)
CASES = {
    "smpl6890_old": (11, 6890, "smpl", False, 111, False),
    "smpl6890_new": (11, 6890, "smpl", True, 152, False),
    "tree321_old": (12, 321, "random", False, 113, False),
    "tree321_new": (12, 321, "random", True, 104, False),
    "tree321_zero": (12, 321, "random", True, 115, True),
}


def case_model(name):
    seed, V, tree = CASES[name][:3]
    return synthetic_smpl(seed, V, SMPL_PARENTS if tree == "smpl" else random_tree(seed))


def case_params(name):
    return draw_params(CASES[name][4], zero_pose=CASES[name][5])


# ------------------------------------------------------------------------------------------- voxelisation
VOXEL_SIZE = (0.005, 0.005, 0.005)
BAND = 1e-3  # of a voxel, around a fractional part of 1/2
# (case whose reference vertices are voxelised, pad mode)
VOXEL_CASES = [("smpl6890_old", "zju"), ("smpl6890_new", "big_box"), ("smpl6890_new", "snapshot"), ("tree321_old", "zju"),
               ("tree321_new", "big_box"), ("tree321_zero", "snapshot")]
PADS = {"zju": (0.0, 0.0, 0.05), "big_box": (0.05, 0.05, 0.05), "snapshot": (0.0, 0.1, 0.0)}


def padded_min_max(p, pad):
    """min / max over the rows of a float32 [n,3], padded as the reference pads: a float32 operation on the float32 result."""
    lo, hi = np.min(p, axis=0), np.max(p, axis=0)
    assert lo.dtype == np.float32
    for a in range(3):
        if PADS[pad][a]:
            lo[a] -= PADS[pad][a]
            hi[a] += PADS[pad][a]
    return np.stack([lo, hi])


def host_frame(verts, Rh, Th, pad, voxel_size=VOXEL_SIZE):
    """The host frame of the package: train_rays.multi_view_frame ('zju', 'big_box'), novel_view.rotate_smpl_frame(t = 0)
    ('snapshot')."""
    from neuralbody_amd.novel_view import rotate_smpl_frame
    from neuralbody_amd.train_rays import multi_view_frame

    if pad == "snapshot":
        return rotate_smpl_frame(verts, Rh, Th, 0.0, voxel_size)
    return multi_view_frame(verts, Rh, Th, voxel_size, big_box=(pad == "big_box"))


def coord_f64(verts, R, Th, pad, voxel_size=VOXEL_SIZE):
    """The voxel coordinates before rounding, in float64 from the float32 inputs (R: the float32 matrix) -> ([V,3] dhw, raw
    extents [3] dhw before the ceil)."""
    s = np.matmul(np.asarray(verts, np.float64) - np.asarray(Th, np.float64).reshape(1, 3), np.asarray(R, np.float64))
    lo = s.min(axis=0) - np.array(PADS[pad])
    hi = s.max(axis=0) + np.array(PADS[pad])
    vs = np.array(voxel_size, np.float64)
    return (s - lo)[:, ::-1] / vs, (hi - lo)[::-1] / vs


def near_band(c64):
    return np.abs((c64 - np.floor(c64)) - 0.5) <= BAND


def voxel_case_check(verts, Rh, Th, pad):
    """What a voxelisation case has to satisfy to be a test case: every raw extent (voxels) at least 2 from a multiple of 32,
    so that out_sh does not hang on a rounding; at most 1 % of the coordinates in the band."""
    host = host_frame(verts, Rh, Th, pad)
    c64, raw = coord_f64(verts, host["R"], host["Th"], pad)
    m = np.mod(raw, 32.0)
    band = float(near_band(c64).mean())
    return {"raw": np.round(raw, 2), "band": band, "ok": bool(np.all((m >= 2.0) & (m <= 30.0)) and band <= 0.01)}


# ------------------------------------------------------------------------------------------- the voxeliser, operation by operation
# What nb_smpl_voxelize computes, in its own order (include/nb_hip.h, the header of csrc/nb_smpl.hip), so that the device can be held
# to it at EVERY coordinate, the ones next to a half-integer included:
#   d = fl32(v - Th);  s_i = fma(d2, R[2,i], fma(d1, R[1,i], fl32(d0 R[0,i])));  lo, hi = min, max over the vertices;
#   the pad as one float32 operation on each (an unpadded axis adds 0);  coord (dhw) = rint(float64(fl32(s - lo)) / vs), half to even;
#   out_sh (dhw) = (ceil(float64(fl32(hi - lo)) / vs) | 31) + 1;  summary = can_bounds' six floats bit-cast | out_sh.
# The others are MUTANTS: what a careless rewrite would compute instead.  tests/voxelize_cases.py holds the cases that tell them apart.
VOXELIZERS = {
    "exact": {},
    "vs_reversed": dict(reverse_vs=True),      # voxel_size read in xyz order
    "half_away": dict(rounding="half_away"),   # round() of C instead of rint()
    "unfused": dict(arith="unfused"),          # every product and sum rounded on its own, left to right
    "floor_plus_1": dict(extent="floor_plus_1"),  # floor(x) + 1 in place of ceil(x)
}
VOXEL_MUTANTS = tuple(k for k in VOXELIZERS if k != "exact")


def smpl_space_f32(verts, R, Th, arith="chain"):
    """(v - Th) . R in float32, column by column, in the kernel's order -> [V,3] float32."""
    from tests.cull_cases import dot3

    verts, R, Th = np.asarray(verts, np.float32), np.asarray(R, np.float32), np.asarray(Th, np.float32).reshape(3)
    d = [verts[:, k] - Th[k] for k in range(3)]
    s = np.stack([dot3(d, R[:, i], arith) for i in range(3)], axis=1)
    assert s.dtype == np.float32
    return s


def voxelize_f32(verts, R, Th, voxel_size, pad, variant="exact"):
    """One frame: verts [V,3], R [3,3], Th [3] float32, voxel_size three Python floats (dhw), pad a key of PADS -> dict(coord [V,3]
    i32 (dhw), bounds [2,3] f32 (SMPL space), out_sh [3] i32 (dhw), summary [9] i32) as restatement `variant` computes them."""
    kw = VOXELIZERS[variant]
    verts = np.asarray(verts, np.float32)
    vs = np.array([float(v) for v in voxel_size], np.float64)
    if kw.get("reverse_vs"):
        vs = vs[::-1]
    pd = np.array(PADS[pad], np.float32)
    s = smpl_space_f32(verts, R, Th, kw.get("arith", "chain"))
    wlo, whi = verts.min(axis=0) - pd, verts.max(axis=0) + pd
    slo, shi = s.min(axis=0) - pd, s.max(axis=0) + pd
    assert wlo.dtype == whi.dtype == slo.dtype == shi.dtype == np.float32
    c = (s - slo[None])[:, ::-1].astype(np.float64) / vs[None]
    coord = np.rint(c) if kw.get("rounding", "rint") == "rint" else np.trunc(c + np.copysign(0.5, c))
    e = (shi - slo)[::-1].astype(np.float64) / vs
    cells = np.ceil(e) if kw.get("extent", "ceil") == "ceil" else np.floor(e) + 1.0
    out_sh = (cells.astype(np.int32) | 31) + 1
    summary = np.concatenate([np.stack([wlo, whi]).reshape(-1).view(np.int32), out_sh])
    return {"coord": coord.astype(np.int32), "bounds": np.stack([slo, shi]), "out_sh": out_sh, "summary": summary}
