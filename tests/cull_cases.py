"""The sample cull's projection (cull_project / cull_inside / cull_pixel, csrc/nb_march_common.h) at pixel edges: cameras, points and
candidate restatements shared by tests/test_cull_cases_host.py and tests/test_gpu_cull.py.  CPU only; nothing here touches the library.

What the cull is held to.  The reference forms the projection with two matrix products and an add (torch.matmul in the renderers,
np.dot in the mesh dataset).  On the CPU both evaluate a row of a 3 x 3 product as the ASCENDING FMA CHAIN
    fma(p2, R2, fma(p1, R1, p0 * R0))
(tests/golden/cull_edges.npz records it from the unmodified reference; tests/test_cull_cases_host.py holds `chain` below to that
fixture at every point).  `chain` is therefore the one restatement the device is held to; the others are MUTANTS: arithmetic a
compiler or a careless rewrite could produce instead, each of which must be told apart from `chain` by the points below.

    chain            t_i = fma(p2, RT_i2, fma(p1, RT_i1, p0 RT_i0)) + RT_i3;  q_i = fma(t2, K_i2, fma(t1, K_i1, t0 K_i0));  q.xy / q.z
    unfused          every product and sum rounded on its own, left to right
    contract_first   fma(p0, R0, p1 * R1), then fma(p2, R2, .): what contracting the first add of the unfused expression gives
    floor_half       chain, the pixel taken as floor(x + .5) instead of rint
    trunc            chain, the pixel taken by truncation

The points.  A checkerboard mask (mask[y, x] = (x + y) & 1) turns any one-pixel difference in x or y into another answer.  Along a
line of fixed float32 (y, z) the float64 pixel coordinate is bisected in x to k + 0.5 for every eighth column k the line crosses; the
float32 x there and its 8 nextafter neighbours on either side are case points; lines of fixed (x, z) do the same for rows.  The float32
projection's error is some tens of ulp of x, so the candidates round to different pixels on a good share of these points
(counts: fixture_counts, asserted per camera by the host test).  The plain cases (`pow2`) use a power-of-two camera, where the
pixel can be stated by hand: exact ties of both parities, q.z < 0, q.z == 0 (inf and NaN: pixel 0), far off each image side,
coordinates beyond 9e18 (pixel 0) and just below (the clamp).

fma32 is exact: the float64 product of two float32 numbers is exact, TwoSum gives the error of the float64 sum, and a float64 sum that
lands on a float32 midpoint is moved off it towards the true value before the final rounding — no double rounding is left.  The
host test checks it against rational arithmetic.
"""
import functools

import numpy as np

F32 = np.float32
H = W = 512
NEIGHBOURS = 8  # nextafter neighbours on each side of a crossing
EVERY = 8       # every eighth pixel column / row a line crosses
# fixture condition, per camera: case points on which the candidates pick different pixels
MIN_CHAIN_VS_UNFUSED, MIN_CHAIN_VS_CONTRACT_FIRST = 32, 8


# ------------------------------------------------------------------------------------------------------------------- arithmetic
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded (see the module docstring)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, F32).astype(np.float64) for v in (a, b, c)))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = np.ascontiguousarray(p + c).reshape(-1)
        p, c = p.reshape(-1), c.reshape(-1)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        tie = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) & (e != 0) & np.isfinite(s) & np.isfinite(e)
        s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32).reshape(a.shape)


def dot3(a, m, arith):
    """sum_k a[k] m[k] of three float32 arrays a[k] and three float32 scalars m[k], in the order `arith` names."""
    if arith == "chain":
        return fma32(a[2], m[2], fma32(a[1], m[1], a[0] * m[0]))
    if arith == "unfused":
        return (a[0] * m[0] + a[1] * m[1]) + a[2] * m[2]
    if arith == "contract_first":
        return fma32(a[2], m[2], fma32(a[0], m[0], a[1] * m[1]))
    raise KeyError(arith)


def project(cam, p, arith="chain"):
    """The float32 pixel coordinates (x, y) of points p [N, 3] before rounding.  cam: dict(K [3,3], RT [3,4]) float32 and, for the
    _msk renderer's pre-affine (if_clight_renderer_msk.py:18-29), R, Th, R0, Th0: q = p - Th, can = q R, p' = can R0^T + Th0."""
    p = np.asarray(p, F32)
    a = [p[:, 0], p[:, 1], p[:, 2]]
    with np.errstate(all="ignore"):
        if "R0" in cam:
            R, Th, R0, Th0 = (np.asarray(cam[k], F32) for k in ("R", "Th", "R0", "Th0"))
            q = [a[k] - Th[k] for k in range(3)]
            can = [dot3(q, R[:, j], arith) for j in range(3)]
            a = [dot3(can, R0[i, :], arith) + Th0[i] for i in range(3)]
        RT, K = np.asarray(cam["RT"], F32), np.asarray(cam["K"], F32)
        t = [dot3(a, RT[i, :3], arith) + RT[i, 3] for i in range(3)]
        q = [dot3(t, K[i, :], arith) for i in range(3)]
        assert all(v.dtype == F32 for v in t + q)
        return q[0] / q[2], q[1] / q[2]


def pixel_index(f, size, rounding="rint"):
    """cull_pixel: round (half to even), 0 for a value that is not finite or beyond the int64 range, clamp to [0, size - 1]."""
    f = np.asarray(f, F32)
    with np.errstate(all="ignore"):
        r = {"rint": np.rint, "floor_half": lambda v: np.floor(v + F32(0.5)), "trunc": np.trunc}[rounding](f)
        assert r.dtype == F32
        r = np.where(np.abs(r) < F32(9.0e18), r, F32(0.0))
    return np.clip(r, 0, size - 1).astype(np.int64)


RESTATEMENTS = {"chain": ("chain", "rint"), "unfused": ("unfused", "rint"), "contract_first": ("contract_first", "rint"),
                "floor_half": ("chain", "floor_half"), "trunc": ("chain", "trunc")}
MUTANTS = tuple(k for k in RESTATEMENTS if k != "chain")


def pixels(cam, p, name="chain"):
    """-> (x, y) int64: the pixel restatement `name` looks a point up at."""
    arith, rounding = RESTATEMENTS[name]
    x, y = project(cam, p, arith)
    return pixel_index(x, W, rounding), pixel_index(y, H, rounding)


def checkerboard():
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((xx + yy) & 1).astype(np.uint8)


def inside(cams, p, name="chain"):
    """cull_inside against the checkerboard in every view of `cams` (a list): bool [N]."""
    out = np.ones(len(p), bool)
    for cam in cams:
        x, y = pixels(cam, p, name)
        out &= ((x + y) & 1) != 0
    return out


def project_f64(cam, p):
    """The same projection in float64 of the float32 inputs -> (x, y)."""
    a = np.asarray(p, np.float64)
    if "R0" in cam:
        a = (a - np.asarray(cam["Th"], np.float64)) @ np.asarray(cam["R"], np.float64)
        a = a @ np.asarray(cam["R0"], np.float64).T + np.asarray(cam["Th0"], np.float64)
    RT, K = np.asarray(cam["RT"], np.float64), np.asarray(cam["K"], np.float64)
    q = (a @ RT[:, :3].T + RT[:, 3]) @ K.T
    return q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]


# ---------------------------------------------------------------------------------------------------------------------- cameras
def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


# the middle of the 'small_dense' scene's body (its Th); the lines stay within HALF of it on every axis: inside the posed box, whose
# smallest half-extent is 0.15 > sqrt(3) HALF
CENTRE = np.array([0.05, -0.1, 0.2])
HALF = 0.085


def pinhole(yaw, pitch, roll, distance, focal, cx, cy):
    """A camera `distance` from CENTRE looking at it: x_cam = R x + T -> dict(K, RT) float32."""
    R = rotation(yaw, pitch, roll)
    eye = CENTRE - distance * R[2]
    K = np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]])
    cam = dict(K=K.astype(F32), RT=np.concatenate([R, (-R @ eye).reshape(3, 1)], 1).astype(F32))
    assert (cam["RT"][:, :3] != 0).all() and focal != round(focal) and cx != round(cx) and cy != round(cy)
    return cam


# yaw, pitch, roll, distance, focal, principal point: the body spans most of the 512 x 512 image in each
_CAMERAS = ((0.7, 0.15, 0.11, 0.8, 2469.5, 255.5, 260.25), (-0.5, -0.3, -0.23, 0.75, 2234.25, 249.75, 251.5),
            (2.6, 0.25, 0.37, 0.85, 2641.75, 262.25, 257.75))
# offsets of the lines from CENTRE, in units of HALF: (the two fixed coordinates) of the lines along x, of the lines along y
_LINES_X = ((0.31, -0.47), (-0.62, 0.55))
_LINES_Y = ((-0.38, 0.29), (0.71, -0.66))
# the power-of-two camera of the plain cases: pixel = 256 (X, Y) / (Z + 2) + 256
POW2 = dict(K=np.array([[256, 0, 256], [0, 256, 256], [0, 0, 1]], F32), RT=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2]], F32))
SET_NAMES = ("cam0", "cam1", "cam2", "pre", "pow2")
EDGE_SETS = SET_NAMES[:4]


@functools.lru_cache(maxsize=None)
def camera(name):
    """The camera of a case set.  'pre': the _msk renderer's set: R, Th are the pose of the 'small_dense' scene (what the march
    kernels read from the scene), R0 / Th0 a snapshot pose a small rotation and a few centimetres away."""
    if name == "pow2":
        return POW2
    if name != "pre":
        return pinhole(*_CAMERAS[int(name[3:])])
    from tests.golden import scenes

    batch = scenes.build("small_dense")[3]
    cam = pinhole(-2.2, -0.2, 0.29, 0.9, 2711.25, 258.25, 253.75)
    cam.update(R=np.ascontiguousarray(batch["R"][0], F32), Th=np.ascontiguousarray(batch["Th"].reshape(3), F32),
               R0=rotation(0.13, -0.08, 0.05).astype(F32), Th0=np.array([0.0437, -0.0913, 0.2071], F32))
    assert (cam["R"] != 0).all() and (cam["R0"] != 0).all() and np.abs(cam["Th"] - CENTRE).max() < 1e-6
    return cam


# ----------------------------------------------------------------------------------------------------------------------- points
def _neighbours(x):
    """x [n] float32 -> [n, 2 NEIGHBOURS + 1]: x and its nextafter neighbours, ascending."""
    cols = [x]
    lo = hi = x
    for _ in range(NEIGHBOURS):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        cols = [lo] + cols + [hi]
    return np.stack(cols, 1)


def edge_line(cam, axis, fixed):
    """Case points along the line of direction `axis` (0: x, crossing columns; 1: y, crossing rows) whose other two coordinates are
    `fixed` (float32, in axis order) and whose moving coordinate runs over CENTRE[axis] -+ HALF -> (coords [n] float32 of the moving
    axis, n = 17 x crossings, ascending per crossing; the crossed pixel boundaries k + 0.5 [n])."""
    others = [a for a in range(3) if a != axis]

    def coord(v):
        p = np.empty((len(v), 3))
        p[:, axis] = v
        p[:, others[0]], p[:, others[1]] = float(fixed[0]), float(fixed[1])
        return project_f64(cam, p)[axis]

    a, b = float(F32(CENTRE[axis] - HALF)), float(F32(CENTRE[axis] + HALF))
    ua, ub = coord(np.array([a]))[0], coord(np.array([b]))[0]
    rising = ub > ua
    lo_u, hi_u = min(ua, ub), max(ua, ub)
    ks = np.arange(np.ceil(lo_u - 0.5), np.floor(hi_u - 0.5) + 1)[::EVERY]
    ks = ks[(ks >= 1) & (ks <= (W if axis == 0 else H) - 3)]  # both pixels beside the edge are on the mask: no clamp hides a difference
    lo, hi = np.full(len(ks), a), np.full(len(ks), b)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = (coord(mid) < ks + 0.5) == rising
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    x = _neighbours((0.5 * (lo + hi)).astype(F32))
    return x.reshape(-1), np.repeat(ks + 0.5, x.shape[1])


@functools.lru_cache(maxsize=None)
def lines(name):
    """The lines of an edge set -> tuple of dict(axis, fixed (float32 [2]), coords [n] float32, edge [n], points [n, 3] float32)."""
    cam = camera(name)
    out = []
    for axis, offs in ((0, _LINES_X), (1, _LINES_Y)):
        others = [a for a in range(3) if a != axis]
        for off in offs:
            fixed = (CENTRE[others] + HALF * np.array(off)).astype(F32)
            coords, edge = edge_line(cam, axis, fixed)
            pts = np.empty((len(coords), 3), F32)
            pts[:, axis] = coords
            pts[:, others[0]], pts[:, others[1]] = fixed
            pts.setflags(write=False)
            out.append(dict(axis=axis, fixed=fixed, coords=coords, edge=edge, points=pts))
    return tuple(out)


# name, point, the pixel it is looked up at
_T = 1.0 / 256.0
PLAIN = tuple(
    # exact ties at depth 1 (Z = -1): x = 256 X + 256 = k + .5 -> k even stays, k odd goes up (half to even)
    [("tie-x-%d" % k, ((k + 0.5 - 256) * _T, (100 - 256) * _T, -1.0), (k if k % 2 == 0 else k + 1, 100)) for k in (10, 11, 300, 301, 0, 509)] +
    [("tie-y-%d" % k, ((77 - 256) * _T, (k + 0.5 - 256) * _T, -1.0), (77, k if k % 2 == 0 else k + 1)) for k in (20, 21, 400, 401, 0, 509)] +
    [("tie-xy", ((6.5 - 256) * _T, (7.5 - 256) * _T, -1.0), (6, 8)),
     ("tie-neg", ((-1.5 - 256) * _T, (-0.5 - 256) * _T, -1.0), (0, 0)),   # -1.5 -> -2, -0.5 -> -0: both clamp to 0
     ("tie-last", ((510.5 - 256) * _T, (511.5 - 256) * _T, -1.0), (510, 511)),  # 511.5 -> 512 -> clamp
     # behind the camera (Z + 2 = -1): projected like any other point, mirrored
     ("behind", (0.25, -0.125, -3.0), (192, 288)),
     ("behind-off", (2.0, 2.0, -3.0), (0, 0)),
     # q.z == 0: +inf, -inf, NaN -> pixel 0
     ("z0-pp", (1.0, 1.0, -2.0), (0, 0)), ("z0-nn", (-1.0, -1.0, -2.0), (0, 0)), ("z0-nan", (0.0, 0.0, -2.0), (0, 0)),
     ("z0-pn", (1.0, -1.0, -2.0), (0, 0)), ("z0-nan-p", (0.0, 1.0, -2.0), (0, 0)),
     # far off each side
     ("off-left", (-100.0, 0.0, -1.0), (0, 256)), ("off-right", (100.0, 0.0, -1.0), (511, 256)),
     ("off-top", (0.0, -3000.0, -1.0), (256, 0)), ("off-bottom", (0.0, 3000.0, -1.0), (256, 511)),
     ("off-corner", (4096.0, -4096.0, -1.0), (511, 0)),
     # beyond the int64 range: pixel 0, not the last one; 2^62 px still clamps
     ("huge-x", (1.0e30, 0.0, -1.0), (0, 256)), ("huge-neg-y", (0.0, -1.0e30, -1.0), (256, 0)), ("huge-both", (3.0e20, 3.0e20, -1.0), (0, 0)),
     ("large-x", (2.0 ** 54, 0.0, -1.0), (511, 256)), ("large-neg-x", (-2.0 ** 54, 0.0, -1.0), (0, 256))])


@functools.lru_cache(maxsize=None)
def points(name):
    """All case points of a set, float32 [N, 3] (never written to): the lines in order, or the plain cases."""
    if name == "pow2":
        pts = np.array([c[1] for c in PLAIN], F32)
        assert (pts.astype(np.float64) == np.array([c[1] for c in PLAIN]))[np.abs(pts) < 1e19].all()  # the stated points are float32 numbers
    else:
        pts = np.concatenate([ln["points"] for ln in lines(name)])
    pts.setflags(write=False)
    return pts


def views(name):
    """The views a set's points are culled against in the fixture and the one-view device tests."""
    return [camera(name)]


def mesh_comparable(cam, p):
    """Points whose pixel coordinates are finite and below 2^31: the mesh dataset casts to int32, whose result beyond that range is
    not defined (the renderers cast to int64; the device follows them)."""
    x, y = project(cam, p, "chain")
    with np.errstate(invalid="ignore"):
        return (np.abs(x) < F32(2.0 ** 31)) & (np.abs(y) < F32(2.0 ** 31))


def fixture_counts(name):
    """-> dict: the number of case points of a set on which `chain` and each mutant look up different pixels."""
    cam, p = camera(name), points(name)
    x0, y0 = pixels(cam, p, "chain")
    out = {}
    for m in MUTANTS:
        x, y = pixels(cam, p, m)
        out[m] = int(((x != x0) | (y != y0)).sum())
    x1, y1 = pixels(cam, p, "unfused")
    x2, y2 = pixels(cam, p, "contract_first")
    out["unfused_vs_contract_first"] = int(((x1 != x2) | (y1 != y2)).sum())
    return out


# ----------------------------------------------------------------------------------------------------- a mesh for the silhouette
SILHOUETTE_SEED = 316  # found by trying seeds 0 .. 316 on the CPU (half a minute); 400 scalings of ico320 and of ico1280 alone gave none


def silhouette_case():
    """One frame of the ico1280 ellipsoid of tests/silhouette_ref.py (642 vertices, 96 x 128, its three orbit views), scaled and
    moved by SILHOUETTE_SEED so that in view 0 one vertex snaps to another 1/256 pixel under the unfused projection than under the
    FMA chain AND the covered pixels change (369 vertex snaps differed over the search; one changed a mask)
    -> dict(verts [1, V, 3] float32, faces, Ks, RTs, H, W)."""
    from tests import silhouette_ref as sil

    kind, _, (Hs, Ws), yaws, distance, focal = sil.BAND_CASES["ico1280"]
    v0, faces = sil.mesh_of(kind)
    rs = np.random.RandomState(SILHOUETTE_SEED)
    v = (F32(rs.uniform(0.7, 1.1)) * v0 + rs.uniform(-0.05, 0.05, 3).astype(F32)).astype(F32)
    Ks, RTs = sil.orbit(yaws, distance, focal * Hs, Hs, Ws)
    return dict(verts=v[None], faces=faces, Ks=Ks, RTs=RTs, H=Hs, W=Ws)


# ------------------------------------------------------------------------------------------------------------- rays for the march
def march_rays(names, n_rays):
    """n_rays rays of S = 2 samples whose two sample positions are case points of the sets `names`, EXACTLY: ray_o has 0 on the line's
    axis and the line's fixed coordinates elsewhere, ray_d is the axis' unit vector, near / far are two coordinates of the line and
    t_vals = (0, 1), so that z_lin gives near 1 + far 0 = near and near 0 + far 1 = far, and ray_point 0 + 1 z = z (the other axes:
    o + 0 z = o).  The points on which chain and unfused (then chain and contract_first) disagree in the line's own view come first.
    -> dict(ray_o, ray_d [n, 3], near, far [n], t_vals [2], points [n, 2, 3]) float32."""
    pool = []
    for name in names:
        cam = camera(name)
        for ln in lines(name):
            x0, y0 = pixels(cam, ln["points"], "chain")
            rank = np.zeros(len(x0), np.int64)
            for w, m in ((2, "unfused"), (1, "contract_first")):
                x, y = pixels(cam, ln["points"], m)
                rank += w * ((x != x0) | (y != y0))
            order = np.argsort(-rank, kind="stable")
            pool.append((ln, order[: len(order) // 2 * 2].reshape(-1, 2)))
    rays, k = [], 0
    while len(rays) < n_rays:  # round-robin over the lines
        took = False
        for ln, pairs in pool:
            if k < len(pairs) and len(rays) < n_rays:
                rays.append((ln, pairs[k]))
                took = True
        assert took, "not enough case points for %d rays" % n_rays
        k += 1
    o, d = np.zeros((n_rays, 3), F32), np.zeros((n_rays, 3), F32)
    near, far = np.zeros(n_rays, F32), np.zeros(n_rays, F32)
    pts = np.zeros((n_rays, 2, 3), F32)
    for r, (ln, (i, j)) in enumerate(rays):
        others = [a for a in range(3) if a != ln["axis"]]
        o[r, others[0]], o[r, others[1]] = ln["fixed"]
        d[r, ln["axis"]] = 1.0
        near[r], far[r] = ln["coords"][i], ln["coords"][j]
        pts[r, 0], pts[r, 1] = ln["points"][i], ln["points"][j]
    return dict(ray_o=o, ray_d=d, near=near, far=far, t_vals=np.array([0.0, 1.0], F32), points=pts)
