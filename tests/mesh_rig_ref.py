"""Numpy restatements of csrc/nb_mesh_rig.hip (nb_mesh_closest, nb_mesh_rig_bind) and the cases its tests share.

Every function takes a `dtype`.  In np.float32 it is written operation by operation as the header of nb_mesh_rig.hip says — every
intermediate a float32 array, every dot product (x0 y0 + x1 y1) + x2 y2, no fused operation — so that the device's closest query
can be held to its bits.  In np.float64 the same expressions are the model the float32 ones (and through them the device) are
measured against:

    closest: the region walk of Ericson 5.1.5 per (point, triangle), exhaustive, argmin with the lower index on a tie
    bind:    w_j, T = [I|0] + sum_j w_j (A_j - [I|0]), y = rot^T (x - Th), v_shaped = adj(M) / det(M) (y - t),
             v_template = v_shaped - sum_l S_l beta_l; the rigid fallback where !(|det M| >= 2^-10)
    unpose:  the M^-1 (y - t) step alone (the reference's ppts_to_pts, lib/utils/blend_utils.py:73-82)

The body's transforms A_j and rot(Rh) come from `transforms`, smpl_ref.forward's chain stopped before the vertices."""
import numpy as np

from tests import silhouette_ref, smpl_ref

TILE = 64                # triangles per tile of nb_mesh_closest
DET_MIN = 2.0 ** -10     # the degenerate-blend bound of nb_mesh_rig_bind
N_JOINTS, N_BETAS = smpl_ref.N_JOINTS, smpl_ref.N_BETAS


# ------------------------------------------------------------------------------------------- bodies
def surface_smpl(seed, level, radii=(0.35, 0.9, 0.15)):
    """smpl_ref.synthetic_smpl's recipe with an ellipsoidal icosphere as v_template and its faces as f: a body with a surface."""
    v, f = silhouette_ref.icosphere(level, radii)
    model = smpl_ref.synthetic_smpl(seed, v.shape[0], smpl_ref.SMPL_PARENTS)
    model["v_template"], model["f"] = v, f.astype(np.int64)
    return model


def vertex_normals(verts, faces):
    """float64 unit normals, the normalised sum of the incident faces' area-weighted normals."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], n)
    return out / np.linalg.norm(out, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------- closest point
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def region_walk(p, a, b, c, ab, ac, dtype):
    """(v, w) of the closest point of every triangle for every point (broadcast over the leading axes; the last axis is xyz)."""
    one, zero = dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        # the interior, then the regions in reverse order so that the first test that holds decides
        va0, vb0, vc0 = np.where(va < zero, zero, va), np.where(vb < zero, zero, vb), np.where(vc < zero, zero, vc)
        denom = one / ((va0 + vb0) + vc0)
        v, w = vb0 * denom, vc0 * denom
        wbc = e1 / (e1 + e2)
        r = (va <= zero) & (e1 >= zero) & (e2 >= zero)
        v, w = np.where(r, one - wbc, v), np.where(r, wbc, w)
        r = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
        v, w = np.where(r, zero, v), np.where(r, d2 / (d2 - d6), w)
        r = (d6 >= zero) & (d5 <= d6)
        v, w = np.where(r, zero, v), np.where(r, one, w)
        r = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
        v, w = np.where(r, d1 / (d1 - d3), v), np.where(r, zero, w)
        r = (d3 >= zero) & (d4 <= d3)
        v, w = np.where(r, one, v), np.where(r, zero, w)
        r = (d1 <= zero) & (d2 <= zero)
        v, w = np.where(r, zero, v), np.where(r, zero, w)
    assert v.dtype == dtype and w.dtype == dtype
    return v, w


def closest(points, verts, faces, dtype=np.float32, pairs_per_chunk=1 << 18):
    """Exhaustive: points [P,3], verts [V,3] (float32 numbers), faces [Nf,3] -> (face int32 [P], bary dtype [P,3], dist2 dtype [P]).
    A face with an index outside 0..V-1 or a non-finite dist2 is skipped; face = -1, bary = 0, dist2 = inf where nothing is left."""
    p = np.asarray(points, np.float32).astype(dtype).reshape(-1, 3)
    v = np.asarray(verts, np.float32).astype(dtype).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = p.shape[0]
    face, bary, dist2 = np.full(P, -1, np.int32), np.zeros((P, 3), dtype), np.full(P, np.inf, dtype)
    keep = np.flatnonzero(((f >= 0) & (f < v.shape[0])).all(axis=1))
    if keep.size == 0:
        return face, bary, dist2
    a, b, c = v[f[keep, 0]][None], v[f[keep, 1]][None], v[f[keep, 2]][None]
    ab, ac = b - a, c - a
    step = max(1, pairs_per_chunk // keep.size)
    for s in range(0, P, step):
        pp = p[s:s + step, None, :]
        vv, ww = region_walk(pp, a, b, c, ab, ac, dtype)
        with np.errstate(all="ignore"):
            q = (a + ab * vv[..., None]) + ac * ww[..., None]
            e = pp - q
            d = _dot(e, e)
        assert d.dtype == dtype
        d = np.where(np.isfinite(d), d, dtype(np.inf))
        k = np.argmin(d, axis=1)  # the first minimum: the lowest face index, `keep` ascends
        rows = np.arange(pp.shape[0])
        dk = d[rows, k]
        ok = np.isfinite(dk)
        vk, wk = vv[rows, k], ww[rows, k]
        face[s:s + step] = np.where(ok, keep[k], -1)
        bary[s:s + step] = np.where(ok[:, None], np.stack([(dtype(1) - vk) - wk, vk, wk], axis=1), dtype(0))
        dist2[s:s + step] = np.where(ok, dk, dtype(np.inf))
    return face, bary, dist2


def surface_point(verts, faces, face, bary):
    """float64: sum_i bary_i vert_i of the chosen faces."""
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    return np.einsum("pk,pkd->pd", np.asarray(bary, np.float64), t)


def distance_excess(points, verts, faces, face, bary):
    """d64(p, q) - min_f d64(p, f) per point, q the point (face, bary) names: how much farther than the float64 closest point the
    answer lies (metres; it can be slightly negative, bary need not sum to 1 exactly)."""
    q = surface_point(verts, faces, face, bary)
    d = np.linalg.norm(np.asarray(points, np.float64) - q, axis=1)
    return d - np.sqrt(closest(points, verts, faces, np.float64)[2])


# ------------------------------------------------------------------------------------------- transforms of the body
def transforms(model, poses, shapes, Rh, dtype=np.float64):
    """-> (A [24,3,4] the relative transforms, rot [3,3] = rot(Rh), in `dtype`): smpl_ref.forward's chain."""
    f = lambda a: np.asarray(a, np.float32).astype(dtype)  # noqa: E731
    parents = smpl_ref.parents_of(model)
    v_shaped = f(model["v_template"]) + np.matmul(f(model["shapedirs"]), f(shapes).reshape(N_BETAS))
    J = np.matmul(f(model["J_regressor"]), v_shaped)
    R = smpl_ref.rodrigues_lbs(f(poses).reshape(N_JOINTS, 3), dtype)
    G = np.zeros((N_JOINTS, 4, 4), dtype)
    for j in range(N_JOINTS):
        L = np.eye(4, dtype=dtype)
        L[:3, :3] = R[j]
        L[:3, 3] = J[j] if parents[j] < 0 else J[j] - J[parents[j]]
        G[j] = L if parents[j] < 0 else np.matmul(G[parents[j]], L)
    A = G[:, :3, :].copy()
    A[:, :, 3] -= np.matmul(G[:, :3, :3], J[:, :, None])[:, :, 0]
    assert A.dtype == dtype
    return A, smpl_ref.rodrigues_lbs(f(Rh).reshape(1, 3), dtype)[0]


def _blend(w, A, dtype):
    """T [P,12] = sum_j w_j (A_j - [I|0]), j ascending; the identity is added where M is formed."""
    D = (A - np.eye(3, 4, dtype=dtype)[None]).reshape(N_JOINTS, 12)
    T = np.zeros((w.shape[0], 12), dtype)
    for j in range(N_JOINTS):
        T = T + w[:, j:j + 1] * D[j][None]
    return T, D


def _matrix(T, dtype):
    M = T.reshape(-1, 3, 4)[:, :, :3].copy()
    for k in range(3):
        M[:, k, k] = dtype(1) + M[:, k, k]
    C = np.empty_like(M)  # cofactors
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            C[:, r, c] = M[:, r1, c1] * M[:, r2, c2] - M[:, r1, c2] * M[:, r2, c1]
    det = (M[:, 0, 0] * C[:, 0, 0] + M[:, 0, 1] * C[:, 0, 1]) + M[:, 0, 2] * C[:, 0, 2]
    return M, C, det


def _solve(C, det, T, y):
    """adj(M) / det . (y - t), row by row."""
    with np.errstate(all="ignore"):
        d = y - T.reshape(-1, 3, 4)[:, :, 3]
        return np.stack([((C[:, 0, r] / det) * d[:, 0] + (C[:, 1, r] / det) * d[:, 1]) + (C[:, 2, r] / det) * d[:, 2] for r in range(3)], axis=1)


def unpose(y, w, A, dtype=np.float64):
    """Body-frame points y [P,3] with weights w [P,24] and the transforms A [24,3,4] -> (the rest-pose points M^-1 (y - t), det M):
    ppts_to_pts of the reference, with the blend written around the identity.  No rigid fallback here."""
    y, w, A = (np.asarray(a).astype(dtype) for a in (y, w, A))
    T, _ = _blend(w, A[:, :3, :], dtype)
    _, C, det = _matrix(T, dtype)
    return _solve(C, det, T, y), det


def bind(model, poses, shapes, Rh, Th, points, face, bary, dtype=np.float64):
    """nb_mesh_rig_bind -> dict(weights [24,P], shapedirs [10,3P], v_template [P,3], status [4], det [P] before any fallback)."""
    f = lambda a: np.asarray(a, np.float32).astype(dtype)  # noqa: E731
    A, rot = transforms(model, poses, shapes, Rh, dtype)
    W, S, faces = f(model["weights"]), f(model["shapedirs"]), np.asarray(model["f"], np.int64)
    x, b, face = f(points).reshape(-1, 3), f(bary).reshape(-1, 3), np.asarray(face, np.int64)
    P, V = x.shape[0], W.shape[0]
    bound = (face >= 0) & (face < faces.shape[0])
    idx = faces[np.where(bound, face, 0)]
    bound &= ((idx >= 0) & (idx < V)).all(axis=1)
    idx = np.where(bound[:, None], idx, 0)
    b = np.where(bound[:, None], b, dtype(0))
    w = (b[:, 0:1] * W[idx[:, 0]] + b[:, 1:2] * W[idx[:, 1]]) + b[:, 2:3] * W[idx[:, 2]]
    w[~bound] = np.eye(N_JOINTS, dtype=dtype)[0]
    T, D = _blend(w, A, dtype)
    _, C, det0 = _matrix(T, dtype)
    det = det0.copy()
    degenerate = bound & ~(np.abs(det0) >= dtype(DET_MIN))
    rigid = ~bound | degenerate
    jm = np.where(degenerate, np.argmax(w, axis=1), 0)  # argmax: the first, so the lowest j on a tie
    w[rigid] = np.eye(N_JOINTS, dtype=dtype)[jm[rigid]]
    T[rigid] = D[jm[rigid]]
    _, C2, _ = _matrix(T, dtype)
    C[rigid], det[rigid] = C2[rigid], dtype(1)
    dx = x - f(Th).reshape(1, 3)
    y = np.stack([(rot[0, k] * dx[:, 0] + rot[1, k] * dx[:, 1]) + rot[2, k] * dx[:, 2] for k in range(3)], axis=1)
    v_shaped = _solve(C, det, T, y)
    sd = (b[:, 0, None, None] * S[idx[:, 0]] + b[:, 1, None, None] * S[idx[:, 1]]) + b[:, 2, None, None] * S[idx[:, 2]]  # [P,3,10]
    beta = f(shapes).reshape(N_BETAS)
    acc = np.zeros((P, 3), dtype)
    for l in range(N_BETAS):
        acc = acc + sd[:, :, l] * beta[l]
    out = {"weights": np.ascontiguousarray(w.T), "shapedirs": np.ascontiguousarray(sd.transpose(2, 0, 1).reshape(N_BETAS, 3 * P)),
           "v_template": v_shaped - acc, "status": np.array([int((~bound).sum()), int(degenerate.sum()), 0, 0], np.int32), "det": det0}
    assert all(out[k].dtype == dtype for k in ("weights", "shapedirs", "v_template"))
    return out


def rig_forward(model, rig, poses, shapes, Rh, Th, dtype=np.float64):
    """World vertices [P,3] of a rig (the dict of `bind`, or float32 arrays under the same names) driven by the BODY `model`'s
    joints: nb_smpl_pose with new_params = 0 on the rig's arrays."""
    f = lambda a: np.asarray(a).astype(dtype)  # noqa: E731
    A, rot = transforms(model, poses, shapes, Rh, dtype)
    w, vt = f(rig["weights"]).T, f(rig["v_template"])
    P = vt.shape[0]
    sd = f(rig["shapedirs"]).reshape(N_BETAS, P, 3)
    beta = np.asarray(shapes, np.float32).astype(dtype).reshape(N_BETAS)
    acc = np.zeros((P, 3), dtype)
    for l in range(N_BETAS):
        acc = acc + sd[l] * beta[l]
    v = vt + acc
    T, _ = _blend(np.ascontiguousarray(w), A, dtype)
    T = T.reshape(P, 3, 4)
    s = v + (np.einsum("pik,pk->pi", T[:, :, :3], v) + T[:, :, 3])
    out = np.matmul(s, rot.T) + np.asarray(Th, np.float32).astype(dtype).reshape(1, 3)
    assert out.dtype == dtype
    return out


# ------------------------------------------------------------------------------------------- cases
def draw(seed, sigma=0.15, zero_pose=False):
    """smpl_ref.draw_params with the mild poses (sigma 0.15 rad) the bind tests use."""
    return smpl_ref.draw_params(seed, zero_pose=zero_pose, sigma=sigma)


# (model seed, icosphere level, parameter seed): generic bind cases.  The host suite asserts that the float64 model has no vertex
# under DET_MIN for any of them (a cap of zero, not a measurement)
BIND_CASES = {"ico2": (31, 2, 131), "ico3": (32, 3, 132)}


def query_points(verts, faces, seed, n_random=96):
    """The points of the closest-query cases around the surface (verts, faces), float32 [n,3]: exactly on vertices, on edge
    midpoints, at face centroids, inside the body, 1 mm and 0.5 m outside, and one NaN."""
    rs = np.random.RandomState(seed)
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    f = f[((f >= 0) & (f < len(v))).all(axis=1)]
    nv = min(len(v), 40)
    pick = f[rs.randint(0, len(f), 40)]
    tri = v[pick].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    centroid = tri.mean(axis=1)
    parts = [v[rs.choice(len(v), nv, replace=False)], (0.5 * (tri[:, 0] + tri[:, 1])), centroid, centroid + 1e-3 * n, centroid + 0.5 * n,
             rs.uniform(-0.5, 0.5, (n_random, 3)) * np.ptp(v.astype(np.float64), axis=0)[None] + v.astype(np.float64).mean(axis=0)[None],
             np.array([[np.nan, 0.0, 0.0]])]
    return np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(np.float32)


def lattice_points(verts, n, margin=0.03):
    """n points in lattice order (x slowest, z fastest, as marching cubes emits its vertices) over the padded box of `verts`."""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(axis=0) - margin, v.max(axis=0) + margin
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.linspace(lo[k], hi[k], side) for k in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    return g[:n].astype(np.float32)


def odd_faces(faces, n_verts):
    """The face list with an out-of-range index, a negative one, a repeated-vertex face and a collinear (zero-area) face put in
    front, so that they would win every tie."""
    bad = np.array([[0, 1, n_verts], [-1, 2, 3], [1, 1, 3], [2, 2, 2]], np.int32)
    return np.concatenate([bad, np.asarray(faces, np.int32)])


DEGENERATE_JOINTS = (1, 2)  # siblings under the root


def degenerate_case(seed=41, level=2, n=7):
    """A body whose joints 1 and 2 are turned by +-pi/2 about x — rotations that differ by pi about one axis — with `n` vertices
    weighted 1/2, 1/2 on the two: there the blend is diag(1, cos, cos) with cos(pi/2) = 0, singular.  Every other vertex keeps
    its weights on joints outside the two subtrees (whose transforms are the identity).  -> dict(model, params, vertices)."""
    model = surface_smpl(seed, level)
    parents = smpl_ref.SMPL_PARENTS
    moved = set(DEGENERATE_JOINTS)
    for j in range(N_JOINTS):
        if parents[j] in moved:
            moved.add(j)
    W = model["weights"].astype(np.float64)
    cols = sorted(moved)
    W[:, 0] += W[:, cols].sum(axis=1)
    W[:, cols] = 0.0
    rs = np.random.RandomState(seed)
    special = np.sort(rs.choice(W.shape[0], n, replace=False))
    W[special] = 0.0
    W[special, DEGENERATE_JOINTS[0]] = W[special, DEGENERATE_JOINTS[1]] = 0.5
    model["weights"] = W.astype(np.float32)
    poses, shapes, Rh, Th = draw(seed + 100, zero_pose=True)
    poses[3 * DEGENERATE_JOINTS[0]], poses[3 * DEGENERATE_JOINTS[1]] = np.float32(np.pi / 2), np.float32(-np.pi / 2)
    return {"model": model, "params": (poses, shapes, Rh, Th), "vertices": special}


def fixture_case(seed=51, level=2):
    """The inputs ppts_to_pts is recorded for (tests/golden/mesh_rig.npz): body-frame points y [N,3] 2 cm off a posed body's
    vertices, their weights [N,24] and the transforms A [24,4,4], all float32."""
    model = surface_smpl(seed, level)
    poses, shapes, Rh, _ = draw(seed + 100)
    A, _ = transforms(model, poses, shapes, Rh, np.float64)
    zero3 = np.zeros(3, np.float32)
    body = smpl_ref.forward(model, poses, shapes, zero3, zero3)  # Rh = 0, Th = 0: the body's own frame
    y = body + 0.02 * vertex_normals(body, model["f"])
    A4 = np.tile(np.eye(4)[None], (N_JOINTS, 1, 1))
    A4[:, :3, :] = A
    return y.astype(np.float32), model["weights"].astype(np.float32), A4.astype(np.float32)


def bind_case(name, new_params=False):
    """-> dict(model, params, points float32 [P,3]): the body of BIND_CASES[name] in its bind frame and a mesh around it — a shell
    2 cm off every vertex of the posed body (float64 model, rounded), and points 1 mm off face centroids."""
    seed, level, pseed = BIND_CASES[name]
    model, params = surface_smpl(seed, level), draw(pseed)
    body = smpl_ref.forward(model, *params, new_params=new_params)
    tri = body[np.asarray(model["f"])]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    centroid = tri.mean(axis=1) + 1e-3 * n / np.linalg.norm(n, axis=1, keepdims=True)
    points = np.concatenate([body + 0.02 * vertex_normals(body, model["f"]), centroid[::3]]).astype(np.float32)
    return {"model": model, "params": params, "points": points, "new_params": new_params}


# ------------------------------------------------------------------------------------------- the float32 restatement's own error
def e_ref_closest(points, verts, faces):
    """E_ref_closest of a case: the largest |distance excess| (metres) of the float32 restatement's answers against the float64
    model, over the points it answers."""
    face, bary, _ = closest(points, verts, faces, np.float32)
    ok = face >= 0
    if not ok.any():
        return 0.0
    return float(np.abs(distance_excess(np.asarray(points)[ok], verts, faces, face[ok], bary[ok])).max())


def e_ref_bind(model, params, points, face, bary):
    """-> (dict name -> max |float32 restatement - float64 model| over weights, shapedirs, v_template, the two binds)."""
    b32, b64 = (bind(model, *params, points, face, bary, dt) for dt in (np.float32, np.float64))
    return {k: float(np.abs(b32[k].astype(np.float64) - b64[k]).max()) for k in ("weights", "shapedirs", "v_template")}, b32, b64


def e_ref_unpose(y, w, A):
    """E_ref_unpose: max |float32 restatement - float64 model| of the rest-pose points."""
    return float(np.abs(unpose(y, w, A, np.float32)[0].astype(np.float64) - unpose(y, w, A, np.float64)[0]).max())
