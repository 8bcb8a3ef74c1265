"""Numpy references of nb_mesh_vertex_normals and nb_mesh_render (csrc/nb_mesh_render.hip), and the camera of the reference's
tools/render_mesh.py as it states it.

  reference_normals / reference_render   float64 on UNSNAPPED vertices: per pixel centre the nearest covering triangle and its
                                         interpolated colour -- what the pictures mean.
  snapped_normals / snapped_render       include/nb_hip.h's definition, operation for operation, in numpy float32 / int64 (numpy
                                         float32 arithmetic rounds every operation to nearest, as the kernels' operators do with
                                         contraction off) -- what the kernels compute, bit for bit.
  stable                                 the pixels whose centre is farther than tau = 1/256 px from every projected edge.  The snap
                                         moves a vertex by at most sqrt(2) * 0.5 / 256 + (fp32 projection error) ~ 2.8e-3 px < tau,
                                         so on a stable pixel the snapped and the unsnapped triangles cover alike.
  gl_chain                               look-at rotation and translation, axis_adj, the ortho matrix, NDC -> window, the row flip.
"""
import math

import numpy as np

TAU = 1.0 / 256.0
MAX_PIXEL = 32768.0
f32 = np.float32


def _valid(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


# ------------------------------------------------------------------------------------------- normals
def reference_normals(verts, faces):
    """compute_normal of tools/render_mesh.py:32-51 in float64; a face with an index outside the vertices is skipped."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[_valid(f, len(v))]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1), 1e-8)[:, None]
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], n)
    return out / np.maximum(np.linalg.norm(out, axis=1), 1e-8)[:, None]


def _length(x, y, z):
    return np.maximum(np.sqrt((x * x + y * y) + z * z), f32(1e-8))


def snapped_normals(verts, faces):
    """-> float32 [V,3], the bits nb_mesh_vertex_normals writes."""
    v = np.ascontiguousarray(verts, f32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[_valid(f, len(v))]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    assert nx.dtype == f32
    with np.errstate(all="ignore"):
        ln = _length(nx, ny, nz)
        q = np.stack([(nx / ln) * f32(2.0 ** 20), (ny / ln) * f32(2.0 ** 20), (nz / ln) * f32(2.0 ** 20)], axis=1)
        ok = (np.abs(q) <= f32(2.0 ** 21)).all(axis=1)  # False for a NaN
    qi = np.rint(q[ok]).astype(np.int64)
    acc = np.zeros((len(v), 3), np.int64)
    for k in range(3):
        np.add.at(acc, f[ok][:, k], qi)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    s = acc.astype(np.int32).astype(f32) * f32(2.0 ** -20)
    ln = _length(s[:, 0], s[:, 1], s[:, 2])
    out = s / ln[:, None]
    assert out.dtype == f32
    return out


# ------------------------------------------------------------------------------------------- pictures
def _ordered_bits(d):
    u = np.ascontiguousarray(d, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def snapped_render(verts, normals, faces, cam, H, W):
    """One view of nb_mesh_render on the host -> (rgb float32 [H,W,3], face_id int32 [H,W], depth float32 [H,W])."""
    v, n, cam = np.ascontiguousarray(verts, f32), np.ascontiguousarray(normals, f32), np.ascontiguousarray(cam, f32).reshape(24)
    M, N = cam[:12].reshape(3, 4), cam[12:21].reshape(3, 3)
    V = len(v)
    with np.errstate(all="ignore"):
        r = [((M[i, 0] * v[:, 0] + M[i, 1] * v[:, 1]) + M[i, 2] * v[:, 2]) + M[i, 3] for i in range(3)]
        col = np.stack([f32(0.5) * ((N[i, 0] * n[:, 0] + N[i, 1] * n[:, 1]) + N[i, 2] * n[:, 2]) + f32(0.5) for i in range(3)], axis=1)
        assert all(x.dtype == f32 for x in r) and col.dtype == f32
        ok = (np.abs(r[0]) <= f32(MAX_PIXEL)) & (np.abs(r[1]) <= f32(MAX_PIXEL)) & (np.abs(r[2]) <= np.finfo(f32).max)
        sx = np.where(ok, np.rint(f32(256) * np.where(ok, r[0], f32(0))), 0).astype(np.int64)
        sy = np.where(ok, np.rint(f32(256) * np.where(ok, r[1], f32(0))), 0).astype(np.int64)
    keys = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    rgb = np.ones((H, W, 3), f32)
    face_id = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf, f32)
    for t, face in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        i0, i1, i2 = (int(k) for k in face)
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V or not (ok[i0] and ok[i1] and ok[i2]):
            continue
        area = (sx[i1] - sx[i0]) * (sy[i2] - sy[i0]) - (sy[i1] - sy[i0]) * (sx[i2] - sx[i0])
        if area == 0:
            continue
        if area < 0:
            i1, i2 = i2, i1
        idx = (i0, i1, i2)
        px, py = [int(sx[k]) for k in idx], [int(sy[k]) for k in idx]
        # the centres 256 i + 128 inside [min, max]: ceil((min - 128) / 256) .. floor((max - 128) / 256)
        x0, x1 = max(-((128 - min(px)) // 256), 0), min((max(px) - 128) // 256, W - 1)
        y0, y1 = max(-((128 - min(py)) // 256), 0), min((max(py) - 128) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(256 * np.arange(x0, x1 + 1, dtype=np.int64) + 128, 256 * np.arange(y0, y1 + 1, dtype=np.int64) + 128)
        E = []
        for i in range(3):  # the edge opposite vertex i
            p, q = (i + 1) % 3, (i + 2) % 3
            E.append((px[q] - px[p]) * (Y - py[p]) - (py[q] - py[p]) * (X - px[p]))
        cover = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
        if not cover.any():
            continue
        with np.errstate(all="ignore"):
            total = (E[0] + E[1] + E[2]).astype(f32)
            l1, l2 = E[1].astype(f32) / total, E[2].astype(f32) / total

            def mix(a0, a1, a2):
                return (a0 + l1 * (a1 - a0)) + l2 * (a2 - a0)

            d = mix(r[2][idx[0]], r[2][idx[1]], r[2][idx[2]])
            assert d.dtype == f32
            key = (_ordered_bits(d) << np.uint64(32)) | np.uint64(t)
            box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            win = cover & (np.abs(d) <= np.finfo(f32).max) & (key < keys[box])
            keys[box] = np.where(win, key, keys[box])
            depth[box] = np.where(win, d, depth[box])
            face_id[box] = np.where(win, np.int32(t), face_id[box])
            for ch in range(3):
                rgb[box + (ch,)] = np.where(win, mix(col[idx[0], ch], col[idx[1], ch], col[idx[2], ch]), rgb[box + (ch,)])
    return rgb, face_id, depth


def snapped_stack(verts, normals, faces, cams, H, W):
    out = [snapped_render(verts, normals, faces, cam, H, W) for cam in np.asarray(cams).reshape(-1, 24)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def _project64(verts, cam):
    cam = np.asarray(cam, np.float64).reshape(24)
    return np.asarray(verts, np.float64) @ cam[:12].reshape(3, 4)[:, :3].T + cam[:12].reshape(3, 4)[:, 3]


def reference_render(verts, normals, faces, cam, H, W):
    """float64, unsnapped: per pixel centre (i + 1/2, j + 1/2) the covering triangle of smallest interpolated depth (the lower
    index on a tie) and its interpolated colour 0.5 N n + 0.5 -> (rgb float64 [H,W,3], face_id int32 [H,W], depth float64 [H,W]).
    `normals` are the float64 reference_normals; `cam` is the float32 row the device gets."""
    p = _project64(verts, cam)
    col = 0.5 * np.asarray(normals, np.float64) @ np.asarray(cam, np.float64).reshape(24)[12:21].reshape(3, 3).T + 0.5
    rgb, face_id, depth = np.ones((H, W, 3)), np.full((H, W), -1, np.int32), np.full((H, W), np.inf)
    for t, face in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        if face.min() < 0 or face.max() >= len(p):
            continue
        a, b, c = p[face[0]], p[face[1]], p[face[2]]
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0.0:
            continue
        x0, x1 = max(int(math.ceil(min(a[0], b[0], c[0]) - 0.5)), 0), min(int(math.floor(max(a[0], b[0], c[0]) - 0.5)), W - 1)
        y0, y1 = max(int(math.ceil(min(a[1], b[1], c[1]) - 0.5)), 0), min(int(math.floor(max(a[1], b[1], c[1]) - 0.5)), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        l1 = ((a[0] - c[0]) * (Y - c[1]) - (a[1] - c[1]) * (X - c[0])) / area  # the edge c -> a, opposite b
        l2 = ((b[0] - a[0]) * (Y - a[1]) - (b[1] - a[1]) * (X - a[0])) / area  # the edge a -> b, opposite c
        l0 = 1.0 - l1 - l2
        d = l0 * a[2] + l1 * b[2] + l2 * c[2]
        box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        win = (l0 >= 0) & (l1 >= 0) & (l2 >= 0) & (d < depth[box])
        depth[box] = np.where(win, d, depth[box])
        face_id[box] = np.where(win, np.int32(t), face_id[box])
        for ch in range(3):
            rgb[box + (ch,)] = np.where(win, l0 * col[face[0], ch] + l1 * col[face[1], ch] + l2 * col[face[2], ch], rgb[box + (ch,)])
    return rgb, face_id, depth


def stable(verts, faces, cam, H, W, tau=TAU):
    """bool [H,W]: the pixel's centre is farther than `tau` px from every projected edge (as a segment) of every face."""
    p = _project64(verts, cam)[:, :2]
    out = np.ones((H, W), bool)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[_valid(f, len(p))]
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    for ia, ib in edges:
        a, b = p[ia], p[ib]
        x0, x1 = max(int(math.floor(min(a[0], b[0]) - 0.5 - tau)), 0), min(int(math.ceil(max(a[0], b[0]) - 0.5 + tau)), W - 1)
        y0, y1 = max(int(math.floor(min(a[1], b[1]) - 0.5 - tau)), 0), min(int(math.ceil(max(a[1], b[1]) - 0.5 + tau)), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        e = b - a
        ee = float(e @ e)
        s = np.clip(((X - a[0]) * e[0] + (Y - a[1]) * e[1]) / ee, 0.0, 1.0) if ee > 0.0 else np.zeros_like(X)
        dist = np.hypot(X - (a[0] + s * e[0]), Y - (a[1] + s * e[1]))
        out[y0:y1 + 1, x0:x1 + 1] &= dist > tau
    return out


# ------------------------------------------------------------------------------------------- the reference's camera, as stated
NEAR, FAR = -100.0, 10.0  # render_mesh.py:101-102


def _make_rotate(rx, ry, rz):
    """render_mesh.py:54-86: Rz Ry Rx."""
    sx, sy, sz, cx, cy, cz = math.sin(rx), math.sin(ry), math.sin(rz), math.cos(rx), math.cos(ry), math.cos(rz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


def dataset_rotation(dataset):
    return _make_rotate(0.0, 0.0, 0.0) if dataset == "zju_mocap" else _make_rotate(0.0, math.radians(90), math.radians(90))


def turned(verts, dataset):
    """render_mesh.py:132-136: the vertices through rot and the dataset's rotation, float64."""
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    return np.asarray(verts, np.float64) @ rot.T @ dataset_rotation(dataset).T


def gl_chain(lo, hi, k, H, W, dataset="zju_mocap", ortho_ratio=1.2):
    """View k of render_mesh.py:120-170 as 4 x 4 matrices applied to an object-space vertex, float64 ->
    (window [3,4]: the affine to (x_px, y_px from the top row, z_window), normal [3,3]: the rotation of the vertices the normals are
    computed from).  z_window = (z_ndc + 1) / 2 is what GL_LESS compares."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def affine(R, t=(0.0, 0.0, 0.0)):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, t
        return m

    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    model = affine(dataset_rotation(dataset)) @ affine(rot)                 # :133, :136
    model = affine(np.eye(3), -0.5 * (hi + lo)) @ model                     # :141
    model = affine(np.eye(3) / (hi[1] - lo[1])) @ model                     # :142
    turn = _make_rotate(0.0, math.radians(-90), 0.0)                        # :148-149
    for _ in range(k + 1):                                                  # :157-158, once per picture before it is drawn
        turn = _make_rotate(0.0, math.radians(-4), 0.0) @ turn
    model = affine(turn) @ model
    # camera.py:81-105 with eye = (0, 0, 2), center = 0, up = (0, 1, 0)
    eye, center, up = np.array([0.0, 0.0, 2.0]), np.zeros(3), np.array([0.0, 1.0, 0.0])
    d = -(eye - center) / np.linalg.norm(eye - center)
    right = -np.cross(up, d)
    u = np.cross(d, right)
    rot_mat = np.stack([right, u, d])
    trans = -rot_mat.T @ eye
    axis_adj = np.diag([1.0, -1.0, -1.0, 1.0])
    model_view = axis_adj @ affine(rot_mat, trans)                          # camera.py:167-173
    width, height = 1.0, H / W                                              # render_mesh.py:99
    left, rgt, bottom, top = -width * ortho_ratio / 2, width * ortho_ratio / 2, -height * ortho_ratio / 2, height * ortho_ratio / 2
    ortho = np.eye(4)                                                       # glm.py:114-123 (returned transposed)
    ortho[0, 0], ortho[1, 1], ortho[2, 2] = 2.0 / (rgt - left), 2.0 / (top - bottom), -2.0 / (FAR - NEAR)
    ortho[0, 3], ortho[1, 3], ortho[2, 3] = -(rgt + left) / (rgt - left), -(top + bottom) / (top - bottom), -(FAR + NEAR) / (FAR - NEAR)
    ndc = ortho @ model_view @ model
    window = np.stack([0.5 * W * (ndc[0] + ndc[3]), 0.5 * H * (ndc[1] + ndc[3]), 0.5 * (ndc[2] + ndc[3])])  # the viewport transform
    window[1] = H * ndc[3] - window[1]                                      # np.flip of the rows: y from the top
    return window[:, :4], (turn @ dataset_rotation(dataset) @ rot)
