"""Numpy reference of nb_smpl_silhouette (csrc/nb_silhouette.hip), in float64 on UNSNAPPED vertices, and the meshes and cameras the
silhouette tests share.

The kernel snaps a projected vertex to 1/256 pixel, which moves it by at most
    delta = sqrt(2) * 0.5 / 256 + (fp32 projection error) ~ 2.8e-3 px.
With tau = 1/256 px > delta, per triangle T:
    hi = the pixels whose square of half-side 1/2 + tau meets T,
    lo = the pixels whose square of half-side 1/2 meets T eroded by tau: T scaled about its incentre by 1 - tau / r (r the inradius),
         empty when r <= tau,
both by the one separating-axis test (`square_meets_triangle`).  The snapped triangle T' satisfies T' within T (+) B_delta and
T (-) B_delta within T' (convex sets), so a correct kernel gives   union(lo) <= mask <= union(hi).
The band union(hi) \\ union(lo) is where the reference does not decide; the host suite caps it at BAND_CAP of a mask's pixels for
every mesh the device tests use.
"""
import math

import numpy as np

TAU = 1.0 / 256.0
BAND_CAP = 0.0025
MIN_DEPTH, MAX_PIXEL = 0.01, 32768.0


# ------------------------------------------------------------------------------------------- meshes
def icosphere(level, radii=(1.0, 1.0, 1.0)):
    """A closed icosphere of 20 * 4^level faces (outward winding), its unit-sphere vertices scaled by `radii` ->
    (verts [V,3] float32, faces [Nf,3] int32)."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return (np.array(verts) * np.array(radii, np.float64)).astype(np.float32), np.array(faces, np.int32)


def tetrahedron(size=1.0):
    """Four vertices, four faces."""
    verts = size * np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64)
    return verts.astype(np.float32), np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


ELLIPSOID = (0.30, 0.45, 0.22)  # radii in metres of the ellipsoidal icospheres


# ------------------------------------------------------------------------------------------- cameras
def look_at(eye, target, focal, H, W, centre=None):
    """A pinhole camera at `eye` looking at `target`, image y down -> (K [3,3], RT [3,4]) float64, x_cam = R x + T."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    cx, cy = centre if centre is not None else ((W - 1) / 2.0 + 0.21, (H - 1) / 2.0 - 0.13)  # off the pixel lattice's symmetries
    K = np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]])
    return K, np.concatenate([R, (-R @ eye).reshape(3, 1)], axis=1)


def orbit(yaws, distance, focal, H, W, target=(0.0, 0.0, 0.0), pitch=0.15):
    """Cameras on a circle around `target` -> (Ks [nv,3,3], RTs [nv,3,4]) float32 as the device gets them."""
    Ks, RTs = [], []
    for yaw in yaws:
        eye = np.asarray(target, np.float64) + distance * np.array([math.sin(yaw) * math.cos(pitch), math.sin(pitch),
                                                                     -math.cos(yaw) * math.cos(pitch)])
        K, RT = look_at(eye, target, focal, H, W)
        Ks.append(K)
        RTs.append(RT)
    return np.stack(Ks).astype(np.float32), np.stack(RTs).astype(np.float32)


def project(verts, K, RT):
    """float64 projection of the float32 inputs -> (uv [V,2], depth [V])."""
    p = np.asarray(verts, np.float64) @ np.asarray(RT, np.float64)[:, :3].T + np.asarray(RT, np.float64)[:, 3]
    q = p @ np.asarray(K, np.float64).T
    return q[:, :2] / q[:, 2:3], p[:, 2]


def view_culls(verts, K, RT):
    """False for a view the kernel fills with 1: a vertex nearer than MIN_DEPTH or projecting beyond MAX_PIXEL."""
    uv, depth = project(verts, K, RT)
    return bool((depth >= MIN_DEPTH).all() and (np.abs(uv) <= MAX_PIXEL).all())


# ------------------------------------------------------------------------------------------- coverage
def square_meets_triangle(tri, half, H, W, out):
    """Sets out[y, x] (bool [H,W]) for every pixel whose closed square centre -+ `half` meets the closed triangle `tri` [3,2]
    (float64 pixel coordinates): the square overlaps the triangle's bounding box and, with the triangle oriented to positive
    area, E_i(centre) + half (|dx_i| + |dy_i|) >= 0 for each edge.  A triangle of zero area is the segment of its longest edge
    (both signs of that edge's function), or a point (the box alone)."""
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    x0, x1 = max(int(math.ceil(lo[0] - half)), 0), min(int(math.floor(hi[0] + half)), W - 1)
    y0, y1 = max(int(math.ceil(lo[1] - half)), 0), min(int(math.floor(hi[1] + half)), H - 1)
    if x0 > x1 or y0 > y1:
        return
    X, Y = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64))
    a, b, c = tri
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if area < 0:
        b, c = c, b
    ok = np.ones(X.shape, bool)
    edges = [(a, b), (b, c), (c, a)]
    if area == 0:
        p, q = max(edges, key=lambda e: float(np.abs(e[1] - e[0]).sum()))
        edges = [(p, q), (q, p)] if np.any(p != q) else []
    for p, q in edges:
        dx, dy = q[0] - p[0], q[1] - p[1]
        ok &= dx * (Y - p[1]) - dy * (X - p[0]) + half * (abs(dx) + abs(dy)) >= 0
    out[y0:y1 + 1, x0:x1 + 1] |= ok


def eroded(tri, tau=TAU):
    """`tri` scaled about its incentre by 1 - tau / r, r the inradius; None when r <= tau (nothing is left)."""
    a, b, c = tri
    la, lb, lc = np.linalg.norm(b - c), np.linalg.norm(c - a), np.linalg.norm(a - b)
    per = la + lb + lc
    area2 = abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
    if per == 0.0 or area2 / per <= tau:  # r = 2 * area / perimeter
        return None
    centre = (la * a + lb * b + lc * c) / per
    return centre + (1.0 - tau / (area2 / per)) * (tri - centre)


def lo_hi(verts, faces, K, RT, H, W, tau=TAU):
    """-> (lo, hi) bool [H,W] of one view that culls (view_culls)."""
    uv, _ = project(verts, K, RT)
    lo, hi = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for f in np.asarray(faces):
        tri = uv[f]
        square_meets_triangle(tri, 0.5 + tau, H, W, hi)
        small = eroded(tri, tau)
        if small is not None:
            square_meets_triangle(small, 0.5, H, W, lo)
    return lo, hi


def lo_hi_stack(verts, faces, Ks, RTs, H, W):
    """verts [F,V,3], Ks [nv,3,3], RTs [nv,3,4] -> (lo, hi) bool [F,nv,H,W]."""
    F, nv = verts.shape[0], Ks.shape[0]
    lo, hi = np.zeros((F, nv, H, W), bool), np.zeros((F, nv, H, W), bool)
    for f in range(F):
        for v in range(nv):
            assert view_culls(verts[f], Ks[v], RTs[v]), (f, v)
            lo[f, v], hi[f, v] = lo_hi(verts[f], faces, Ks[v], RTs[v], H, W)
    return lo, hi


def band_fraction(lo, hi):
    """The largest share of a mask's pixels the reference leaves open, over the leading dimensions."""
    assert not (lo & ~hi).any()
    return float((hi & ~lo).reshape(-1, lo.shape[-2] * lo.shape[-1]).mean(axis=1).max())


def surface_points(verts, faces, n, seed):
    """n points uniform in barycentric coordinates on randomly chosen faces -> float64 [n,3]."""
    rs = np.random.RandomState(seed)
    f = np.asarray(faces)[rs.randint(0, len(faces), n)]
    w = rs.dirichlet((1.0, 1.0, 1.0), n)
    return np.einsum("nk,nkd->nd", w, np.asarray(verts, np.float64)[f])


def cull_pixels(points, K, RT, H, W):
    """The pixel the sample cull looks a point up at (if_clight_renderer_mmsk.py:30-33): float64 projection, round half to even,
    clamp -> (x, y) int arrays."""
    uv, _ = project(points, K, RT)
    return np.clip(np.rint(uv[:, 0]).astype(np.int64), 0, W - 1), np.clip(np.rint(uv[:, 1]).astype(np.int64), 0, H - 1)


def dilate(mask, border):
    """cv2.dilate(mask, ones((border, border))) of a bool / uint8 [...,H,W]: pixels outside the image are ignored."""
    m = np.asarray(mask).astype(bool)
    h = border // 2
    H, W = m.shape[-2:]
    pad = np.zeros(m.shape[:-2] + (H + 2 * h, W + 2 * h), bool)
    pad[..., h:h + H, h:h + W] = m
    out = np.zeros_like(m)
    for dy in range(border):
        for dx in range(border):
            out |= pad[..., dy:dy + H, dx:dx + W]
    return out


# ------------------------------------------------------------------------------------------- the cases the suites share
# name -> (mesh, frame scalings, (H, W), yaws of the cull views, camera distance in metres, focal over H)
BAND_CASES = {
    "ico320": (("ico", 2), (1.0, 0.8), (45, 61), (0.2, 1.4, 2.9), 2.0, 1.3),
    "ico1280": (("ico", 3), (1.0,), (96, 128), (0.2, 1.4, 2.9), 2.0, 1.3),
    "ico5120": (("ico", 4), (1.0,), (128, 128), (0.2, 1.4, 2.9), 2.0, 1.3),
}


def mesh_of(kind):
    return icosphere(kind[1], ELLIPSOID) if kind[0] == "ico" else tetrahedron(kind[1])


def band_case(name):
    """-> dict(verts [F,V,3] float32, faces, Ks, RTs, H, W)."""
    kind, scales, (H, W), yaws, distance, focal = BAND_CASES[name]
    v, faces = mesh_of(kind)
    verts = np.stack([(np.float32(s) * v).astype(np.float32) for s in scales])
    Ks, RTs = orbit(yaws, distance, focal * H, H, W)
    return dict(verts=verts, faces=faces, Ks=Ks, RTs=RTs, H=H, W=W)


def path_case():
    """The tetrahedron cases of the device suite at 96 x 128, three views:
      view 0  close: the faces fill most of the image (boxes far beyond 16 x 16: the workgroup-per-triangle path),
      view 1  the same direction pulled back: every face under 16 px (the thread-per-triangle path),
      view 2  close and aimed beside the body: triangles partly off the image; frame 1 is the body moved 1.5 m along y, wholly
              off the close views.
    The face list holds both windings and a repeated-vertex face of zero area."""
    H, W = 96, 128
    v, faces = tetrahedron(0.25)
    faces = np.concatenate([faces[:2], faces[2:, ::-1], np.array([[1, 1, 3], [2, 0, 2]], np.int32)]).astype(np.int32)
    verts = np.stack([v, (v + np.array([0.0, 1.5, 0.0], np.float32)).astype(np.float32)])
    cams = [look_at((0.5, 0.3, -1.1), (0, 0, 0), 1.9 * H, H, W), look_at((4.0, 2.4, -8.8), (0, 0, 0), 1.9 * H, H, W),
            look_at((-0.4, 0.2, -1.0), (-0.45, 0.1, 0.0), 1.9 * H, H, W)]
    Ks, RTs = np.stack([c[0] for c in cams]).astype(np.float32), np.stack([c[1] for c in cams]).astype(np.float32)
    return dict(verts=verts, faces=faces, Ks=Ks, RTs=RTs, H=H, W=W)


# ------------------------------------------------------------------------------------------- the kernel's own definition
def snapped_mask(verts, faces, K, RT, H, W, arith="chain"):
    """include/nb_hip.h's definition of one (frame, view) evaluated on the host: the fp32 projection in nb_cull's arithmetic
    (`arith`: the FMA chains of tests/cull_cases.py, which the device is held to; the other names there are the mutants the
    tests tell apart from it), the snap to 1/256 pixel, integer edge functions -> uint8 [H,W]."""
    from tests.cull_cases import dot3

    f32 = np.float32
    v, K, RT = np.asarray(verts, f32), np.asarray(K, f32), np.asarray(RT, f32)
    a = [v[:, 0], v[:, 1], v[:, 2]]
    t = [dot3(a, RT[i, :3], arith) + RT[i, 3] for i in range(3)]
    q = [dot3(t, K[i, :], arith) for i in range(3)]
    assert all(a.dtype == f32 for a in t + q)
    with np.errstate(all="ignore"):
        u, w = q[0] / q[2], q[1] / q[2]
        ok = (t[2] >= f32(MIN_DEPTH)) & (np.abs(u) <= f32(MAX_PIXEL)) & (np.abs(w) <= f32(MAX_PIXEL))
    if not ok.all():
        return np.ones((H, W), np.uint8)
    sx, sy = np.rint(f32(256) * u).astype(np.int64), np.rint(f32(256) * w).astype(np.int64)
    out = np.zeros((H, W), np.uint8)
    for ia, ib, ic in np.asarray(faces):
        a, b, c = (int(sx[ia]), int(sy[ia])), (int(sx[ib]), int(sy[ib])), (int(sx[ic]), int(sy[ic]))
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0:
            continue
        if area < 0:
            b, c = c, b
        xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
        x0, x1 = max(-((128 - min(xs)) // 256), 0), min((max(xs) + 128) // 256, W - 1)  # ceil((min - 128) / 256) .. floor((max + 128) / 256)
        y0, y1 = max(-((128 - min(ys)) // 256), 0), min((max(ys) + 128) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(256 * np.arange(x0, x1 + 1, dtype=np.int64), 256 * np.arange(y0, y1 + 1, dtype=np.int64))
        ok = np.ones(X.shape, bool)
        for p, q2 in ((a, b), (b, c), (c, a)):
            dx, dy = q2[0] - p[0], q2[1] - p[1]
            ok &= dx * (Y - p[1]) - dy * (X - p[0]) + 128 * (abs(dx) + abs(dy)) >= 0
        out[y0:y1 + 1, x0:x1 + 1] |= ok.astype(np.uint8)
    return out


def snapped_stack(verts, faces, Ks, RTs, H, W):
    return np.stack([np.stack([snapped_mask(verts[f], faces, Ks[v], RTs[v], H, W) for v in range(Ks.shape[0])])
                     for f in range(verts.shape[0])])
