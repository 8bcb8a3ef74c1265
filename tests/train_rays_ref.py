"""numpy restatement of nb_train_rays (include/nb_hip.h) for arbitrary uniforms `u`: hull test, the two candidate classes in
np.argwhere order, the round schedule, float64 rays / near / far in the kernel's operation order, hits kept in draw order,
padding rows.  Needs numpy alone, so it also runs where only the GPU tests run."""
import os

import numpy as np

H36M, PLAIN = "h36m", "plain"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inv3(m):
    """csrc/nb_ray.h inv3: the adjugate over the determinant, in this order."""
    a, b, c, d, e, f, g, h, i = (float(v) for v in np.asarray(m, np.float64).reshape(9))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    r = 1.0 / det
    return np.array([(e * i - f * h) * r, (c * h - b * i) * r, (b * f - c * e) * r, (f * g - d * i) * r, (a * i - c * g) * r,
                     (c * d - a * f) * r, (d * h - e * g) * r, (b * g - a * h) * r, (a * e - b * d) * r]).reshape(3, 3)


def hull_mask(hull, H, W):
    """Pixels whose centre lies inside or on the CCW polygon `hull` [n,2] (x, y): every edge function >= 0, in integers."""
    hull = np.asarray(hull, np.int64).reshape(-1, 2)
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    inside = np.ones((H, W), bool)
    for e in range(len(hull)):
        (ax, ay), (bx, by) = hull[e], hull[(e + 1) % len(hull)]
        inside &= (bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0
    return inside


def classes(msk, in_hull, mode):
    """(body, bound) candidate masks (if_nerf_data_utils.py:79,99,108 / :160-161,181,190)."""
    m = msk.astype(np.int64) * in_hull
    if mode == H36M:
        return m == 1, in_hull & (m != 100)
    return m != 0, in_hull.copy()


def camera_origin(R, T):
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    return np.array([-(R[0, a] * T[0] + R[1, a] * T[1] + R[2, a] * T[2]) for a in range(3)])


def pixel_rays(K, R, T, ys, xs):
    """float64 ray directions of the pixels (ys, xs) -> (o [3], d [n,3]); csrc/nb_ray.h pixel_ray_f64, product by product."""
    Kinv = inv3(K)
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    o = camera_origin(R, T)
    x, y = np.asarray(xs).astype(np.float32).astype(np.float64), np.asarray(ys).astype(np.float32).astype(np.float64)
    pc = [(x * Kinv[a, 0] + y * Kinv[a, 1]) + Kinv[a, 2] for a in range(3)]
    pc = [pc[a] - T[a] for a in range(3)]
    pw = [(pc[0] * R[0, a] + pc[1] * R[1, a]) + pc[2] * R[2, a] for a in range(3)]
    return o, np.stack([pw[a] - o[a] for a in range(3)], axis=-1).reshape(-1, 3)


def near_far64(bounds, o, d):
    """get_near_far (if_nerf_data_utils.py:54-69) on float64 rays, all rays kept: (near, far, hit)."""
    b = np.asarray(bounds, np.float32).reshape(2, 3).astype(np.float64)
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    v = d / n[:, None]
    v[(v < 1e-5) & (v > -1e-10)] = 1e-5
    v[(v > -1e-5) & (v < 1e-10)] = -1e-5
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (b[:1] - o[None]) / v, (b[1:2] - o[None]) / v
        tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
        return tn / n, tf / n, tn < tf


def pick(u, count):
    k = np.floor(u.astype(np.float64) * float(count)).astype(np.int64)
    return np.clip(k, 0, count - 1)


def sample(img, msk, K, R, T, bounds, hull, mode, body_ratio, u):
    """-> dict(rgb, ray_o, ray_d [n,3] f32, near, far [n] f32, pixel [n,2] i32 (y, x), mask_at_box [n] bool, status [4] i32)"""
    H, W = msk.shape
    n_rounds, n_rays = u.shape
    in_hull = hull_mask(hull, H, W)
    body, bound = classes(msk, in_hull, mode)
    cand = {True: np.argwhere(body), False: np.argwhere(bound)}
    o, d0 = pixel_rays(K, R, T, [0], [0])
    out = {"rgb": np.zeros((n_rays, 3), np.float32), "ray_o": np.tile(o.astype(np.float32), (n_rays, 1)),
           "ray_d": np.tile(d0.astype(np.float32), (n_rays, 1)), "near": np.zeros(n_rays, np.float32),
           "far": np.zeros(n_rays, np.float32), "pixel": np.full((n_rays, 2), -1, np.int32), "mask_at_box": np.zeros(n_rays, bool)}
    filled = rounds = 0
    while rounds < n_rounds and filled < n_rays:
        deficit = n_rays - filled
        n_body = int(float(deficit) * body_ratio)
        coords = []
        for is_body, lo, hi in ((True, 0, n_body), (False, n_body, deficit)):
            c = cand[is_body]
            if len(c) and hi > lo:
                coords.append(c[pick(u[rounds, lo:hi], len(c))])
        rounds += 1
        if not coords:
            continue
        coord = np.concatenate(coords, axis=0)
        _, d = pixel_rays(K, R, T, coord[:, 0], coord[:, 1])
        near, far, hit = near_far64(bounds, o, d)
        k = int(hit.sum())
        sl = slice(filled, filled + k)
        out["rgb"][sl] = img[coord[hit, 0], coord[hit, 1]]
        out["ray_d"][sl] = d[hit].astype(np.float32)
        out["near"][sl], out["far"][sl] = near[hit].astype(np.float32), far[hit].astype(np.float32)
        out["pixel"][sl] = coord[hit]
        out["mask_at_box"][sl] = True
        filled += k
    out["status"] = np.array([filled, rounds, len(cand[True]), len(cand[False])], np.int32)
    return out


# ------------------------------------------------------------------------------------------- the fixture
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "train_rays.npz"))


def replayed_uniforms(g, name, n_rounds=4):
    """The logged randint draws as uniforms: u = (k + 0.5) / high lands in the middle of candidate k's interval, so
    floor(u * high) = k for every high < 2^22 whatever the float32 rounding of u.  Rounds the reference did not need get 0.5."""
    ks, highs, sizes = g[name + "/draws_k"], g[name + "/draws_high"], g[name + "/draws_size"]
    N = int(g[name + "/N"])
    u = np.full((n_rounds, N), 0.5, np.float32)
    for r in range(len(ks)):
        nb, nr = (int(v) for v in sizes[r])
        u[r, :nb] = ((ks[r, :nb] + 0.5) / float(highs[r, 0])).astype(np.float32)
        u[r, nb:nb + nr] = ((ks[r, nb:nb + nr] + 0.5) / float(highs[r, 1])).astype(np.float32)
    return u


def case_inputs(g, name):
    return dict(img=g[name + "/img"], msk=g[name + "/msk"], K=g[name + "/K"], R=g[name + "/R"], T=g[name + "/T"],
                bounds=g[name + "/bounds"], hull=g[name + "/hull"], mode=str(g[name + "/mode"]))
