"""Numpy restatement of the ray bounds (csrc/nb_silhouette.hip: nb_body_depth_range; csrc/nb_ray_bounds.hip: nb_depth_range_widen;
csrc/nb_raygen.hip: nb_raygen_body), include/nb_hip.h's definitions evaluated on the host, and the cases their suites share.  CPU only.

    depth_range   silhouette_ref.snapped_mask's loop, every triangle carrying the min / max of its three vertices' fp32 camera depths
                  (R v + T).z in the `chain` arithmetic of tests/cull_cases.py, the value the projection computes
    widen         a brute-force border x border window (pixels outside the image ignored), then aligned tile x tile blocks
    body_cut      near' = max(near, lo - margin), far' = min(far, hi + margin) in float32, kept iff near' < far', on given near / far

The MUTANTS are definitions a careless rewrite could produce instead; tests/test_ray_bounds_host.py tells each apart from the
definition on the cases below."""
import functools

import numpy as np

from tests import silhouette_ref as sil
from tests.cull_cases import dot3

F32 = np.float32
INF = F32(np.inf)
EMPTY = (INF, -INF)      # a pixel no triangle covers
UNBOUNDED = (-INF, INF)  # every pixel of a view that does not bound


# ------------------------------------------------------------------------------------------- nb_body_depth_range
def depth_range(verts, faces, K, RT, H, W, coverage="square", depth="vertices"):
    """One (frame, view) -> float32 [H,W,2].  `coverage`: 'square' (the definition: the pixel's closed square meets the closed snapped
    triangle) or the mutant 'centre' (the pixel's centre lies in it); `depth`: 'vertices' (the definition: min / max of the three
    vertex depths) or the mutant 'barycentric' (the plane's depth at the pixel's centre, for both ends)."""
    v, K, RT = np.asarray(verts, F32), np.asarray(K, F32), np.asarray(RT, F32)
    a = [v[:, 0], v[:, 1], v[:, 2]]
    t = [dot3(a, RT[i, :3], "chain") + RT[i, 3] for i in range(3)]
    q = [dot3(t, K[i, :], "chain") for i in range(3)]
    assert all(x.dtype == F32 for x in t + q)
    with np.errstate(all="ignore"):
        u, w = q[0] / q[2], q[1] / q[2]
        ok = (t[2] >= F32(sil.MIN_DEPTH)) & (np.abs(u) <= F32(sil.MAX_PIXEL)) & (np.abs(w) <= F32(sil.MAX_PIXEL))
    out = np.empty((H, W, 2), F32)
    if not ok.all():
        out[...] = UNBOUNDED
        return out
    out[...] = EMPTY
    sx, sy = np.rint(F32(256) * u).astype(np.int64), np.rint(F32(256) * w).astype(np.int64)
    z = t[2]
    slack = 128 if coverage == "square" else 0
    for ia, ib, ic in np.asarray(faces):
        if not (0 <= ia < len(v) and 0 <= ib < len(v) and 0 <= ic < len(v)):
            continue
        a, b, c = (int(sx[ia]), int(sy[ia])), (int(sx[ib]), int(sy[ib])), (int(sx[ic]), int(sy[ic]))
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0:
            continue
        za, zb, zc = z[ia], z[ib], z[ic]
        if area < 0:
            b, c, zb, zc, area = c, b, zc, zb, -area
        xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
        x0, x1 = max(-((128 - min(xs)) // 256), 0), min((max(xs) + 128) // 256, W - 1)
        y0, y1 = max(-((128 - min(ys)) // 256), 0), min((max(ys) + 128) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(256 * np.arange(x0, x1 + 1, dtype=np.int64), 256 * np.arange(y0, y1 + 1, dtype=np.int64))
        cover = np.ones(X.shape, bool)
        E = []
        for p, q2 in ((a, b), (b, c), (c, a)):
            dx, dy = q2[0] - p[0], q2[1] - p[1]
            E.append(dx * (Y - p[1]) - dy * (X - p[0]))
            cover &= E[-1] + slack * (abs(dx) + abs(dy)) >= 0
        if depth == "vertices":
            lo = np.full(X.shape, min(za, zb, zc), F32)
            hi = np.full(X.shape, max(za, zb, zc), F32)
        else:  # E[1], E[2], E[0] over the area weigh a, b, c
            lo = hi = ((E[1] * float(za) + E[2] * float(zb) + E[0] * float(zc)) / float(area)).astype(F32)
        box = out[y0:y1 + 1, x0:x1 + 1]
        box[..., 0] = np.where(cover, np.minimum(box[..., 0], lo), box[..., 0])
        box[..., 1] = np.where(cover, np.maximum(box[..., 1], hi), box[..., 1])
    return out


def depth_range_stack(verts, faces, Ks, RTs, H, W, **kw):
    """verts [F,V,3], Ks [nv,3,3], RTs [nv,3,4] -> float32 [F,nv,H,W,2]."""
    return np.stack([np.stack([depth_range(verts[f], faces, Ks[v], RTs[v], H, W, **kw) for v in range(Ks.shape[0])])
                     for f in range(verts.shape[0])])


# ------------------------------------------------------------------------------------------- nb_depth_range_widen
def widen(rng, border, tile, wrap=False):
    """float32 [...,H,W,2] -> the same shape.  `wrap`: the mutant whose window wraps around the image edges."""
    r = np.asarray(rng, F32)
    H, W = r.shape[-3:-1]
    h = border // 2
    win = np.empty_like(r)
    for y in range(H):
        ys = [yy % H for yy in range(y - h, y + h + 1)] if wrap else list(range(max(y - h, 0), min(y + h, H - 1) + 1))
        rows = r[..., ys, :, :]
        for x in range(W):
            xs = [xx % W for xx in range(x - h, x + h + 1)] if wrap else list(range(max(x - h, 0), min(x + h, W - 1) + 1))
            w = rows[..., xs, :]
            win[..., y, x, 0] = w[..., 0].min(axis=(-2, -1))
            win[..., y, x, 1] = w[..., 1].max(axis=(-2, -1))
    out = np.empty_like(r)
    for y0 in range(0, H, tile):
        for x0 in range(0, W, tile):
            blk = win[..., y0:y0 + tile, x0:x0 + tile, :]
            out[..., y0:y0 + tile, x0:x0 + tile, 0] = blk[..., 0].min(axis=(-2, -1))[..., None, None]
            out[..., y0:y0 + tile, x0:x0 + tile, 1] = blk[..., 1].max(axis=(-2, -1))[..., None, None]
    return out


# ------------------------------------------------------------------------------------------- nb_raygen_body
def body_cut(near, far, lo, hi, margin):
    """float32 arrays of the same shape -> (near', far', keep)."""
    near, far, lo, hi = (np.asarray(a, F32) for a in (near, far, lo, hi))
    m = F32(margin)
    n2, f2 = np.maximum(near, lo - m), np.minimum(far, hi + m)
    assert n2.dtype == F32 and f2.dtype == F32
    return n2, f2, n2 < f2


def raygen_body(box_rays, rng, margin):
    """nb_raygen_body from nb_raygen's own output: box_rays = (ray_o [n,3], ray_d [n,3], near [n], far [n], mask [H*W] uint8) numpy,
    the first n = mask.sum() rows; rng float32 [H,W,2] -> (ray_o, ray_d, near, far, mask, n_rays) of the rays that are left."""
    ray_o, ray_d, near, far, mask = box_rays
    idx = np.flatnonzero(mask)
    assert len(idx) == len(near)
    r = np.asarray(rng, F32).reshape(-1, 2)[idx]
    n2, f2, keep = body_cut(near, far, r[:, 0], r[:, 1], margin)
    new_mask = np.zeros_like(mask)
    new_mask[idx[keep]] = 1
    return ray_o[keep], ray_d[keep], n2[keep], f2[keep], new_mask, int(keep.sum())


# ------------------------------------------------------------------------------------------- cases
CASES = ("paths",) + tuple(sil.BAND_CASES)
SMALL = (45, 61)


@functools.lru_cache(maxsize=None)
def case(name):
    """'paths': silhouette_ref.path_case (96 x 128, F = 2, nv = 3: large, small and clipped triangles, both windings, zero-area
    faces; every view bounds).  A BAND_CASES name: its icosphere in two frames (scaled 1 and 0.8) seen by its three orbit cameras at
    45 x 61, pulled in to 0.9 m so that the body leaves the image; `case_ranges` replaces its last view by one that is too near.
    -> dict(verts [2,V,3] float32, faces, Ks, RTs [3,...] float32, H, W), never written to."""
    if name == "paths":
        c = sil.path_case()
    else:
        kind, _, _, yaws, _, focal = sil.BAND_CASES[name]
        v, faces = sil.mesh_of(kind)
        H, W = SMALL
        Ks, RTs = sil.orbit(yaws, 0.9, focal * H, H, W)
        c = dict(verts=np.stack([v, (F32(0.8) * v).astype(F32)]), faces=faces, Ks=Ks, RTs=RTs, H=H, W=W)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def with_near_view(c, frame=0, vertex=17):
    """The case with its LAST view replaced by a camera 5 mm in front of `vertex` of `frame`, looking at the body's middle: that
    (frame, view) does not bound."""
    v = np.asarray(c["verts"][frame], np.float64)
    centre = v.mean(axis=0)
    n = (v[vertex] - centre) / np.linalg.norm(v[vertex] - centre)
    K, RT = sil.look_at(v[vertex] + 0.005 * n, centre, 1.3 * c["H"], c["H"], c["W"])
    Ks, RTs = c["Ks"].copy(), c["RTs"].copy()
    Ks[-1], RTs[-1] = K.astype(F32), RT.astype(F32)
    return dict(c, Ks=Ks, RTs=RTs)


@functools.lru_cache(maxsize=None)
def case_ranges(name):
    """(the case, its depth_range_stack), the band cases with_near_view: computed once, shared, never written to."""
    c = case(name) if name == "paths" else with_near_view(case(name))
    r = depth_range_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], c["H"], c["W"])
    r.setflags(write=False)
    return c, r
