"""numpy restatements for the mesh lattice (neuralbody_amd/mesh_lattice.py, csrc/nb_lattice.hip), written from the reference's
lines and not from the kernels:

  * prepare_inside_pts (lib/datasets/light_stage/multi_view_mesh_dataset.py:117-140) twice — with the reference's float32
    lib/utils/base_utils.py:17-26 `project` (np.dot in float32: the ascending FMA chain per row, which the device computes too:
    precision "f32" equals the device at EVERY point, the near band included), and in float64 with np.rint;
  * cv2.dilate with a border x border kernel of ones (:111-113);
  * the NEAR BAND: lattice points whose float64 pixel coordinate in any view lies within BAND px of a half-integer, where a
    float32 projection (any summation order: its error is ~1e-5 px at these image sizes) may round to the other pixel.

Pixels: round half to even, clamp to the image; a non-finite coordinate becomes pixel 0 (documented at cull_pixel,
csrc/nb_march_common.h); a point behind the camera is projected like any other and lands wherever the clamp puts it.
"""
import numpy as np

BAND = 1e-3  # px


def dilate(msks, border):
    """cv2.dilate(m, np.ones((border, border), np.uint8)) of every mask of a [V,H,W] uint8 stack: the maximum over the window
    centred on the pixel, pixels outside the image ignored."""
    assert border % 2 == 1 and msks.ndim == 3
    h = border // 2
    V, H, W = msks.shape
    padded = np.zeros((V, H + 2 * h, W + 2 * h), msks.dtype)
    padded[:, h:h + H, h:h + W] = msks
    out = np.zeros_like(msks)
    for dy in range(border):
        for dx in range(border):
            out = np.maximum(out, padded[:, dy:dy + H, dx:dx + W])
    return out


def _pixels(xy, H, W):
    """cull_pixel: rint, then 0 for a non-finite value or one beyond the int64 range, then the clamp"""
    xy = np.asarray(xy, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.rint(xy)
        r = np.where(np.abs(r) < 9.0e18, r, 0.0)
    x = np.clip(r[:, 0], 0, W - 1).astype(np.int64)
    y = np.clip(r[:, 1], 0, H - 1).astype(np.int64)
    return x, y


def project_f32(xyz, K, RT):
    """lib/utils/base_utils.py:17-26 on float32 arrays, its two np.dot written out as the FMA chains they evaluate to
    (tests/cull_cases.py::project, held to the reference's own answers by tests/golden/cull_edges.npz): no BLAS decides here"""
    from tests import cull_cases

    x, y = cull_cases.project(dict(K=K, RT=RT), xyz.astype(np.float32), "chain")
    return np.stack([x, y], axis=1)


def project_f64(xyz, K, RT):
    xyz, K, RT = xyz.astype(np.float64), K.astype(np.float64), RT.astype(np.float64)
    cam = xyz @ RT[:, :3].T + RT[:, 3]
    uv = cam @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return uv[:, :2] / uv[:, 2:]


def lattice_points(axes):
    """[X*Y*Z, 3] float32 in 'ij' order (multi_view_mesh_dataset.py:157-158)"""
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32).reshape(-1, 3)


def inside_and_band(axes, msks, Ks, RTs):
    """One float64 pass over the lattice -> (inside uint8 [X,Y,Z], near band bool [X,Y,Z]).  inside: prepare_inside_pts against
    DILATED masks [V,H,W] (non-zero = body).  band: the pixel coordinate (x or y) in some view is within BAND of a half-integer,
    or not finite."""
    pts = lattice_points(axes)
    V, H, W = msks.shape
    ins, band = np.ones(len(pts), bool), np.zeros(len(pts), bool)
    for v in range(V):
        xy = project_f64(pts, Ks[v], RTs[v])
        x, y = _pixels(xy, H, W)
        ins &= msks[v][y, x] != 0
        with np.errstate(invalid="ignore"):
            band |= (~np.isfinite(xy)).any(1) | (np.abs(xy - np.floor(xy) - 0.5) < BAND).any(1)
    sh = [len(a) for a in axes]
    return ins.astype(np.uint8).reshape(sh), band.reshape(sh)


def inside(axes, msks, Ks, RTs, precision="f64"):
    if precision == "f64":
        return inside_and_band(axes, msks, Ks, RTs)[0]
    return inside_f32_at(lattice_points(axes), msks, Ks, RTs).astype(np.uint8).reshape([len(a) for a in axes])


def inside_f32_at(pts, msks, Ks, RTs):
    """The float32 restatement on the points pts [n,3] alone -> bool [n]: what the device computes, point for point."""
    V, H, W = msks.shape
    ins = np.ones(len(pts), bool)
    for v in range(V):
        x, y = _pixels(project_f32(pts, Ks[v], RTs[v]), H, W)
        ins &= msks[v][y, x] != 0
    return ins


def near_band(axes, msks, Ks, RTs):
    return inside_and_band(axes, msks, Ks, RTs)[1]
