"""numpy restatements of nb_mask_band and nb_image_undistort (csrc/nb_image_prep.hip), written from the definitions in
include/nb_hip.h and not from the kernels: the same float64 and float32 operations in the same order, one numpy operation per
rounding (numpy never fuses a multiply into an add).

  * band(label, border): get_mask of lib/datasets/light_stage/multi_view_dataset.py:58-64;
  * source_uv(cam, H, W): the float64 source position of every full-resolution pixel (cv2.initUndistortRectifyMap with R = I and
    newCameraMatrix = K), unquantised;
  * undistort_u8 / undistort_f32: cv2.remap(INTER_LINEAR, BORDER_CONSTANT) through the 1/32-pixel fixed-point map;
  * frame(rgb, msk, cam, n, fill): the whole of nb_image_undistort for one view.
"""
import numpy as np

from tests.lattice_ref import dilate

I32_MIN, I32_MAX = -2147483648, 2147483647


def camera_constants(K, D):
    """fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 as float64 [12] from K [3,3] and OpenCV's D (k1 k2 p1 p2 [k3 [k4 k5 k6]])."""
    K, D = np.asarray(K, np.float64).reshape(3, 3), np.asarray(D, np.float64).reshape(-1)
    assert len(D) in (4, 5, 8)
    d = np.zeros(8)
    d[:len(D)] = D
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]], np.float64)


def band(label, border):
    """[V,H,W] uint8 -> [V,H,W] uint8: m = (label != 0); 100 where the window's maximum and minimum of m differ, else m."""
    m = (label != 0).astype(np.uint8)
    d = dilate(m, border)
    e = 1 - dilate(1 - m, border)  # the minimum with pixels outside the image ignored
    out = m.copy()
    out[(d - e) == 1] = 100
    return out


def source_uv(cam, H, W):
    """-> (u [H,W], v [H,W]) float64: where output pixel (row i, column j) reads the source, in source pixels."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(c) for c in cam)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    with np.errstate(all="ignore"):
        x = (j - cx) / fx
        y = (i - cy) / fy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + cx
        v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + cy
    return u, v


def _fixed32(a):
    with np.errstate(all="ignore"):
        t = np.rint(a * 32.0)
    t = np.where(np.isnan(t), float(I32_MIN), np.clip(t, float(I32_MIN), float(I32_MAX)))
    return t.astype(np.int64)


def taps(cam, H, W):
    """-> (sx, sy, ax, ay) int64 [H,W]: the integer parts and the 1/32 fractions of the fixed-point map."""
    u, v = source_uv(cam, H, W)
    iu, iv = _fixed32(u), _fixed32(v)
    return iu >> 5, iv >> 5, iu & 31, iv & 31


def _gather(img, y, x):
    """img[y, x] with 0 outside the image; img [H,W] or [H,W,C]"""
    H, W = img.shape[:2]
    ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    val = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
    return np.where(ok[..., None] if img.ndim == 3 else ok, val, 0).astype(img.dtype), ok


def tap_census(cam, H, W):
    """-> (fraction of pixels with at least one tap outside the image, fraction with all four outside)"""
    sx, sy, _, _ = taps(cam, H, W)
    inside = [(yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) for yy, xx in ((sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1))]
    n_in = sum(i.astype(np.int64) for i in inside)
    return float((n_in < 4).mean()), float((n_in == 0).mean())


def undistort_u8(msk, cam):
    """[H,W] uint8 -> [H,W] uint8"""
    H, W = msk.shape
    sx, sy, ax, ay = taps(cam, H, W)
    s = np.full((H, W), 512, np.int64)
    for (yy, xx), w in (((sy, sx), (32 - ay) * (32 - ax)), ((sy, sx + 1), (32 - ay) * ax), ((sy + 1, sx), ay * (32 - ax)),
                        ((sy + 1, sx + 1), ay * ax)):
        s += _gather(msk, yy, xx)[0].astype(np.int64) * w
    return (s >> 10).astype(np.uint8)


def undistort_f32(rgb, cam):
    """[H,W,3] uint8 -> [H,W,3] float32: the float path on S = byte / 255.f"""
    return remap_f32(rgb.astype(np.float32) / np.float32(255.0), cam)


def remap_f32(S, cam):
    """[H,W,C] float32 -> [H,W,C] float32: the float path on any float32 image"""
    assert S.dtype == np.float32 and S.ndim == 3
    H, W = S.shape[:2]
    sx, sy, ax, ay = taps(cam, H, W)
    fx, fy = ax.astype(np.float32) / np.float32(32.0), ay.astype(np.float32) / np.float32(32.0)
    gx, gy = np.float32(1.0) - fx, np.float32(1.0) - fy
    w00, w01, w10, w11 = (gy * gx)[..., None], (gy * fx)[..., None], (fy * gx)[..., None], (fy * fx)[..., None]
    s00, s01 = _gather(S, sy, sx)[0], _gather(S, sy, sx + 1)[0]
    s10, s11 = _gather(S, sy + 1, sx)[0], _gather(S, sy + 1, sx + 1)[0]
    out = ((s00 * w00 + s01 * w01) + s10 * w10) + s11 * w11
    assert out.dtype == np.float32
    return out


def frame(rgb, msk, cam, n=1, fill=None):
    """nb_image_undistort of one view: rgb [H,W,3] uint8 or None, msk [H,W] uint8 or None -> (img float32 [H/n,W/n,3] or None,
    msk uint8 [H/n,W/n] or None)."""
    img_out = msk_out = None
    if msk is not None:
        msk_out = np.ascontiguousarray(undistort_u8(msk, cam)[::n, ::n])
    if rgb is not None:
        full = undistort_f32(rgb, cam)
        H, W = full.shape[:2]
        acc = np.zeros((H // n, W // n, 3), np.float32)
        for dy in range(n):
            for dx in range(n):
                acc = acc + full[dy::n, dx::n]
        img_out = acc * (np.float32(1.0) / np.float32(n * n))
        assert img_out.dtype == np.float32
        if fill is not None:
            img_out[msk_out == 0] = {"black": 0.0, "white": 1.0}[fill]
    return img_out, msk_out
