"""Photographed frames on the device: what the reference's datasets do to every image file with OpenCV on the host
(lib/datasets/light_stage/multi_view_dataset.py:54-66 get_mask: cv2.erode, cv2.dilate; :121-142 cv2.undistort of a float32 image
and a uint8 mask, cv2.resize INTER_AREA / INTER_NEAREST, the background fill; lib/datasets/light_stage/
multi_view_mesh_dataset.py:102-109 cv2.undistort of every view's mask) with the files' bytes uploaded and two kernels:

    host (per file)                                device (HIP)
    decode (imageio or PIL), 3 + 1 bytes / pixel -> nb_mask_band -> nb_image_undistort -> img fp32 [H/n, W/n, 3], msk uint8

`DeviceImagePrep` is what `LightStageFrameSource(prep=...)` and `LightStageMeshSource(prep=...)` call instead of cv2; the plugins
choose with the YAML key `image_prep` (`select_prep`).
"""
import numpy as np
import torch

from . import ops

BORDER = 5  # multi_view_dataset.py:61
PREP_MODES = ("auto", "cv2", "device")


def camera_constants(K, D):
    """K [3,3] and OpenCV's distortion vector D (k1 k2 p1 p2 [k3 [k4 k5 k6]], any shape with 4, 5 or 8 entries) -> float64 [12]:
    fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6, the constants of nb_image_undistort (missing coefficients are 0)."""
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("K has shape %s, expected (3, 3)" % (K.shape,))
    D = np.asarray(D, np.float64).reshape(-1)
    if len(D) not in (4, 5, 8):
        raise ValueError("D has %d entries; cv2.undistort's models with 4, 5 or 8 coefficients are built" % len(D))
    d = np.zeros(8, np.float64)
    d[:len(D)] = D
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d])


def reduction_factor(ratio, H, W):
    """cfg.ratio -> the integer n = 1 / ratio that divides H and W (multi_view_dataset.py:136-138 resizes to int(H ratio));
    ValueError for any other ratio: only the integer case of INTER_AREA / INTER_NEAREST is built."""
    ratio = float(ratio)
    n = int(round(1.0 / ratio)) if 0.0 < ratio <= 1.0 else 0
    if n < 1 or abs(n * ratio - 1.0) > 1e-9 or H % n or W % n:
        raise ValueError("ratio = %r: 1 / ratio must be an integer that divides H = %d and W = %d" % (ratio, H, W))
    return n


def decode(path):
    """The file's pixels as the reference's imageio.imread gives them; PIL where imageio does not import."""
    try:
        import imageio
    except ImportError:
        from PIL import Image

        with Image.open(path) as im:
            return np.array(im)  # a copy the file no longer backs (np.asarray's is read-only)
    return np.asarray(imageio.imread(path))


def _decode_mask(path):
    m = decode(path)
    if m.ndim != 2:
        raise ValueError("mask %s decodes to shape %s, expected two dimensions (a CIHP label image)" % (path, m.shape))
    if m.dtype != np.uint8:
        m = (m != 0).astype(np.uint8)  # only (label != 0) is ever used
    return m


class DeviceImagePrep:
    """`frame()` and `masks()` decode on the host, upload bytes and enqueue the kernels; nothing is read back."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def frame(self, img_path, msk_path, K, D, H, W, ratio, mask_bkgd, white_bkgd):
        """multi_view_dataset.py:121-142 for one image -> (img fp32 [H ratio, W ratio, 3], msk uint8 [H ratio, W ratio]) on the
        device; msk is 0 / 1 / 100 interpolated as cv2.undistort interpolates it."""
        H, W = int(H), int(W)
        n = reduction_factor(ratio, H, W)
        cam = camera_constants(K, D)
        img = decode(img_path)
        if img.shape != (H, W, 3) or img.dtype != np.uint8:
            raise ValueError("image %s is %s %s, expected uint8 (%d, %d, 3): resizing a file to cfg.H x cfg.W "
                             "(multi_view_dataset.py:123) is not built" % (img_path, img.dtype, img.shape, H, W))
        label = _decode_mask(msk_path)
        if label.shape != (H, W):
            raise ValueError("mask %s is %s, the image is (%d, %d)" % (msk_path, label.shape, H, W))
        band = ops.mask_band(self._dev(label)[None], BORDER)[0]
        fill = ("white" if white_bkgd else "black") if mask_bkgd else None
        return ops.image_undistort(self._dev(img), band, cam, n, fill)

    def masks(self, paths, Ks, Ds):
        """multi_view_mesh_dataset.py:102-109 for the V views of a frame -> uint8 [V,H,W] on the device: cv2.undistort of
        (label != 0), not dilated."""
        paths = list(paths)
        if len(paths) < 1 or len(paths) != len(Ks) or len(paths) != len(Ds):
            raise ValueError("masks: %d paths, %d K, %d D" % (len(paths), len(Ks), len(Ds)))
        cams = np.stack([camera_constants(K, D) for K, D in zip(Ks, Ds)])
        labels = [_decode_mask(p) for p in paths]
        for p, m in zip(paths, labels):
            if m.shape != labels[0].shape:
                raise ValueError("mask %s is %s, the first view's is %s" % (p, m.shape, labels[0].shape))
        body = ops.mask_band(self._dev(np.stack(labels)), 1)  # border 1: (label != 0), no band
        return ops.image_undistort(None, body, cams)[1]


def select_prep(mode, device):
    """The YAML key `image_prep` -> None (the sources' cv2 path) or a DeviceImagePrep: 'cv2', 'device', or 'auto' = cv2 where
    it imports (nothing changes there), else the device."""
    if mode not in PREP_MODES:
        raise ValueError("image_prep = %r, expected one of %s" % (mode, ", ".join(PREP_MODES)))
    if mode == "auto":
        try:
            import cv2  # noqa: F401

            mode = "cv2"
        except ImportError:
            mode = "device"
    return DeviceImagePrep(device) if mode == "device" else None
