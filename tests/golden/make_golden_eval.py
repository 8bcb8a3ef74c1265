"""Generate tests/golden/eval_metrics.npz by driving the UNMODIFIED reference evaluator
(lib/evaluators/if_nerf.py::Evaluator.evaluate) on CPU through oracle/ref_harness.py.  Run from the repo root, where the
reference tree exists:   python tests/golden/make_golden_eval.py

The evaluator's two imports that do not exist on this stack are seeded into sys.modules BEFORE ref_harness.load() (which
uses setdefault):
  * skimage.measure.compare_ssim — removed from scikit-image after 0.17; restated here from scikit-image 0.14.2's algorithm
    (requirements.txt:6) on scipy.ndimage.uniform_filter
  * cv2.boundingRect in numpy, cv2.imwrite as a no-op (the comparison PNGs are not part of the fixture)

The fixture holds the synthetic inputs and the reference's mse / psnr / ssim per case: data only.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.dirname(os.path.abspath(__file__))
BOXES = {}  # what the cv2.boundingRect stand-in returned during the current evaluate()


def compare_ssim(X, Y, win_size=None, gradient=False, data_range=None, multichannel=False, gaussian_weights=False,
                 full=False, **kwargs):
    """scikit-image 0.14.2 skimage.measure.compare_ssim, the uniform-window path the reference takes."""
    from scipy.ndimage import uniform_filter

    assert X.shape == Y.shape and not gradient and not gaussian_weights and not full
    if multichannel:
        return float(np.mean([compare_ssim(X[..., c], Y[..., c], win_size=win_size, data_range=data_range)
                              for c in range(X.shape[-1])]))
    K1, K2 = kwargs.pop("K1", 0.01), kwargs.pop("K2", 0.03)
    use_sample_covariance = kwargs.pop("use_sample_covariance", True)
    if win_size is None:
        win_size = 7
    if np.any((np.asarray(X.shape) - win_size) < 0):
        raise ValueError("win_size exceeds image extent.  If the input is a multichannel (color) image, set multichannel=True.")
    if data_range is None:
        assert X.dtype.kind == "f"
        dmin, dmax = -1, 1  # skimage.util.dtype.dtype_range of every float type
        data_range = dmax - dmin
    ndim = X.ndim
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    NP = win_size ** ndim
    cov_norm = NP / (NP - 1) if use_sample_covariance else 1.0
    ux, uy = uniform_filter(X, size=win_size), uniform_filter(Y, size=win_size)
    uxx, uyy, uxy = uniform_filter(X * X, size=win_size), uniform_filter(Y * Y, size=win_size), uniform_filter(X * Y, size=win_size)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    R = data_range
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (win_size - 1) // 2
    return S[tuple(slice(pad, -pad) for _ in range(ndim))].mean()


def bounding_rect(mask):
    ys, xs = np.nonzero(mask)
    box = (0, 0, 0, 0) if len(xs) == 0 else (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))
    BOXES["last"] = box
    return box


def seed_modules():
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    skm.compare_ssim = compare_ssim
    sk.measure = skm
    sys.modules["skimage"], sys.modules["skimage.measure"] = sk, skm
    cv2 = types.ModuleType("cv2")
    cv2.boundingRect = bounding_rect
    cv2.imwrite = lambda *a, **k: True
    sys.modules["cv2"] = cv2


def smooth_pair(H, W, seed, noise=0.05):
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64) / H, np.arange(W, dtype=np.float64) / W, indexing="ij")
    gt = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + 1.0), 0.5 + 0.4 * np.cos(5.0 * yy - 0.5), 0.5 + 0.4 * np.sin(4.0 * (xx + yy))], -1)
    pred = np.clip(gt + 0.03 * np.sin(9.0 * (xx - yy))[..., None] + noise * rs.standard_normal(gt.shape), 0.0, 1.0)
    return pred.astype(np.float32), gt.astype(np.float32)


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def cases():
    """name -> (mask [H,W] bool, white_bkgd, eval_whole_img, identical)"""
    out = {}
    out["black_bkgd"] = (ellipse(96, 80, 50, 38, 40, 27), 0, 0, False)
    out["white_bkgd"] = (ellipse(96, 80, 50, 38, 40, 27), 1, 0, False)
    out["whole_img"] = (ellipse(72, 100, 30, 55, 22, 31), 1, 1, False)
    out["two_borders"] = (ellipse(64, 90, 10, 12, 30, 40), 0, 0, False)  # reaches x = 0 and y = 0
    m = np.zeros((100, 128), bool)
    m[12:70, 9:50] = True
    m[30:45, 20:35] = False  # a hole: keeps the background inside the crop
    m[40:93, 77:119] = ellipse(53, 42, 26, 21, 26, 20)  # a second component
    out["holes_two_components"] = (m, 1, 0, False)
    m = np.zeros((48, 40), bool)
    m[9:33, 17:24] = True  # crop exactly 7 wide: one column of windows
    out["crop_7_wide"] = (m, 0, 0, False)
    out["identical"] = (ellipse(80, 96, 40, 50, 30, 36), 0, 0, True)
    return out


def main():
    seed_modules()
    from oracle import ref_harness as rh

    ns = rh.load()
    import lib.evaluators.if_nerf as ref_eval  # the reference's module, unmodified

    assert ref_eval.compare_ssim is compare_ssim and ref_eval.cv2.boundingRect is bounding_rect
    cfg = ns.cfg
    store = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        cfg.result_dir = tmp
        for i, (name, (mask, white, whole, identical)) in enumerate(cases().items()):
            H, W = mask.shape
            pred, gt = smooth_pair(H, W, seed=100 + i)
            rgb_pred, rgb_gt = pred[mask], gt[mask]
            if identical:
                rgb_pred = rgb_gt.copy()
            cfg.H, cfg.W, cfg.ratio = H, W, 1.0
            cfg.white_bkgd, cfg.eval_whole_img = bool(white), bool(whole)
            ev = ref_eval.Evaluator()
            output = {"rgb_map": torch.from_numpy(rgb_pred)[None]}
            batch = {"rgb": torch.from_numpy(rgb_gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(1, -1)),
                     "frame_index": torch.tensor([i]), "cam_ind": torch.tensor([0])}
            BOXES.pop("last", None)
            with np.errstate(divide="ignore"):
                ev.evaluate(output, batch)
            box = BOXES.get("last", (0, 0, W, H))  # eval_whole_img never asks for the box
            names.append(name)
            store[name + "/mask"] = mask
            store[name + "/rgb_pred"] = rgb_pred
            store[name + "/rgb_gt"] = rgb_gt
            store[name + "/flags"] = np.array([white, whole], np.int32)
            store[name + "/box"] = np.array(box, np.int32)
            store[name + "/metrics"] = np.array([ev.mse[0], ev.psnr[0], ev.ssim[0]], np.float64)
            print("%-22s %3dx%-3d n=%5d box=%s mse=%.9g psnr=%.9g ssim=%.15g" % (name, H, W, mask.sum(), box, ev.mse[0], ev.psnr[0], ev.ssim[0]))
    store["names"] = np.array(names)
    path = os.path.join(OUT, "eval_metrics.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
