"""numpy-only float64 restatement of the reference's per-view metrics (lib/evaluators/if_nerf.py:47-74 with
scikit-image 0.14.2's compare_ssim): scatter at mask_at_box, tight box of the mask, 49-shift window sums, S, means.
Needs neither scipy, skimage nor cv2, so it also runs where only the GPU tests run."""
import numpy as np

WIN = 7
SSIM_DATA_RANGE = 2.0  # compare_ssim's dtype_range for float images is (-1, 1); the reference passes no data_range
K1, K2 = 0.01, 0.03


def bounding_rect(mask):
    """cv2.boundingRect of a mask: (x, y, w, h) of the non-zero pixels, (0, 0, 0, 0) when there are none."""
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def scatter(mask, rgb, white_bkgd):
    """if_nerf.py:56-59: float64 [H,W,3] image filled with the background, the compacted rays at the mask."""
    img = np.zeros(mask.shape + (3,)) + int(white_bkgd)
    img[mask.astype(bool)] = rgb
    return img


def window_sums(a):
    """Sum over every 7 x 7 window that lies fully inside a [h,w] array -> [h-6, w-6]."""
    h, w = a.shape
    out = np.zeros((h - WIN + 1, w - WIN + 1))
    for dy in range(WIN):
        for dx in range(WIN):
            out += a[dy:dy + h - WIN + 1, dx:dx + w - WIN + 1]
    return out


def ssim(img_pred, img_gt):
    """compare_ssim(pred, gt, multichannel=True) of scikit-image 0.14.2 on float images: uniform 7 x 7 window, sample
    covariance, mean of S without the 3-pixel border (= over the fully inside windows), then over the channels."""
    if min(img_pred.shape[:2]) < WIN:
        raise ValueError("win_size exceeds image extent")
    n = float(WIN * WIN)
    cov_norm = n / (n - 1.0)
    c1, c2 = (K1 * SSIM_DATA_RANGE) ** 2, (K2 * SSIM_DATA_RANGE) ** 2
    per_channel = []
    for ch in range(img_pred.shape[2]):
        x, y = img_pred[..., ch].astype(np.float64), img_gt[..., ch].astype(np.float64)
        ux, uy = window_sums(x) / n, window_sums(y) / n
        uxx, uyy, uxy = window_sums(x * x) / n, window_sums(y * y) / n, window_sums(x * y) / n
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        per_channel.append(s.mean())
    return float(np.mean(per_channel))


def metrics(mask, rgb_pred, rgb_gt, white_bkgd=False, whole_img=False):
    """mask [H,W] bool, rgb_pred / rgb_gt [n,3] float32 -> dict(mse, psnr, ssim, box=(x, y, w, h), n_windows).
    ssim is NaN where compare_ssim raises (crop under 7 pixels on a side)."""
    mask = np.asarray(mask).astype(bool)
    H, W = mask.shape
    rgb_pred, rgb_gt = np.asarray(rgb_pred, np.float32), np.asarray(rgb_gt, np.float32)
    img_pred, img_gt = scatter(mask, rgb_pred, white_bkgd), scatter(mask, rgb_gt, white_bkgd)
    with np.errstate(divide="ignore", invalid="ignore"):
        if whole_img:
            mse = float(np.mean((img_pred - img_gt) ** 2))
            box = (0, 0, W, H)
        else:
            d = rgb_pred - rgb_gt  # fp32, like the reference's arrays; summed in float64 here
            mse = float(np.mean((d * d).astype(np.float64))) if d.size else float("nan")
            box = bounding_rect(mask)
        psnr = float(-10.0 * np.log(mse) / np.log(10.0))
    x, y, w, h = box
    if w >= WIN and h >= WIN:
        s = ssim(img_pred[y:y + h, x:x + w], img_gt[y:y + h, x:x + w])
        n_windows = (w - WIN + 1) * (h - WIN + 1)
    else:
        s, n_windows = float("nan"), 0
    return dict(mse=mse, psnr=psnr, ssim=s, box=box, n_windows=n_windows)


def ellipse_case(H, W, seed, white_bkgd=False, noise=0.05):
    """Procedural view: smooth images plus noise inside an elliptical mask -> (mask [H,W] bool, pred [n,3], gt [n,3]) fp32."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cy, cx, ry, rx = 0.52 * H, 0.47 * W, 0.41 * H, 0.33 * W
    mask = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    u, v = xx / W, yy / H
    gt = np.stack([0.5 + 0.4 * np.sin(6.0 * u + 1.0), 0.5 + 0.4 * np.cos(5.0 * v - 0.5), 0.5 + 0.4 * np.sin(4.0 * (u + v))], -1)
    pred = np.clip(gt + 0.03 * np.sin(9.0 * (u - v))[..., None] + noise * rs.standard_normal(gt.shape), 0.0, 1.0)
    return mask, pred[mask].astype(np.float32), gt[mask].astype(np.float32)
