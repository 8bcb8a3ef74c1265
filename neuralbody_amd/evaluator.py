"""`Evaluator` — drop-in for zju3dv/neuralbody lib/evaluators/if_nerf.py::Evaluator (the quality protocol of
`run.py --type evaluate`, run.py:41-69, and of Trainer.val, lib/train/trainers/trainer.py:85-110).

`evaluate(output, batch)` enqueues ONE nb_eval_metrics call per view on data that is already on the device and reads
nothing back; `summarize()` fetches all views with one copy, writes the reference's `metrics.npy` and prints the three
means.  The reference's per-view device-to-host copies, numpy scatter and float64 SSIM on the host are gone.
"""
import os

import numpy as np
import torch

from . import ops


class EvalConfig:
    """The cfg keys the evaluator reads (lib/evaluators/if_nerf.py:23,55,61,77; eval_save_images is this package's)."""

    def __init__(self, H, W, white_bkgd=False, eval_whole_img=False, result_dir="data/result", eval_save_images=False):
        self.H, self.W = int(H), int(W)  # int(cfg.H * cfg.ratio), int(cfg.W * cfg.ratio)
        self.white_bkgd = bool(white_bkgd)
        self.eval_whole_img = bool(eval_whole_img)
        self.result_dir = result_dir
        self.eval_save_images = bool(eval_save_images)  # the comparison PNGs of if_nerf.py:30-41, off by default


def _view_id(v):
    """frame_index / cam_ind as given (tensor or int) -> int; called in summarize() only."""
    if v is None:
        return -1
    if isinstance(v, torch.Tensor):
        return int(v.reshape(-1)[0].item())
    return int(np.asarray(v).reshape(-1)[0])


class Evaluator:
    def __init__(self, cfg):
        self.cfg = cfg
        self._Image = None
        if cfg.eval_save_images:
            from PIL import Image  # raises here, not after a whole evaluation run

            self._Image = Image
        self._views = []  # per view: ([8] fp64 device tensor, frame_index, cam_ind, images or None)

    # -- if_nerf.py:47-74, batch index 0 only like the reference
    def evaluate(self, output, batch):
        """Enqueue the metrics of one view.  No synchronisation, no read-back."""
        rgb_pred = output["rgb_map"]
        if not isinstance(rgb_pred, torch.Tensor) or not rgb_pred.is_cuda:
            raise ops.NbError("output['rgb_map'] must be a tensor on a HIP device (got %s); the evaluator has no host path" % (
                rgb_pred.device if isinstance(rgb_pred, torch.Tensor) else type(rgb_pred).__name__))
        dev = rgb_pred.device
        cfg = self.cfg
        rgb_pred = rgb_pred[0].detach().to(torch.float32).contiguous()
        rgb_gt = batch["rgb"][0].detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        mask = batch["mask_at_box"][0].detach().to(device=dev, non_blocking=True).reshape(-1)
        if mask.dtype != torch.uint8:
            mask = mask.ne(0).to(torch.uint8)
        white, whole = bool(cfg.white_bkgd), bool(cfg.eval_whole_img)
        with torch.cuda.device(dev):
            out = ops.eval_metrics(mask, cfg.H, cfg.W, rgb_pred, rgb_gt, white_bkgd=white, whole_img=whole)
            images = None
            if self._Image is not None:  # uint8 on device; cropped and written in summarize()
                images = tuple((ops.image_assemble(mask, rgb, white_bkgd=white, scale=255.0)[0].clamp_(0.0, 255.0)
                                .to(torch.uint8).reshape(int(cfg.H), int(cfg.W), 3)) for rgb in (rgb_pred, rgb_gt))
        self._views.append((out, batch.get("frame_index"), batch.get("cam_ind"), images))

    def _fetch(self):
        """All pending views as one [n, 8] float64 host array: one copy, one synchronisation."""
        if not self._views:
            return np.zeros((0, 8))
        return torch.stack([v[0] for v in self._views]).cpu().numpy()

    # the reference's list attributes; each read costs one synchronising copy of the pending views
    @property
    def mse(self):
        """Per-view MSE of the views evaluated since the last summarize() (one device synchronisation per read)."""
        return [float(v) for v in self._fetch()[:, 0]]

    @property
    def psnr(self):
        """Per-view PSNR (one device synchronisation per read)."""
        return [float(v) for v in self._fetch()[:, 1]]

    @property
    def ssim(self):
        """Per-view SSIM, NaN where compare_ssim would have raised (one device synchronisation per read)."""
        return [float(v) for v in self._fetch()[:, 2]]

    def _save_images(self, vals):
        result_dir = os.path.join(self.cfg.result_dir, "comparison")
        os.makedirs(result_dir, exist_ok=True)
        for row, (_, frame, cam, images) in zip(vals, self._views):
            x, y, w, h = (int(v) for v in row[3:7])
            for img, tail in zip(images, ("", "_gt")):
                crop = img[y:y + h, x:x + w].cpu().numpy()
                if crop.size:
                    self._Image.fromarray(crop).save(
                        "%s/frame%04d_view%04d%s.png" % (result_dir, _view_id(frame), _view_id(cam), tail))

    # -- if_nerf.py:76-91
    def summarize(self):
        """Writes cfg.result_dir/metrics.npy ({'mse', 'psnr', 'ssim'} lists, the reference's layout), prints the means,
        clears the state and returns the means (the reference returns None, which its own Trainer.val cannot update its
        statistics with).  Raises ValueError for a view whose crop is under 7 pixels on a side — compare_ssim's error,
        deferred to here."""
        vals = self._fetch()
        views = self._views
        try:
            bad = np.flatnonzero(np.isnan(vals[:, 2]))
            if len(bad):
                i = int(bad[0])
                raise ValueError("win_size exceeds image extent: view %d (frame %d, cam %d) has a %d x %d crop, SSIM needs 7 x 7" % (
                    i, _view_id(views[i][1]), _view_id(views[i][2]), int(vals[i, 5]), int(vals[i, 6])))
            if self._Image is not None:
                self._save_images(vals)
        finally:
            self._views = []
        result_dir = self.cfg.result_dir
        print("the results are saved at {}".format(result_dir))
        result_path = os.path.join(result_dir, "metrics.npy")
        os.makedirs(os.path.dirname(result_path) or ".", exist_ok=True)
        metrics = {"mse": [float(v) for v in vals[:, 0]], "psnr": [float(v) for v in vals[:, 1]],
                   "ssim": [float(v) for v in vals[:, 2]]}
        np.save(result_path, metrics)
        means = {k: float(np.mean(v)) for k, v in metrics.items()}
        print("mse: {}".format(means["mse"]))
        print("psnr: {}".format(means["psnr"]))
        print("ssim: {}".format(means["ssim"]))
        return means
