"""trainer_path plugin: `NetworkWrapper(net)` with the reference's forward contract
(lib/train/trainers/if_nerf_clight.py:8-37): returns (ret, loss, scalar_stats, image_stats) with the
masked MSE of rgb_map against batch['rgb'].  Under torch.enable_grad() with trainable parameters
Renderer.render takes the differentiable HIP path (neuralbody_amd/training.py), so loss.backward() fills the
gradients of every parameter; under no_grad it is the fused inference march.

Two more terms of the TRAINING step (gradients enabled), both off unless their YAML key is set (not reference keys; absent or 0 =
off, and forward() then runs the reference's statements alone):

    mask_loss_weight: mu          loss += mu * smooth_l1_loss(acc_map[mask_at_box], occupancy[mask_at_box]) — the acc_crit the
                                  reference wrapper instantiates (:16) and never applies; needs `train_ray_mask: True` so that the
                                  dataset adds `occupancy` (plugins/light_stage_dataset.py); scalar_stats['mask_loss']
    distortion_loss_weight: lam   loss += lam * mean(ops.ray_distortion(weights, z_vals)[mask_at_box]) — compactness of each ray's
                                  weights (include/nb_hip.h: nb_ray_distortion); scalar_stats['distortion_loss']
"""
import os
import sys

import torch
import torch.nn as nn

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd import ops  # noqa: E402
from neuralbody_amd.plugins.if_clight_renderer import Renderer  # noqa: E402


class NetworkWrapper(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.renderer = Renderer(self.net)
        self.img2mse = lambda x, y: torch.mean((x - y) ** 2)
        self.acc_crit = torch.nn.functional.smooth_l1_loss

    def forward(self, batch):
        # both terms belong to the training step: under no_grad (Trainer.val on the test split, whose items carry no occupancy and
        # whose inference dict carries no z_vals) the loss is the reference's
        train = torch.is_grad_enabled()
        mu = float(getattr(cfg, "mask_loss_weight", 0) or 0) if train else 0.0
        lam = float(getattr(cfg, "distortion_loss_weight", 0) or 0) if train else 0.0
        if mu != 0.0 and "occupancy" not in batch:
            raise KeyError("mask_loss_weight = %g needs batch['occupancy']: set train_ray_mask: True so that the training dataset "
                           "adds it (plugins/light_stage_dataset.py)" % mu)
        ret = self.renderer.render(batch)
        scalar_stats = {}
        loss = 0
        mask = batch["mask_at_box"]
        img_loss = self.img2mse(ret["rgb_map"][mask], batch["rgb"][mask])
        scalar_stats.update({"img_loss": img_loss})
        loss += img_loss
        if mu != 0.0:
            mask_loss = self.acc_crit(ret["acc_map"][mask], batch["occupancy"][mask].to(ret["acc_map"]))
            scalar_stats.update({"mask_loss": mask_loss})
            loss += mu * mask_loss
        if lam != 0.0:
            w, z = ret["weights"], ret["z_vals"]
            S = w.shape[-1]
            dist = ops.ray_distortion(w.reshape(-1, S), z.reshape(-1, S).float().contiguous()).view(w.shape[:-1])
            distortion_loss = torch.mean(dist[mask])
            scalar_stats.update({"distortion_loss": distortion_loss})
            loss += lam * distortion_loss
        scalar_stats.update({"loss": loss})
        image_stats = {}
        return ret, loss, scalar_stats, image_stats
