"""trainer_path plugin of the vanilla-NeRF baseline: `NetworkWrapper(net)` with the reference's forward contract
(lib/train/trainers/nerf.py:8-37): returns (ret, loss, scalar_stats, image_stats) with img_loss, the MSE of rgb_map against
batch['rgb'] over mask_at_box, and img_loss0, the MSE of rgb0 over ALL rays (as the reference writes it).  Under
torch.enable_grad() the network must be trainable (nerf_trainable: True, plugins/nerf.py): VolumeRenderer.render then takes the
differentiable HIP path (neuralbody_amd/nerf.py) and loss.backward() fills the gradients of all 48 parameters.  The optimizer and
the scheduler stay the reference's (lib/train/optimizer.py, lib/train/scheduler.py)."""
import os
import sys

import torch
import torch.nn as nn

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from neuralbody_amd.plugins.volume_renderer import Renderer  # noqa: E402


class NetworkWrapper(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.renderer = Renderer(self.net)
        self.img2mse = lambda x, y: torch.mean((x - y) ** 2)
        self.acc_crit = torch.nn.functional.smooth_l1_loss

    def forward(self, batch):
        if torch.is_grad_enabled() and not getattr(self.net, "trainable", False):
            raise RuntimeError("the NeRF baseline's network is inference only: set nerf_trainable: True in the YAML to train it "
                               "(plugins/nerf.py), or call the wrapper under torch.no_grad()")
        ret = self.renderer.render(batch)
        scalar_stats = {}
        loss = 0
        mask = batch["mask_at_box"]
        img_loss = self.img2mse(ret["rgb_map"][mask], batch["rgb"][mask])
        scalar_stats.update({"img_loss": img_loss})
        loss += img_loss
        if "rgb0" in ret:
            img_loss0 = self.img2mse(ret["rgb0"], batch["rgb"])
            scalar_stats.update({"img_loss0": img_loss0})
            loss += img_loss0
        scalar_stats.update({"loss": loss})
        image_stats = {}
        return ret, loss, scalar_stats, image_stats
