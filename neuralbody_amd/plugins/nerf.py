"""network_path plugin of the vanilla-NeRF baseline (configs/nerf/nerf_313.yaml): `Network()` with the reference's zero-argument
constructor, reading the reference's global cfg (lib/networks/nerf.py:115-131 reads cfg.xyz_res / cfg.view_res, cfg.netdepth /
cfg.netwidth and their _fine twins, cfg.use_viewdirs).

    nerf_trainable: True    (not a reference key; absent = off) builds NerfNetwork(trainable=True): train() / eval() then switch
                            modes and train_net.py trains the baseline with trainer_path: plugins/nerf_trainer.py"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402  (the reference's config module; run from the reference checkout)

from neuralbody_amd.nerf import NerfNetwork as _NerfNetwork  # noqa: E402


class Network(_NerfNetwork):
    def __init__(self):
        super().__init__(netdepth=cfg.netdepth, netwidth=cfg.netwidth, netdepth_fine=cfg.netdepth_fine,
                         netwidth_fine=cfg.netwidth_fine, use_viewdirs=cfg.use_viewdirs, xyz_res=cfg.xyz_res, view_res=cfg.view_res,
                         precision=str(getattr(cfg, "nerf_precision", "auto")),  # not a reference key: "auto" unless set
                         trainable=bool(getattr(cfg, "nerf_trainable", False)))
        super().train(False)

    def train(self, mode=True):
        """run.py:57,89 call network.train() before they evaluate or visualise (the Neural Body encoder's BatchNorm wants batch
        statistics there).  This network has neither BatchNorm nor dropout and is inference only, so the mode stays eval: the
        reference's entry points then run unedited.  Gradients are still refused (NerfNetwork._inference_only).  A trainable
        network (nerf_trainable: True) switches modes as any module does: training mode is what turns the stratified jitter on."""
        return super().train(mode if self.trainable else False)
