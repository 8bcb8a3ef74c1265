"""renderer_path plugin of the vanilla-NeRF baseline: `Renderer(net)` bound to the reference's global cfg
(lib/networks/renderer/volume_renderer.py:6-8; cfg.N_samples :48, cfg.lindisp :49, cfg.perturb :56,90, cfg.raw_noise_std /
cfg.white_bkgd :80, cfg.N_importance :82, cfg.chunk :153)."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.nerf import VolumeRenderer as _VolumeRenderer  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time (run.py mutates cfg.perturb after import, run.py:50,82)."""

    N_samples = property(lambda self: int(cfg.N_samples))
    N_importance = property(lambda self: int(cfg.N_importance))
    perturb = property(lambda self: float(cfg.perturb))
    raw_noise_std = property(lambda self: float(cfg.raw_noise_std))
    white_bkgd = property(lambda self: bool(cfg.white_bkgd))
    lindisp = property(lambda self: bool(cfg.lindisp))
    chunk = property(lambda self: int(cfg.chunk))
    H = property(lambda self: int(cfg.H * cfg.ratio))  # image_rays geometry, lib/utils/render_utils.py:121-122
    W = property(lambda self: int(cfg.W * cfg.ratio))


class Renderer(_VolumeRenderer):
    def __init__(self, net):
        super().__init__(net, _LiveCfg())
