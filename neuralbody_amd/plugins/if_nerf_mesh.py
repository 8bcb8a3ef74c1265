"""evaluator_path / visualizer_path plugin for mesh extraction: `Evaluator()` and `Visualizer()` bound to the reference's global
cfg (lib/evaluators/if_nerf_mesh.py reads cfg.mesh_th :12 and cfg.result_dir :15; lib/visualizers/if_nerf_mesh.py reads
cfg.result_dir :30).  Select them with

    evaluator_path /path/to/neuralbody_amd/plugins/if_nerf_mesh.py evaluator_module lib.evaluators.if_nerf_mesh
    visualizer_path /path/to/neuralbody_amd/plugins/if_nerf_mesh.py visualizer_module lib.visualizers.if_nerf_mesh
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.mesh_io import MeshEvaluator as _Evaluator, MeshVisualizer as _Visualizer  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time."""

    mesh_th = property(lambda self: float(cfg.mesh_th))
    result_dir = property(lambda self: cfg.result_dir)
    mesh_render = property(lambda self: bool(getattr(cfg, "mesh_render", False)))  # not a reference key: off unless set
    mesh_render_dataset = property(lambda self: str(getattr(cfg, "mesh_render_dataset", "zju_mocap")))
    mesh_render_color = property(lambda self: bool(getattr(cfg, "mesh_render_color", False)))  # likewise; needs mesh_color
    mesh_render_size = property(lambda self: tuple(int(v) for v in getattr(cfg, "mesh_render_size", (512, 512))))


class Evaluator(_Evaluator):
    def __init__(self):
        super().__init__(_LiveCfg())


class Visualizer(_Visualizer):
    def __init__(self):
        super().__init__(_LiveCfg())
