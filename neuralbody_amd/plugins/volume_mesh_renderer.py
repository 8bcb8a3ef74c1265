"""renderer_path plugin for the mesh of the vanilla-NeRF baseline (lib/networks/renderer/volume_mesh_renderer.py): `Renderer(net)`
bound to the reference's global cfg (cfg.N_importance :50,60, cfg.mesh_th :102); selected by the `mesh_cfg` overlay of
configs/nerf/nerf_313.yaml:127-144.  The network stays plugins/nerf.py (the overlay names latent_xyzc; options given on the
command line are merged again after the overlay, lib/config/config.py:166-169, so network_path wins):

    run.py --type visualize --cfg_file configs/nerf/nerf_313.yaml vis_mesh True network_path $NB/nerf.py
           renderer_path $NB/volume_mesh_renderer.py visualizer_path $NB/if_nerf_mesh.py
           test_dataset_path $NB/light_stage_mesh_dataset.py"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.nerf import NerfMeshRenderer as _Renderer  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time.  mesh_backend, mesh_components, mesh_color and mesh_normals are not reference keys:
    off ("auto", "all", False, "faces") unless set in the YAML, with the meanings they have in plugins/if_mesh_renderer.py."""

    mesh_th = property(lambda self: float(cfg.mesh_th))
    N_importance = property(lambda self: int(cfg.N_importance))
    mesh_backend = property(lambda self: str(getattr(cfg, "mesh_backend", "auto")))
    mesh_components = property(lambda self: getattr(cfg, "mesh_components", "all"))
    mesh_color = property(lambda self: bool(getattr(cfg, "mesh_color", False)))
    mesh_normals = property(lambda self: str(getattr(cfg, "mesh_normals", "faces")))


class Renderer(_Renderer):
    def __init__(self, net):
        super().__init__(net, _LiveCfg())
