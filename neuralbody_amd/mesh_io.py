"""`MeshEvaluator` and `MeshVisualizer` — drop-ins for zju3dv/neuralbody lib/evaluators/if_nerf_mesh.py::Evaluator and
lib/visualizers/if_nerf_mesh.py::Visualizer (`run.py --type evaluate` / `--type visualize` with the `mesh_cfg` overlay): they
consume the `{"cube", "mesh"}` dict of RendererMesh.render.  plugins/if_nerf_mesh.py binds them to the reference's cfg."""
import os

import numpy as np
import torch

PAD = 10  # the np.pad of if_mesh_renderer.py:46 that both consumers slice off again


def _scalar(v):
    return int(v.reshape(-1)[0].item()) if isinstance(v, torch.Tensor) else int(np.asarray(v).reshape(-1)[0])


def occupied_points(cube, pts, mesh_th, pad=PAD):
    """lib/evaluators/if_nerf_mesh.py:8-12: pts[cube[pad:-pad, pad:-pad, pad:-pad] > mesh_th] as a host array.  `cube` is the
    float64 ndarray of render() or the device cube of density_cube(); in the second case the selection runs on the device and
    only the selected points are downloaded."""
    if isinstance(cube, torch.Tensor) and cube.is_cuda:
        sel = cube[pad:-pad, pad:-pad, pad:-pad] > mesh_th
        return pts.detach().to(cube.device)[sel].cpu().numpy()
    cube = np.asarray(cube.detach().cpu() if isinstance(cube, torch.Tensor) else cube)[pad:-pad, pad:-pad, pad:-pad]
    pts = pts.detach().cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts)
    return pts[cube > mesh_th]


class MeshEvaluator:
    def __init__(self, cfg):
        self.cfg = cfg  # mesh_th, result_dir

    def evaluate(self, output, batch):
        pts = occupied_points(output["cube"], batch["pts"][0], float(self.cfg.mesh_th))
        result_dir = os.path.join(self.cfg.result_dir, "pts")
        os.makedirs(result_dir, exist_ok=True)
        result_path = os.path.join(result_dir, "{}.npy".format(_scalar(batch["i"])))
        np.save(result_path, pts)
        return result_path

    def summarize(self):
        return {}


class MeshVisualizer:
    def __init__(self, cfg):
        # result_dir; optional mesh_render (off unless set), mesh_render_dataset ("zju_mocap"), mesh_render_size (H, W),
        # mesh_render_color (off unless set: a second picture set in the vertex colours of a mesh that has them, cfg.mesh_color)
        self.cfg = cfg
        print("the results are saved at {}".format(os.path.join(cfg.result_dir, "mesh")))

    def visualize(self, output, batch):
        result_dir = os.path.join(self.cfg.result_dir, "mesh")
        os.makedirs(result_dir, exist_ok=True)
        result_path = os.path.join(result_dir, "{:04d}.ply".format(_scalar(batch["frame_index"])))
        output["mesh"].export(result_path)
        if getattr(self.cfg, "mesh_render", False):
            self.render_turntable(output["mesh"], os.path.join(result_dir, "mesh{}_render".format(_scalar(batch["frame_index"]))))
        if getattr(self.cfg, "mesh_render_color", False):
            self.render_turntable(output["mesh"], os.path.join(result_dir, "mesh{}_color".format(_scalar(batch["frame_index"]))),
                                  colors=True)
        return result_path

    def render_turntable(self, mesh, directory, colors=False):
        """tools/render_mesh.py on the mesh just written: the 91 normal-shaded views as `directory/%d.jpg`, drawn on the device
        (neuralbody_amd/mesh_render.py) -> the paths.  colors: the views in the mesh's vertex colours instead.  This package's own
        TriMesh with vertex_normals (cfg.mesh_normals: field) is shaded with those; every other mesh — a trimesh.Trimesh, whose
        `vertex_normals` property is trimesh's own estimate, included — with the triangles' own (nb_mesh_vertex_normals), as before."""
        from .mesh import TriMesh
        from .mesh_render import MeshTurntable

        H, W = getattr(self.cfg, "mesh_render_size", (512, 512))
        turntable = MeshTurntable(int(H), int(W), dataset=getattr(self.cfg, "mesh_render_dataset", "zju_mocap"),
                                  device=getattr(self.cfg, "mesh_render_device", "cuda:0"))
        normals = mesh.vertex_normals if isinstance(mesh, TriMesh) and not colors else None
        if normals is not None:
            normals = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).to(turntable.device)
        return turntable.save(turntable.render(mesh, normals=normals, colors=colors), directory)
