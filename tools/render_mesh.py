"""The normal-shaded turntable of an extracted mesh, drawn on the device: zju3dv/neuralbody's tools/render_mesh.py (which needs an
OpenGL context: pyglet, PyOpenGL, GLSL) with its command line, for a headless node.

    python tools/render_mesh.py --exp_name xyz_313 --dataset zju_mocap [--mesh_ind 0] [-ww 512] [-hh 512] [--result_dir data/result/if_nerf]
                                [--color]

reads  {result_dir}/{exp_name}/mesh/{mesh_ind:04d}.ply  (MeshVisualizer's output) and writes the 91 views
{result_dir}/{exp_name}/mesh/mesh{mesh_ind}_render/%d.jpg  (neuralbody_amd/mesh_render.py has the camera and the shading).
--color (not a reference option) draws the vertex colours of a mesh written with mesh_color instead, into mesh{mesh_ind}_color.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-ww", "--width", type=int, default=512)
    ap.add_argument("-hh", "--height", type=int, default=512)
    ap.add_argument("--exp_name", type=str, required=True)
    ap.add_argument("--dataset", type=str, default="zju_mocap")
    ap.add_argument("--mesh_ind", type=int, default=0)
    ap.add_argument("--result_dir", type=str, default=os.path.join("data", "result", "if_nerf"))
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--color", action="store_true")
    a = ap.parse_args(argv)
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_render import MeshTurntable

    data_root = os.path.join(a.result_dir, a.exp_name, "mesh")
    ply = os.path.join(data_root, "{:04d}.ply".format(a.mesh_ind))
    out_dir = os.path.join(data_root, "mesh{}_{}".format(a.mesh_ind, "color" if a.color else "render"))
    print("the results are saved at {}".format(out_dir))
    if not os.path.exists(ply):
        raise SystemExit("no mesh at %s (run the mesh visualizer first)" % ply)
    turntable = MeshTurntable(a.height, a.width, dataset=a.dataset, device=a.device)
    mesh = TriMesh.load_ply(ply)
    if a.color and mesh.vertex_colors is None:
        raise SystemExit("%s holds no vertex colours (write it with mesh_color: True)" % ply)
    paths = turntable.save(turntable.render(mesh, colors=a.color), out_dir)
    print("%d views written" % len(paths))
    return paths


if __name__ == "__main__":
    main()
