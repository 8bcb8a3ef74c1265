"""An extracted mesh in other poses: binds a triangle mesh to the SMPL body of its frame and draws it driven by other frames'
parameters, on the device (neuralbody_amd/mesh_rig.py; no marching, no network).

    python tools/animate_mesh.py mesh.ply SMPL_NEUTRAL.pkl params/0.npy params/ out_dir
                                 [--rig out.npz] [--color] [--view 0] [--spin] [--size 512] [--dataset zju_mocap] [--new_params]

mesh.ply: MeshVisualizer's output, or any binary triangle PLY in the body's world frame; the pickle: the SMPL model (its `f` is
the surface the mesh binds to); params/0.npy: EasyMocap's parameters of the frame the mesh was extracted in; then the driving
frames — a directory of {i}.npy taken in numeric order, or a comma-separated list of files.  Writes out_dir/anim/%04d.jpg, one
picture per driving frame seen by turntable view --view (--spin: the view advances with the frame).  --rig also writes the rig
(RiggedMesh.save).  --color draws the mesh's vertex colours instead of the normal shading.  --new_params: the bind frame's
parameters are of the kind that needs pose blend shapes (cfg.new_params of the reference's SMPL fits)."""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_params(path):
    p = np.load(path, allow_pickle=True).item()
    return {k: np.asarray(p[k], np.float32).reshape(-1) for k in ("poses", "shapes", "Rh", "Th")}


def driving_files(spec):
    if os.path.isdir(spec):
        names = [n for n in os.listdir(spec) if re.fullmatch(r"\d+\.npy", n)]
        return [os.path.join(spec, n) for n in sorted(names, key=lambda n: int(n[:-4]))]
    return [s for s in spec.split(",") if s]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("smpl")
    ap.add_argument("bind_params")
    ap.add_argument("drive")
    ap.add_argument("out_dir")
    ap.add_argument("--rig", type=str, default=None)
    ap.add_argument("--color", action="store_true")
    ap.add_argument("--view", type=int, default=0)
    ap.add_argument("--spin", action="store_true")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dataset", type=str, default="zju_mocap")
    ap.add_argument("--new_params", action="store_true")
    ap.add_argument("--device", type=str, default="cuda:0")
    a = ap.parse_args(argv)
    from neuralbody_amd import mesh_rig
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_render import MeshTurntable, _jpeg_writer, to_bgr8
    from neuralbody_amd.smpl_pose import SmplModel

    files = driving_files(a.drive)
    if not files:
        raise SystemExit("no driving parameters at %s (a directory of {i}.npy, or a comma-separated list)" % a.drive)
    write = _jpeg_writer()
    mesh = TriMesh.load_ply(a.mesh)
    if a.color and mesh.vertex_colors is None:
        raise SystemExit("%s holds no vertex colours (write it with mesh_color: True)" % a.mesh)
    body = SmplModel.from_pkl(a.smpl, a.device)
    b = load_params(a.bind_params)
    rig = mesh_rig.bind_mesh(body, mesh, None, b["poses"], b["shapes"], b["Rh"], b["Th"], new_params=a.new_params)
    print("bound %d vertices to %d body triangles (%d rigidly: degenerate blends)" % (rig.n_verts, len(body.faces), rig.n_degenerate))
    if a.rig:
        print("rig written to %s" % rig.save(a.rig))
    drive = [load_params(f) for f in files]
    images = mesh_rig.animate(rig, *(np.stack([d[k] for d in drive]) for k in ("poses", "shapes", "Rh", "Th")),
                              MeshTurntable(a.size, a.size, dataset=a.dataset, device=a.device), colors=a.color, view=a.view, spin=a.spin)
    out = os.path.join(a.out_dir, "anim")
    os.makedirs(out, exist_ok=True)
    bgr = to_bgr8(images)
    paths = []
    for k in range(bgr.shape[0]):
        paths.append(os.path.join(out, "%04d.jpg" % k))
        write(paths[-1], bgr[k])
    print("%d frames written to %s" % (len(paths), out))
    return paths


if __name__ == "__main__":
    main()
