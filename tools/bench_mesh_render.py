"""Times the device turntable (csrc/nb_mesh_render.hip, neuralbody_amd/mesh_render.py) on the mesh RendererMesh.extract_mesh makes
of the synthetic mesh scene (tests/golden/scenes.py::build_mesh): the 91 views at 512 x 512, under HIP events per call after 3
warm-up calls, and writes profiles/mesh_render.json with V, T and
  normals       ops.mesh_vertex_normals (a memset and two launches),
  render        MeshTurntable's loop of ops.mesh_render calls over the 91 views (raster and resolve), and per view,
  resolve_only  the same loop with an EMPTY triangle list: the key fill and the resolve kernel writing background, no winner to
                decode -- a lower bound of the resolve stage,
  raster        render - resolve_only: derived, not measured on its own (the stages share one C call).
The reference draws these pictures with an OpenGL context, which a headless node does not have: there is nothing to compare with,
and no speed-up is claimed.

    python tools/bench_mesh_render.py [--reps 20] [--out profiles/mesh_render.json]
"""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import _head, event_ms  # noqa: E402

DEV = "cuda:0"
IMG = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render.json"))
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    from neuralbody_amd import ops
    from neuralbody_amd.mesh_render import MeshTurntable
    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from tests import helpers as H
    from tests.golden import scenes

    _, sd, batch = scenes.build_mesh()
    rend = RendererMesh(H.make_network(sd, DEV, True, "f32"), RenderConfig(mesh_th=5.0))
    with torch.no_grad():
        verts, tris = rend.extract_mesh(H.device_batch(batch, DEV))
    V, T = int(verts.shape[0]), int(tris.shape[0])
    tt = MeshTurntable(IMG, IMG, device=DEV)
    cams = tt.cams(verts)
    normals = ops.mesh_vertex_normals(verts, tris)
    acc = torch.empty((V, 3), dtype=torch.int32, device=DEV)
    n = tt.views_per_call
    out = torch.empty((tt.n_views, IMG, IMG, 3), dtype=torch.float32, device=DEV)
    scratch = ops.mesh_render_scratch(n, IMG, IMG, T, DEV)
    none = tris[:0].contiguous()

    def loop(faces):
        for k in range(0, tt.n_views, n):
            ops.mesh_render(verts, normals, faces, cams[k:k + n], IMG, IMG, out=out[k:k + n], scratch=scratch)

    t_normals = event_ms(lambda: ops.mesh_vertex_normals(verts, tris, out=normals, scratch=acc), a.reps, 3)
    t_render = event_ms(lambda: loop(tris), a.reps, 3)
    covered = float((out != 1.0).any(-1).float().mean())
    t_resolve = event_ms(lambda: loop(none), a.reps, 3)
    res = {"tool": "tools/bench_mesh_render.py", "head": a.head or _head(), "box": socket.gethostname(),
           "device": torch.cuda.get_device_name(0), "timing": "HIP events per call after 3 warm-up calls",
           "mesh": dict(vertices=V, triangles=T), "views": tt.n_views, "views_per_call": n, "image": [IMG, IMG],
           "covered_pixel_share": covered, "normals": t_normals, "render": t_render,
           "render_ms_per_view": t_render["mean_ms"] / tt.n_views, "resolve_only": t_resolve,
           "raster_derived_ms": t_render["mean_ms"] - t_resolve["mean_ms"],
           "note": "resolve_only renders an empty triangle list (key fill + resolve writing background): a lower bound of the resolve "
                   "stage; raster_derived_ms = render - resolve_only is not a measurement of its own.  No OpenGL baseline exists on a "
                   "headless node; no speed-up is claimed."}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("V = %d, T = %d: normals %.4f ms, render %.3f ms (%.4f ms per view), resolve only %.3f ms" % (
        V, T, t_normals["mean_ms"], t_render["mean_ms"], res["render_ms_per_view"], t_resolve["mean_ms"]))


if __name__ == "__main__":
    main()
