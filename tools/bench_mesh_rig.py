"""Times the animatable mesh (csrc/nb_mesh_rig.hip, neuralbody_amd/mesh_rig.py).  The bind mesh is the marching-cubes surface of the
synthetic scene at the mesh pass's resolution; the body is a level-5 ellipsoidal icosphere (10 242 vertices, 20 480 faces against
SMPL's 13 776) fitted inside the mesh's box, with tests/smpl_ref.py's synthetic skinning.  Reported, HIP events around each call
after 10 warm-up calls, 50 calls:
  (a) nb_mesh_closest exhaustive (NB_CLOSEST_EXHAUSTIVE, a bench-only flag) and culled (the default), as point-triangle tests per
      second of the EXHAUSTIVE count P x Nf for both, the fraction of (wave, tile) pairs the culled query skipped, and whether the
      two runs gave the same bits,
  (b) nb_mesh_rig_bind,
  (c) a repose per frame: nb_smpl_pose on the rig + nb_mesh_vertex_normals + one 512 x 512 view,
  (d) the host stand-in of (a): the float32 numpy restatement (tests/mesh_rig_ref.py) on at most 16 threads, on a slice of the
      points (wall clock).
It reports numbers and gates nothing.

    python tools/bench_mesh_rig.py [--reps 50] [--host-points 256] [--out profiles/mesh_rig.json]
"""
import argparse
import json
import os
import socket
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import _head, event_ms  # noqa: E402

DEV = "cuda:0"
IMG = 512
WARMUP = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-points", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_rig.json"))
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    from neuralbody_amd import mesh_rig, ops
    from neuralbody_amd.mesh_render import MeshTurntable
    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from neuralbody_amd.smpl_pose import SmplModel, pack_params
    from tests import helpers as H
    from tests import mesh_rig_ref as ref
    from tests.golden import scenes

    _, sd, batch = scenes.build_mesh()
    rend = RendererMesh(H.make_network(sd, DEV, True, "f32"), RenderConfig(mesh_th=5.0))
    with torch.no_grad():
        points, tris = rend.extract_mesh(H.device_batch(batch, DEV))
    points, tris = points.contiguous(), tris.contiguous()
    lo, hi = points.amin(0).cpu().numpy().astype(np.float64), points.amax(0).cpu().numpy().astype(np.float64)
    arrays = ref.surface_smpl(61, 5, radii=tuple(0.42 * (hi - lo)))
    params = (np.zeros(72, np.float32), np.zeros(10, np.float32), np.zeros(3, np.float32), (0.5 * (lo + hi)).astype(np.float32))
    body = SmplModel.from_arrays(arrays, DEV)
    native, dev_arrays = body.native()
    rows = pack_params(*params).to(DEV)
    ws = torch.empty((1, 512), dtype=torch.float32, device=DEV)
    verts = ops.smpl_pose(native, rows, False, ws=ws)[0][0].contiguous()
    faces = dev_arrays["faces"]
    P, V, Nf = int(points.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    scratch = ops.mesh_closest_scratch(V, Nf, DEV)
    out = [torch.empty((P,), dtype=torch.int32, device=DEV), torch.empty((P, 3), device=DEV), torch.empty((P,), device=DEV)]

    def query(**kw):
        return ops.mesh_closest(points, verts, faces, scratch=scratch, face=out[0], bary=out[1], dist2=out[2], **kw)

    t_ex = event_ms(lambda: query(exhaustive=True), a.reps, WARMUP)
    exhaustive = [t.clone() for t in out]
    t_cull = event_ms(query, a.reps, WARMUP)
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(exhaustive, out))
    query(count_tiles=True)
    skipped, met = ops.mesh_closest_tile_counts(scratch)
    face, bary = out[0], out[1]
    t_bind = event_ms(lambda: ops.mesh_rig_bind(native, rows[0], ws[0], faces, points, face, bary), a.reps, WARMUP)
    dist = out[2].sqrt()

    rig = mesh_rig.bind_mesh(body, points, tris, *params)
    rnative, _ = rig.native()
    drive = pack_params(*ref.draw(62)).to(DEV)
    table = MeshTurntable(IMG, IMG, device=DEV)
    rverts = torch.empty((1, P, 3), device=DEV)
    joints, rws = torch.empty((1, 24, 3), device=DEV), torch.empty((1, 512), device=DEV)
    ops.smpl_pose(rnative, drive, False, rverts, joints, rws)
    cams = table.cams(rverts[0])[:1].contiguous()
    normals, acc = torch.empty((P, 3), device=DEV), torch.empty((P, 3), dtype=torch.int32, device=DEV)
    img = torch.empty((1, IMG, IMG, 3), device=DEV)
    rscratch = ops.mesh_render_scratch(1, IMG, IMG, int(tris.shape[0]), DEV)

    def repose():
        ops.smpl_pose(rnative, drive, False, rverts, joints, rws)
        ops.mesh_vertex_normals(rverts[0], tris, out=normals, scratch=acc)
        ops.mesh_render(rverts[0], normals, tris, cams, IMG, IMG, out=img, scratch=rscratch)

    t_repose = event_ms(repose, a.reps, WARMUP)
    t_pose = event_ms(lambda: ops.smpl_pose(rnative, drive, False, rverts, joints, rws), a.reps, WARMUP)

    # the host stand-in on a slice of the points, split over the threads
    n_host = min(a.host_points, P)
    hp, hv, hf = points[:n_host].cpu().numpy(), verts.cpu().numpy(), faces.cpu().numpy()
    threads = min(16, os.cpu_count() or 1)
    parts = [hp[i::threads] for i in range(threads) if len(hp[i::threads])]
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        got = list(pool.map(lambda q: ref.closest(q, hv, hf, np.float32), parts))
        host_s = time.perf_counter() - t0
    host_face = np.empty(n_host, np.int32)
    for i, g in enumerate(got):
        host_face[i::threads] = g[0]
    tests = float(P) * Nf
    res = {"tool": "tools/bench_mesh_rig.py", "head": a.head or _head(), "box": socket.gethostname(),
           "device": torch.cuda.get_device_name(0),
           "timing": "HIP events per call after %d warm-up calls; host_*: perf_counter" % WARMUP,
           "mesh": dict(vertices=P, triangles=int(tris.shape[0])), "body": dict(vertices=V, triangles=Nf, icosphere_level=5),
           "mesh_to_body_distance_lattice_units": dict(mean=float(dist.mean()), max=float(dist.max())),
           "closest_exhaustive": t_ex, "closest_culled": t_cull,
           "closest_prepass_included": "both times include the prepass (six small launches)",
           "tests_per_second_exhaustive": tests / (t_ex["mean_ms"] * 1e-3),
           "tests_per_second_culled_of_the_exhaustive_count": tests / (t_cull["mean_ms"] * 1e-3),
           "culled_over_exhaustive": t_cull["mean_ms"] / t_ex["mean_ms"],
           "tiles_skipped": skipped, "tiles_met": met, "tile_fraction_skipped": skipped / max(met, 1),
           "culled_equals_exhaustive_bits": bool(same), "degenerate_vertices": int(rig.n_degenerate),
           "bind": t_bind, "repose_pose_normals_one_view": t_repose, "repose_pose_only": t_pose, "image": [IMG, IMG],
           "host_closest_float32_numpy": dict(points=n_host, threads=threads, seconds=host_s, tests_per_second=n_host * float(Nf) / host_s,
                                              faces_equal_device=bool(np.array_equal(host_face, exhaustive[0][:n_host].cpu().numpy()))),
           "note": "reports numbers and gates nothing; the default of nb_mesh_closest is whichever of the two queries is faster here"}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("P = %d, body V = %d, Nf = %d: closest exhaustive %.3f ms (%.3g tests/s), culled %.3f ms, %.1f %% of tiles skipped, same bits: %s"
          % (P, V, Nf, t_ex["mean_ms"], res["tests_per_second_exhaustive"], t_cull["mean_ms"], 100 * res["tile_fraction_skipped"], same))
    print("bind %.4f ms; repose (pose + normals + one %d^2 view) %.4f ms, pose alone %.4f ms; host restatement %.3g tests/s on %d threads"
          % (t_bind["mean_ms"], IMG, t_repose["mean_ms"], t_pose["mean_ms"], res["host_closest_float32_numpy"]["tests_per_second"], threads))


if __name__ == "__main__":
    main()
