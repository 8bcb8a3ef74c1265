"""Times the clean-up of an extracted mesh: on the mesh of the mesh test scene's cube at the reference's 5 mm step and on the mesh of
the synthetic 320^3 lattice of tools/bench_mesh.py with stray blobs added,
  (a) the device clean-up: ops.mesh_components + mesh_component_select + mesh_compact ("largest"; one 8-byte read of the counts),
  (b) the host path it replaces, in the same run: download of the mesh, scipy.sparse.csgraph.connected_components, numpy
      compaction, upload of the result,
  (c) separately, the colour pass of the scene's cleaned mesh: normals, nb_mesh_color_query, ONE calculate_density_color on the
      frame's volumes, nb_mesh_color_finish,
and writes profiles/mesh_clean.json.  The condition is relative: (a) must not exceed (b).  Both are reported either way.
HIP events per call after warm-up; mean, min and max over --reps calls (the counts of tools/bench_mesh.py).

    python tools/bench_mesh_clean.py [--reps 30] [--out profiles/mesh_clean.json] [--head <commit>]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import SCENE_STEP, SYNTH_SIDE, _head, event_ms, synthetic_cube  # noqa: E402

N_FLOATERS = 40


def host_clean(vertices, triangles):
    """What a user does today: the mesh to the host, scipy's components, the largest one (by faces) cut out with numpy, back up."""
    import scipy.sparse
    import scipy.sparse.csgraph

    v, t = vertices.cpu().numpy(), triangles.cpu().numpy()
    V = len(v)
    rows, cols = np.concatenate([t[:, 0], t[:, 0]]), np.concatenate([t[:, 1], t[:, 2]])
    graph = scipy.sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V))
    _, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    faces_of = np.bincount(comp[t[:, 0]])
    keep = comp == faces_of.argmax()
    vpos = np.cumsum(keep) - 1
    fkeep = keep[t[:, 0]]
    v2, t2 = v[keep], vpos[t[fkeep]].astype(np.int32)
    return torch.from_numpy(v2).to(vertices.device), torch.from_numpy(t2).to(vertices.device)


def device_clean(vertices, triangles):
    from neuralbody_amd import ops

    scratch = ops.mesh_clean_scratch(vertices.shape[0], triangles.shape[0], vertices.device)
    label = ops.mesh_components(triangles, vertices.shape[0], scratch=scratch)
    keep, stats = ops.mesh_component_select(label, triangles, "largest", scratch=scratch)
    return ops.mesh_compact(vertices, triangles, keep, scratch=scratch) + (stats, scratch)


def bench_mesh(name, cube, iso, reps):
    from neuralbody_amd import ops

    v, t = ops.marching_cubes(cube, iso)
    dv, dt, stats, scratch = device_clean(v, t)
    hv, ht = host_clean(v, t)
    same = bool(torch.equal(dv, hv) and torch.equal(dt, ht))  # a tie between largest components aside, the two agree exactly
    stats = stats.tolist()
    t_dev = event_ms(lambda: device_clean(v, t), reps, warmup=3)
    t_host = event_ms(lambda: host_clean(v, t), reps, warmup=3)
    return dict(mesh=name, cube=list(cube.shape), iso=iso, vertices=len(v), triangles=len(t), components=stats[0],
                kept_vertices=len(dv), kept_triangles=len(dt), give_up_word=int(ops.mesh_give_up(scratch).item()),
                device_equals_host=same, device_clean=t_dev, host_clean=t_host,
                device_over_host=t_dev["mean_ms"] / t_host["mean_ms"],
                device_not_slower_than_host=bool(t_dev["mean_ms"] <= t_host["mean_ms"]))


def scene(dev):
    """The mesh test scene at the reference's step: -> (renderer, device batch, cube)."""
    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from tests import helpers as H
    from tests import synthetic as syn
    from tests.golden import scenes

    r, sd, batch = scenes.build_mesh()
    pts, inside = syn.make_density_lattice(syn.make_body(**r["body"]), step=SCENE_STEP)
    batch = dict(batch, pts=pts[None], inside=inside[None])
    rend = RendererMesh(H.make_network(sd, dev, True, H.DEFAULT_PRECISION), RenderConfig(mesh_th=5.0))
    bd = H.device_batch(batch, dev)
    with torch.no_grad():
        cube, volumes = rend._density_cube(bd)
    return rend, bd, cube.contiguous(), volumes


def with_floaters(cube, n=N_FLOATERS):
    """Small blobs of density away from the body, as a low mesh_th leaves them: n spheres of radius 2 to 4 in the empty cells."""
    side = cube.shape[0]
    g = torch.Generator().manual_seed(1)
    ax = torch.arange(side, dtype=torch.float32, device=cube.device)
    out, placed = cube.clone(), 0
    while placed < n:
        c = (4 + (side - 9) * torch.rand(3, generator=g)).round().long().tolist()
        rad = 2.0 + 2.0 * float(torch.rand(1, generator=g))
        lo, hi = [max(k - 6, 0) for k in c], [min(k + 7, side) for k in c]
        box = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
        if float(out[box].max()) > 0.0:  # taken: by the body or by another floater
            continue
        x, y, z = torch.meshgrid(ax[box[0]], ax[box[1]], ax[box[2]], indexing="ij")
        d = torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        out[box] = (20.0 * (1.0 - d / rad)).clamp_(0.0, 20.0)
        placed += 1
    return out.contiguous()


def bench_colors(rend, bd, cube, volumes, reps):
    from neuralbody_amd import ops

    with torch.no_grad():
        v, t = rend.extract_mesh(bd, cube=cube, components="largest")
    step, origin = rend._world_frame(bd, v)
    step, origin = step.contiguous(), origin.contiguous()

    def decode(wpts, viewdir):
        feature_volume, sp_input = volumes()
        return rend.net.calculate_density_color(wpts, viewdir, feature_volume, sp_input)

    def colors():
        with torch.no_grad():
            normals = ops.mesh_vertex_normals(rend._to_world(v, bd), t)
            return ops.mesh_vertex_colors(v, normals, step, origin, rend.PAD, decode)

    rgb_f = colors()[0]
    return dict(vertices=len(v), triangles=len(t), rgb_min=float(rgb_f.min()), rgb_max=float(rgb_f.max()),
                color_pass=event_ms(colors, reps, warmup=3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda:0")
    rend, bd, cube, volumes = scene(dev)
    rec_scene = bench_mesh("mesh test scene at step %g" % SCENE_STEP, cube, 5.0, args.reps)
    if not rec_scene["triangles"]:
        raise SystemExit("the scene lattice holds no surface at iso 5: nothing was measured")
    print(json.dumps(rec_scene))
    rec_colors = bench_colors(rend, bd, cube, volumes, args.reps)
    print(json.dumps(rec_colors))
    rec_synth = bench_mesh("synthetic %d^3 with %d floaters" % (SYNTH_SIDE, N_FLOATERS), with_floaters(synthetic_cube(dev)), 5.0, args.reps)
    print(json.dumps(rec_synth))
    ok = rec_scene["device_not_slower_than_host"] and rec_synth["device_not_slower_than_host"]
    rec = dict(tool="tools/bench_mesh_clean.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0), timing="HIP events per call after 3 warm-up calls",
               condition="device components + select + compact <= download + scipy connected_components + numpy compaction + upload",
               meets_condition=bool(ok), meshes=[rec_scene, rec_synth], scene_colors=rec_colors)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
