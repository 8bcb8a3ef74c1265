"""Times mesh extraction: on the lattice of the mesh test scene at the reference's 5 mm step and on a synthetic 320^3 lattice
  (a) `RendererMesh.density_cube` (scene lattice only),
  (b) what the host path does to the cube before PyMCubes even starts: `cube.double().cpu().numpy()`,
  (c) marching cubes on the device, `ops.marching_cubes` (count, one read of the counts, emit), plus the download of the mesh,
  (d) (c)'s algorithmic bytes over its time as a fraction of the 8 TB/s HBM peak,
and writes profiles/mesh_extract.json.  The condition is relative: (c) must not exceed (b), the least the host path can cost
(it excludes the host marching cubes itself).  HIP events per call after warm-up; mean, min and max over --reps calls.

    python tools/bench_mesh.py [--reps 30] [--out profiles/mesh_extract.json] [--head <commit>]
"""
import argparse
import json
import os
import socket
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s
SCENE_STEP = 0.005  # multi_view_mesh_dataset.py:145
SYNTH_SIDE = 320


def _head():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()), reps=reps)


def algorithmic_bytes(n, n_vert, n_tri):
    """One read of the cube per pass (2 x 4 N), the flags written (12 N edges + 4 N cells), each scan reading its flags twice and
    writing the positions once (3 x 16 N), the outputs (12 V + 12 T) and the positions the emission looks up (4 V + 4 T + 12 T)."""
    return 8 * n + 16 * n + 48 * n + 12 * n_vert + 12 * n_tri + 4 * n_vert + 16 * n_tri


def bench_cube(name, cube, iso, reps):
    from neuralbody_amd import ops

    n = cube.numel()

    def host_prep():  # the host path up to the call of mcubes.marching_cubes
        return cube.double().cpu().numpy()

    def device_mesh():
        v, t = ops.marching_cubes(cube, iso)
        return v.cpu().numpy(), t.cpu().numpy()

    def device_mesh_no_download():
        ops.marching_cubes(cube, iso)

    v, t = device_mesh()
    t_b = event_ms(host_prep, reps, warmup=3)
    t_c = event_ms(device_mesh, reps, warmup=3)
    t_k = event_ms(device_mesh_no_download, reps, warmup=3)
    nbytes = algorithmic_bytes(n, len(v), len(t))
    rec = dict(lattice=name, shape=list(cube.shape), points=n, iso=iso, vertices=len(v), triangles=len(t),
               host_cube_prep=t_b, device_marching_cubes_with_download=t_c, device_marching_cubes=t_k,
               algorithmic_bytes=nbytes, hbm_fraction=nbytes / (t_k["mean_ms"] * 1e-3) / HBM_PEAK,
               hbm_fraction_with_download=nbytes / (t_c["mean_ms"] * 1e-3) / HBM_PEAK,
               device_over_host_prep=t_c["mean_ms"] / t_b["mean_ms"],
               device_not_slower_than_host_prep=bool(t_c["mean_ms"] <= t_b["mean_ms"]))
    return rec


def scene_cube(dev, reps):
    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from tests import helpers as H
    from tests import synthetic as syn
    from tests.golden import scenes

    r, sd, batch = scenes.build_mesh()
    body = syn.make_body(**r["body"])
    pts, inside = syn.make_density_lattice(body, step=SCENE_STEP)
    batch = dict(batch, pts=pts[None], inside=inside[None])
    net = H.make_network(sd, dev, True, H.DEFAULT_PRECISION)  # batch statistics, as the fixture of this scene was rendered
    rend = RendererMesh(net, RenderConfig(mesh_th=5.0))
    bd = H.device_batch(batch, dev)

    def density():
        with torch.no_grad():
            return rend.density_cube(bd)

    cube = density().contiguous()
    return cube, event_ms(density, reps, warmup=3), int(inside.sum())


def synthetic_cube(dev, side=SYNTH_SIDE):
    """A body-sized blob: the union of a few soft spheres, density scale of the scene (values up to ~20, iso 5)."""
    ax = torch.arange(side, dtype=torch.float32, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    g = torch.Generator().manual_seed(0)
    cube = torch.zeros((side, side, side), dtype=torch.float32, device=dev)
    for _ in range(6):
        c = (0.3 + 0.4 * torch.rand(3, generator=g)) * side
        rad = (0.08 + 0.1 * float(torch.rand(1, generator=g))) * side
        d = torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        cube = torch.maximum(cube, (20.0 * (1.0 - d / rad)).clamp_(0.0, 20.0))
    return cube.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda:0")
    cube, t_density, n_inside = scene_cube(dev, args.reps)
    scene = bench_cube("mesh test scene at step %g" % SCENE_STEP, cube, 5.0, args.reps)
    if not scene["triangles"]:
        raise SystemExit("the scene lattice holds no surface at iso 5: nothing was measured")
    scene["density_cube"] = t_density
    scene["inside_points"] = n_inside
    print(json.dumps(scene))
    synth = bench_cube("synthetic %d^3" % SYNTH_SIDE, synthetic_cube(dev), 5.0, args.reps)
    print(json.dumps(synth))
    ok = scene["device_not_slower_than_host_prep"] and synth["device_not_slower_than_host_prep"]
    rec = dict(tool="tools/bench_mesh.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0), timing="HIP events per call after 3 warm-up calls",
               condition="device marching cubes + download of the mesh <= cube.double().cpu().numpy() of the host path",
               meets_condition=bool(ok), hbm_peak_bytes_per_s=HBM_PEAK, lattices=[scene, synth])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
