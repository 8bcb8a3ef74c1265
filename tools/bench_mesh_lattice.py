"""Times the mesh pass's query lattice: on the lattice of the mesh test scene at the reference's 5 mm step and on a synthetic
200 x 200 x 400 lattice, both against 4 views of 512 x 512,
  (a) the device stages one by one: nb_mask_dilate, nb_lattice_carve, nb_lattice_gather (count + fill), nb_lattice_scatter,
      with their algorithmic bytes over their time as a fraction of the 8 TB/s HBM peak,
  (b) the whole device item (uploads of the axes and raw masks, dilate, carve; on the scene lattice also
      MeshLatticeDataset.__getitem__ itself, host preparation included),
  (c) the host item it replaces, on the same box in the same run: np.meshgrid of the lattice, the numpy restatement of
      prepare_inside_pts (multi_view_mesh_dataset.py:117-140, 5 x 5 dilation included) and the upload of `pts` and `inside`,
  (d) RendererMesh.density_cube fed by either (scene lattice only): the `pts` batch and the axes batch,
and writes profiles/mesh_lattice.json.  The condition is relative: (b) must not exceed (c) on both lattices.  Device work is
timed with HIP events per call after warm-up, host work with perf_counter around a synchronised call.

    python tools/bench_mesh_lattice.py [--reps 30] [--host-reps 3] [--out profiles/mesh_lattice.json] [--head <commit>]
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import HBM_PEAK, _head, event_ms  # noqa: E402

SCENE_STEP = 0.005  # multi_view_mesh_dataset.py:150 with the shipped voxel_size
SYNTH_DIMS = (200, 200, 400)
N_VIEWS, IMG = 4, 512
PAD = 10


def wall_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()), reps=reps)


def host_item(axes, msks_raw, Ks, RT, dev):
    """What the reference's __getitem__ does with the lattice (:150-160) and what Trainer.to_cuda then uploads."""
    from tests import lattice_ref as lr

    pts = np.stack(np.meshgrid(*[a.astype(np.float64) for a in axes], indexing="ij"), axis=-1).astype(np.float32)
    msks = lr.dilate(msks_raw, 5)
    pts3d = pts.reshape(-1, 3)
    inside = np.ones(len(pts3d), np.uint8)
    H, W = msks.shape[1:]
    for v in range(len(msks)):
        ind = inside == 1
        pts2d = np.round(lr.project_f32(pts3d[ind], Ks[v], RT[v])).astype(np.int32)
        pts2d[:, 0] = np.clip(pts2d[:, 0], 0, W - 1)
        pts2d[:, 1] = np.clip(pts2d[:, 1], 0, H - 1)
        inside[ind] = msks[v][pts2d[:, 1], pts2d[:, 0]]
    inside = inside.reshape(pts.shape[:-1])
    return torch.from_numpy(pts).to(dev), torch.from_numpy(inside).to(dev)


def bench_lattice(name, axes, msks_raw, Ks, RT, dev, reps, host_reps):
    from neuralbody_amd import ops

    dims = [len(a) for a in axes]
    n = dims[0] * dims[1] * dims[2]
    n_pad = (dims[0] + 2 * PAD) * (dims[1] + 2 * PAD) * (dims[2] + 2 * PAD)
    n_pix = int(msks_raw.size)
    RT_d, Ks_d = torch.from_numpy(RT).to(dev), torch.from_numpy(Ks).to(dev)
    scratch = ops.lattice_scratch(dims, dev)

    def device_item():
        ax = [torch.from_numpy(a).to(dev) for a in axes]
        dil = ops.mask_dilate(torch.from_numpy(msks_raw).to(dev), 5)
        cull, keep = ops.make_cull(dil, RT_d, Ks_d)
        return ax, ops.lattice_carve(ax, cull, scratch=scratch)

    ax, (inside, n_inside) = device_item()
    total = int(n_inside.item())
    raw_d = torch.from_numpy(msks_raw).to(dev)
    dil = ops.mask_dilate(raw_d, 5)
    cull, keep = ops.make_cull(dil, RT_d, Ks_d)
    wpts = torch.empty((total, 3), dtype=torch.float32, device=dev)
    lin = torch.empty(total, dtype=torch.int32, device=dev)
    alpha = torch.rand((1, total, 1), device=dev)

    def gather():
        ops.lattice_gather(ax, inside, scratch=scratch)
        ops.lattice_gather(ax, inside, wpts, lin, scratch=scratch)

    stages = {
        "mask_dilate": (lambda: ops.mask_dilate(raw_d, 5, out=dil), 2 * n_pix),
        "lattice_carve": (lambda: ops.lattice_carve(ax, cull, scratch=scratch, inside=inside, n_inside=n_inside), 2 * n + n_pix),
        "lattice_gather": (gather, 4 * n + 16 * total),
        "lattice_scatter": (lambda: ops.lattice_scatter(alpha, lin, dims, PAD), 8 * total + 4 * total + 4 * n_pad),
    }
    rec = dict(lattice=name, dims=dims, points=n, inside_points=total, views=int(msks_raw.shape[0]),
               image=list(msks_raw.shape[1:]), stages={})
    for k, (fn, nbytes) in stages.items():
        t = event_ms(fn, reps, warmup=3)
        rec["stages"][k] = dict(t, algorithmic_bytes=nbytes, hbm_fraction=nbytes / (t["mean_ms"] * 1e-3) / HBM_PEAK)
    rec["device_item"] = event_ms(device_item, reps, warmup=3)
    rec["device_item_wall"] = wall_ms(device_item, reps)
    rec["device_item_uploaded_bytes"] = 4 * sum(dims) + n_pix
    host_pts, host_inside = host_item(axes, msks_raw, Ks, RT, dev)
    agree = float((host_inside == inside).float().mean())
    rec["host_item_wall"] = wall_ms(lambda: host_item(axes, msks_raw, Ks, RT, dev), host_reps, warmup=0)
    rec["host_item_uploaded_bytes"] = 13 * n
    rec["host_and_device_bitmaps_agree_fraction"] = agree
    rec["device_over_host"] = rec["device_item_wall"]["mean_ms"] / rec["host_item_wall"]["mean_ms"]
    rec["device_item_not_slower_than_host_item"] = bool(rec["device_item_wall"]["mean_ms"] <= rec["host_item_wall"]["mean_ms"])
    return rec, host_pts, host_inside, ax, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_lattice.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_lattice needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    from neuralbody_amd.mesh_lattice import MemoryMeshSource, MeshLatticeConfig, MeshLatticeDataset, lattice_axes
    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from tests import helpers as H
    from tests import synthetic as syn
    from tests.golden import scenes

    dev = torch.device("cuda:0")
    r, sd, batch = scenes.build_mesh()
    body = syn.make_body(**r["body"])
    msks_raw, Ks, RT = syn.make_view_masks(body, IMG, IMG, n_views=N_VIEWS, focal_factor=1.8, distance=1.6, dilate=6)
    cb = body["can_bounds"]

    axes = lattice_axes(cb, (SCENE_STEP,) * 3)
    scene, pts, host_inside, ax, inside = bench_lattice("mesh test scene at step %g" % SCENE_STEP, axes, msks_raw, Ks, RT, dev,
                                                        args.reps, args.host_reps)
    rh_, th_ = np.array(r["body"]["rh"], np.float64), np.array(r["body"]["th"], np.float32).reshape(1, 3)
    ds = MeshLatticeDataset(MemoryMeshSource([(msks_raw, body["world_verts"], rh_, th_)], Ks, RT[:, :, :3], RT[:, :, 3:]),
                            MeshLatticeConfig(num_train_frame=r["num_train_frame"], voxel_size=(SCENE_STEP,) * 3), device=dev)
    assert torch.equal(ds[0]["inside"], inside)
    scene["dataset_getitem_wall"] = wall_ms(lambda: ds[0], args.reps)
    net = H.make_network(sd, dev, True, H.DEFAULT_PRECISION)
    rend = RendererMesh(net, RenderConfig(mesh_th=5.0))
    common = {k: v for k, v in H.device_batch(batch, dev).items() if k not in ("pts", "inside")}
    bd_pts = dict(common, pts=pts[None], inside=inside[None])
    bd_axes = dict(common, inside=inside[None], axis_x=ax[0][None], axis_y=ax[1][None], axis_z=ax[2][None])

    def density(bd):
        with torch.no_grad():
            return rend.density_cube(bd)

    scene["density_cubes_equal"] = bool(torch.equal(density(bd_pts), density(bd_axes)))
    scene["density_cube_from_pts"] = event_ms(lambda: density(bd_pts), args.reps, warmup=3)
    scene["density_cube_from_axes"] = event_ms(lambda: density(bd_axes), args.reps, warmup=3)
    print(json.dumps(scene))
    del pts, bd_pts

    axes = [np.linspace(cb[0, a], cb[1, a], m).astype(np.float32) for a, m in enumerate(SYNTH_DIMS)]
    synth = bench_lattice("synthetic %d x %d x %d" % SYNTH_DIMS, axes, msks_raw, Ks, RT, dev, args.reps, args.host_reps)[0]
    print(json.dumps(synth))
    ok = scene["device_item_not_slower_than_host_item"] and synth["device_item_not_slower_than_host_item"]
    rec = dict(tool="tools/bench_mesh_lattice.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0),
               timing="device: HIP events per call after 3 warm-up calls; host and *_wall: perf_counter around a synchronised call",
               condition="device item (upload axes + raw masks, dilate, carve; wall clock) <= host item (meshgrid, numpy "
                         "prepare_inside_pts, upload of pts and inside; wall clock) on both lattices",
               meets_condition=bool(ok), hbm_peak_bytes_per_s=HBM_PEAK, lattices=[scene, synth])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
