"""Times the field normals on the bench scene (bench.build_scene: 512 x 512 rays, 64 samples) and writes profiles/field_normals.json:
  (a) render() of one view with and without normals=True, and the three stages behind the march one by one on that view's weights:
      nb_normal_select (count + place), Network.calculate_density_gradient at the selected samples, nb_normal_composite; beside them
      the selected share of the samples and the mean of acc_map - normal_acc (the weight the threshold leaves out),
  (b) the mesh case: calculate_density_gradient per 100 000 points beside calculate_density(precision="f32") of the same points
      (the first 100 000 selected samples stand in for mesh vertices: points on the surface).
No threshold is set on these numbers: the file is the record.  Device work is timed with HIP events per call after warm-up.

    python tools/bench_field_normals.py [--reps 5] [--out profiles/field_normals.json] [--head <commit>]
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

SIZE, N_SAMPLES, MESH_POINTS = 512, 64, 100000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_normals.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_field_normals needs an MI355X: a CPU run gives no timing")
    import bench
    from neuralbody_amd import ops

    dev = torch.device("cuda:0")
    sd, body, net, rend, bd, n = bench.build_scene(dev, SIZE, SIZE, N_SAMPLES)
    w_min = float(rend.cfg.normal_weight_min)
    with torch.no_grad():
        sp = rend.prepare_sp_input(bd)
        fv = net.encode_sparse_voxels(sp)
        out = rend.render(bd, feature_volume=fv, normals=True)
        ro, rd, near, far = (bd[k][0].contiguous() for k in ("ray_o", "ray_d", "near", "far"))
        weights = out["weights"][0].contiguous()
        t_vals = net.t_vals(N_SAMPLES, dev)
        scratch = ops.scan_scratch(n * N_SAMPLES, dev)
        total = int(ops.normal_select(ro, rd, near, far, t_vals, None, weights, w_min, scratch=scratch)[1].item())
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        wpts = torch.empty((total, 3), dtype=torch.float32, device=dev)

        def select():
            ops.normal_select(ro, rd, near, far, t_vals, None, weights, w_min, scratch=scratch)
            ops.normal_select(ro, rd, near, far, t_vals, None, weights, w_min, idx, wpts, scratch=scratch)

        select()
        grad = net.calculate_density_gradient(wpts[None], fv, sp)[1][0]
        view = dict(
            rays=n, samples=N_SAMPLES, precision=net.march_precision(), normal_weight_min=w_min, selected_samples=total,
            selected_share=total / float(n * N_SAMPLES), rays_with_a_normal=int((out["normal_map"][0] != 0).any(1).sum()),
            mean_acc_minus_normal_acc=float((out["acc_map"] - out["normal_acc"]).mean()),
            render=event_ms(lambda: rend.render(bd, feature_volume=fv), args.reps, warmup=2),
            render_with_normals=event_ms(lambda: rend.render(bd, feature_volume=fv, normals=True), args.reps, warmup=1),
            select=event_ms(select, args.reps, warmup=1),
            gradient=event_ms(lambda: net.calculate_density_gradient(wpts[None], fv, sp), args.reps, warmup=1),
            composite=event_ms(lambda: ops.normal_composite(idx, grad, weights), args.reps, warmup=1))
        print(json.dumps(view))
        m = min(MESH_POINTS, total)
        verts = wpts[:m][None].contiguous()
        mesh = dict(points=m,
                    density_gradient=event_ms(lambda: net.calculate_density_gradient(verts, fv, sp), args.reps, warmup=1),
                    density_f32=event_ms(lambda: net.calculate_density(verts, fv, sp, precision="f32"), args.reps, warmup=1))
        mesh["gradient_ms_per_100k"] = mesh["density_gradient"]["mean_ms"] * 1e5 / max(m, 1)
        mesh["density_ms_per_100k"] = mesh["density_f32"]["mean_ms"] * 1e5 / max(m, 1)
        print(json.dumps(mesh))
    rec = dict(tool="tools/bench_field_normals.py", head=args.head or _head(), box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               timing="HIP events per call after warm-up; render_with_normals includes the 8-byte read-back of the selected count",
               condition="none: nobody has measured these before; the file is the record", view=view, mesh_vertices=mesh)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
