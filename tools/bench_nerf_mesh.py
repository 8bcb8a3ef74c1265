"""Times the mesh pass of the vanilla-NeRF baseline (neuralbody_amd/nerf.py: NerfMeshRenderer) on an MI355X and writes
profiles/nerf_mesh.json:

  * nb_nerf_density against nb_nerf_decode on the same 2^20 points, per arithmetic that is built: nb_nerf_decode was the only route
    to a density before.  The two are launched alternately, so that both see the same machine; their fourth column / output are
    compared bit for bit at that size.  The trunk is 491 520 of the 593 920 multiply-adds the packed blob holds per point (0.83);
  * the stages of one extraction on a 240 x 400 x 120 lattice with an ellipsoid `inside`: the gather's count pass and gather, the
    density, the scatter, marching cubes, and the optional queries (face normals, field normals = density_gradient +
    nb_normal_composite, colours = one forward + nb_mesh_color_finish), HIP events around each, after a warm-up of every shape.

    python tools/bench_nerf_mesh.py [--reps 5] [--out profiles/nerf_mesh.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
POINTS = 1 << 20
DIMS, HALF, SEMI = (240, 400, 120), (0.6, 1.0, 0.3), (0.58, 0.97, 0.29)
MACS_TRUNK, MACS_BLOB = 491520, 593920  # multiply-adds per point the packed matrices hold, K padded to whole chunks


def _stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "nerf_mesh.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf_mesh needs an MI355X: a CPU run gives no timing")
    from neuralbody_amd import build as nb_build
    from neuralbody_amd import mesh_extract, nerf, ops
    from tests import nerf_ref as ref  # the fixture's weight recipe: the tool measures the field the tests check

    dev = torch.device("cuda:0")
    fx = dict(np.load(os.path.join(HERE, "tests", "golden", "nerf_mesh.npz")))
    sd = ref.make_state_dict(fx["alpha_shift"])
    iso = float(fx["iso"][1])
    rec = dict(tool="tools/bench_nerf_mesh.py", head=args.head, sources_sha256=nb_build._digest(),
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, macs_trunk=MACS_TRUNK, macs_blob=MACS_BLOB,
               expected_ratio_from_flops=MACS_TRUNK / MACS_BLOB,
               timing="HIP events around each call, a synchronise after each; every shape warmed up once before its timed calls")

    def network(prec):
        net = nerf.NerfNetwork(precision=prec)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return net.to(dev).eval()

    rs = np.random.RandomState(0)
    pts = torch.from_numpy(rs.uniform(-0.6, 0.6, (POINTS, 3)).astype(np.float32)).to(dev)
    d = torch.zeros_like(pts)
    d[:, 2] = 1.0
    z = torch.zeros((POINTS, 1), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for prec in sorted(ops.NERF_PRECISIONS):
            net = network(prec)
            blob = net.packed("fine")
            alpha, raw = torch.empty(POINTS, device=dev), torch.empty((POINTS, 1, 4), device=dev)
            density = lambda: ops.nerf_density(blob, pts, prec, out=alpha)  # noqa: E731
            decode = lambda: ops.nerf_decode(blob, pts, d, z, prec, out=raw)  # noqa: E731
            density(), decode()
            torch.cuda.synchronize()
            same = bool(torch.equal(alpha.view(torch.int32), raw[:, 0, 3].contiguous().view(torch.int32)))
            t_den, t_dec = [], []
            for _ in range(args.reps):  # alternately: both see the same machine
                t_den.append(_time(density)[0])
                t_dec.append(_time(decode)[0])
            rec["density_vs_decode_" + prec] = dict(
                points=POINTS, density=_stats(t_den), decode=_stats(t_dec), ratio_of_means=float(np.mean(t_den) / np.mean(t_dec)),
                ratio_of_minima=float(np.min(t_den) / np.min(t_dec)), same_bits_as_decode=same,
                density_tflops=2.0 * MACS_TRUNK * POINTS / (np.min(t_den) * 1e-3) / 1e12)
            print(prec, json.dumps(rec["density_vs_decode_" + prec]))

        # one extraction, stage by stage: the default arithmetic, the fine module
        net = network("auto")
        axes = [torch.linspace(-h, h, n, device=dev) for h, n in zip(HALF, DIMS)]
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)
        inside = (((grid / torch.tensor(SEMI, device=dev)) ** 2).sum(-1) <= 1.0).to(torch.uint8).contiguous()
        del grid
        batch = {"axis_x": axes[0][None], "axis_y": axes[1][None], "axis_z": axes[2][None], "inside": inside[None],
                 "wbounds": torch.tensor([[[-h for h in HALF], list(HALF)]], device=dev)}
        stages = {}

        def stage(name, fn):
            ms, out = _time(fn)
            stages.setdefault(name, []).append(ms)
            return out

        info = {}
        for rep in range(args.reps + 1):
            scratch = ops.lattice_scratch(list(DIMS), dev)
            total = stage("gather_count", lambda: int(ops.lattice_gather(axes, inside, scratch=scratch)[1].item()))
            wpts = torch.empty((total, 3), dtype=torch.float32, device=dev)
            lin = torch.empty(total, dtype=torch.int32, device=dev)
            stage("gather", lambda: ops.lattice_gather(axes, inside, wpts, lin, scratch=scratch))
            alpha = stage("density", lambda: net.density(wpts, model="fine"))
            cube = stage("scatter", lambda: ops.lattice_scatter(alpha, lin, list(DIMS), mesh_extract.PAD))
            v, t = stage("marching_cubes", lambda: ops.marching_cubes(cube, iso))
            wv = mesh_extract.to_world(v, batch)
            face = stage("face_normals", lambda: ops.mesh_vertex_normals(wv, t))
            V = v.shape[0]
            grad = stage("density_gradient", lambda: net.density_gradient(wv, model="fine")[1])
            unit = stage("normal_composite", lambda: ops.normal_composite(torch.arange(V, dtype=torch.int32, device=dev), grad,
                                                                           torch.ones((V, 1), device=dev))[0])
            normals = torch.where((unit != 0).any(1, keepdim=True), unit, face).contiguous()
            step, origin = mesh_extract.world_frame(batch, v)
            q, viewdir = stage("color_query", lambda: ops.mesh_color_query(v, normals, step.contiguous(), origin.contiguous(),
                                                                           mesh_extract.PAD))
            raw = stage("color_forward", lambda: net(q[:, None].contiguous(), viewdir, model="fine"))
            stage("color_finish", lambda: ops.mesh_color_finish(raw.reshape(-1, 4).contiguous()))
            info = dict(lattice=list(DIMS), inside_points=total, vertices=int(V), triangles=int(t.shape[0]), iso=iso,
                        arithmetic=net.nerf_precision())
            if rep == 0:  # the warm-up pass of every shape
                stages.clear()
            del wpts, lin, alpha, cube, v, t, wv, face, grad, unit, normals, q, viewdir, raw
        rec["extraction"] = dict(info, stages={k: _stats(v) for k, v in stages.items()},
                                 total_ms=float(sum(np.mean(v) for v in stages.values())))
        print(json.dumps(rec["extraction"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
