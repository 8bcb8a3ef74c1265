"""Times the training step with the mask and distortion losses on the scene of `bench.py --mode train` (1024 rays x 64 samples) and
writes profiles/train_losses.json.  HIP events, 5 warm-ups, the legs alternated inside one call:

  step      the default step (rgb loss alone) / with the mask loss on acc_map / with the mask and the distortion loss
  kernels   nb_composite_bwd against nb_composite_bwd_maps with all five cotangents (1024 x 64); nb_ray_distortion at 1024 x 64 and at
            262 144 x 64, with and without its gradient
  parent    `python bench.py --mode train` of this checkout and of the parent commit's checkout (--parent-root), alternated as
            child processes BEFORE this process opens the device: both numbers and the run-to-run spread

    python tools/bench_train_losses.py [--parent-root <parent checkout, built>] [--reps 20] [--out profiles/train_losses.json]
"""
import argparse
import json
import os
import socket
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, N_SAMPLES, N_RAYS, WARMUP = 512, 64, 1024, 5
MU, LAMBDA = 1.0, 0.01


def _stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()), reps=int(ms.size))


def bench_train_child(root, steps):
    """train_step_ms of one `bench.py --mode train` child process in `root`."""
    out = subprocess.run([sys.executable, "bench.py", "--mode", "train", "--gpus", "1", "--steps", str(steps), "--warmup", str(WARMUP)],
                         cwd=root, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
    for line in reversed(out.strip().splitlines()):
        if line.startswith("{"):
            rec = json.loads(line)
            assert rec["metric"] == "train_step_ms", rec["metric"]
            return float(rec["value"])
    raise RuntimeError("no JSON line from bench.py in %s" % root)


def alternate(legs, reps):
    """legs: {name: call}; 5 warm-ups of each, then `reps` rounds of every leg in turn, one HIP-event pair per call."""
    import torch

    for _ in range(WARMUP):
        for call in legs.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, call in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: _stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent-runs", type=int, default=3)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "train_losses.json"))
    args = ap.parse_args()
    rec = dict(tool="tools/bench_train_losses.py", head=args.head, box=socket.gethostname(), rays=N_RAYS, samples=N_SAMPLES,
               mask_loss_weight=MU, distortion_loss_weight=LAMBDA,
               timing="HIP events around one call, %d warm-ups, legs alternated; parent: host clock of bench.py --mode train" % WARMUP)
    if args.parent_root:
        runs = {"this_commit": [], "parent_commit": []}
        for _ in range(args.parent_runs):
            runs["parent_commit"].append(bench_train_child(os.path.abspath(args.parent_root), args.reps))
            runs["this_commit"].append(bench_train_child(HERE, args.reps))
        spread = max(max(v) - min(v) for v in runs.values())
        rec["default_step_vs_parent"] = dict(
            command="python bench.py --mode train --gpus 1 --steps %d --warmup %d" % (args.reps, WARMUP), train_step_ms=runs,
            this_commit_mean_ms=float(np.mean(runs["this_commit"])), parent_commit_mean_ms=float(np.mean(runs["parent_commit"])),
            difference_ms=float(np.mean(runs["this_commit"]) - np.mean(runs["parent_commit"])), spread_ms=float(spread))
        print(json.dumps(rec["default_step_vs_parent"]))
    else:
        rec["default_step_vs_parent"] = "not measured"

    sys.path.insert(0, HERE)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_train_losses needs an MI355X: a CPU run gives no timing")
    import bench
    from neuralbody_amd import ops

    dev = torch.device("cuda:0")
    rec["device"] = torch.cuda.get_device_name(0)
    sd, body, net, rend, bd, n_rays = bench.build_scene(dev, SIZE, SIZE, N_SAMPLES, "f32")
    rend.cfg.perturb = 1.0
    g = torch.Generator(device="cpu").manual_seed(0)
    pick = torch.randperm(n_rays, generator=g)[:N_RAYS].to(dev)
    tb = dict(bd)
    for k in ("ray_o", "ray_d", "near", "far"):
        tb[k] = bd[k][:, pick].contiguous()
    tb["mask_at_box"] = torch.ones((1, N_RAYS), dtype=torch.bool, device=dev)
    target = torch.rand((1, N_RAYS, 3), generator=g).to(dev)
    occupancy = (torch.rand((1, N_RAYS), generator=g) < 0.5).float().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)

    def step(mask_loss, distortion_loss):
        out = rend.render(tb)
        loss = torch.mean((out["rgb_map"] - target) ** 2)
        if mask_loss:
            loss = loss + MU * torch.nn.functional.smooth_l1_loss(out["acc_map"], occupancy)
        if distortion_loss:
            loss = loss + LAMBDA * torch.mean(ops.ray_distortion(out["weights"][0], out["z_vals"][0].contiguous()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(net.parameters(), 40)
        opt.step()

    rec["step"] = alternate({"default": lambda: step(False, False), "mask": lambda: step(True, False),
                             "mask_and_distortion": lambda: step(True, True)}, args.reps)
    print(json.dumps(rec["step"]))

    def rays(n):
        gg = torch.Generator(device=dev).manual_seed(n)
        r = lambda *s: torch.randn(s, device=dev, generator=gg)  # noqa: E731
        z = torch.sort(torch.rand((n, N_SAMPLES), device=dev, generator=gg) * 2 + 1, dim=1)[0].contiguous()
        return dict(raw=r(n, N_SAMPLES, 4) * 2, z=z, d=r(n, 3), g_rgb=r(n, 3), g_acc=r(n), g_depth=r(n), g_disp=r(n), g_w=r(n, N_SAMPLES))

    c = rays(N_RAYS)
    big = rays(262144)
    w_small = ops.composite(c["raw"], c["z"], c["d"], False)[3]
    w_big = ops.composite(big["raw"], big["z"], big["d"], False)[3]
    rec["kernels"] = alternate({
        "composite_bwd_1024x64": lambda: ops.composite_bwd(c["raw"], c["z"], c["d"], c["g_rgb"], False, c["g_acc"], c["g_depth"]),
        "composite_bwd_maps_five_cotangents_1024x64": lambda: ops.composite_bwd_maps(
            c["raw"], c["z"], c["d"], False, c["g_rgb"], c["g_acc"], c["g_depth"], c["g_disp"], c["g_w"]),
        "ray_distortion_1024x64": lambda: ops.ray_distortion_raw(w_small, c["z"]),
        "ray_distortion_loss_only_1024x64": lambda: ops.ray_distortion_raw(w_small, c["z"], want_grad=False),
        "ray_distortion_262144x64": lambda: ops.ray_distortion_raw(w_big, big["z"]),
        "ray_distortion_loss_only_262144x64": lambda: ops.ray_distortion_raw(w_big, big["z"], want_grad=False)}, args.reps)
    rec["kernels"]["note"] = "each call includes its output allocation (torch.empty) in front of the launch"
    print(json.dumps(rec["kernels"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
