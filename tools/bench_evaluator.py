"""Times the evaluator on the bench scene: per view at 512 x 512 x 64 and 1024 x 1024 x 128
  * `Evaluator.evaluate` on the device (HIP events over `--reps` calls after warm-up),
  * the host path it replaces on the same data: device-to-host copies + the numpy float64 restatement of the reference's
    evaluator (tests/metrics_ref.py), one CPU thread,
  * the render step of the same view (`Renderer.render`),
and writes profiles/eval_metrics.json.  The target is stated against the render step measured in the same run: evaluate
should cost under 5 % of it (the box-to-box spread README.md reports for the render itself).

    python tools/bench_evaluator.py [--reps 30] [--out profiles/eval_metrics.json] [--head <commit>]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET_FRACTION = 0.05
SHAPES = ((512, 64), (1024, 128))


def _head():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def event_ms(fn, reps, warmup):
    """Mean / min / max milliseconds of fn() over `reps` calls, each bracketed by HIP events on the current stream."""
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
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=reps)


def bench_shape(dev, size, n_samples, reps, host_reps):
    import bench
    from neuralbody_amd.evaluator import EvalConfig, Evaluator
    from tests import metrics_ref as mr

    sd, body, net, rend, bd, n = bench.build_scene(dev, size, size, n_samples)
    pose = bench.build_poses(dev, body, bd, size, size, n_poses=2)[bench_pose()]
    with torch.no_grad():
        out = rend.render(pose)
    # ground truth: the render itself, perturbed (seeded, made on the device)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = (out["rgb_map"] + 0.05 * torch.randn(out["rgb_map"].shape, device=dev, generator=g)).clamp_(0.0, 1.0)
    batch = dict(pose, rgb=gt, frame_index=torch.tensor([0]), cam_ind=torch.tensor([bench_pose()]))

    with tempfile.TemporaryDirectory() as tmp:
        ev = Evaluator(EvalConfig(H=size, W=size, white_bkgd=rend.cfg.white_bkgd, result_dir=tmp))

        def evaluate():
            ev.evaluate(out, batch)

        t_eval = event_ms(evaluate, reps, warmup=5)
        got = ev.summarize()

    def render():
        with torch.no_grad():
            rend.render(pose)

    t_render = event_ms(render, reps, warmup=3)

    def host():  # what lib/evaluators/if_nerf.py does per view: three device-to-host copies, then numpy
        t0 = time.perf_counter()
        p = out["rgb_map"][0].detach().cpu().numpy()
        q = batch["rgb"][0].detach().cpu().numpy()
        m = batch["mask_at_box"][0].detach().cpu().numpy().reshape(size, size)
        t1 = time.perf_counter()
        r = mr.metrics(m, p, q, rend.cfg.white_bkgd)
        return t1 - t0, time.perf_counter() - t1, r

    torch.set_num_threads(1)
    host()
    runs = [host() for _ in range(host_reps)]
    ref = runs[-1][2]
    t_host = dict(copy_ms=1e3 * float(np.mean([r[0] for r in runs])), numpy_ms=1e3 * float(np.mean([r[1] for r in runs])),
                  reps=host_reps, threads=1)
    t_host["mean_ms"] = t_host["copy_ms"] + t_host["numpy_ms"]
    frac = t_eval["mean_ms"] / t_render["mean_ms"]
    rec = dict(view="%dx%dx%d" % (size, size, n_samples), rays=n, crop=list(ref["box"]), n_windows=ref["n_windows"],
               evaluate=t_eval, render=t_render, host_path=t_host, evaluate_over_render=frac,
               host_path_over_evaluate=t_host["mean_ms"] / t_eval["mean_ms"], target_fraction=TARGET_FRACTION,
               meets_target=bool(frac < TARGET_FRACTION),
               metrics=dict(device=got, host=dict(mse=ref["mse"], psnr=ref["psnr"], ssim=ref["ssim"])),
               ssim_abs_diff=abs(got["ssim"] - ref["ssim"]))
    print(json.dumps(rec))
    return rec


def bench_pose():
    from tests.golden import scenes

    return scenes.BENCH_POSE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluator needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda:0")
    views = [bench_shape(dev, size, s, args.reps, args.host_reps) for size, s in SHAPES]
    rec = dict(tool="tools/bench_evaluator.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0), timing="HIP events per call; host path: perf_counter, one thread",
               target="evaluate < %.0f %% of the same view's render step, both measured in this run" % (100 * TARGET_FRACTION),
               meets_target=all(v["meets_target"] for v in views), views=views)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
