"""Times the training-ray sampler at the bench's training shape (512 x 512 image, N_rand = 1024):
  * one `TrainRaySampler.sample` call on the device (HIP events over `--reps` calls after warm-up), and its kernels one by one
    (classification, the two scans, the sampling workgroup) from torch.profiler's device timeline,
  * the training step it feeds, measured in the same run by `bench.py --mode train` in a child process,
  * the host time of the numpy restatement (tests/train_rays_ref.py, one thread) on the same inputs: the stand-in for what the
    reference's sample_ray_h36m costs per item in a DataLoader worker,
and writes profiles/train_rays.json.  No threshold is set: what to read off is the sampler's share of the step.

    python tools/bench_train_rays.py [--reps 50] [--out profiles/train_rays.json] [--head <commit>] [--no-step]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZE, N_RAND = 512, 1024
GROUPS = (("classify", ("classify_kernel",)), ("scans", ("scan_",)), ("sample", ("sample_kernel",)))


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


def scene():
    """The bench body seen by a 512 x 512 camera, an elliptical h36m mask (1 inside, a 100 ring) and a random image."""
    from tests import synthetic as syn
    from neuralbody_amd.train_rays import bound_hull

    body = syn.make_body(seed=0)
    K, R, T = syn.make_camera(body, SIZE, SIZE)
    yy, xx = np.meshgrid(np.arange(float(SIZE)), np.arange(float(SIZE)), indexing="ij")
    r = ((yy - 0.5 * SIZE) / (0.36 * SIZE)) ** 2 + ((xx - 0.5 * SIZE) / (0.2 * SIZE)) ** 2
    msk = np.zeros((SIZE, SIZE), np.uint8)
    msk[r <= 1.0] = 100
    msk[r <= 0.9] = 1
    img = np.random.RandomState(0).uniform(0, 1, (SIZE, SIZE, 3)).astype(np.float32)
    hull = bound_hull(body["can_bounds"], K, np.concatenate([R, T], axis=1))
    return dict(img=img, msk=msk, K=K, R=R, T=T, bounds=body["can_bounds"], hull=hull, mode="h36m")


def kernel_split(fn, reps):
    """Mean device microseconds per call of each kernel group, from torch.profiler; None where the profiler gives no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {name: 0.0 for name, _ in GROUPS}
        seen = 0
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            for name, pats in GROUPS:
                if any(p in ev.key for p in pats) and t > 0:
                    out[name] += float(t) / reps
                    seen += 1
        return {k + "_us": v for k, v in out.items()} if seen else None
    except Exception as e:  # the timeline is extra: the event timing above stands without it
        return {"error": "%s: %s" % (type(e).__name__, e)}


def train_step_ms():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "train", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and "train_step_ms" in line:
            return float(json.loads(line)["value"])
    raise SystemExit("bench.py --mode train gave no result line:\n" + out.stdout[-2000:] + out.stderr[-2000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_rays.json"))
    ap.add_argument("--head", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the bench.py --mode train child run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_rays needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    step_ms = None if args.no_step else train_step_ms()  # the child has the device to itself

    from neuralbody_amd.train_rays import TrainRaySampler
    from tests import train_rays_ref as trr

    dev = torch.device("cuda:0")
    c = scene()
    img, msk = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["msk"]).to(dev)
    s = TrainRaySampler(SIZE, SIZE, N_RAND, mode=c["mode"], device=dev, seed=0)
    u = s.uniforms()

    def sample():
        return s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"], u=u, hull=c["hull"])

    def sample_with_rand():  # what the dataset does per item: the uniforms are drawn too
        return s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"], hull=c["hull"])

    t_call = event_ms(sample, args.reps, warmup=10)
    t_item = event_ms(sample_with_rand, args.reps, warmup=10)
    split = kernel_split(sample, args.reps)
    got = {k: v.cpu().numpy() for k, v in sample().items()}
    status = s.check()

    torch.set_num_threads(1)
    uh = u.cpu().numpy()
    host = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        ref = trr.sample(u=uh, body_ratio=0.5, **c)
        host.append(time.perf_counter() - t0)
    same = bool(np.array_equal(got["pixel"], ref["pixel"]) and all(
        np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)) for k in ("rgb", "ray_o", "ray_d", "near", "far")))
    rec = dict(tool="tools/bench_train_rays.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0), shape="%dx%d, N_rand %d, h36m, 4 rounds" % (SIZE, SIZE, N_RAND),
               timing="HIP events per call after 10 warm-up calls; kernels: torch.profiler device timeline; host: perf_counter, one thread",
               status=dict(zip(("n_filled", "rounds_used", "count_body", "count_bound"), status)),
               sample=t_call, sample_with_uniforms=t_item, kernels=split, train_step_ms=step_ms,
               sample_over_step=None if step_ms is None else t_item["mean_ms"] / step_ms,
               host_restatement=dict(mean_ms=1e3 * float(np.mean(host[1:])), reps=args.host_reps, threads=1),
               bitwise_equal_to_restatement=same)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
