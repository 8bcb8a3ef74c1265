"""Times hierarchical sampling on the bench scene (bench.build_scene: 512 x 512 rays, 64 samples) and writes profiles/importance.json:
one view rendered with N_importance 0, 32 and 64 in one process, each run split into the coarse march, nb_importance_sample, the
decode of the new points, nb_importance_merge and nb_composite (HIP events around every call of a stage, summed per render), beside
the whole render() call.  The N_importance = 0 render is recorded beside the same view timed on the parent commit: run the tool there
first with --plain-only (it then uses nothing the parent lacks) and hand the file over with --parent; the two means must agree within
the run-to-run spread (largest max - min over the repeats of either side), which shows that the feature costs nothing when it is off.

    python tools/bench_importance.py --plain-only --root <parent checkout> --out parent.json
    python tools/bench_importance.py --parent parent.json [--reps 10] [--out profiles/importance.json]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, N_SAMPLES, N_IMPORTANCE = 512, 64, (0, 32, 64)
STAGES = ("march", "importance_sample", "fine_decode", "importance_merge", "composite")


def _stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()), reps=int(ms.size))


class StageClock:
    """HIP events around every call of the wrapped functions; `collect()` sums them per stage after a synchronisation."""

    def __init__(self):
        self.events = []

    def wrap(self, stage, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.events.append((stage, e0, e1))
            return out

        return timed

    def collect(self):
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for stage, e0, e1 in self.events:
            out[stage] += e0.elapsed_time(e1)
        self.events = []
        return out


def time_render(call, reps, warmup, clock=None):
    """Whole-call HIP-event times of `call()` over `reps` repeats and, with a clock, the per-stage sums of every repeat."""
    for _ in range(warmup):
        call()
    if clock is not None:
        clock.collect()
    whole, stages = [], {s: [] for s in STAGES}
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        whole.append(e0.elapsed_time(e1))
        if clock is not None:
            for s, v in clock.collect().items():
                stages[s].append(v)
    rec = dict(render=_stats(whole))
    if clock is not None:
        rec["stages"] = {s: _stats(v) for s, v in stages.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=HERE, help="the checkout whose bench.py and neuralbody_amd are timed")
    ap.add_argument("--plain-only", action="store_true", help="time render() without the feature only (runs on the parent commit)")
    ap.add_argument("--parent", default=None, help="the --plain-only record of the parent commit")
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_importance needs an MI355X: a CPU run gives no timing")
    import bench
    import neuralbody_amd
    from neuralbody_amd import ops

    assert os.path.abspath(neuralbody_amd.__file__).startswith(root + os.sep), "neuralbody_amd was not imported from --root"
    dev = torch.device("cuda:0")
    sd, body, net, rend, bd, n = bench.build_scene(dev, SIZE, SIZE, N_SAMPLES)
    rec = dict(tool="tools/bench_importance.py", head=args.head, box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               rays=n, samples=N_SAMPLES, precision=net.march_precision(),
               timing="HIP events; render = one render() call of the view on the frame's feature volumes (no encoder pass); stages = "
                      "events around every call of the stage inside that render, summed")
    with torch.no_grad():
        fv = net.encode_sparse_voxels(rend.prepare_sp_input(bd))
        plain = time_render(lambda: rend.render(bd, feature_volume=fv), args.reps, warmup=3)
        if args.plain_only:
            rec["plain_render"] = plain["render"]
        else:
            clock = StageClock()
            net.render_rays = clock.wrap("march", net.render_rays)
            net.calculate_density_color = clock.wrap("fine_decode", net.calculate_density_color)
            ops.importance_sample = clock.wrap("importance_sample", ops.importance_sample)
            ops.importance_merge = clock.wrap("importance_merge", ops.importance_merge)
            ops.composite = clock.wrap("composite", ops.composite)
            runs = {}
            for N in N_IMPORTANCE:
                runs[str(N)] = time_render(lambda N=N: rend.render(bd, feature_volume=fv, n_importance=N), args.reps, warmup=2, clock=clock)
                print(N, json.dumps(runs[str(N)]))
            rec["n_importance"] = runs
            rec["plain_render_before_wrapping"] = plain["render"]
            if args.parent:
                with open(args.parent) as f:
                    parent = json.load(f)
                a, b = runs["0"]["render"], parent["plain_render"]
                spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
                rec["off_vs_parent"] = dict(this_commit=a, parent_commit=b, parent_head=parent.get("head"),
                                            difference_ms=a["mean_ms"] - b["mean_ms"], spread_ms=spread,
                                            agree=bool(abs(a["mean_ms"] - b["mean_ms"]) <= spread))
                print(json.dumps(rec["off_vs_parent"]))
    out = args.out or os.path.join(HERE, "profiles", "importance.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out)
    if not args.plain_only and args.parent and not rec["off_vs_parent"]["agree"]:
        raise SystemExit("N_importance = 0 and the parent commit differ by more than the run-to-run spread")


if __name__ == "__main__":
    main()
