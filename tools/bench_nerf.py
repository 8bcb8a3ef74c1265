"""Times the vanilla-NeRF baseline (neuralbody_amd/nerf.py) on an MI355X and writes profiles/nerf_baseline.json:

  * one 512 x 512 view through VolumeRenderer at 64 + 128 samples and at 64 + 0, per arithmetic that is built, with the share of every
    launch (HIP events around every call of a stage inside render(), summed per view);
  * the same MLP on 2^20 points as nb_nerf_decode and as the chain the package offered before it: one ops.sgemm per layer with torch
    element-wise steps (embedding, bias, relu, concatenations) — the yardstick the fused kernel has to beat;
  * the fused kernel's fraction of its MFMA peak at the nominal 2.4 GHz, counting the 593 408 multiply-adds of one evaluation and
    none of the padding: 'f32' against the fp32 MFMA (64 flop per clock per SIMD, 4 SIMDs per CU), 'f16x3' against the fp16 MFMA
    (16 x that) with the three products it executes per multiply-add;
  * the accuracy the GPU tests measure on the fixture: the device's gap to the float64 model beside the reference's own (e_ref).

    python tools/bench_nerf.py [--reps 3] [--out profiles/nerf_baseline.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SIZE, N_SAMPLES, N_IMPORTANCE, CHAIN_POINTS = 512, 64, 128, 1 << 20
MACS = 63 * 256 + 4 * 256 ** 2 + 319 * 256 + 2 * 256 ** 2 + 256 ** 2 + 256 + 283 * 128 + 128 * 3
STAGES = ("decode_coarse", "decode_fine", "composite", "importance_sample", "importance_merge_z")
CLOCK_HZ = 2.4e9


def _stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def _timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


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
            self.events.append((stage(*a, **k) if callable(stage) else stage, e0, e1))
            return out

        return timed

    def collect(self):
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for stage, e0, e1 in self.events:
            out[stage] += e0.elapsed_time(e1)
        self.events = []
        return out


def embed(x, n_freq):
    return torch.cat([x] + [f(x * 2.0 ** k) for k in range(n_freq) for f in (torch.sin, torch.cos)], -1)


def chain(mod, pts, viewdirs, ops):
    """Nerf.forward (lib/networks/nerf.py:45-65) as per-layer ops.sgemm launches with torch element-wise steps."""
    e_p, e_v = embed(pts, 10), embed(viewdirs, 4)
    h = e_p
    for i, lin in enumerate(mod.pts_linears):
        h = torch.relu_(ops.sgemm(h, lin.weight, trans_b=True).add_(lin.bias))
        if i == 4:
            h = torch.cat([e_p, h], -1)
    alpha = ops.sgemm(h, mod.alpha_linear.weight, trans_b=True).add_(mod.alpha_linear.bias)
    feature = ops.sgemm(h, mod.feature_linear.weight, trans_b=True).add_(mod.feature_linear.bias)
    h = torch.cat([feature, e_v], -1)
    h = torch.relu_(ops.sgemm(h, mod.views_linears[0].weight, trans_b=True).add_(mod.views_linears[0].bias))
    rgb = ops.sgemm(h, mod.rgb_linear.weight, trans_b=True).add_(mod.rgb_linear.bias)
    return torch.cat([rgb, alpha], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "nerf_baseline.json"))
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf needs an MI355X: a CPU run gives no timing")
    from neuralbody_amd import nerf, ops
    from tests import nerf_ref as ref  # the fixture's weight recipe and the float64 model: the tool measures what the tests check

    dev = torch.device("cuda:0")
    fx = dict(np.load(os.path.join(HERE, "tests", "golden", "nerf_baseline.npz")))
    sd = ref.make_state_dict(fx["alpha_shift"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = cus * 4 * 64 * CLOCK_HZ  # fp32 MFMA: 64 flop per clock per SIMD
    from neuralbody_amd import build as nb_build

    # which tree: the digest build.py stamps the library with (every .hip / .h source and the flags); --head adds a commit name
    rec = dict(tool="tools/bench_nerf.py", head=args.head, sources_sha256=nb_build._digest(), compute_units=cus,
               fp32_mfma_peak_tflops=peak / 1e12, fp16_mfma_peak_tflops=16 * peak / 1e12, macs_per_point=MACS,
               auto=nerf.AUTO_ARITHMETIC,
               timing="HIP events; view = one VolumeRenderer.render() of %d x %d rays in chunks of 32768; stages = events around every "
                      "call of the stage inside that render, summed; the rest of a view is torch glue (depths, concatenation)" % (SIZE, SIZE))

    # rays of a view: the fixture's camera, a ray per pixel
    rs = np.random.RandomState(0)
    n = SIZE * SIZE
    o = torch.from_numpy((np.array([0.1, -0.2, -2.6]) + rs.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)).to(dev)
    d = torch.from_numpy(np.concatenate([rs.uniform(-0.35, 0.35, (n, 2)), rs.uniform(0.9, 1.3, (n, 1))], -1).astype(np.float32)).to(dev)
    near = torch.full((n,), 1.7, device=dev)
    far = torch.full((n,), 3.1, device=dev)
    batch = {"ray_o": o[None], "ray_d": d[None], "near": near[None], "far": far[None]}

    clock = StageClock()
    real_decode = ops.nerf_decode
    ops.composite = clock.wrap("composite", ops.composite)
    ops.importance_sample = clock.wrap("importance_sample", ops.importance_sample)
    ops.importance_merge_z = clock.wrap("importance_merge_z", ops.importance_merge_z)
    rec["views"] = {}
    with torch.no_grad():
        for prec in sorted(ops.NERF_PRECISIONS):
            pipe = peak if prec == "f32" else 16 * peak / 3.0  # useful flop per second at a full matrix pipe (f16x3: three products)
            net = nerf.NerfNetwork(precision=prec)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            net = net.to(dev).eval()
            fine_blob = net.packed("fine")
            ops.nerf_decode = clock.wrap(lambda packed, *a, **k: "decode_fine" if packed is fine_blob else "decode_coarse", real_decode)
            for N in (N_IMPORTANCE, 0):
                r = nerf.VolumeRenderer(net, nerf.VolumeRendererConfig(N_samples=N_SAMPLES, N_importance=N, perturb=0.0))
                r.render(batch)
                clock.collect()
                whole, stages = [], {s: [] for s in STAGES}
                for _ in range(args.reps):
                    whole += _timed(lambda: r.render(batch), 1, warmup=0)
                    for s, v in clock.collect().items():
                        stages[s].append(v)
                pts = n * (N_SAMPLES + (N_SAMPLES + N if N else 0))
                dec = np.mean(stages["decode_coarse"]) + np.mean(stages["decode_fine"])
                rec["views"]["%s_%d+%d" % (prec, N_SAMPLES, N)] = dict(
                    view=_stats(whole), stages={s: _stats(v) for s, v in stages.items()}, points_decoded=pts,
                    decode_tflops=2.0 * MACS * pts / (dec * 1e-3) / 1e12, decode_fraction_of_peak=2.0 * MACS * pts / (dec * 1e-3) / pipe)
                print(prec, N, json.dumps(rec["views"]["%s_%d+%d" % (prec, N_SAMPLES, N)]))
            ops.nerf_decode = real_decode

            # the yardstick: the same module on the same 2^20 points, fused and as a chain of sgemm launches
            m = CHAIN_POINTS // N_SAMPLES
            z = (near[:m, None] * (1.0 - torch.linspace(0, 1, N_SAMPLES, device=dev)) + far[:m, None] * torch.linspace(0, 1, N_SAMPLES, device=dev))
            z = z.contiguous()
            pts3 = (o[:m, None, :] + d[:m, None, :] * z[..., None]).reshape(-1, 3).contiguous()
            vd = (d[:m] / d[:m].norm(dim=-1, keepdim=True))[:, None, :].expand(m, N_SAMPLES, 3).reshape(-1, 3).contiguous()
            fused = _timed(lambda: net.decode(o[:m].contiguous(), d[:m].contiguous(), z), args.reps)
            chained = _timed(lambda: chain(net.model, pts3, vd, ops), args.reps)
            gap = float((chain(net.model, pts3, vd, ops).view(m, N_SAMPLES, 4) - net.decode(o[:m].contiguous(), d[:m].contiguous(), z)).abs().max())
            rec["chain_%s" % prec] = dict(points=CHAIN_POINTS, fused=_stats(fused), sgemm_chain=_stats(chained),
                                          speedup=float(np.mean(chained) / np.mean(fused)), max_abs_difference=gap,
                                          fused_fraction_of_peak=2.0 * MACS * CHAIN_POINTS / (np.mean(fused) * 1e-3) / pipe)
            print(prec, json.dumps(rec["chain_%s" % prec]))
            if np.mean(fused) >= np.mean(chained):
                raise SystemExit("the fused kernel does not beat the per-layer chain")

        # accuracy on the fixture: raw against the float64 model at the fixture's depths (tests/test_gpu_nerf.py holds 'f32' to 8 x e_ref)
        fo, fd = torch.from_numpy(fx["ray_o"]).to(dev), torch.from_numpy(fx["ray_d"]).to(dev)
        cases = (("model", "", fx["z_coarse"], fx["raw_coarse"]), ("model_fine", "fine", fx["z_fine"], fx["raw_fine"]))
        want64 = {m: ref.forward(sd, m, ref.points_f32(fx["ray_o"], fx["ray_d"], z), ref.viewdirs_device(fx["ray_d"])) for m, _, z, _ in cases}
        e_ref = max(float(np.abs(ref.forward(sd, m, ref.points_f32(fx["ray_o"], fx["ray_d"], z), fx["viewdirs"]) - want).max())
                    for m, _, z, want in cases)
        rec["accuracy"] = dict(e_ref=e_ref, note="max |raw - float64 model| at the fixture's coarse and fine depths; e_ref: the "
                                                 "reference's own fp32 forward; 'f32' is allowed 8 x e_ref")
        for prec in sorted(ops.NERF_PRECISIONS):
            net = nerf.NerfNetwork(precision=prec)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            net = net.to(dev).eval()
            rec["accuracy"]["device_gap_" + prec] = max(
                float(np.abs(want64[m] - net.decode(fo, fd, torch.from_numpy(z).to(dev), model=model).cpu().numpy()).max())
                for m, model, z, _ in cases)
        print(json.dumps(rec["accuracy"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
