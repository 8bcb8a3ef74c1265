"""Times the vanilla-NeRF baseline's training step (neuralbody_amd/nerf.py, trainable=True) on an MI355X and writes
profiles/nerf_train.json:

  * one training step at 1024 rays x (64 + 128) samples, forward + backward + Adam, with the share of every launch family (HIP
    events around every call of a stage inside the step, summed per step);
  * nb_nerf_bwd_chain against the same input-gradient chain as ops.sgemm(relu_mask=, colsum=) launches on the same tap
    (nerf.input_gradients, the product path), the yardstick tools/bench_nerf.py uses for the forward; the fused kernel leaves
    the bias gradients to one ops.colsum over the d-tap, timed beside it, so both sides deliver the same quantities;
  * nb_nerf_decode_tap against nb_nerf_decode('f32') at the same points: the price of the tap;
  * the accuracy of one step on the fixture: every gradient's max |diff| / max |ref| against the float64 step at the device's
    depths (tests/nerf_train_ref.py), beside the reference's own fp32 distance recorded in tests/golden/nerf_train_step.npz;
  * with --parent-tree DIR (a checkout of the parent commit with its built library in neuralbody_amd/lib): VolumeRenderer.render
    of a 512 x 512 view with the feature off, this tree and that one as child processes alternated twice, the spread between the
    runs of one tree beside the difference of the trees.

    python tools/bench_nerf_train.py [--reps 5] [--parent-tree DIR] [--out profiles/nerf_train.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAND, N_SAMPLES, N_IMPORTANCE, SIZE = 1024, 64, 128, 512
STAGES = ("pack", "decode_tap_coarse", "decode_tap_fine", "composite", "importance_sample", "importance_merge_z",
          "composite_bwd_maps", "input_gradients_sgemm", "weight_gradients_sgemm", "head_bias_colsum", "adam")


def view_child(tree, reps):
    """Child process: VolumeRenderer.render of a 512 x 512 view under no_grad with the package of `tree`, one JSON line."""
    sys.path.insert(0, tree)
    import torch

    from neuralbody_amd import nerf

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    n = SIZE * SIZE
    o = torch.from_numpy((np.array([0.1, -0.2, -2.6]) + rs.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)).to(dev)
    d = torch.from_numpy(np.concatenate([rs.uniform(-0.35, 0.35, (n, 2)), rs.uniform(0.9, 1.3, (n, 1))], -1).astype(np.float32)).to(dev)
    batch = {"ray_o": o[None], "ray_d": d[None], "near": torch.full((1, n), 1.7, device=dev), "far": torch.full((1, n), 3.1, device=dev)}
    torch.manual_seed(0)
    net = nerf.NerfNetwork().to(dev).eval()
    r = nerf.VolumeRenderer(net, nerf.VolumeRendererConfig(N_samples=N_SAMPLES, N_importance=N_IMPORTANCE, perturb=0.0))
    ms = []
    with torch.no_grad():
        r.render(batch)
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.render(batch)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    print(json.dumps({"tree": tree, "module": os.path.dirname(nerf.__file__), "ms": ms}))


def _stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "nerf_train.json"))
    ap.add_argument("--head", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--view-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.view_child:
        return view_child(os.path.abspath(args.view_child), args.reps)
    sys.path.insert(0, HERE)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf_train needs an MI355X: a CPU run gives no timing")
    from neuralbody_amd import build as nb_build
    from neuralbody_amd import nerf, ops
    from tests import nerf_ref as ref
    from tests import nerf_train_ref as tr

    dev = torch.device("cuda:0")
    golden = dict(np.load(os.path.join(HERE, "tests", "golden", "nerf_train_step.npz")))
    sd = ref.make_state_dict(np.load(os.path.join(HERE, "tests", "golden", "nerf_baseline.npz"))["alpha_shift"])
    rec = dict(tool="tools/bench_nerf_train.py", head=args.head, sources_sha256=nb_build._digest(),
               shape="%d rays x (%d + %d) samples" % (N_RAND, N_SAMPLES, N_IMPORTANCE),
               tap_bytes_per_step=4 * (ops.NERF_TAP_COLS + ops.NERF_DTAP_COLS) * N_RAND * (2 * N_SAMPLES + N_IMPORTANCE),
               timing="HIP events; step = render under gradients + loss.backward() + Adam.step(); stages = events around every call "
                      "of the stage inside that step, summed; the rest of a step is torch glue (loss, depths, autograd bookkeeping)")

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(reps):
            e0, e1 = events()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    # ---------------------------------------------------------------- the step
    rs = np.random.RandomState(0)
    o = torch.from_numpy((np.array([0.1, -0.2, -2.6]) + rs.uniform(-0.05, 0.05, (N_RAND, 3))).astype(np.float32)).to(dev)
    d = torch.from_numpy(np.concatenate([rs.uniform(-0.35, 0.35, (N_RAND, 2)), rs.uniform(0.9, 1.3, (N_RAND, 1))], -1)
                         .astype(np.float32)).to(dev)
    batch = {"ray_o": o[None], "ray_d": d[None], "near": torch.full((1, N_RAND), 1.7, device=dev),
             "far": torch.full((1, N_RAND), 3.1, device=dev), "rgb": torch.rand((1, N_RAND, 3), device=dev),
             "mask_at_box": torch.rand((1, N_RAND), device=dev) < 0.8}
    net = nerf.NerfNetwork(trainable=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    renderer = nerf.VolumeRenderer(net, nerf.VolumeRendererConfig(N_samples=N_SAMPLES, N_importance=N_IMPORTANCE, perturb=1.0))
    log = []

    def wrap(stage, fn):
        def run(*a, **k):
            e0, e1 = events()
            e0.record()
            out = fn(*a, **k)
            e1.record()
            log.append((stage(*a, **k) if callable(stage) else stage, e0, e1))
            return out
        return run

    real = {k: getattr(ops, k) for k in ("nerf_pack", "nerf_decode_tap", "composite", "importance_sample", "importance_merge_z",
                                         "composite_bwd_maps", "sgemm", "colsum")}
    ops.nerf_pack = wrap("pack", real["nerf_pack"])
    ops.nerf_decode_tap = wrap(lambda packed, ro, rd, z, **k: "decode_tap_fine" if z.shape[1] > N_SAMPLES else "decode_tap_coarse",
                               real["nerf_decode_tap"])
    for k, stage in (("composite", "composite"), ("importance_sample", "importance_sample"), ("importance_merge_z", "importance_merge_z"),
                     ("composite_bwd_maps", "composite_bwd_maps"), ("colsum", "head_bias_colsum"),
                     ("sgemm", lambda *a, **k: "weight_gradients_sgemm" if k.get("trans_a") else "input_gradients_sgemm")):
        setattr(ops, k, wrap(stage, real[k]))
    adam = wrap("adam", opt.step)

    def step():
        ret = renderer.render(batch)
        mask = batch["mask_at_box"]
        loss = torch.mean((ret["rgb_map"][mask] - batch["rgb"][mask]) ** 2) + torch.mean((ret["rgb0"] - batch["rgb"]) ** 2)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        adam()
        return loss

    def collect():
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for stage, e0, e1 in log:
            out[stage] += e0.elapsed_time(e1)
        del log[:]
        return out

    step()
    collect()
    whole, stages, losses = [], {s: [] for s in STAGES}, []
    for _ in range(args.reps):
        e0, e1 = events()
        e0.record()
        loss = step()
        e1.record()
        torch.cuda.synchronize()
        whole.append(e0.elapsed_time(e1))
        losses.append(float(loss.detach()))
        for s, v in collect().items():
            stages[s].append(v)
    for k, fn in real.items():
        setattr(ops, k, fn)
    mean = float(np.mean(whole))
    rec["step"] = dict(step=_stats(whole), stages={s: dict(_stats(v), share=float(np.mean(v)) / mean) for s, v in stages.items()},
                       unaccounted_share=1.0 - sum(float(np.mean(v)) for v in stages.values()) / mean, losses=losses,
                       peak_memory_gb=torch.cuda.max_memory_allocated() / 1e9)
    print("step", json.dumps(rec["step"]))

    # ---------------------------------------------------------------- the chain against per-layer sgemm launches; the tap's price
    with torch.no_grad():
        S = N_SAMPLES + N_IMPORTANCE
        n_pts = N_RAND * S
        t = torch.linspace(0, 1, S, device=dev)
        z = (1.7 * (1.0 - t) + 3.1 * t)[None].expand(N_RAND, S).contiguous()
        fwd, weights = net.packed_train("fine")
        bwd = ops.nerf_pack_bwd({k: v.detach() for k, v in net.model_fine.named_parameters()})
        raw, tap = ops.nerf_decode_tap(fwd, o, d, z)
        d_raw = torch.randn((n_pts, 4), device=dev)
        dtap = torch.empty((n_pts, ops.NERF_DTAP_COLS), device=dev)
        bias = torch.zeros(ops.NERF_DTAP_COLS, device=dev)

        def fused(colsum):
            ops.nerf_bwd_chain(bwd, tap, d_raw, dtap=dtap)
            if colsum:
                ops.colsum(dtap, out=bias)  # all ten bias gradients in one launch over the contiguous d-tap

        t_fused = timed(lambda: fused(False), args.reps)
        t_fused_sums = timed(lambda: fused(True), args.reps)
        t_chain = timed(lambda: nerf.input_gradients(tap, d_raw, weights), args.reps)  # the product path: sums in the epilogues
        got, sums = nerf.input_gradients(tap, d_raw, weights)
        bias.zero_()
        fused(True)
        gap, scale = float((got - dtap).abs().max()), float(dtap.abs().max())
        rec["chain"] = dict(points=n_pts, nb_nerf_bwd_chain=_stats(t_fused), with_one_colsum=_stats(t_fused_sums),
                            sgemm_chain_11_launches=_stats(t_chain), speedup=float(np.mean(t_fused_sums) / np.mean(t_chain)),
                            max_abs_difference=gap, max_abs_gradient=scale,
                            max_abs_bias_difference=float((sums - bias).abs().max()), max_abs_bias=float(bias.abs().max()),
                            faster="nb_nerf_bwd_chain" if np.mean(t_fused_sums) < np.mean(t_chain) else "sgemm chain",
                            product_path="sgemm chain",  # nerf.input_gradients, what nerf._DecodeTrain.backward runs
                            dtap_gb=4 * ops.NERF_DTAP_COLS * n_pts / 1e9, tap_gb=4 * ops.NERF_TAP_COLS * n_pts / 1e9,
                            chain_traffic_gb_per_s=4 * (ops.NERF_DTAP_COLS + 2304) * n_pts / (np.mean(t_fused) * 1e-3) / 1e9)
        print("chain", json.dumps(rec["chain"]))
        plain = timed(lambda: ops.nerf_decode(fwd, o, d, z, "f32"), args.reps)
        tapped = timed(lambda: ops.nerf_decode_tap(fwd, o, d, z, out=raw, tap=tap), args.reps)
        rec["tap"] = dict(points=n_pts, nb_nerf_decode_f32=_stats(plain), nb_nerf_decode_tap=_stats(tapped),
                          ratio=float(np.mean(tapped) / np.mean(plain)),
                          tap_store_gb_per_s=4 * ops.NERF_TAP_COLS * n_pts / (np.mean(tapped) * 1e-3) / 1e9)
        print("tap", json.dumps(rec["tap"]))

    # ---------------------------------------------------------------- accuracy of one step on the fixture
    fo, fd, near, far = ref.fixture_rays()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.zero_grad(set_to_none=True)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    fbatch = {"ray_o": td(fo)[None], "ray_d": td(fd)[None], "near": td(near)[None], "far": td(far)[None]}
    ret = renderer.render(fbatch, t_rand=td(golden["t_rand"])[None], u=td(golden["u"])[None])
    mask, rgb = td(golden["mask_at_box"])[None], td(golden["rgb"])[None]
    loss = torch.mean((ret["rgb_map"][mask] - rgb[mask]) ** 2) + torch.mean((ret["rgb0"] - rgb) ** 2)
    loss.backward()
    z_coarse = tr.jitter_f32(ref.coarse_depths_f32(near, far, N_SAMPLES), golden["t_rand"])
    want = tr.train_step(sd, fo, fd, z_coarse, ret["z_vals"][0].detach().cpu().numpy(), golden["rgb"], golden["mask_at_box"])
    errs = {k: tr.rel_err(p.grad.cpu().numpy(), want["grads"][k]) for k, p in net.named_parameters()}
    worst = max(errs, key=errs.get)
    rec["accuracy"] = dict(measure="max |gradient - float64| / max |float64| per tensor, 48 tensors, one step on the 96 fixture rays",
                           budget=tr.GRAD_TOL, device_worst=errs[worst], device_worst_tensor=worst,
                           reference_fp32_worst=float(golden["ref_err_worst"]), loss=float(loss.detach()),
                           loss_float64_at_device_depths=want["loss"], loss_reference=float(golden["loss"]))
    print("accuracy", json.dumps(rec["accuracy"]))

    # ---------------------------------------------------------------- the inference view against the parent commit
    if args.parent_tree:
        runs = {"this": [], "parent": []}
        for _ in range(2):
            for name, tree in (("this", HERE), ("parent", os.path.abspath(args.parent_tree))):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--view-child", tree, "--reps", str(args.reps)],
                                     check=True, timeout=300, stdout=subprocess.PIPE, cwd=tree).stdout.decode()
                child = json.loads(out.strip().splitlines()[-1])
                assert child["module"].startswith(tree), child
                runs[name].append(float(np.mean(child["ms"])))
        spread = max(abs(v[0] - v[1]) / min(v) for v in runs.values())
        diff = (np.mean(runs["this"]) - np.mean(runs["parent"])) / np.mean(runs["parent"])
        rec["view_512_feature_off"] = dict(runs_ms=runs, spread_between_runs_of_one_tree=float(spread),
                                           this_over_parent_minus_1=float(diff),
                                           note="child processes alternated twice (this, parent, this, parent), %d renders each after one "
                                                "warm-up; precision 'auto', 64 + 128 samples, no gradients" % args.reps)
        print("view", json.dumps(rec["view_512_feature_off"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
