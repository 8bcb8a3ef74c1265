"""Measures ray bounds from the posed body (neuralbody_amd/ray_bounds.py, csrc/nb_ray_bounds.hip, nb_body_depth_range) on the scene
and the synthetic SMPL-sized model of tools/bench_pose_cull.py at 512 x 512, and writes profiles/ray_bounds.json.  No threshold is
set here; DESIGN.md §4.19 holds the tables.
  (a) under HIP events, 5 warm-up calls and 10 repeats per leg, the legs alternating: nb_raygen, and the three stages
      nb_body_depth_range, nb_depth_range_widen and nb_raygen_body (tile 8),
  (b) rays kept over box rays and the mean of (far' - near') / (far - near) over the kept rays, for tile 1 and tile 8,
  (c) Renderer.render of the view's batch and the nb_march inside it (its own events; nanoseconds per sample = march time over
      rays x N_samples), for the box and for body bounds with tile 1 and tile 8, at N_samples 64 and 32, the legs alternating,
  (d) with --parent-root DIR (a built checkout of the parent commit): the feature-off view, NovelViewRenderer.render_view without
      body_bounds, as child processes of this tree and of the parent's alternating.

    python tools/bench_ray_bounds.py [--out profiles/ray_bounds.json] [--parent-root DIR] [--rounds 2]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --child ROOT: this file run against the package, tools and tests of another checkout (the parent commit's)
ROOT = os.path.abspath(sys.argv[sys.argv.index("--child") + 1]) if "--child" in sys.argv else HERE
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_mesh import _head  # noqa: E402
from tools.bench_pose_cull import DEV, IMG, body, camera  # noqa: E402

WARMUP, REPS = 5, 10
MARGIN = 0.05


def alternating_ms(legs, reps=REPS, warmup=WARMUP, march=False):
    """legs: {name: fn}.  Every repeat runs each leg once, in order, between two HIP events -> {name: dict(mean_ms, min_ms, max_ms,
    std_ms, reps)}; with `march` also {name: the same of the nb_march launches inside the call}."""
    from neuralbody_amd import ops

    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in legs}
    inner = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if march:
                ops.MARCH_EVENTS = []
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
            if march:
                inner[k].append(ops.MARCH_EVENTS)
                ops.MARCH_EVENTS = None
    torch.cuda.synchronize()

    def stats(ms):
        ms = np.array(ms)
        return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()), reps=len(ms))

    out = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in evs.items()}
    if not march:
        return out
    return out, {k: stats([sum(a.elapsed_time(b) for a, b in call) for call in v]) for k, v in inner.items()}


def scene():
    """The first frame of tools/bench_pose_cull.py's body, its camera, and the eval-mode network of that tool."""
    from tests import helpers as H
    from tests import synthetic as syn

    drv, stacked, V, Nf = body()
    one = [s[:1] for s in stacked]
    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, False, H.DEFAULT_PRECISION)
    return drv, one, V, Nf, net


def child():
    """Feature-off: render_view of the box's rays, HIP events around the call -> one JSON line."""
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer

    drv, one, _, _, net = scene()
    (frame, can_bounds), = drv.frames(*one, 0, True)
    K, RT = camera(can_bounds, 0.35)
    nv = NovelViewRenderer(Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=IMG, W=IMG)), IMG, IMG, DEV)
    n = nv.render_view(K, RT, can_bounds, frame)["n_rays"]
    t = alternating_ms({"render_view": lambda: nv.render_view(K, RT, can_bounds, frame)})["render_view"]
    print(json.dumps(dict(n_rays=int(n), **t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ray_bounds.json"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--head", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child()
    from neuralbody_amd import ops
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.ray_bounds import BodyBounds
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from neuralbody_amd.smpl_pose import cull_border
    from tests import helpers as H

    drv, one, V, Nf, net = scene()
    (frame, can_bounds), = drv.frames(*one, 0, True, body=True)
    verts, faces = frame["body_verts"], frame["body_faces"]
    K, RT = camera(can_bounds, 0.35)
    border = cull_border(can_bounds, K[None], RT[None], MARGIN)
    K32 = torch.from_numpy(K.astype(np.float32)).to(DEV)[None]
    RT32 = torch.from_numpy(RT.astype(np.float32)).to(DEV)[None]

    # (a)
    raw = ops.body_depth_range(verts, faces, RT32, K32, IMG, IMG)
    scratch = ops.body_depth_range_scratch(1, V, Nf, 1, DEV)
    wide = ops.depth_range_widen(raw[0, 0], border, 8)
    out_w = torch.empty_like(wide)
    stages = alternating_ms({
        "nb_raygen": lambda: ops.raygen(IMG, IMG, K, RT[:, :3], RT[:, 3], can_bounds, DEV),
        "nb_body_depth_range": lambda: ops.body_depth_range(verts, faces, RT32, K32, IMG, IMG, out=raw, scratch=scratch),
        "nb_depth_range_widen": lambda: ops.depth_range_widen(raw[0, 0], border, 8, out=out_w),
        "nb_raygen_body": lambda: ops.raygen_body(IMG, IMG, K, RT[:, :3], RT[:, 3], can_bounds, wide, MARGIN)})

    # (b), and the batches of (c)
    plain = {k: v for k, v in frame.items() if k not in NovelViewRenderer.BODY_KEYS}
    renderers = {N: Renderer(net, RenderConfig(N_samples=N, perturb=0.0, H=IMG, W=IMG)) for N in (64, 32)}
    batches = {"box": NovelViewRenderer(renderers[64], IMG, IMG, DEV).view_batch(K, RT, can_bounds, plain)}
    for tile in (1, 8):
        nv = NovelViewRenderer(renderers[64], IMG, IMG, DEV, body_bounds=BodyBounds(MARGIN, tile))
        batches["body tile %d" % tile] = nv.view_batch(K, RT, can_bounds, frame)
    box = batches["box"]
    pos = torch.cumsum(box["mask_at_box"][0].long(), 0) - 1  # pixel -> its ray among the box's
    rays = {}
    for name, b in batches.items():
        kept = pos[b["mask_at_box"][0].bool()]
        ratio = (b["far"][0] - b["near"][0]) / (box["far"][0, kept] - box["near"][0, kept])
        rays[name] = dict(n_rays=int(b["ray_o"].shape[1]), kept_over_box=float(b["ray_o"].shape[1]) / float(box["ray_o"].shape[1]),
                          mean_interval_over_box=float(ratio.mean()))

    # (c)
    render = {}
    for N, rend in renderers.items():
        with torch.no_grad():
            call, march = alternating_ms({name: (lambda b=b: rend.render(b)) for name, b in batches.items()}, march=True)
        for name in batches:
            n = rays[name]["n_rays"]
            render["N_samples %d, %s" % (N, name)] = dict(render=call[name], march=march[name], n_rays=n,
                                                           march_ns_per_sample=march[name]["mean_ms"] * 1e6 / (n * N))

    # (d)
    off = None
    if a.parent_root:
        roots = {"parent": os.path.abspath(a.parent_root), "this": HERE}
        runs = {k: [] for k in roots}
        for _ in range(a.rounds):
            for k, root in roots.items():
                line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", root], cwd=root).decode().strip().splitlines()[-1]
                runs[k].append(json.loads(line))
        off = {k: dict(mean_ms=float(np.mean([r["mean_ms"] for r in v])), runs=v) for k, v in runs.items()}
        off["spread_ms"] = max(max(r["mean_ms"] for r in v) - min(r["mean_ms"] for r in v) for v in runs.values())

    res = {"tool": "tools/bench_ray_bounds.py", "head": a.head or _head(), "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around each call, %d warm-up calls and %d repeats per leg, the legs of a table alternating; march: the "
                     "events around nb_march inside the same calls" % (WARMUP, REPS),
           "mesh": dict(vertices=V, triangles=Nf), "image": [IMG, IMG], "margin_m": MARGIN, "border_px": int(border),
           "precision": str(H.DEFAULT_PRECISION), "stages": stages, "rays": rays, "render": render, "feature_off_view": off}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, t in stages.items():
        print("%-22s %.4f ms (min %.4f, max %.4f)" % (k, t["mean_ms"], t["min_ms"], t["max_ms"]))
    for k, r in rays.items():
        print("%-12s %6d rays (%.3f of the box's), mean interval %.3f of the box's" % (k, r["n_rays"], r["kept_over_box"], r["mean_interval_over_box"]))
    for k, r in render.items():
        print("%-28s render %.3f ms, march %.3f ms, %.2f ns / sample" % (k, r["render"]["mean_ms"], r["march"]["mean_ms"], r["march_ns_per_sample"]))
    if off:
        print("feature off: parent %.3f ms, this %.3f ms (spread between runs %.3f ms)" % (off["parent"]["mean_ms"], off["this"]["mean_ms"], off["spread_ms"]))


if __name__ == "__main__":
    main()
