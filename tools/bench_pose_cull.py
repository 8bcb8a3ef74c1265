"""Times the silhouette cull of pose-driven frames (csrc/nb_silhouette.hip, neuralbody_amd/smpl_pose.py) on a synthetic closed
mesh with SMPL's counts (6890 vertices, 13776 triangles: a slim latitude-longitude ellipsoid, 84 rings of 82 and two poles, lying along the diagonal of
its box) skinned by
the seeded synthetic model of tests/smpl_ref.py:
  (a) under HIP events, per call after 3 warm-up calls: nb_smpl_silhouette for 4 views at 512 x 512 (F = 1 and F = 16 frames per
      call) and the one nb_mask_dilate of a frame at the border PoseDriver.frames computes for the default 0.05 m margin,
  (b) the 16-frame 512 x 512 NovelViewRenderer.render_views loop fed by PoseDriver.views, through Renderer (every sample marched)
      and through RendererMmsk with cull_cameras (silhouettes and dilation inside the loop), alternating in one process on one
      box, wall clock around a synchronised loop,
  (c) the share of the march's samples that survive the cull, counted with the cull's own arithmetic in torch (not a timed path),
and writes profiles/pose_cull.json.  The condition: loop (b) with culling is faster per frame than without, by more than the
run-to-run spread (max - min over the calls) of the unculled loop in this process; no speed-up is claimed when it is false.

    python tools/bench_pose_cull.py [--reps 30] [--out profiles/pose_cull.json]
"""
import argparse
import json
import math
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import _head, event_ms  # noqa: E402

DEV = "cuda:0"
IMG = 512
LOOP_FRAMES = 16
N_CULL = 4
BOX = (0.3, 0.5, 0.2)  # of the synthetic model whose shape and pose bases move the mesh


def closed_mesh(rings=84, segments=82, radii=(0.05, 0.27, 0.045), tilt=0.47):
    """-> (verts [2 + rings * segments, 3] float32, faces [2 * segments * rings, 3] int64) of a closed ellipsoid: slim, and
    tilted by `tilt` rad about z so that it lies along the diagonal of its 0.26 x 0.49 x 0.09 m box and fills about a tenth of the
    padded box nb_raygen marches, roughly what a standing body fills of its own."""
    th = np.pi * (np.arange(rings) + 1.0) / (rings + 1.0)
    ph = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(segments)), np.outer(np.sin(th), np.sin(ph))], -1)
    verts = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]]) * np.array(radii)
    idx = lambda r, s: 1 + r * segments + s % segments  # noqa: E731
    south = 1 + rings * segments
    faces = [(0, idx(0, s + 1), idx(0, s)) for s in range(segments)]
    for r in range(rings - 1):
        for s in range(segments):
            faces += [(idx(r, s), idx(r, s + 1), idx(r + 1, s)), (idx(r, s + 1), idx(r + 1, s + 1), idx(r + 1, s))]
    faces += [(south, idx(rings - 1, s), idx(rings - 1, s + 1)) for s in range(segments)]
    rot = np.array([[math.cos(tilt), -math.sin(tilt), 0.0], [math.sin(tilt), math.cos(tilt), 0.0], [0.0, 0.0, 1.0]])
    return (verts @ rot.T).astype(np.float32), np.array(faces, np.int64)


def body():
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel
    from tests import smpl_ref as sr

    verts, faces = closed_mesh()
    arrays = sr.synthetic_smpl(21, len(verts), sr.SMPL_PARENTS, box=BOX)
    arrays["v_template"], arrays["f"] = verts, faces
    # the synthetic model moves every vertex on its own (random skinning weights, white-noise bases), which crumples a surface into
    # triangles tens of pixels wide; SMPL's weights and bases are smooth.  Here: each vertex follows the two joints next to its
    # place along the body (a partition of unity), and the bases are scaled to sub-pixel noise
    place = (verts[:, 1] - verts[:, 1].min()) / np.ptp(verts[:, 1]) * (sr.N_JOINTS - 1)
    j0 = np.minimum(place.astype(np.int64), sr.N_JOINTS - 2)
    w = np.zeros((len(verts), sr.N_JOINTS), np.float64)
    w[np.arange(len(verts)), j0], w[np.arange(len(verts)), j0 + 1] = 1.0 - (place - j0), place - j0
    arrays["weights"] = w.astype(np.float32)
    arrays["shapedirs"] = (0.02 * arrays["shapedirs"]).astype(np.float32)
    arrays["posedirs"] = (0.02 * arrays["posedirs"]).astype(np.float32)
    drv = PoseDriver(SmplModel.from_arrays(arrays, DEV))
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(LOOP_FRAMES)]
    # every frame keeps the first one's Rh and Th: the subject stays inside one rig of cull cameras, as on a light stage
    return drv, [np.stack([p[k] if k < 2 else P[0][k] for p in P]) for k in range(4)], len(verts), len(faces)


def camera(can_bounds, yaw):
    from tests import synthetic as syn

    K, R, T = syn.make_camera({"can_bounds": can_bounds}, IMG, IMG, focal_factor=2.5, distance=1.5, yaw=yaw)
    return K, np.concatenate([R, T.reshape(3, 1)], axis=1)


def wall_series(fns, reps, warmup):
    """The calls of `fns` alternating, each timed around a synchronised call -> one list of milliseconds per function."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms, per=1):
    a = np.array(ms) / per
    return dict(mean_ms=float(a.mean()), min_ms=float(a.min()), max_ms=float(a.max()), std_ms=float(a.std()), reps=len(ms))


def surviving_share(batch, n_samples):
    """Samples of the batch's rays (the march's z values without jitter) that project onto a set pixel of every mask, in the
    cull's fp32 operation order."""
    ro, rd, near, far = batch["ray_o"][0], batch["ray_d"][0], batch["near"][0], batch["far"][0]
    t = torch.linspace(0.0, 1.0, n_samples, device=ro.device)
    z = near[:, None] * (1.0 - t) + far[:, None] * t
    p = ro[:, None, :] + rd[:, None, :] * z[..., None]
    msks, Ks, RTs = batch["msks"][0], batch["Ks"][0], batch["RT"][0]
    keep = torch.ones(p.shape[:2], dtype=torch.bool, device=p.device)
    for v in range(msks.shape[0]):
        c = ((p[..., 0] * RTs[v, :, 0, None, None] + p[..., 1] * RTs[v, :, 1, None, None]) + p[..., 2] * RTs[v, :, 2, None, None]) \
            + RTs[v, :, 3, None, None]
        q = (c[0] * Ks[v, :, 0, None, None] + c[1] * Ks[v, :, 1, None, None]) + c[2] * Ks[v, :, 2, None, None]
        x = (q[0] / q[2]).round().long().clamp(0, msks.shape[2] - 1)
        y = (q[1] / q[2]).round().long().clamp(0, msks.shape[1] - 1)
        keep &= msks[v][y, x] != 0
    return float(keep.float().mean()), int(keep.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cull.json"))
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    from neuralbody_amd import ops
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer, RendererMmsk
    from neuralbody_amd.smpl_pose import cull_border
    from tests import helpers as H
    from tests import synthetic as syn

    drv, stacked, V, Nf = body()
    probe = drv.frames(*stacked, 0, True)
    cull_cams = [camera(probe[0][1], 0.35 + 2.0 * math.pi * k / N_CULL) for k in range(N_CULL)]
    cull = (np.stack([c[0] for c in cull_cams]), np.stack([c[1] for c in cull_cams]), IMG, IMG)
    K32 = torch.from_numpy(cull[0].astype(np.float32)).to(DEV)
    RT32 = torch.from_numpy(cull[1].astype(np.float32)).to(DEV)
    faces = drv.model.faces_device()
    verts = drv.vertices(*stacked, True)

    # (a)
    kernels = {}
    for F in (1, LOOP_FRAMES):
        v = verts[:F].contiguous()
        out = torch.empty((F, N_CULL, IMG, IMG), dtype=torch.uint8, device=DEV)
        scratch = ops.smpl_silhouette_scratch(F, V, Nf, N_CULL, DEV)
        t = event_ms(lambda: ops.smpl_silhouette(v, faces, RT32, K32, IMG, IMG, out=out, scratch=scratch), a.reps, 3)
        t["ms_per_frame"] = t["mean_ms"] / F
        t["output_bytes"] = int(out.numel())
        kernels["nb_smpl_silhouette F=%d" % F] = t
    raw = ops.smpl_silhouette(verts, faces, RT32, K32, IMG, IMG)
    borders = [cull_border(cb, cull[0], cull[1], 0.05) for _, cb in probe]
    dil = torch.empty_like(raw[0])
    t = event_ms(lambda: ops.mask_dilate(raw[0], borders[0], out=dil), a.reps, 3)
    t["border"] = int(borders[0])
    kernels["nb_mask_dilate of one frame (4 views)"] = t
    coverage = dict(raw=float(raw.float().mean()), dilated=float(ops.mask_dilate(raw[0], borders[0]).float().mean()))

    # (b)
    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, False, H.DEFAULT_PRECISION)
    cfg = RenderConfig(N_samples=64, perturb=0.0, H=IMG, W=IMG)
    nv_base = NovelViewRenderer(Renderer(net, cfg), IMG, IMG, DEV)
    nv_cull = NovelViewRenderer(RendererMmsk(net, cfg), IMG, IMG, DEV)
    cams = [camera(cb, 0.35) for _, cb in probe]

    def run(nv, **kw):
        n = 0
        for o in nv.render_views(drv.views(cams, *stacked, 0, True, **kw)):
            n += o["n_rays"]
        return n

    n_rays = run(nv_base)
    assert run(nv_cull, cull_cameras=cull) == n_rays
    ms_base, ms_cull = wall_series([lambda: run(nv_base), lambda: run(nv_cull, cull_cameras=cull)], a.reps, 3)
    base, culled = stats(ms_base, LOOP_FRAMES), stats(ms_cull, LOOP_FRAMES)
    spread = base["max_ms"] - base["min_ms"]
    gain = base["mean_ms"] - culled["mean_ms"]

    # (c)
    shares = []
    for view in drv.views(cams, *stacked, 0, True, cull_cameras=cull):
        shares.append(surviving_share(nv_cull.view_batch(*view), cfg.N_samples)[0])

    res = {"tool": "tools/bench_pose_cull.py", "head": a.head or _head(), "box": socket.gethostname(),
           "device": torch.cuda.get_device_name(0),
           "timing": "kernels: HIP events per call after 3 warm-up calls; render_loop: perf_counter around a synchronised 16-frame "
                     "loop, the two renderers alternating, after 3 warm-up loops each",
           "mesh": dict(vertices=V, triangles=Nf, extent_m=[float(x) for x in np.ptp(closed_mesh()[0], axis=0)]), "cull_views": N_CULL, "image": [IMG, IMG], "cull_margin_m": 0.05,
           "borders": [int(b) for b in borders], "mask_coverage": coverage, "kernels": kernels,
           "render_loop": dict(frames=LOOP_FRAMES, rays_per_loop=int(n_rays), precision=str(H.DEFAULT_PRECISION),
                               unculled_ms_per_frame=base, culled_ms_per_frame=culled, gain_ms_per_frame=gain,
                               unculled_spread_ms_per_frame=spread),
           "surviving_sample_share": dict(mean=float(np.mean(shares)), min=float(np.min(shares)), max=float(np.max(shares))),
           "condition": "the culled loop is faster per frame than the unculled loop by more than the unculled loop's max - min over "
                        "its calls in this process",
           "meets_condition": bool(gain > spread)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, t in kernels.items():
        print("%s: %.4f ms (min %.4f, max %.4f)" % (k, t["mean_ms"], t["min_ms"], t["max_ms"]))
    print("render loop per frame: unculled %.3f ms (spread %.3f), culled %.3f ms, gain %.3f ms; %.1f %% of the samples survive" % (
        base["mean_ms"], spread, culled["mean_ms"], gain, 100.0 * float(np.mean(shares))))
    print("meets_condition:", res["meets_condition"])


if __name__ == "__main__":
    main()
