"""Times pose-driven frames (neuralbody_amd/smpl_pose.py) on a 6890-vertex synthetic SMPL model (tests/smpl_ref.py), for F = 1 and
F = 16 frames per call, with and without the pose blend shapes:
  (a) the device calls one by one under HIP events: nb_smpl_pose (its two launches together: one wave per frame, then the
      vertices; the C entry cannot launch the first alone, so the same call on a 12-vertex model — the per-frame wave plus ONE
      workgroup of the vertex kernel — is reported as an UPPER BOUND of it) and nb_smpl_voxelize,
  (b) the whole device frame, PoseDriver.frames: pinned upload, the three launches, the summary's copy and its event (wall clock),
  (c) the host frame it replaces, on the same box in the same run: the float32 numpy restatement of SMPLlayer.forward
      (tests/smpl_ref.py), train_rays.multi_view_frame and the uploads of its arrays from pageable memory (wall clock),
  (d) the 512 x 512 render loop each feeds: NovelViewRenderer.render_views over 16 distinct frames of a small body, the views
      coming from PoseDriver.views or from a generator that makes each frame on the host as in (c),
  (e) the accuracy of the vertices on the fixture's cases: max |device - float64 restatement| over the reference's own E_ref,
and writes profiles/smpl_pose.json.  The condition is relative: (b) <= (c) for both F, and the loop of (d) with the driver no
slower than with host frames.

    python tools/bench_smpl_pose.py [--reps 30] [--host-reps 5] [--out profiles/smpl_pose.json]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import _head, event_ms  # noqa: E402
from tools.bench_mesh_lattice import wall_ms  # noqa: E402

DEV = "cuda:0"
IMG = 512
LOOP_FRAMES = 16


def host_frame(model, p, new_params, dev):
    """One frame the way the package makes it today: vertices on the host, multi_view_frame, six uploads."""
    from neuralbody_amd.train_rays import multi_view_frame
    from tests import smpl_ref as sr

    verts = sr.forward(model, p[0], p[1], p[2], p[3], new_params, np.float32)
    fr = multi_view_frame(verts, p[2], p[3])
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    frame = {"coord": up(fr["coord"][None], np.int32), "out_sh": up(fr["out_sh"][None], np.int32),
             "bounds": up(fr["bounds"][None], np.float32), "R": up(fr["R"][None], np.float32),
             "Th": up(fr["Th"].reshape(1, 1, 3), np.float32), "latent_index": up(np.zeros(1), np.int64)}
    return frame, fr["can_bounds"]


def bench_frames(host_model, model, F, new_params, reps, host_reps):
    from neuralbody_amd import ops
    from neuralbody_amd.smpl_pose import PoseDriver, pack_params
    from tests import smpl_ref as sr

    P = [sr.draw_params(300 + i) for i in range(F)]
    stacked = [np.stack([p[k] for p in P]) for k in range(4)]
    native, _ = model.native()
    params = pack_params(*stacked).to(DEV)
    verts, joints = ops.smpl_pose(native, params, new_params)
    ws = torch.empty((F, 512), device=DEV)
    t_pose = event_ms(lambda: ops.smpl_pose(native, params, new_params, verts, joints, ws), reps, 3)
    t_vox = event_ms(lambda: ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], (0.005,) * 3, "zju"), reps, 3)
    drv = PoseDriver(model)
    t_dev = wall_ms(lambda: drv.frames(*stacked, 0, new_params), reps, warmup=3)
    t_host = wall_ms(lambda: [host_frame(host_model, p, new_params, DEV) for p in P], host_reps, warmup=1)
    return dict(F=F, new_params=new_params, V=model.n_verts, nb_smpl_pose=t_pose, nb_smpl_voxelize=t_vox, device_frames_wall=t_dev,
                host_frames_wall=t_host, device_over_host=t_dev["mean_ms"] / t_host["mean_ms"])


def bench_prologue(reps):
    """nb_smpl_pose on a 12-vertex model: the per-frame wave plus one workgroup of the vertex kernel, an upper bound of the
    first launch alone."""
    from neuralbody_amd import ops
    from neuralbody_amd.smpl_pose import SmplModel, pack_params
    from tests import smpl_ref as sr

    m = sr.synthetic_smpl(5, 12, sr.SMPL_PARENTS)
    model = SmplModel.from_arrays(m, DEV)
    native, _ = model.native()
    out = {}
    for F in (1, 16):
        P = [sr.draw_params(300 + i) for i in range(F)]
        params = pack_params(*[np.stack([p[k] for p in P]) for k in range(4)]).to(DEV)
        out["F=%d" % F] = event_ms(lambda: ops.smpl_pose(native, params, True), reps, 3)
    return out


def bench_loop(reps):
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel
    from tests import helpers as H
    from tests import smpl_ref as sr
    from tests import synthetic as syn

    host_model = sr.synthetic_smpl(21, 6890, sr.SMPL_PARENTS, box=(0.3, 0.5, 0.2))
    model = SmplModel.from_arrays(host_model, DEV)
    drv = PoseDriver(model)
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(LOOP_FRAMES)]
    stacked = [np.stack([p[k] for p in P]) for k in range(4)]
    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, False, H.DEFAULT_PRECISION)
    nv = NovelViewRenderer(Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=IMG, W=IMG)), IMG, IMG, DEV)
    cams = []
    for _, cb in drv.frames(*stacked, 0, True):
        K, R, T = syn.make_camera({"can_bounds": cb}, IMG, IMG, focal_factor=2.5, distance=1.5)
        cams.append((K, np.concatenate([R, T.reshape(3, 1)], axis=1)))

    def host_views():
        for f, p in enumerate(P):
            frame, cb = host_frame(host_model, p, True, DEV)
            yield cams[f][0], cams[f][1], cb, frame

    def run(views):
        n = 0
        for out in nv.render_views(views):
            n += out["n_rays"]
        return n

    n_rays = run(drv.views(cams, *stacked, 0, True))
    t_drv = wall_ms(lambda: run(drv.views(cams, *stacked, 0, True)), reps, warmup=2)
    t_host = wall_ms(lambda: run(host_views()), reps, warmup=2)
    return dict(frames=LOOP_FRAMES, image=[IMG, IMG], rays_per_loop=int(n_rays), precision=str(H.DEFAULT_PRECISION),
                driver_views_wall=t_drv, host_views_wall=t_host, driver_ms_per_frame=t_drv["mean_ms"] / LOOP_FRAMES,
                host_ms_per_frame=t_host["mean_ms"] / LOOP_FRAMES, driver_over_host=t_drv["mean_ms"] / t_host["mean_ms"])


def accuracy():
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel
    from tests import smpl_ref as sr

    gold = np.load(os.path.join(ROOT, "tests", "golden", "smpl_pose.npz"))
    out, models = {}, {}
    for name in sorted(sr.CASES):
        key = sr.CASES[name][:3]
        if key not in models:
            host = sr.case_model(name)
            models[key] = (host, SmplModel.from_arrays(host, DEV))
        host, model = models[key]
        p, new_params = sr.case_params(name), sr.CASES[name][3]
        got = PoseDriver(model).vertices(*p, new_params)[0].cpu().numpy().astype(np.float64)
        err = float(np.abs(got - sr.forward(host, *p, new_params, np.float64)).max())
        e_ref = float(gold[name + "/E_ref"])
        out[name] = dict(max_abs_err_m=err, E_ref_m=e_ref, ratio=err / e_ref)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smpl_pose.json"))
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    from neuralbody_amd.smpl_pose import SmplModel
    from tests import smpl_ref as sr

    host_model = sr.case_model("smpl6890_new")
    model = SmplModel.from_arrays(host_model, DEV)
    frames = [bench_frames(host_model, model, F, new_params, a.reps, a.host_reps) for F in (1, 16) for new_params in (True, False)]
    loop = bench_loop(a.loop_reps)
    res = {"tool": "tools/bench_smpl_pose.py", "head": a.head or _head(), "box": socket.gethostname(),
           "device": torch.cuda.get_device_name(0),
           "timing": "nb_*: HIP events per call after 3 warm-up calls; *_wall: perf_counter around a synchronised call",
           "condition": "device frames (wall) <= host frames (wall) for F = 1 and 16, and the 16-frame 512 x 512 render_views loop fed "
                        "by PoseDriver.views no slower than fed by host frames",
           "meets_condition": bool(all(f["device_over_host"] <= 1.0 for f in frames) and loop["driver_over_host"] <= 1.0),
           "frames": frames, "prologue_upper_bound_pose_call_on_a_12_vertex_model": bench_prologue(a.reps), "render_loop": loop,
           "vertex_accuracy": accuracy()}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for fr in frames:
        print("F=%2d new_params=%d: pose %.4f ms, voxelize %.4f ms, device frames %.3f ms, host frames %.3f ms" % (
            fr["F"], fr["new_params"], fr["nb_smpl_pose"]["mean_ms"], fr["nb_smpl_voxelize"]["mean_ms"],
            fr["device_frames_wall"]["mean_ms"], fr["host_frames_wall"]["mean_ms"]))
    print("render loop: driver %.2f ms / frame, host %.2f ms / frame" % (loop["driver_ms_per_frame"], loop["host_ms_per_frame"]))
    print("accuracy ratios:", {k: round(v["ratio"], 2) for k, v in res["vertex_accuracy"].items()})
    print("meets_condition:", res["meets_condition"])


if __name__ == "__main__":
    main()
