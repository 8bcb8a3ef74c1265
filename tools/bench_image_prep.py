"""Times the device image preparation (neuralbody_amd/image_prep.py, csrc/nb_image_prep.hip) at the light-stage size:
  * one 1024 x 1024 frame (RGB + CIHP label image) at ratio 0.5 and at ratio 1, and the four 1024 x 1024 masks of a mesh item;
  * per case the device time of the kernels alone on bytes already resident (HIP events around `--batch` back-to-back calls, per
    call), the time end to end (PNG decode, upload of 3 + 1 bytes per pixel, kernels; perf_counter around a synchronised call)
    and its decode share, and the bytes the kernels must move over the HBM peak of MI355X_MICROARCH.md as the floor;
  * the training step the frames feed, measured in the same run by `bench.py --mode train` in a child process,
and writes profiles/image_prep.json.  No threshold is set.  The host path this replaces (cv2.undistort of a float32 image,
cv2.resize, cv2.erode / cv2.dilate) cannot be timed where OpenCV is not installed, and the file says so instead of a number.

    python tools/bench_image_prep.py [--reps 30] [--batch 20] [--out profiles/image_prep.json] [--head <commit>] [--no-step]
"""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_mesh import HBM_PEAK, _head, event_ms  # noqa: E402
from tools.bench_mesh_lattice import wall_ms  # noqa: E402
from tools.bench_train_rays import train_step_ms  # noqa: E402

SIZE, N_MASKS = 1024, 4
K = np.array([[1100.0, 0.0, 517.3], [0.0, 1095.0, 498.6], [0.0, 0.0, 1.0]])
D = np.array([-0.25, 0.12, 0.0008, -0.0005, 0.02])  # of the size the light stage's cameras carry


def photo(seed):
    """A picture with structure at every scale (so that the PNG decode is no best case) and a body-shaped label image."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    base = 120 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] * np.array([1.0, 0.8, 0.6])
    rgb = np.clip(base + rng.normal(0, 12, (SIZE, SIZE, 3)), 0, 255).astype(np.uint8)
    body = ((yy - 0.5 * SIZE) / (0.42 * SIZE)) ** 2 + ((xx - 0.5 * SIZE) / (0.16 * SIZE)) ** 2 < 1.0
    label = np.where(body, 1 + (yy // 64) % 19, 0).astype(np.uint8)
    return rgb, label


def per_call(t, batch):
    return {k: (v / batch if k.endswith("_ms") else v) for k, v in t.items()}


def frame_bytes(n):
    px = SIZE * SIZE
    return dict(mask_band=2 * px, image_undistort=4 * px + 13 * px // (n * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_prep.json"))
    ap.add_argument("--head", default=None)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_prep needs an MI355X: a CPU run gives no timing")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    step_ms = None if args.no_step else train_step_ms()  # the child has the device to itself

    from PIL import Image

    from neuralbody_amd import ops
    from neuralbody_amd.image_prep import BORDER, DeviceImagePrep, camera_constants, decode

    dev = torch.device("cuda:0")
    prep = DeviceImagePrep(dev)
    cam = camera_constants(K, D)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for v in range(N_MASKS):
            rgb, label = photo(v)
            img_p, msk_p = os.path.join(tmp, "%d.png" % v), os.path.join(tmp, "m%d.png" % v)
            Image.fromarray(rgb).save(img_p)
            Image.fromarray(label).save(msk_p)
            paths.append((img_p, msk_p))
        rgb, label = photo(0)
        rgb_d, label_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(label).to(dev)[None]
        band_d = torch.empty_like(label_d)
        decode_frame = wall_ms(lambda: (decode(paths[0][0]), decode(paths[0][1])), args.reps)
        for ratio in (0.5, 1.0):
            n = int(round(1.0 / ratio))

            def kernels():
                for _ in range(args.batch):
                    ops.mask_band(label_d, BORDER, out=band_d)
                    ops.image_undistort(rgb_d, band_d[0], cam, n, "black")

            def band_only():
                for _ in range(args.batch):
                    ops.mask_band(label_d, BORDER, out=band_d)

            def undistort_only():
                for _ in range(args.batch):
                    ops.image_undistort(rgb_d, band_d[0], cam, n, "black")

            nbytes = frame_bytes(n)
            rec = dict(case="frame %d x %d, ratio %g" % (SIZE, SIZE, ratio), n=n,
                       kernels=per_call(event_ms(kernels, args.reps, warmup=3), args.batch),
                       mask_band=per_call(event_ms(band_only, args.reps, warmup=3), args.batch),
                       image_undistort=per_call(event_ms(undistort_only, args.reps, warmup=3), args.batch),
                       end_to_end_wall=wall_ms(lambda: prep.frame(paths[0][0], paths[0][1], K, D, SIZE, SIZE, ratio, True, False),
                                               args.reps),
                       decode_wall=decode_frame, uploaded_bytes=4 * SIZE * SIZE, algorithmic_bytes=nbytes)
            total = sum(nbytes.values())
            rec["hbm_floor_ms"] = total / HBM_PEAK * 1e3
            rec["kernels_over_floor"] = rec["kernels"]["mean_ms"] / rec["hbm_floor_ms"]
            rec["hbm_fraction"] = total / (rec["kernels"]["mean_ms"] * 1e-3) / HBM_PEAK
            cases.append(rec)
            print(json.dumps(rec))

        labels_d = torch.from_numpy(np.stack([photo(v)[1] for v in range(N_MASKS)])).to(dev)
        body_d = torch.empty_like(labels_d)
        cams = np.stack([cam] * N_MASKS)
        mpaths = [p[1] for p in paths]

        def mask_kernels():
            for _ in range(args.batch):
                ops.mask_band(labels_d, 1, out=body_d)
                ops.image_undistort(None, body_d, cams)

        nbytes = 4 * N_MASKS * SIZE * SIZE  # band: read + write; undistort: read + write
        rec = dict(case="%d masks %d x %d" % (N_MASKS, SIZE, SIZE),
                   kernels=per_call(event_ms(mask_kernels, args.reps, warmup=3), args.batch),
                   end_to_end_wall=wall_ms(lambda: prep.masks(mpaths, [K] * N_MASKS, [D] * N_MASKS), args.reps),
                   decode_wall=wall_ms(lambda: [decode(p) for p in mpaths], args.reps),
                   uploaded_bytes=N_MASKS * SIZE * SIZE, algorithmic_bytes=nbytes, hbm_floor_ms=nbytes / HBM_PEAK * 1e3)
        rec["kernels_over_floor"] = rec["kernels"]["mean_ms"] / rec["hbm_floor_ms"]
        rec["hbm_fraction"] = nbytes / (rec["kernels"]["mean_ms"] * 1e-3) / HBM_PEAK
        cases.append(rec)
        print(json.dumps(rec))

    out = dict(tool="tools/bench_image_prep.py", head=args.head or _head(), box=socket.gethostname(),
               device=torch.cuda.get_device_name(0),
               timing="kernels: HIP events around %d back-to-back calls after 3 warm-up batches, divided by %d; *_wall: perf_counter "
                      "around a synchronised call, PNG decode by %s included" % (
                          args.batch, args.batch, "imageio" if "imageio" in sys.modules else "PIL"),
               hbm_peak_bytes_per_s=HBM_PEAK, train_step_ms=step_ms,
               frame_end_to_end_over_step=None if step_ms is None else cases[0]["end_to_end_wall"]["mean_ms"] / step_ms,
               host_cv2_path="not measured: OpenCV is not installed where this ran, so the host path this replaces has no number here",
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("bench_image_prep: %.1f s" % (time.time() - t0))
