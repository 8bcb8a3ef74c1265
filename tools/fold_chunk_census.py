"""Host restatement of the folded first layer's voxel lists (nb_march_fold.hip: boxes -> table -> 16-voxel chunks) for one view:
how long the lists are, how much of them is inactive, and how many chunks hold no active voxel at all — the chunks the march
neither fetches nor multiplies.  Structural counts, emulated on the CPU (numpy only, nothing is read from the kernel):

  * active sets: the occupied voxels of the body, carried through the four strided convolutions (kernel 3, stride 2, padding 1:
    an output voxel is active iff one of its 27 inputs is) — rows that the ReLU happens to zero are still counted active;
  * a workgroup = one 8 x 8 pixel tile of the image at one depth step; per level its box is the clamped floor / floor + 1 of
    the 64 samples' level coordinates (prep_boxes), its voxels are listed x fastest (tbl_issue), the four levels end to end,
    padded to 16; a list longer than 128 is marched in passes of 128 (chunk boundaries stay where they are).

    python tools/fold_chunk_census.py [--scene bench|<golden scene>] [--pose 1] [--size 512] [--samples 64] [--tile-stride 3]
                                      [--out profiles/fold_chunk_census_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import synthetic as syn  # noqa: E402

TILE, CHUNK, K_CAP, KM_CAP = 8, 16, 128, 1024
VOXEL = 0.005
MFMA_PER_CHUNK, MFMA_BEHIND_FC0 = 12, 264  # per wave and depth step (bench.py: fc_1 96, fc_2 96, colour head 48 + 24)


def build_view(scene, pose, size, samples):
    """-> (body, ray_o, ray_d, near, far [H*W rays, row-major], H, W, samples)"""
    if scene == "bench":  # bench.build_scene / build_poses
        body = syn.make_body(seed=0)
        H = W = size
        K, R, T = syn.full_coverage_camera(body, H, W, yaw=0.35 + 0.12 * pose, pitch=0.1 - 0.03 * pose)
    else:
        from tests.golden import scenes

        r = scenes.SCENES[scene]
        body = syn.make_body(**r["body"])
        H, W, samples = r["cam"]["H"], r["cam"]["W"], r["n_samples"]
        K, R, T = syn.make_camera(body, H, W, focal_factor=r["cam"]["focal_factor"], distance=r["cam"]["distance"])
    ray_o, ray_d, near, far, mask = syn.host_image_rays(H, W, K, R, T, body["can_bounds"])
    if not mask.all():
        raise SystemExit("the view must see the bounding box in every pixel (%d of %d do): tiles are whole" % (mask.sum(), mask.size))
    return body, ray_o, ray_d, near, far, H, W, samples


def active_sets(body):
    """Per level the active voxels [D, H, W] bool, from the body's occupied voxels."""
    out_sh = [int(s) for s in body["out_sh"]]
    a = np.zeros(out_sh, bool)
    c = body["coord"]
    a[c[:, 0], c[:, 1], c[:, 2]] = True
    n_occupied = int(a.sum())
    levels = []
    for _ in range(4):
        dims = [(s - 1) // 2 + 1 for s in a.shape]  # (s + 2 - 3) // 2 + 1
        p = np.pad(a, 1)
        o = np.zeros(dims, bool)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    o |= p[dz:dz + 2 * dims[0]:2, dy:dy + 2 * dims[1]:2, dx:dx + 2 * dims[2]:2][:dims[0], :dims[1], :dims[2]]
        levels.append(o)
        a = o
    return levels, n_occupied, out_sh


def level_coords(body, pts, out_sh, dims):
    """Index coordinates (x, y, z of grid_sample = W, H, D) of world points in a level of size dims = (D, H, W): [n, 3]."""
    can = (pts - body["Th"].reshape(1, 3).astype(np.float64)) @ body["R"].astype(np.float64)
    lo = body["bounds"][0].astype(np.float64)
    out = []
    for ax, (sz, osh) in enumerate(zip((dims[2], dims[1], dims[0]), (out_sh[2], out_sh[1], out_sh[0]))):  # x, y, z
        g = (can[:, ax] - lo[ax]) / VOXEL / osh * 2.0 - 1.0
        out.append(np.clip((g + 1.0) / 2.0 * (sz - 1), -2.0, sz + 1.0))
    return np.stack(out, 1)


def census(scene="bench", pose=1, size=512, samples=64, tile_stride=3):
    body, ray_o, ray_d, near, far, H, W, S = build_view(scene, pose, size, samples)
    levels, n_occupied, out_sh = active_sets(body)
    t = np.linspace(0.0, 1.0, S)
    ty, tx = np.meshgrid(np.arange(H // TILE), np.arange(W // TILE), indexing="ij")
    tiles = np.stack([ty[::tile_stride, ::tile_stride].ravel(), tx[::tile_stride, ::tile_stride].ravel()], 1)
    py, px = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
    n_steps = len(tiles) * S
    Ks = np.zeros(n_steps, np.int64)
    n_lvl = np.zeros((n_steps, 4), np.int64)
    act_lvl = np.zeros((n_steps, 4), np.int64)
    chunks = np.zeros(n_steps, np.int64)
    dead = np.zeros(n_steps, np.int64)
    lead_dead = np.zeros(n_steps, np.int64)
    k = 0
    for tyi, txi in tiles:
        ray = ((tyi * TILE + py) * W + txi * TILE + px).ravel()
        z = near[ray, None].astype(np.float64) * (1.0 - t)[None] + far[ray, None].astype(np.float64) * t[None]  # [64, S]
        pts = ray_o[ray, None].astype(np.float64) + ray_d[ray, None].astype(np.float64) * z[..., None]  # [64, S, 3]
        boxes = []
        for L, act in enumerate(levels):
            D_, H_, W_ = act.shape
            idx = np.floor(level_coords(body, pts.reshape(-1, 3), out_sh, act.shape)).astype(np.int64).reshape(TILE * TILE, S, 3)
            hi_lim = np.array([W_ - 1, H_ - 1, D_ - 1])
            lo = np.clip(idx, 0, hi_lim).min(0)       # [S, 3]
            hi = np.clip(idx + 1, 0, hi_lim).max(0)
            boxes.append((lo, hi))
        for s in range(S):
            flags = []
            for L, act in enumerate(levels):
                lo, hi = boxes[L][0][s], boxes[L][1][s]
                sub = act[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].ravel()  # z slowest, x fastest: the table's order
                n_lvl[k, L] = sub.size
                act_lvl[k, L] = int(sub.sum())
                flags.append(sub)
            f = np.concatenate(flags)
            Ks[k] = f.size
            nch = -(-f.size // CHUNK)
            live = np.pad(f, (0, nch * CHUNK - f.size)).reshape(nch, CHUNK).any(1)
            chunks[k] = nch
            dead[k] = nch - int(live.sum())
            lead_dead[k] = nch if not live.any() else int(np.argmax(live))
            k += 1
    inactive = 1.0 - act_lvl.sum() / n_lvl.sum()
    live_hist = np.bincount(chunks - dead)
    res = {
        "tool": "tools/fold_chunk_census.py", "scene": scene, "pose": pose, "image": [H, W], "samples": S, "tile_stride": tile_stride,
        "note": "structural counts emulated on the host, not read from the kernel; a voxel is active iff the strided convolutions reach it",
        "out_sh": out_sh, "occupied_voxels": n_occupied, "active_voxels_per_level": [int(a.sum()) for a in levels],
        "level_dims": [list(a.shape) for a in levels],
        "workgroup_steps": int(n_steps),
        "box_voxels_mean_per_level": [round(float(v), 2) for v in n_lvl.mean(0)],
        "box_active_voxels_mean_per_level": [round(float(v), 2) for v in act_lvl.mean(0)],
        "steps_with_level_box_entirely_inactive": [round(float(v), 4) for v in (act_lvl == 0).mean(0)],
        "K_mean": round(float(Ks.mean()), 2), "K_p99": int(np.percentile(Ks, 99)), "K_max": int(Ks.max()),
        "steps_K_gt_128": float((Ks > K_CAP).mean()), "steps_K_gt_1024": float((Ks > KM_CAP).mean()),
        "inactive_share_of_list_entries": round(float(inactive), 4),
        "chunks_per_step": round(float(chunks.mean()), 3),
        "dead_chunks_per_step": round(float(dead.mean()), 3),
        "dead_share_of_chunks": round(float(dead.sum() / chunks.sum()), 4),
        "leading_dead_chunks_per_step": round(float(lead_dead.mean()), 3),
        "steps_without_a_live_chunk": round(float((dead == chunks).mean()), 4),
        "live_chunks_histogram": {str(i): int(n) for i, n in enumerate(live_hist) if n},
        "mfma_per_wave_step": {"all_chunks": round(MFMA_BEHIND_FC0 + MFMA_PER_CHUNK * float(chunks.mean()), 2),
                               "live_chunks": round(MFMA_BEHIND_FC0 + MFMA_PER_CHUNK * float((chunks - dead).mean()), 2),
                               "removed": round(MFMA_PER_CHUNK * float(dead.mean()), 2)},
    }
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="bench", help="'bench' (bench.py's body and full-coverage cameras) or a scene of tests/golden/scenes.py")
    ap.add_argument("--pose", type=int, default=1, help="bench: pose of the timed cycle (camera yaw 0.35 + 0.12 pose)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--tile-stride", type=int, default=3, help="every n-th 8 x 8 tile of the image in both directions")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = census(args.scene, args.pose, args.size, args.samples, args.tile_stride)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
