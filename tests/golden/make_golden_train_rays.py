"""Generate tests/golden/train_rays.npz by driving the UNMODIFIED reference samplers
(lib/utils/if_nerf/if_nerf_data_utils.py::sample_ray_h36m and ::sample_ray) on CPU through oracle/ref_harness.py.  Run from the
repo root, where the reference tree exists:   python tests/golden/make_golden_train_rays.py

cv2 does not exist on this stack; the one function the samplers call is seeded into sys.modules BEFORE ref_harness.load()
(which uses setdefault):
  * cv2.fillPoly — a STAND-IN that fills the closed convex hull of the polygon's points (pixel centres inside or on it).
    The fixture says so in `rasteriser`.  Everything else is the reference's own: the mask product, the 100 rule, argwhere
    order, the round schedule, the float64 near/far, the concatenation order and the dtypes.

np.random.randint is wrapped to log every call's (high, size, values), so a test can replay the draws as uniforms
u = (k + 0.5) / high.  The fixture holds synthetic inputs, the logged draws and the reference's outputs: data only.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from neuralbody_amd import train_rays as tr  # noqa: E402
from tests import synthetic as syn  # noqa: E402
from tests import train_rays_ref as trr  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
RASTERISER = ("stand-in for cv2.fillPoly: the closed convex hull of each polygon's points (pixel centres inside or on it); "
              "OpenCV was not available where this fixture was made")
DRAWS = []  # (high, size, values) of every np.random.randint call of the current case


def fill_poly(mask, polys, color):
    for pts in polys:
        hull = tr.convex_hull(np.asarray(pts).reshape(-1, 2))
        assert len(hull) >= 3, "degenerate polygon: pick another box or camera"
        mask[trr.hull_mask(hull, mask.shape[0], mask.shape[1])] = color
    return mask


def seed_modules():
    cv2 = types.ModuleType("cv2")
    cv2.fillPoly = fill_poly
    sys.modules["cv2"] = cv2


def logged_randint(low, high=None, size=None, dtype=int):
    vals = _randint(low, high, size)
    assert low == 0
    DRAWS.append((int(high), int(size), np.array(vals, np.int64)))
    return vals


def body_mask(H, W, cy, cx, ry, rx, ring, label=1):
    """An elliptical body of `label` with a `ring`-pixel border of 100 (multi_view_dataset.py:60-64 marks the mask's border)."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    r = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
    rin = ((yy - cy) / (ry - ring)) ** 2 + ((xx - cx) / (rx - ring)) ** 2
    msk = np.zeros((H, W), np.uint8)
    msk[r <= 1.0] = 100
    msk[rin <= 1.0] = label
    return msk


def cases():
    """name -> dict(H, W, N, mode, body kwargs, camera kwargs, mask, seed)"""
    out = {}
    out["A"] = dict(H=48, W=40, N=96, mode="h36m", seed=11,
                    body=dict(seed=5, box=(0.5, 0.9, 0.3), rh=(0.1, 0.3, 0.0), th=(0.1, 0.0, 0.2), n_verts=64),
                    cam=dict(focal_factor=1.3, distance=2.0, yaw=0.5, pitch=0.2), msk=body_mask(48, 40, 25, 19, 17, 9, 2))
    out["B"] = dict(H=64, W=64, N=1024, mode="h36m", seed=12,
                    body=dict(seed=6, box=(0.6, 1.0, 0.3), rh=(0.0, -0.4, 0.1), th=(0.0, 0.1, 0.0), n_verts=64),
                    cam=dict(focal_factor=1.1, distance=2.0, yaw=-0.7, pitch=0.3), msk=body_mask(64, 64, 30, 33, 24, 14, 3))
    m = body_mask(48, 40, 22, 21, 18, 10, 2, label=2)
    m[m == 100] = 5  # plain mode: every non-zero label is body, 100 has no special meaning
    m[10:14, 18:24] = 200
    m[30:33, 15:20] = 1
    out["C"] = dict(H=48, W=40, N=96, mode="plain", seed=13,
                    body=dict(seed=7, box=(0.5, 0.8, 0.3), rh=(0.2, 0.1, 0.1), th=(0.0, 0.0, 0.1), n_verts=64),
                    cam=dict(focal_factor=1.2, distance=2.0, yaw=0.2, pitch=-0.3), msk=m)
    return out


def main():
    global _randint
    seed_modules()
    from oracle import ref_harness as rh

    ns = rh.load()
    import lib.utils.if_nerf.if_nerf_data_utils as du  # the reference's module, unmodified

    assert du.cv2.fillPoly is fill_poly
    cfg = ns.cfg
    cfg.body_sample_ratio, cfg.face_sample_ratio = 0.5, 0.0
    _randint = np.random.randint
    np.random.randint = logged_randint
    store, names, rounds_needed = {"rasteriser": np.array(RASTERISER)}, [], {}
    try:
        for name, c in cases().items():
            H, W, N = c["H"], c["W"], c["N"]
            body = syn.make_body(**c["body"])
            K, R, T = syn.make_camera(body, H, W, **c["cam"])
            rh_, th_ = np.array(c["body"]["rh"], np.float64), np.array(c["body"]["th"], np.float32).reshape(1, 3)
            frame = tr.multi_view_frame(body["world_verts"], rh_, th_)
            bounds = frame["can_bounds"]
            assert np.array_equal(bounds, body["can_bounds"])
            img = np.random.RandomState(c["seed"]).uniform(0, 1, (H, W, 3)).astype(np.float32)
            msk = c["msk"]
            assert not (msk == 13).any()  # the face label would add a randint call
            hull = tr.bound_hull(bounds, K, np.concatenate([R, T], axis=1))
            bound_mask = du.get_bound_2d_mask(bounds, K, np.concatenate([R, T], axis=1), H, W)
            assert np.array_equal(bound_mask.astype(bool), trr.hull_mask(hull, H, W)), "six quads != hull of the 8 corners"
            fn = du.sample_ray_h36m if c["mode"] == "h36m" else du.sample_ray
            del DRAWS[:]
            np.random.seed(c["seed"])
            rgb, ray_o, ray_d, near, far, coord, mask_at_box = fn(img, msk, K, R, T, bounds, N, "train")
            assert len(DRAWS) % 2 == 0 and len(rgb) >= N
            n_rounds = len(DRAWS) // 2
            rounds_needed[name] = n_rounds
            ks = np.full((n_rounds, N), -1, np.int64)
            highs, sizes = np.zeros((n_rounds, 2), np.int64), np.zeros((n_rounds, 2), np.int64)
            for r in range(n_rounds):
                (hb, sb, vb), (hr, sr, vr) = DRAWS[2 * r], DRAWS[2 * r + 1]
                ks[r, :sb], ks[r, sb:sb + sr] = vb, vr
                highs[r], sizes[r] = (hb, hr), (sb, sr)
            names.append(name)
            for k, v in dict(img=img, msk=msk, K=K, R=R, T=T, bounds=bounds, hull=hull, N=np.array(N), mode=np.array(c["mode"]),
                             draws_k=ks, draws_high=highs, draws_size=sizes, rgb=rgb, ray_o=ray_o, ray_d=ray_d, near=near,
                             far=far, coord=coord, mask_at_box=mask_at_box).items():
                store["%s/%s" % (name, k)] = v
            if name == "A":
                store["A/xyz"], store["A/Rh"], store["A/Th"] = body["world_verts"], rh_, th_
                for k, v in frame.items():
                    store["A/frame_" + k] = v
                t = du.sample_ray_h36m(img, msk, K, R, T, bounds, N, "test")
                for k, v in zip(("rgb", "ray_o", "ray_d", "near", "far", "coord", "mask_at_box"), t):
                    store["D/" + k] = v
            print("%s %dx%d N=%d %s: rounds %d, candidates body %d bound %d, kept %d, hull %s" % (
                name, H, W, N, c["mode"], n_rounds, highs[0, 0], highs[0, 1], len(rgb), hull.tolist()))
            for k, v in (("rgb", rgb), ("ray_o", ray_o), ("ray_d", ray_d), ("near", near), ("far", far)):
                assert v.dtype == np.float32, k
    finally:
        np.random.randint = _randint
    assert max(rounds_needed.values()) >= 2, rounds_needed  # the deficit rounds are exercised
    assert max(rounds_needed.values()) <= 3, rounds_needed  # n_rounds = 4 never hides a shortfall
    store["names"] = np.array(names)
    path = os.path.join(OUT, "train_rays.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
