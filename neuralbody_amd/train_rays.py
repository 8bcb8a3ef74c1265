"""Training rays on the device: what the reference's datasets do per item in DataLoader workers
(lib/datasets/light_stage/multi_view_dataset.py:120-182 -> lib/utils/if_nerf/if_nerf_data_utils.py:72-232: whole-image
get_rays in float64, six cv2.fillPoly calls, three np.argwhere passes per round, a gather, get_near_far) with the images and
masks resident on the device and one nb_train_rays call per item:

    host (numpy, fp64, per frame / per image)          device (HIP, per item)
    bound_hull, multi_view_frame, frame source   -->   nb_train_rays -> the reference's batch dict as device tensors

`TrainRayDataset` is the cfg-free core of the `train_dataset_path` plugin (plugins/light_stage_dataset.py); it runs in the
training process (`train.num_workers 0`), so `default_collate` stacks device tensors and Trainer.to_cuda has nothing to move.
"""
import os

import numpy as np
import torch

from . import ops
from .novel_view import rodrigues


# ------------------------------------------------------------------------------------------- host, per frame / image
def bound_corners(bounds):
    """lib/utils/if_nerf/if_nerf_data_utils.py:24-37: the 8 corners of the AABB, z fastest."""
    (x0, y0, z0), (x1, y1, z1) = np.asarray(bounds)
    return np.array([[x0, y0, z0], [x0, y0, z1], [x0, y1, z0], [x0, y1, z1], [x1, y0, z0], [x1, y0, z1], [x1, y1, z0],
                     [x1, y1, z1]])


def convex_hull(points):
    """Counter-clockwise convex hull of integer points [n,2] (monotone chain), collinear points dropped."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return np.array(pts, np.int64).reshape(-1, 2)

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) -
                                     (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out

    lower, upper = half(pts), half(reversed(pts))
    return np.array(lower[:-1] + upper[:-1], np.int64).reshape(-1, 2)


def bound_hull(bounds, K, RT):
    """The 2-D bound mask of get_bound_2d_mask (if_nerf_data_utils.py:40-51) as ONE convex polygon: the 8 corners (:24-37)
    projected as lib/utils/base_utils.py:17-26 does, rounded half to even (:43), then their convex hull [n,2] int64 (x, y),
    counter-clockwise.  The reference fills six quads (the second one, 4-5-7-6-5, is really the triangle 5-7-6); their union is
    the silhouette of the box, which is this hull.  cv2.fillPoly also draws each outline with an integer line, which can add
    pixels up to about half a pixel outside an edge: those would only be candidates that still have to pass the exact 3-D
    near < far test."""
    corners = bound_corners(np.asarray(bounds, np.float64))
    K, RT = np.asarray(K, np.float64).reshape(3, 3), np.asarray(RT, np.float64).reshape(3, 4)
    cam = np.dot(corners, RT[:, :3].T) + RT[:, 3:].T
    if not np.all(np.isfinite(cam)) or np.any(cam[:, 2] <= 0):
        raise ValueError("bound_hull: a corner of the box has camera depth <= 0 (%s); its projection means nothing" % (
            np.array2string(cam[:, 2], precision=4),))
    xyz = np.dot(cam, K.T)
    xy = np.round(xyz[:, :2] / xyz[:, 2:]).astype(np.int64)
    hull = convex_hull(xy)
    if len(hull) < 3:
        raise ValueError("bound_hull: the projected box is degenerate (%d distinct hull points)" % len(hull))
    return hull


def multi_view_frame(xyz, Rh, Th, voxel_size=(0.005, 0.005, 0.005), big_box=False):
    """prepare_input of lib/datasets/light_stage/multi_view_dataset.py:68-118 for already-loaded arrays: world vertices `xyz`
    [V,3], SMPL global rotation `Rh` and translation `Th` -> dict(coord [V,3] i32 (dhw), out_sh [3] i32, can_bounds [2,3] f32
    (world), bounds [2,3] f32 (SMPL space), R [3,3] f32, Th f32 as given)."""
    xyz = np.asarray(xyz).astype(np.float32)

    def padded_bounds(p):
        lo, hi = np.min(p, axis=0), np.max(p, axis=0)
        if big_box:
            lo -= 0.05
            hi += 0.05
        else:
            lo[2] -= 0.05
            hi[2] += 0.05
        return lo, hi

    can_bounds = np.stack(padded_bounds(xyz), axis=0)
    R = rodrigues(Rh).astype(np.float32)  # cv2.Rodrigues(Rh)[0].astype(np.float32)
    Th = np.asarray(Th).astype(np.float32)
    xyz = np.dot(xyz - Th, R)
    min_xyz, max_xyz = padded_bounds(xyz)
    bounds = np.stack([min_xyz, max_xyz], axis=0)
    dhw, min_dhw, max_dhw = xyz[:, [2, 1, 0]], min_xyz[[2, 1, 0]], max_xyz[[2, 1, 0]]
    vs = np.array(voxel_size)
    coord = np.round((dhw - min_dhw) / vs).astype(np.int32)
    out_sh = (np.ceil((max_dhw - min_dhw) / vs).astype(np.int32) | 31) + 1
    return {"coord": coord, "out_sh": out_sh, "can_bounds": can_bounds.astype(np.float32), "bounds": bounds.astype(np.float32),
            "R": R, "Th": Th}


# ------------------------------------------------------------------------------------------- device, per item
def _refuse_face_sampling(face_sample_ratio):
    if face_sample_ratio != 0:
        raise ValueError("face_sample_ratio = %r: face sampling is not built (the reference's default is 0, "
                         "lib/config/config.py:129, and its masks never hold the face label 13)" % (face_sample_ratio,))


class TrainRaySampler:
    """`sample()` enqueues one nb_train_rays call and reads nothing back; `check()` looks at the status of the last call."""

    def __init__(self, H, W, n_rays, mode="h36m", body_sample_ratio=0.5, face_sample_ratio=0.0, n_rounds=4, device="cuda:0",
                 seed=0):
        _refuse_face_sampling(face_sample_ratio)
        if mode not in ("h36m", "plain"):
            raise ValueError("mode must be 'h36m' (sample_ray_h36m) or 'plain' (sample_ray), got %r" % (mode,))
        if not 0.0 <= float(body_sample_ratio) <= 1.0:
            raise ValueError("body_sample_ratio = %r is outside [0, 1]" % (body_sample_ratio,))
        if int(n_rays) < 1 or int(n_rounds) < 1 or int(H) < 1 or int(W) < 1:
            raise ValueError("H, W, n_rays and n_rounds must be >= 1")
        self.H, self.W, self.n_rays, self.n_rounds = int(H), int(W), int(n_rays), int(n_rounds)
        self.mode, self.body_sample_ratio = mode, float(body_sample_ratio)
        self.device = torch.device(device)
        self.seed = int(seed)
        self._gen = None  # made on first use: constructing the sampler touches no device
        self._pending = None
        self.n_short = 0  # batches that stayed short of n_rays after n_rounds rounds
        self.n_checked = 0

    def uniforms(self):
        if self._gen is None:
            self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
        return torch.rand((self.n_rounds, self.n_rays), dtype=torch.float32, device=self.device, generator=self._gen)

    def sample(self, img, msk, K, R, T, can_bounds, u=None, hull=None):
        """img [H,W,3] fp32 and msk [H,W] uint8 on the device; K, R [3,3], T [3] and can_bounds [2,3] on the host.
        -> dict of device tensors rgb, ray_o, ray_d, near, far, mask_at_box (bool), pixel (y, x) and status.
        No host synchronisation.  `hull`: bound_hull of the same box and camera, when the caller keeps it."""
        if tuple(img.shape[:2]) != (self.H, self.W):
            raise ValueError("img is %s, the sampler was made for %d x %d" % (tuple(img.shape), self.H, self.W))
        if hull is None:
            RT = np.concatenate([np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 1)], axis=1)
            hull = bound_hull(can_bounds, K, RT)
        if u is None:
            u = self.uniforms()
        elif tuple(u.shape) != (self.n_rounds, self.n_rays):
            raise ValueError("u is %s, expected %s" % (tuple(u.shape), (self.n_rounds, self.n_rays)))
        out = ops.train_rays(img, msk, K, R, T, can_bounds, hull, self.mode, self.body_sample_ratio, u)
        out["mask_at_box"] = out["mask_at_box"].view(torch.bool)  # 0 / 1 bytes
        self._pending = out["status"]
        return out

    def check(self):
        """Read the last sample()'s status back (one 16-byte copy; the work finished a training step ago when the dataset calls
        this).  RuntimeError when a class that had draws has no candidate pixel (the reference raises in randint(0, 0) there);
        a short batch is counted in n_short.  Returns the status as a tuple, None when nothing is pending."""
        if self._pending is None:
            return None
        n_filled, rounds, count_body, count_bound = (int(v) for v in self._pending.cpu().tolist())
        self._pending = None
        self.n_checked += 1
        n_body = int(self.n_rays * self.body_sample_ratio)
        if n_body > 0 and count_body == 0:
            raise RuntimeError("train rays: no body pixel inside the projected box (%d draws asked for one; mode %r)" % (
                n_body, self.mode))
        if self.n_rays - n_body > 0 and count_bound == 0:
            raise RuntimeError("train rays: no pixel inside the projected box (%d draws asked for one)" % (self.n_rays - n_body))
        if n_filled < self.n_rays:
            self.n_short += 1
        return n_filled, rounds, count_body, count_bound


def ray_occupancy(msk, pixel, mode):
    """Foreground mask at the sampler's pixels, float32 [n]: msk [H,W] uint8 and pixel [n,2] int32 (y, x) on the device ->
    msk == 1 in mode 'h36m' (the border band 100 is never drawn), msk != 0 in mode 'plain'; rows the sampler left unfilled
    (pixel = (-1, -1), mask_at_box 0) give 0.  A gather on the device, nothing is read back."""
    y, x = pixel[:, 0].long(), pixel[:, 1].long()
    filled = (y >= 0) & (x >= 0)
    m = msk[y.clamp_min(0), x.clamp_min(0)]
    fg = (m == 1) if mode == "h36m" else (m != 0)
    return (fg & filled).to(torch.float32)


class TrainDataConfig:
    """The cfg keys the dataset core reads (multi_view_dataset.py:52,78,110,169; if_nerf_data_utils.py:83-84)."""

    def __init__(self, N_rand=1024, body_sample_ratio=0.5, face_sample_ratio=0.0, begin_ith_frame=0, frame_interval=1,
                 num_train_frame=1, voxel_size=(0.005, 0.005, 0.005), big_box=False, test_novel_pose=False, mode="h36m",
                 n_rounds=4, seed=0, ray_mask=False):
        """ray_mask (not a reference key): a train item also carries `occupancy` [N_rand] float32, the foreground mask at each
        ray's pixel, for silhouette supervision of acc_map (plugins/if_nerf_clight.py: mask_loss_weight)."""
        self.ray_mask = bool(ray_mask)
        self.N_rand, self.body_sample_ratio, self.face_sample_ratio = int(N_rand), float(body_sample_ratio), face_sample_ratio
        self.begin_ith_frame, self.frame_interval, self.num_train_frame = int(begin_ith_frame), int(frame_interval), int(num_train_frame)
        self.voxel_size, self.big_box, self.test_novel_pose = tuple(voxel_size), bool(big_box), bool(test_novel_pose)
        self.mode, self.n_rounds, self.seed = mode, int(n_rounds), int(seed)


class MemoryFrameSource:
    """Frame source over items already in memory: `items[i]` is the tuple `load(i)` returns."""

    def __init__(self, items):
        self.items = list(items)
        self.n_items = len(self.items)

    def load(self, i):
        return self.items[i]


class TrainRayDataset(torch.utils.data.Dataset):
    """lib/datasets/light_stage/multi_view_dataset.py::Dataset with the per-item work on the device.

    `source`: an object with `n_items` and `load(i) -> (img f32 [H,W,3], msk u8 [H,W], K [3,3], R [3,3], T [3] or [3,1],
    frame_index, cam_ind, xyz [V,3], Rh, Th)`.  Every image and mask is uploaded on first use and stays resident
    (12*H*W + H*W bytes each); every frame's multi_view_frame tensors are kept too."""

    def __init__(self, source, cfg, split="train", device="cuda:0"):
        super().__init__()
        _refuse_face_sampling(cfg.face_sample_ratio)
        self.source, self.cfg, self.split = source, cfg, split
        self.device = torch.device(device)
        self._items, self._frames = {}, {}
        self._sampler = None
        self.last_sample = None  # the sampler's whole output for the last train item (pixel and status included)

    def __len__(self):
        return int(self.source.n_items)

    def latent_index(self, frame_index):
        """multi_view_dataset.py:169-171"""
        if self.cfg.test_novel_pose:
            return self.cfg.num_train_frame - 1
        return (int(frame_index) - self.cfg.begin_ith_frame) // self.cfg.frame_interval

    @property
    def sampler(self):
        return self._sampler

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor) and a.is_cuda:  # a source with a DeviceImagePrep: already where it belongs
            return a
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def _frame(self, frame_index, xyz, Rh, Th):
        fr = self._frames.get(frame_index)
        if fr is None:
            host = multi_view_frame(xyz, Rh, Th, self.cfg.voxel_size, self.cfg.big_box)
            fr = {"can_bounds": host["can_bounds"],
                  "dev": {"coord": self._dev(host["coord"], np.int32), "out_sh": self._dev(host["out_sh"], np.int32),
                          "bounds": self._dev(host["bounds"], np.float32), "R": self._dev(host["R"], np.float32),
                          "Th": self._dev(host["Th"], np.float32),
                          "latent_index": torch.tensor(self.latent_index(frame_index), dtype=torch.int64, device=self.device)}}
            self._frames[frame_index] = fr
        return fr

    def _item(self, index):
        it = self._items.get(index)
        if it is None:
            img, msk, K, R, T, frame_index, cam_ind, xyz, Rh, Th = self.source.load(index)
            K, R = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
            T = np.asarray(T, np.float64).reshape(3, 1)
            fr = self._frame(int(frame_index), xyz, Rh, Th)
            it = {"img": self._dev(img, np.float32), "msk": self._dev(msk, np.uint8), "K": K, "R": R, "T": T,
                  "frame_index": int(frame_index), "cam_ind": int(cam_ind), "frame": fr,
                  "hull": bound_hull(fr["can_bounds"], K, np.concatenate([R, T], axis=1)) if self.split == "train" else None}
            self._items[index] = it
        return it

    def __getitem__(self, index):
        index = int(index)
        if self._sampler is not None:
            self._sampler.check()  # the previous item's status: work that finished a step ago
        it = self._item(index)
        fr = it["frame"]
        H, W = it["img"].shape[:2]
        if self.split == "train":
            if self._sampler is None:
                c = self.cfg
                self._sampler = TrainRaySampler(H, W, c.N_rand, c.mode, c.body_sample_ratio, c.face_sample_ratio, c.n_rounds,
                                                self.device, c.seed)
            s = self._sampler.sample(it["img"], it["msk"], it["K"], it["R"], it["T"], fr["can_bounds"], hull=it["hull"])
            self.last_sample = s
            ret = {k: s[k] for k in ("rgb", "ray_o", "ray_d", "near", "far", "mask_at_box")}
            if getattr(self.cfg, "ray_mask", False):
                ret["occupancy"] = ray_occupancy(it["msk"], s["pixel"], self._sampler.mode)
        else:  # if_nerf_data_utils.py:220-230: every pixel's ray, float32 near/far, compacted by mask_at_box
            ray_o, ray_d, near, far, mask, n_rays = ops.raygen(H, W, it["K"], it["R"], it["T"], fr["can_bounds"], self.device)
            n = int(n_rays.item())
            mask = mask.view(torch.bool)
            ret = {"rgb": it["img"].reshape(-1, 3)[mask], "ray_o": ray_o[:n], "ray_d": ray_d[:n], "near": near[:n],
                   "far": far[:n], "mask_at_box": mask}
        ret.update(fr["dev"])
        ret["frame_index"], ret["cam_ind"] = it["frame_index"], it["cam_ind"]
        return ret


# ------------------------------------------------------------------------------------------- disk source
class LightStageFrameSource:
    """The file side of lib/datasets/light_stage/multi_view_dataset.py, a thin restatement: the item list (:22-50), get_mask
    (:54-66), the image / camera part of __getitem__ (:121-150) and the two np.load calls of prepare_input (:70-72, :87-92).
    imageio and cv2 are imported on first use; everything here runs once per image.  `prep`: an image_prep.DeviceImagePrep
    to do the image and mask work of load() on the device instead (load() then returns device tensors for both, and cv2 is
    never imported); None keeps the cv2 lines."""

    def __init__(self, data_root, human, ann_file, split, training_view, begin_ith_frame, frame_interval, num_train_frame, H, W,
                 ratio, mask_bkgd, white_bkgd, vertices="vertices", params="params", test_novel_pose=False,
                 num_novel_pose_frame=0, prep=None):
        self.prep = prep
        self.data_root, self.human, self.split = data_root, human, split
        annots = np.load(ann_file, allow_pickle=True).item()
        self.cams = annots["cams"]
        num_cams = len(self.cams["K"])
        test_view = [i for i in range(num_cams) if i not in training_view]
        view = list(training_view) if split == "train" else test_view
        if len(view) == 0:
            view = [0]
        i, i_intv, ni = begin_ith_frame, frame_interval, num_train_frame
        if test_novel_pose:
            i = (i + num_train_frame) * i_intv
            ni = num_novel_pose_frame
            if human == "CoreView_390":
                i = 0
        sel = annots["ims"][i:i + ni * i_intv][::i_intv]
        self.ims = np.array([np.array(d["ims"])[view] for d in sel]).ravel()
        self.cam_inds = np.array([np.arange(len(d["ims"]))[view] for d in sel]).ravel()
        self.num_cams = len(view)
        self.n_items = len(self.ims)
        self.H, self.W, self.ratio, self.mask_bkgd, self.white_bkgd = int(H), int(W), ratio, bool(mask_bkgd), bool(white_bkgd)
        self.vertices, self.params = vertices, params

    def get_mask(self, index):
        import cv2
        import imageio

        msk_cihp = imageio.imread(os.path.join(self.data_root, "mask_cihp", self.ims[index])[:-4] + ".png")
        msk = (msk_cihp != 0).astype(np.uint8)
        kernel = np.ones((5, 5), np.uint8)
        msk_erode, msk_dilate = cv2.erode(msk.copy(), kernel), cv2.dilate(msk.copy(), kernel)
        msk[(msk_dilate - msk_erode) == 1] = 100
        return msk

    def load(self, index):
        if self.prep is not None:
            return self._load_device(index)
        import cv2
        import imageio

        img_path = os.path.join(self.data_root, self.ims[index])
        img = imageio.imread(img_path).astype(np.float32) / 255.0
        img = cv2.resize(img, (self.W, self.H))
        msk = self.get_mask(index)
        cam_ind = self.cam_inds[index]
        K, D = np.array(self.cams["K"][cam_ind]), np.array(self.cams["D"][cam_ind])
        img, msk = cv2.undistort(img, K, D), cv2.undistort(msk, K, D)
        R, T = np.array(self.cams["R"][cam_ind]), np.array(self.cams["T"][cam_ind]) / 1000.0
        H, W = int(img.shape[0] * self.ratio), int(img.shape[1] * self.ratio)
        img = cv2.resize(img, (W, H), interpolation=cv2.INTER_AREA)
        msk = cv2.resize(msk, (W, H), interpolation=cv2.INTER_NEAREST)
        if self.mask_bkgd:
            img[msk == 0] = 0
            if self.white_bkgd:
                img[msk == 0] = 1
        K[:2] = K[:2] * self.ratio
        if self.human in ("CoreView_313", "CoreView_315"):
            i = int(os.path.basename(img_path).split("_")[4])
            frame_index = i - 1
        else:
            i = int(os.path.basename(img_path)[:-4])
            frame_index = i
        xyz = np.load(os.path.join(self.data_root, self.vertices, "{}.npy".format(i))).astype(np.float32)
        params = np.load(os.path.join(self.data_root, self.params, "{}.npy".format(i)), allow_pickle=True).item()
        return img, msk, K, R, T, frame_index, int(cam_ind), xyz, params["Rh"], params["Th"]

    def _load_device(self, index):
        """load() with `prep` standing where imageio and cv2 stand above: the same tuple, img and msk on the device."""
        img_path = os.path.join(self.data_root, self.ims[index])
        msk_path = os.path.join(self.data_root, "mask_cihp", self.ims[index])[:-4] + ".png"
        cam_ind = self.cam_inds[index]
        K, D = np.array(self.cams["K"][cam_ind]), np.array(self.cams["D"][cam_ind])
        img, msk = self.prep.frame(img_path, msk_path, K, D, self.H, self.W, self.ratio, self.mask_bkgd, self.white_bkgd)
        R, T = np.array(self.cams["R"][cam_ind]), np.array(self.cams["T"][cam_ind]) / 1000.0
        K[:2] = K[:2] * self.ratio
        if self.human in ("CoreView_313", "CoreView_315"):
            i = int(os.path.basename(img_path).split("_")[4])
            frame_index = i - 1
        else:
            i = int(os.path.basename(img_path)[:-4])
            frame_index = i
        xyz = np.load(os.path.join(self.data_root, self.vertices, "{}.npy".format(i))).astype(np.float32)
        params = np.load(os.path.join(self.data_root, self.params, "{}.npy".format(i)), allow_pickle=True).item()
        return img, msk, K, R, T, frame_index, int(cam_ind), xyz, params["Rh"], params["Th"]
