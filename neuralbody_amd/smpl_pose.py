"""Pose-driven frames on the device: what the reference does offline (zju_smpl/extract_vertices.py: SMPLlayer.forward over lbs,
one vertices/{i}.npy per frame) and then per item on the host (prepare_input of lib/datasets/light_stage/multi_view_dataset.py:
68-118) with the SMPL model resident on the device and the frame made there from its parameters:

    host (per call)                                  device (HIP, three launches for all frames of the call)
    poses | shapes | Rh | Th, one pinned [F,88] -->  nb_smpl_pose (chain, vertices) -> nb_smpl_voxelize --> frame tensors
    can_bounds, out_sh                          <--  summary [F,9], one pinned copy behind an event

A frame is the dict NovelViewRenderer.view_batch documents, so `PoseDriver.views` feeds NovelViewRenderer.render_views as a
turntable's views do, and a frame change uploads 88 floats instead of the frame's coordinates from pageable memory.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib, ops

N_JOINTS, N_POSE_BASIS, N_BETAS, N_PARAMS = _lib.SMPL_JOINTS, _lib.SMPL_POSE_BASIS, _lib.SMPL_BETAS, _lib.SMPL_PARAMS


def _dense(a, dtype):
    """body_model.py:16-19: a scipy.sparse matrix (the pickle's J_regressor) or anything array-like -> ndarray."""
    if hasattr(a, "todense"):
        a = a.todense()
    return np.array(a, dtype=dtype)


class SmplModel:
    """The SMPL model's arrays on a device, laid out for nb_smpl_pose (include/nb_hip.h: nb_smpl_model), uploaded once."""

    def __init__(self, host, parents, device="cuda:0"):
        """`host`: the float32 arrays of `host_arrays`; use from_arrays / from_pkl."""
        self.device = torch.device(device)
        self.parents = [int(p) for p in parents]
        self.n_verts = int(host["v_template"].shape[0])
        self.host = host
        self._dev = None  # made on first use: constructing the model touches no device

    @staticmethod
    def host_arrays(arrays):
        """The pickle's arrays -> (dict of float32 arrays in the kernels' layout, parents).  ValueError for what cannot be skinned
        here: a joint count other than 24, a pose basis other than 207, shapes that do not fit one another."""
        v_template = _dense(arrays["v_template"], np.float32)
        if v_template.ndim != 2 or v_template.shape[1] != 3 or v_template.shape[0] < 1:
            raise ValueError("v_template must be [V,3] with V >= 1, got %s" % (v_template.shape,))
        V = v_template.shape[0]
        weights = _dense(arrays["weights"], np.float32)
        J_regressor = _dense(arrays["J_regressor"], np.float64)
        if "parents" in arrays:
            parents = [int(p) for p in np.asarray(arrays["parents"]).reshape(-1)]
        else:
            parents = [int(p) for p in np.asarray(arrays["kintree_table"])[0]]
        n_joints = {"weights": weights.shape[-1], "J_regressor": J_regressor.shape[0], "parents": len(parents)}
        if set(n_joints.values()) != {N_JOINTS}:
            raise ValueError("the kernels skin %d joints (SMPL); this model has %s (SMPL-H / SMPL-X bodies are not built)" % (
                N_JOINTS, ", ".join("%s: %d" % kv for kv in sorted(n_joints.items()))))
        if weights.shape != (V, N_JOINTS) or J_regressor.shape != (N_JOINTS, V):
            raise ValueError("weights %s and J_regressor %s do not fit %d vertices" % (weights.shape, J_regressor.shape, V))
        row_sums = weights.astype(np.float64).sum(axis=1)
        if np.abs(row_sums - 1.0).max() > 1e-6:  # float32 rounding of a normalised row; beyond it the blend would leave lbs.py
            raise ValueError("the skinning weights of a vertex must sum to 1 (nb_smpl_pose blends the transforms' differences from "
                             "the identity); row sums span %.6f .. %.6f" % (row_sums.min(), row_sums.max()))
        parents[0] = -1  # body_model.py:60 (the pickle holds 2^32 - 1 there)
        if any(not 0 <= p < j for j, p in enumerate(parents) if j > 0):
            raise ValueError("parents[j] must lie in 0 .. j - 1 (a parent before its child), got %s" % (parents,))
        shapedirs = _dense(arrays["shapedirs"], np.float32)
        if shapedirs.ndim != 3 or shapedirs.shape[:2] != (V, 3) or shapedirs.shape[2] < N_BETAS:
            raise ValueError("shapedirs must be [V,3,>=%d], got %s" % (N_BETAS, shapedirs.shape))
        shapedirs = shapedirs[:, :, :N_BETAS]  # shapes [10]: the first ten components, as the [.., 10] einsum of lbs.py:276 needs
        posedirs = _dense(arrays["posedirs"], np.float32)
        if posedirs.shape == (V, 3, N_POSE_BASIS):
            posedirs = posedirs.reshape(3 * V, N_POSE_BASIS).T  # body_model.py:51
        elif posedirs.shape != (N_POSE_BASIS, 3 * V):
            raise ValueError("posedirs must be [V,3,%d] or [%d,3V]: the pose feature is the %d rotation matrices below the root; "
                             "got %s" % (N_POSE_BASIS, N_POSE_BASIS, N_JOINTS - 1, posedirs.shape))
        # J = J_regressor . (v_template + shapedirs . beta) = j_template + j_shapedirs . beta: the regression over V moves here,
        # in float64, rounded once
        j_template = J_regressor @ v_template.astype(np.float64)
        j_shapedirs = np.einsum("jv,vkl->jkl", J_regressor, shapedirs.astype(np.float64))
        host = {"v_template": v_template, "shapedirs": np.ascontiguousarray(shapedirs.reshape(3 * V, N_BETAS).T),
                "posedirs": np.ascontiguousarray(posedirs), "weights": np.ascontiguousarray(weights.T),
                "j_template": j_template.astype(np.float32), "j_shapedirs": j_shapedirs.astype(np.float32)}
        return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in host.items()}, parents

    @classmethod
    def from_arrays(cls, arrays, device="cuda:0"):
        """`arrays`: v_template [V,3], shapedirs [V,3,10], posedirs [V,3,207] or [207,3V], J_regressor [24,V] (dense, or anything
        with .todense()), weights [V,24], and kintree_table [2,24] or parents [24]."""
        host, parents = cls.host_arrays(arrays)
        return cls(host, parents, device)

    @classmethod
    def from_pkl(cls, path, device="cuda:0"):
        """An SMPL_{NEUTRAL,MALE,FEMALE}.pkl as body_model.py:41-42 opens it (unpickling one needs chumpy and scipy importable)."""
        with open(path, "rb") as f:
            data = pickle.load(f, encoding="latin1")
        return cls.from_arrays(data, device)

    def native(self):
        """(NbSmplModel, device tensors): the upload happens on the first call."""
        if self._dev is None:
            if self.device.type != "cuda":
                raise ops.NbError("the SMPL model must live on a HIP device (got %s); the HIP path has no CPU fallback" % (self.device,))
            tensors = {k: torch.from_numpy(v).to(self.device) for k, v in self.host.items()}
            self._dev = ops.make_smpl_model(tensors, self.parents) + (tensors,)
        return self._dev[0], self._dev[2]


def pack_params(poses, shapes, Rh, Th, pin=False):
    """poses [F,72] (or [72]), shapes [F,10] or [1,10] (shared, body_model.py:119-120), Rh, Th [F,3] -> one float32 host tensor
    [F,88], the row layout nb_smpl_pose reads."""
    poses = np.asarray(poses, np.float32).reshape(-1, 72)
    F = poses.shape[0]
    shapes = np.asarray(shapes, np.float32).reshape(-1, N_BETAS)
    Rh, Th = np.asarray(Rh, np.float32).reshape(-1, 3), np.asarray(Th, np.float32).reshape(-1, 3)
    if F < 1 or shapes.shape[0] not in (1, F) or Rh.shape[0] != F or Th.shape[0] != F:
        raise ValueError("poses %s, shapes %s, Rh %s, Th %s do not describe the same frames" % (poses.shape, shapes.shape, Rh.shape,
                                                                                              Th.shape))
    out = torch.empty((F, N_PARAMS), dtype=torch.float32, pin_memory=pin)
    host = out.numpy()
    host[:, :72], host[:, 72:82], host[:, 82:85], host[:, 85:88] = poses, shapes, Rh, Th
    return out


class PoseDriver:
    """Frames of a body from its SMPL parameters.  `voxel_size`: cfg.voxel_size (three Python floats, dhw); `pad`: 'zju'
    (z -+ 0.05, the light-stage datasets), 'big_box' (cfg.big_box) or 'snapshot' (y -+ 0.1, People-Snapshot)."""

    def __init__(self, model, voxel_size=(0.005, 0.005, 0.005), pad="zju", device=None):
        if pad not in _lib.PAD_MODES:
            raise ValueError("pad must be one of %s, got %r" % (sorted(_lib.PAD_MODES), pad))
        self.model, self.pad = model, pad
        self.voxel_size = tuple(float(v) for v in voxel_size)
        if len(self.voxel_size) != 3 or not all(0.0 < v < float("inf") for v in self.voxel_size):
            raise ValueError("voxel_size must be three positive floats, got %r" % (voxel_size,))
        self.device = torch.device(device) if device is not None else model.device
        if self.device != model.device:
            raise ValueError("the driver's device %s is not the model's %s" % (self.device, model.device))

    def _upload(self, poses, shapes, Rh, Th, latent_index=None):
        """One pinned buffer, one copy: the [F,88] parameter rows and, behind them, F int64 latent indices -> (params [F,88]
        fp32, latent [F] int64 or None), views of the one device buffer."""
        rows = pack_params(poses, shapes, Rh, Th)
        F = int(rows.shape[0])
        n_par = F * N_PARAMS * 4  # a multiple of 8: the int64 section is aligned
        host = torch.empty(n_par + (8 * F if latent_index is not None else 0), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        host[:n_par].view(torch.float32).view(F, N_PARAMS).copy_(rows)
        if latent_index is not None:
            lat = np.broadcast_to(np.asarray(latent_index, np.int64).reshape(-1), (F,))
            host[n_par:].view(torch.int64).copy_(torch.from_numpy(np.array(lat)))
        dev = host.to(self.device, non_blocking=True)
        return dev[:n_par].view(torch.float32).view(F, N_PARAMS), (dev[n_par:].view(torch.int64) if latent_index is not None else None)

    def _on_device(self):
        """The calls below enqueue on the current stream of the driver's device, whichever device is current for the caller."""
        if self.device.type != "cuda":
            raise ops.NbError("the driver must live on a HIP device (got %s); the HIP path has no CPU fallback" % (self.device,))
        return torch.cuda.device(self.device)

    def vertices(self, poses, shapes, Rh, Th, new_params=False):
        """-> world vertices, a device fp32 [F,V,3]; nothing is read back."""
        with self._on_device():
            native, _ = self.model.native()
            return ops.smpl_pose(native, self._upload(poses, shapes, Rh, Th)[0], new_params)[0]

    def frames(self, poses, shapes, Rh, Th, latent_index, new_params=False):
        """-> [(frame, can_bounds)] * F.  `frame`: device tensors coord [1,V,3] i32, out_sh [1,3] i32, bounds [1,2,3], R [1,3,3],
        Th [1,1,3], latent_index [1] (views of the call's [F,...] tensors); `can_bounds`: float32 [2,3] on the host, what
        nb_raygen needs of the frame.  One upload, three launches, one wait: for the event behind the summary's copy."""
        with self._on_device():
            native, _ = self.model.native()
            params, latent = self._upload(poses, shapes, Rh, Th, latent_index)
            F = int(params.shape[0])
            verts, _ = ops.smpl_pose(native, params, new_params)
            vox = ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], self.voxel_size, self.pad)
            summary = torch.empty((F, 9), dtype=torch.int32, pin_memory=True)
            summary.copy_(vox["summary"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()  # the copy and what it depends on; nothing enqueued by anyone after this point
        s = summary.numpy()
        out = []
        for f in range(F):
            frame = {"coord": vox["coord"][f:f + 1], "out_sh": vox["out_sh"][f:f + 1], "bounds": vox["bounds"][f:f + 1],
                     "R": vox["R"][f:f + 1], "Th": params[f:f + 1, None, 85:88], "latent_index": latent[f:f + 1]}
            out.append((frame, s[f, :6].copy().view(np.float32).reshape(2, 3)))
        return out

    def views(self, cameras, poses, shapes, Rh, Th, latent_index, new_params=False):
        """Generator of (K, RT, can_bounds, frame) for NovelViewRenderer.render_views.  `cameras`: a list of (K, RT) pairs, one per
        frame, or a list of ONE pair that every frame is seen by.  All frames are made by one call of `frames` before the
        first view is yielded."""
        cameras = list(cameras)
        if any(len(c) != 2 for c in cameras):
            raise ValueError("cameras must be a list of (K, RT) pairs")
        made = self.frames(poses, shapes, Rh, Th, latent_index, new_params)
        if len(cameras) not in (1, len(made)):
            raise ValueError("%d cameras for %d frames (one per frame, or one for all)" % (len(cameras), len(made)))
        for f, (frame, can_bounds) in enumerate(made):
            K, RT = cameras[f if len(cameras) > 1 else 0]
            yield K, RT, can_bounds, frame


# ------------------------------------------------------------------------------------------- dataset core
class PoseDataConfig:
    """The cfg keys the dataset core reads, plus the two of its own (`smpl_new_params`; the model comes in as an object)."""

    def __init__(self, begin_ith_frame=0, frame_interval=1, num_train_frame=1, voxel_size=(0.005, 0.005, 0.005), big_box=False,
                 smpl_new_params=False):
        self.begin_ith_frame, self.frame_interval, self.num_train_frame = int(begin_ith_frame), int(frame_interval), int(num_train_frame)
        self.voxel_size, self.big_box, self.smpl_new_params = tuple(voxel_size), bool(big_box), bool(smpl_new_params)


class MemoryPoseSource:
    """Frames already in memory: `items[i]` = dict(poses, shapes, Rh, Th), seen by one camera K [3,3], R [3,3], T [3] (metres)
    in an H x W image."""

    def __init__(self, items, K, R, T, H, W):
        self.items, self.n_items = list(items), len(items)
        self.K, self.R, self.T, self.H, self.W = K, R, T, int(H), int(W)

    def load(self, i):
        return self.items[i]


class LightStagePoseSource:
    """The file side, a thin restatement of lib/datasets/light_stage/multi_view_perform_dataset.py: the frame count (:29-34), the
    file number of a frame (:52-53), np.load of params/{i}.npy (:74-76), and the camera `view` of the annotations with the image
    reduced by `ratio` (:137-138, render_utils.py:29-50)."""

    def __init__(self, data_root, human, ann_file, view, begin_ith_frame, frame_interval, num_train_frame, H, W, ratio,
                 num_render_frame=-1, params="params"):
        self.data_root, self.human, self.params = data_root, human, params
        cams = np.load(ann_file, allow_pickle=True).item()["cams"]
        self.K = np.array(cams["K"][view], np.float64)
        self.K[:2] = self.K[:2] * ratio
        self.R = np.array(cams["R"][view], np.float64)
        self.T = np.array(cams["T"][view], np.float64).reshape(3) / 1000.0
        self.H, self.W = int(H * ratio), int(W * ratio)
        self.begin_ith_frame, self.frame_interval = int(begin_ith_frame), int(frame_interval)
        self.n_items = int(num_render_frame) if int(num_render_frame) > 0 else int(num_train_frame)

    def load(self, index):
        i = self.begin_ith_frame + index * self.frame_interval
        if self.human in ("CoreView_313", "CoreView_315"):
            i = i + 1
        return np.load(os.path.join(self.data_root, self.params, "{}.npy".format(i)), allow_pickle=True).item()


class PoseFrameDataset(torch.utils.data.Dataset):
    """Item i = frame begin_ith_frame + i * frame_interval, made from its SMPL parameters and seen by the source's camera: the
    batch dict Renderer.render consumes (before collation), all device tensors, with every pixel's ray from nb_raygen."""

    def __init__(self, source, model, cfg, device="cuda:0"):
        super().__init__()
        self.source, self.model, self.cfg = source, model, cfg
        self.device = torch.device(device)

    def __len__(self):
        return int(self.source.n_items)

    def latent_index(self, index):
        """multi_view_perform_dataset.py:131,162"""
        return min(int(index), self.cfg.num_train_frame - 1)

    def __getitem__(self, index):
        index = int(index)
        cfg, src = self.cfg, self.source
        p = src.load(index)
        driver = PoseDriver(self.model, cfg.voxel_size, "big_box" if cfg.big_box else "zju", self.device)
        (frame, can_bounds), = driver.frames(p["poses"], p["shapes"], p["Rh"], p["Th"], self.latent_index(index), cfg.smpl_new_params)
        ray_o, ray_d, near, far, mask, n_rays = ops.raygen(src.H, src.W, src.K, src.R, src.T, can_bounds, self.device)
        n = int(n_rays.item())
        ret = {"ray_o": ray_o[:n], "ray_d": ray_d[:n], "near": near[:n], "far": far[:n], "mask_at_box": mask.view(torch.bool),
               "coord": frame["coord"][0], "out_sh": frame["out_sh"][0], "bounds": frame["bounds"][0], "R": frame["R"][0],
               "Th": frame["Th"][0], "latent_index": frame["latent_index"][0],
               "frame_index": cfg.begin_ith_frame + index * cfg.frame_interval}
        return ret
