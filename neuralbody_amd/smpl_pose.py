"""Pose-driven frames on the device: what the reference does offline (zju_smpl/extract_vertices.py: SMPLlayer.forward over lbs,
one vertices/{i}.npy per frame) and then per item on the host (prepare_input of lib/datasets/light_stage/multi_view_dataset.py:
68-118) with the SMPL model resident on the device and the frame made there from its parameters:

    host (per call)                                  device (HIP, three launches for all frames of the call)
    poses | shapes | Rh | Th, one pinned [F,88] -->  nb_smpl_pose (chain, vertices) -> nb_smpl_voxelize --> frame tensors
    can_bounds, out_sh                          <--  summary [F,9], one pinned copy behind an event

A frame is the dict NovelViewRenderer.view_batch documents, so `PoseDriver.views` feeds NovelViewRenderer.render_views as a
turntable's views do, and a frame change uploads 88 floats instead of the frame's coordinates from pageable memory.

With `cull_cameras` a frame also carries the keys RendererMmsk culls by (msks, Ks, RT): the posed triangles rasterised into those
cameras (nb_smpl_silhouette, enqueued with the launches above) and dilated by a clothing margin (nb_mask_dilate, one launch per
frame once the summary has told the host how near the body is), in place of the masks of photographs
(multi_view_perform_dataset.py:105-127) a pose that was never photographed does not have.
"""
import math
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

    def __init__(self, host, parents, device="cuda:0", faces=None):
        """`host`: the float32 arrays of `host_arrays`, `faces`: the int32 [Nf,3] of `host_faces` or None; use from_arrays /
        from_pkl."""
        self.device = torch.device(device)
        self.parents = [int(p) for p in parents]
        self.n_verts = int(host["v_template"].shape[0])
        self.host = host
        self.faces = faces
        self._dev = None  # made on first use: constructing the model touches no device

    @staticmethod
    def host_faces(arrays, n_verts):
        """The triangle list of the pickle's arrays (`f`, or `faces`) -> a contiguous int32 [Nf,3], or None when they hold none.
        ValueError for a shape other than [Nf,3] with Nf >= 1, or an index outside 0 .. n_verts - 1: the rasteriser trusts it."""
        key = "f" if "f" in arrays else "faces" if "faces" in arrays else None
        if key is None or arrays[key] is None:
            return None
        f = np.asarray(arrays[key])
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
            raise ValueError("the triangle list %r must be integers [Nf,3] with Nf >= 1, got %s %s" % (key, f.dtype, f.shape))
        f = f.astype(np.int64)
        if int(f.min()) < 0 or int(f.max()) >= n_verts:
            raise ValueError("the triangle list %r indexes vertices %d .. %d; the model has 0 .. %d" % (key, int(f.min()), int(f.max()),
                                                                                                   n_verts - 1))
        return np.ascontiguousarray(f, dtype=np.int32)

    @staticmethod
    def host_arrays(arrays):
        """The pickle's arrays -> (dict of float32 arrays in the kernels' layout, parents); see _host_arrays."""
        return SmplModel._host_arrays(arrays)[:2]

    @staticmethod
    def _host_arrays(arrays):
        """The pickle's arrays -> (dict of float32 arrays in the kernels' layout, parents, faces int32 [Nf,3] or None).  ValueError for what cannot be skinned
        here: a joint count other than 24, a pose basis other than 207, shapes that do not fit one another, a triangle list
        (`host_faces`; from_arrays keeps it beside these arrays) that does not index the vertices."""
        v_template = _dense(arrays["v_template"], np.float32)
        if v_template.ndim != 2 or v_template.shape[1] != 3 or v_template.shape[0] < 1:
            raise ValueError("v_template must be [V,3] with V >= 1, got %s" % (v_template.shape,))
        V = v_template.shape[0]
        faces = SmplModel.host_faces(arrays, V)
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
        return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in host.items()}, parents, faces

    @classmethod
    def from_arrays(cls, arrays, device="cuda:0"):
        """`arrays`: v_template [V,3], shapedirs [V,3,10], posedirs [V,3,207] or [207,3V], J_regressor [24,V] (dense, or anything
        with .todense()), weights [V,24], kintree_table [2,24] or parents [24], and optionally the triangles f (or faces) [Nf,3]."""
        host, parents, faces = cls._host_arrays(arrays)
        return cls(host, parents, device, faces)

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
            if self.faces is not None:
                tensors["faces"] = torch.from_numpy(self.faces).to(self.device)
            self._dev = ops.make_smpl_model(tensors, self.parents) + (tensors,)
        return self._dev[0], self._dev[2]

    def faces_device(self):
        """The triangle list on the device, int32 [Nf,3], uploaded with the model."""
        if self.faces is None:
            raise ops.NbError("the SMPL model has no triangle list (no 'f' or 'faces' among its arrays): silhouettes need one")
        return self.native()[1]["faces"]


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


def cull_camera_arrays(cull_cameras):
    """cull_cameras = (Ks [nv,3,3], RTs [nv,3,4] or [nv,4,4], H, W) -> (Ks, RTs [nv,3,4]) float64 on the host, H, W."""
    if len(cull_cameras) != 4:
        raise ValueError("cull_cameras must be (Ks [nv,3,3], RTs [nv,3,4] or [nv,4,4], H, W)")
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a  # noqa: E731
    Ks, RTs = np.asarray(as_np(cull_cameras[0]), np.float64), np.asarray(as_np(cull_cameras[1]), np.float64)
    H, W = int(cull_cameras[2]), int(cull_cameras[3])
    nv = Ks.shape[0] if Ks.ndim == 3 else 0
    if not 1 <= nv <= 64 or Ks.shape != (nv, 3, 3) or RTs.shape not in ((nv, 3, 4), (nv, 4, 4)):
        raise ValueError("cull_cameras: Ks %s, RTs %s (1..64 views, [nv,3,3] and [nv,3,4] or [nv,4,4])" % (Ks.shape, RTs.shape))
    if H < 1 or W < 1:
        raise ValueError("cull_cameras: H = %d, W = %d" % (H, W))
    return Ks, np.ascontiguousarray(RTs[:, :3]), H, W


def cull_border(can_bounds, Ks, RTs, cull_margin=0.05):
    """The dilation that stands for `cull_margin` metres around the body, in pixels of the cull views: z_near = the smallest
    camera depth of the eight corners of `can_bounds` [2,3] over the views, px = ceil(margin * max(fx, fy) / (z_near - margin)) + 1
    (the + 1: the cull's round-to-nearest and its fp32 projection), border = 2 px + 1 -> border, odd, for nb_mask_dilate.
    ValueError when the box comes within the margin of a camera, or the border passes 255."""
    Ks, RTs = np.asarray(Ks, np.float64), np.asarray(RTs, np.float64)[:, :3]
    cb, margin = np.asarray(can_bounds, np.float64).reshape(2, 3), float(cull_margin)
    if not 0.0 <= margin < math.inf:
        raise ValueError("cull_margin = %r m must be a finite length >= 0" % (cull_margin,))
    corners = np.array([[cb[i, 0], cb[j, 1], cb[k, 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    depth = np.einsum("vk,ck->vc", RTs[:, 2, :3], corners) + RTs[:, 2, 3:4]  # [nv,8]
    view = int(np.argmin(depth.min(axis=1)))
    z_near = float(depth.min())
    if not z_near > margin:
        raise ValueError("cull_margin = %g m: the body's box comes within %.4f m of cull camera %d; no finite dilation covers the "
                         "margin" % (margin, z_near, view))
    focal = float(max(Ks[:, 0, 0].max(), Ks[:, 1, 1].max()))
    px = int(math.ceil(margin * focal / (z_near - margin))) + 1
    border = 2 * px + 1
    if border > 255:
        raise ValueError("cull_margin = %g m is %d pixels at cull camera %d (z_near %.4f m, focal %.1f px): border %d > 255, the "
                         "most nb_mask_dilate takes" % (margin, px, view, z_near, focal, border))
    return border


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

    def _upload(self, poses, shapes, Rh, Th, latent_index=None, cull=None):
        """One pinned buffer, one copy: the [F,88] parameter rows and, behind them, F int64 latent indices and the cull cameras
        (`cull`: the (Ks, RTs, H, W) of cull_camera_arrays) -> (params [F,88] fp32, latent [F] int64 or None, (RT [nv,3,4],
        K [nv,3,3]) fp32 or None), views of the one device buffer."""
        rows = pack_params(poses, shapes, Rh, Th)
        F = int(rows.shape[0])
        n_par = F * N_PARAMS * 4  # a multiple of 8: the int64 section is aligned
        n_lat = 8 * F if latent_index is not None else 0
        nv = 0 if cull is None else int(cull[0].shape[0])
        host = torch.empty(n_par + n_lat + 4 * 21 * nv, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        host[:n_par].view(torch.float32).view(F, N_PARAMS).copy_(rows)
        if latent_index is not None:
            lat = np.broadcast_to(np.asarray(latent_index, np.int64).reshape(-1), (F,))
            host[n_par:n_par + n_lat].view(torch.int64).copy_(torch.from_numpy(np.array(lat)))
        if nv:
            cam = np.concatenate([cull[1].reshape(-1), cull[0].reshape(-1)]).astype(np.float32)  # RT [nv,12], then K [nv,9]
            host[n_par + n_lat:].view(torch.float32).copy_(torch.from_numpy(cam))
        dev = host.to(self.device, non_blocking=True)
        cams = None
        if nv:
            c = dev[n_par + n_lat:].view(torch.float32)
            cams = (c[:12 * nv].view(nv, 3, 4), c[12 * nv:].view(nv, 3, 3))
        return (dev[:n_par].view(torch.float32).view(F, N_PARAMS), (dev[n_par:n_par + n_lat].view(torch.int64) if n_lat else None),
                cams)

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

    def silhouettes(self, verts, cull_cameras):
        """verts: device fp32 [F,V,3] (`vertices`), cull_cameras = (Ks [nv,3,3], RTs [nv,3,4] or [nv,4,4], H, W) -> the raw masks,
        device uint8 [F,nv,H,W]: 1 where a triangle of the posed body meets the pixel, before any dilation (nb_smpl_silhouette)."""
        Ks, RTs, H, W = cull_camera_arrays(cull_cameras)
        with self._on_device():
            faces = self.model.faces_device()
            cam = torch.from_numpy(np.concatenate([RTs.reshape(-1), Ks.reshape(-1)]).astype(np.float32))
            cam = (cam.pin_memory() if self.device.type == "cuda" else cam).to(self.device, non_blocking=True)
            nv = Ks.shape[0]
            return ops.smpl_silhouette(verts, faces, cam[:12 * nv].view(nv, 3, 4), cam[12 * nv:].view(nv, 3, 3), H, W)

    def frames(self, poses, shapes, Rh, Th, latent_index, new_params=False, cull_cameras=None, cull_margin=0.05, body=False):
        """-> [(frame, can_bounds)] * F.  `frame`: device tensors coord [1,V,3] i32, out_sh [1,3] i32, bounds [1,2,3], R [1,3,3],
        Th [1,1,3], latent_index [1] (views of the call's [F,...] tensors); `can_bounds`: float32 [2,3] on the host, what
        nb_raygen needs of the frame.  One upload, three launches, one wait: for the event behind the summary's copy.
        `cull_cameras` = (Ks [nv,3,3], RTs [nv,3,4] or [nv,4,4], H, W): every frame also holds msks [1,nv,H,W] uint8, Ks
        [1,nv,3,3] and RT [1,nv,3,4], the keys RendererMmsk.make_cull reads — the body's silhouettes in those cameras
        (`silhouettes`, enqueued behind the voxelisation, before the wait) dilated by `cull_margin` metres (`cull_border` of the
        frame's can_bounds; one nb_mask_dilate per frame after the wait, nothing else waits).
        `body`: every frame also holds body_verts [1,V,3] (a view of the posed world vertices, no copy) and body_faces [Nf,3]
        (the model's triangles): what ray_bounds.BodyBounds bounds a view's rays by (NovelViewRenderer(body_bounds=...))."""
        if not getattr(self.model, "has_codes", True):
            raise ops.NbError("frames are the network's input, and the network holds one latent code per vertex of the SMPL body "
                              "(6890); a %s of %d vertices is geometry only — pose it with `vertices`, draw it with mesh_rig.animate"
                              % (type(self.model).__name__, self.model.n_verts))
        cull = None if cull_cameras is None else cull_camera_arrays(cull_cameras)
        with self._on_device():
            faces = None if cull is None and not body else self.model.faces_device()  # refuses a model without triangles before any launch
            native, _ = self.model.native()
            params, latent, cams = self._upload(poses, shapes, Rh, Th, latent_index, cull)
            F = int(params.shape[0])
            verts, _ = ops.smpl_pose(native, params, new_params)
            vox = ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], self.voxel_size, self.pad)
            summary = torch.empty((F, 9), dtype=torch.int32, pin_memory=True)
            summary.copy_(vox["summary"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            raw = None if cull is None else ops.smpl_silhouette(verts, faces, cams[0], cams[1], cull[2], cull[3])
            ev.synchronize()  # the copy and what it depends on; nothing enqueued by anyone after this point
            s = summary.numpy()
            can_bounds = [s[f, :6].copy().view(np.float32).reshape(2, 3) for f in range(F)]
            if cull is not None:
                borders = [cull_border(cb, cull[0], cull[1], cull_margin) for cb in can_bounds]  # all checked before any launch
                msks = torch.empty_like(raw)
                for f in range(F):
                    ops.mask_dilate(raw[f], borders[f], out=msks[f])
        out = []
        for f in range(F):
            frame = {"coord": vox["coord"][f:f + 1], "out_sh": vox["out_sh"][f:f + 1], "bounds": vox["bounds"][f:f + 1],
                     "R": vox["R"][f:f + 1], "Th": params[f:f + 1, None, 85:88], "latent_index": latent[f:f + 1]}
            if cull is not None:
                frame.update(msks=msks[f:f + 1], Ks=cams[1][None], RT=cams[0][None])
            if body:
                frame.update(body_verts=verts[f:f + 1], body_faces=faces)
            out.append((frame, can_bounds[f]))
        return out

    def views(self, cameras, poses, shapes, Rh, Th, latent_index, new_params=False, cull_cameras=None, cull_margin=0.05, body=False):
        """Generator of (K, RT, can_bounds, frame) for NovelViewRenderer.render_views.  `cameras`: a list of (K, RT) pairs, one per
        frame, or a list of ONE pair that every frame is seen by.  All frames are made by one call of `frames` before the
        first view is yielded.  `cull_cameras`, `cull_margin`, `body`: those of `frames`; the frames then feed a RendererMmsk, or a
        NovelViewRenderer with body_bounds."""
        cameras = list(cameras)
        if any(len(c) != 2 for c in cameras):
            raise ValueError("cameras must be a list of (K, RT) pairs")
        made = self.frames(poses, shapes, Rh, Th, latent_index, new_params, cull_cameras, cull_margin, body)
        if len(cameras) not in (1, len(made)):
            raise ValueError("%d cameras for %d frames (one per frame, or one for all)" % (len(cameras), len(made)))
        for f, (frame, can_bounds) in enumerate(made):
            K, RT = cameras[f if len(cameras) > 1 else 0]
            yield K, RT, can_bounds, frame


# ------------------------------------------------------------------------------------------- dataset core
class PoseDataConfig:
    """The cfg keys the dataset core reads, plus its own (`smpl_new_params`; `cull_views`, the camera indices of the annotations
    whose silhouettes cull the items, empty = none; `cull_margin` in metres; `ray_bounds`: 'box' (nb_raygen) or 'body' (the rays cut
    to the posed body's depth range, ray_bounds.BodyBounds, with `ray_bounds_margin` metres and `ray_bounds_tile` pixels; the model
    comes in as an object)."""

    def __init__(self, begin_ith_frame=0, frame_interval=1, num_train_frame=1, voxel_size=(0.005, 0.005, 0.005), big_box=False,
                 smpl_new_params=False, cull_views=(), cull_margin=0.05, ray_bounds="box", ray_bounds_margin=0.05, ray_bounds_tile=8):
        self.begin_ith_frame, self.frame_interval, self.num_train_frame = int(begin_ith_frame), int(frame_interval), int(num_train_frame)
        self.voxel_size, self.big_box, self.smpl_new_params = tuple(voxel_size), bool(big_box), bool(smpl_new_params)
        self.cull_views, self.cull_margin = tuple(int(v) for v in cull_views), float(cull_margin)
        self.ray_bounds, self.ray_bounds_margin, self.ray_bounds_tile = ray_bounds_mode(ray_bounds), float(ray_bounds_margin), int(ray_bounds_tile)


def ray_bounds_mode(name):
    """The YAML key `ray_bounds`: 'box' or 'body'."""
    if name not in ("box", "body"):
        raise ValueError("ray_bounds must be 'box' or 'body', got %r" % (name,))
    return name


class MemoryPoseSource:
    """Frames already in memory: `items[i]` = dict(poses, shapes, Rh, Th), seen by one camera K [3,3], R [3,3], T [3] (metres)
    in an H x W image.  `cull_cameras`: optionally the (Ks, RTs, H, W) of every camera cfg.cull_views may name."""

    def __init__(self, items, K, R, T, H, W, cull_cameras=None):
        self.items, self.n_items = list(items), len(items)
        self.K, self.R, self.T, self.H, self.W = K, R, T, int(H), int(W)
        self.cull = cull_cameras

    def load(self, i):
        return self.items[i]

    def cull_cameras(self, views):
        if self.cull is None:
            raise ValueError("cull_views %s: this source was given no cull_cameras" % (list(views),))
        Ks, RTs, H, W = cull_camera_arrays(self.cull)
        views = [int(v) for v in views]
        return Ks[views], RTs[views], H, W


class LightStagePoseSource:
    """The file side, a thin restatement of lib/datasets/light_stage/multi_view_perform_dataset.py: the frame count (:29-34), the
    file number of a frame (:52-53), np.load of params/{i}.npy (:74-76), and the camera `view` of the annotations with the image
    reduced by `ratio` (:137-138, render_utils.py:29-50)."""

    def __init__(self, data_root, human, ann_file, view, begin_ith_frame, frame_interval, num_train_frame, H, W, ratio,
                 num_render_frame=-1, params="params"):
        self.data_root, self.human, self.params = data_root, human, params
        cams = np.load(ann_file, allow_pickle=True).item()["cams"]
        self._cams, self._ratio = cams, ratio
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

    def cull_cameras(self, views):
        """The cameras `views` of the annotations as render_utils.load_cam makes them (render_utils.py:37-48: K[:2] * ratio,
        T / 1000) -> (Ks [nv,3,3], RTs [nv,3,4], H, W) at the reduced image size."""
        Ks, RTs = [], []
        for v in views:
            K = np.array(self._cams["K"][int(v)], np.float64)
            K[:2] = K[:2] * self._ratio
            Ks.append(K)
            RTs.append(np.concatenate([np.array(self._cams["R"][int(v)], np.float64),
                                       np.array(self._cams["T"][int(v)], np.float64).reshape(3, 1) / 1000.0], axis=1))
        return np.stack(Ks), np.stack(RTs), self.H, self.W


class PoseFrameDataset(torch.utils.data.Dataset):
    """Item i = frame begin_ith_frame + i * frame_interval, made from its SMPL parameters and seen by the source's camera: the
    batch dict Renderer.render consumes (before collation), all device tensors, with every pixel's ray from nb_raygen.  With
    cfg.cull_views the item also holds msks [nv,H,W], Ks [nv,3,3], RT [nv,3,4]: what RendererMmsk culls by.  With cfg.ray_bounds
    'body' the rays, near / far and mask_at_box are those of ray_bounds.BodyBounds: cut to the posed body's depth range."""

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
        cull_views = tuple(getattr(cfg, "cull_views", ()))
        cull = src.cull_cameras(cull_views) if cull_views else None
        body = ray_bounds_mode(getattr(cfg, "ray_bounds", "box")) == "body"
        (frame, can_bounds), = driver.frames(p["poses"], p["shapes"], p["Rh"], p["Th"], self.latent_index(index), cfg.smpl_new_params,
                                             cull, float(getattr(cfg, "cull_margin", 0.05)), body)
        if body:
            from .ray_bounds import BodyBounds

            RT = np.concatenate([np.asarray(src.R, np.float64).reshape(3, 3), np.asarray(src.T, np.float64).reshape(3, 1)], axis=1)
            bounds = BodyBounds(float(getattr(cfg, "ray_bounds_margin", 0.05)), int(getattr(cfg, "ray_bounds_tile", 8)))
            ray_o, ray_d, near, far, mask, n_rays = bounds.rays(src.H, src.W, src.K, RT, can_bounds, frame["body_verts"],
                                                                frame["body_faces"], self.device)
        else:
            ray_o, ray_d, near, far, mask, n_rays = ops.raygen(src.H, src.W, src.K, src.R, src.T, can_bounds, self.device)
        n = int(n_rays.item())
        ret = {"ray_o": ray_o[:n], "ray_d": ray_d[:n], "near": near[:n], "far": far[:n], "mask_at_box": mask.view(torch.bool),
               "coord": frame["coord"][0], "out_sh": frame["out_sh"][0], "bounds": frame["bounds"][0], "R": frame["R"][0],
               "Th": frame["Th"][0], "latent_index": frame["latent_index"][0],
               "frame_index": cfg.begin_ith_frame + index * cfg.frame_interval}
        if cull is not None:
            ret.update(msks=frame["msks"][0], Ks=frame["Ks"][0], RT=frame["RT"][0])
        return ret
