"""The mesh pass's query lattice on the device: what lib/datasets/light_stage/multi_view_mesh_dataset.py does per item on the
host (a float64 meshgrid of the whole world box, every point projected into every training view in numpy, a 5 x 5 cv2.dilate
per view) with three axis vectors and the raw masks uploaded and the rest done there:

    host (numpy, per frame)                         device (HIP, per item)
    multi_view_frame, lattice_axes, frame source -> nb_mask_dilate -> nb_lattice_carve -> the reference's dict as device tensors

`pts` [X,Y,Z,3] is never built: a lattice point is (axis_x[i], axis_y[j], axis_z[k]), and RendererMesh.density_cube takes a
batch that carries the axes through nb_lattice_gather / nb_lattice_scatter.  `MeshLatticeDataset` is the cfg-free core of the
`test_dataset_path` plugin (plugins/light_stage_mesh_dataset.py); it runs in the visualising process (`train.num_workers 0`).
"""
import os

import numpy as np
import torch

from . import ops
from .train_rays import MemoryFrameSource, multi_view_frame

BORDER = 5  # multi_view_mesh_dataset.py:111


def lattice_axes(can_bounds, voxel_size):
    """multi_view_mesh_dataset.py:150-156,158: the three axes of the lattice over the world box, as the reference forms them —
    np.arange(lo, hi + step, step) on the float32 bounds and the Python-float steps of cfg.voxel_size — rounded to float32 as
    `pts.astype(np.float32)` rounds every coordinate.  -> [x [X], y [Y], z [Z]] float32."""
    can_bounds = np.asarray(can_bounds)
    if can_bounds.shape != (2, 3) or can_bounds.dtype != np.float32:
        raise ValueError("can_bounds must be float32 [2,3] (prepare_input's), got %s %s" % (can_bounds.dtype, can_bounds.shape))
    axes = []
    for a in range(3):
        step = float(voxel_size[a])
        if not step > 0.0:
            raise ValueError("voxel_size[%d] = %r" % (a, voxel_size[a]))
        axes.append(np.arange(can_bounds[0, a], can_bounds[1, a] + step, step).astype(np.float32))
    return axes


class MeshLatticeConfig:
    """The cfg keys the dataset core reads (multi_view_mesh_dataset.py:26,60,92,145,150,170) and `mesh_lattice_pts`."""

    def __init__(self, begin_ith_frame=0, num_train_frame=1, voxel_size=(0.005, 0.005, 0.005), big_box=False,
                 mesh_lattice_pts=False):
        self.begin_ith_frame, self.num_train_frame = int(begin_ith_frame), int(num_train_frame)
        self.voxel_size, self.big_box = tuple(voxel_size), bool(big_box)
        self.mesh_lattice_pts = bool(mesh_lattice_pts)  # also return `pts` [X,Y,Z,3] (12 bytes per lattice point)


class MemoryMeshSource(MemoryFrameSource):
    """Frames already in memory: `items[i]` = (msks, xyz, Rh, Th), with the training views' cameras."""

    def __init__(self, items, Ks, Rs, Ts):
        super().__init__(items)
        self.Ks, self.Rs, self.Ts = Ks, Rs, Ts


class MeshLatticeDataset(torch.utils.data.Dataset):
    """lib/datasets/light_stage/multi_view_mesh_dataset.py::Dataset with the per-item work on the device.

    `source`: an object with `n_items`, the training views' cameras `Ks` [V,3,3], `Rs` [V,3,3], `Ts` [V,3,1] (metres) and
    `load(index) -> (msks u8 [V,H,W], xyz [N,3], Rh, Th)`: item `index`'s raw masks (non-zero = body, undistorted, NOT
    dilated) and its frame's world vertices and SMPL placement.  Every item's tensors are made afresh: nothing of a frame
    is kept, so two items never share a bitmap."""

    def __init__(self, source, cfg, device="cuda:0"):
        super().__init__()
        self.source, self.cfg = source, cfg
        self.device = torch.device(device)
        self._cams = None
        self._scratch = (None, None)  # (dims, scratch): depends on the lattice's size only, reused in stream order

    def __len__(self):
        return int(self.source.n_items)

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor) and a.is_cuda:  # a source with a DeviceImagePrep: already where it belongs
            return a
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def _cameras(self):
        if self._cams is None:
            Ks = np.asarray(self.source.Ks, np.float32).reshape(-1, 3, 3)
            Rs = np.asarray(self.source.Rs, np.float32).reshape(-1, 3, 3)
            Ts = np.asarray(self.source.Ts, np.float32).reshape(-1, 3, 1)
            RT = np.concatenate([Rs, Ts], axis=2)  # multi_view_mesh_dataset.py:126
            self._cams = (self._dev(RT, np.float32), self._dev(Ks, np.float32))
        return self._cams

    def host_item(self, index):
        """The host side of item `index`, nothing touches a device: the reference's dict entries that prepare_input makes
        (numpy, multi_view_mesh_dataset.py:147-148,162-178), the three axes and the raw masks [V,H,W] uint8."""
        index = int(index)
        cfg = self.cfg
        msks, xyz, Rh, Th = self.source.load(index)
        fr = multi_view_frame(xyz, Rh, Th, cfg.voxel_size, cfg.big_box)
        axes = lattice_axes(fr["can_bounds"], cfg.voxel_size)
        if not isinstance(msks, torch.Tensor):  # a device tensor: a source with a DeviceImagePrep made it there
            msks = np.ascontiguousarray(msks, dtype=np.uint8)
        n_views = np.asarray(self.source.Ks).reshape(-1, 3, 3).shape[0]
        if msks.ndim != 3 or msks.shape[0] != n_views:
            raise ValueError("item %d: masks %s for %d views" % (index, tuple(msks.shape), n_views))
        return {"coord": fr["coord"], "out_sh": fr["out_sh"], "wbounds": fr["can_bounds"], "bounds": fr["bounds"], "R": fr["R"],
                "Th": fr["Th"], "latent_index": min(index, cfg.num_train_frame - 1), "frame_index": index + cfg.begin_ith_frame,
                "axis_x": axes[0], "axis_y": axes[1], "axis_z": axes[2], "msks": msks}

    def __getitem__(self, index):
        host = self.host_item(index)
        axes = [self._dev(host[k], np.float32) for k in ("axis_x", "axis_y", "axis_z")]
        dims = [int(a.shape[0]) for a in axes]
        RT, Ks = self._cameras()
        dilated = ops.mask_dilate(self._dev(host["msks"], np.uint8), BORDER)
        cull, keep = ops.make_cull(dilated, RT, Ks)
        if self._scratch[0] != dims:
            self._scratch = (dims, ops.lattice_scratch(dims, self.device))
        inside, _ = ops.lattice_carve(axes, cull, scratch=self._scratch[1])
        del keep  # enqueued: the caching allocator reuses the masks' memory in stream order
        ret = {"coord": self._dev(host["coord"], np.int32), "out_sh": self._dev(host["out_sh"], np.int32), "inside": inside,
               "axis_x": axes[0], "axis_y": axes[1], "axis_z": axes[2],
               "wbounds": self._dev(host["wbounds"], np.float32), "bounds": self._dev(host["bounds"], np.float32),
               "R": self._dev(host["R"], np.float32), "Th": self._dev(host["Th"], np.float32),
               "latent_index": torch.tensor(host["latent_index"], dtype=torch.int64, device=self.device),
               "frame_index": host["frame_index"]}
        if self.cfg.mesh_lattice_pts:
            ret["pts"] = torch.stack(torch.meshgrid(axes[0], axes[1], axes[2], indexing="ij"), dim=-1)
        return ret


# ------------------------------------------------------------------------------------------- disk source
class LightStageMeshSource:
    """The file side of lib/datasets/light_stage/multi_view_mesh_dataset.py, a thin restatement: the frame list and cameras
    (:22-45), the file number of a frame (:48-49), the two np.load calls of prepare_input (:52-54, :69-74) and get_mask
    without its dilation (:102-109).  imageio and cv2 are imported on first use.  `prep`: an image_prep.DeviceImagePrep to
    undistort a frame's masks on the device instead (load() then returns them as one device tensor, and cv2 is never
    imported); None keeps the cv2 lines."""

    def __init__(self, data_root, human, ann_file, training_view, begin_ith_frame, num_train_frame, num_render_frame=-1,
                 vertices="vertices", params="params", prep=None):
        self.prep = prep
        self.data_root, self.human = data_root, human
        annots = np.load(ann_file, allow_pickle=True).item()
        cams = annots["cams"]
        self.begin_ith_frame = int(begin_ith_frame)
        ni = int(num_render_frame) if int(num_render_frame) > 0 else int(num_train_frame)
        i = self.begin_ith_frame
        self.ims = np.array([np.array(d["ims"])[list(training_view)] for d in annots["ims"][i:i + ni]])
        self.Ks = np.array(cams["K"])[list(training_view)].astype(np.float32)
        self.Rs = np.array(cams["R"])[list(training_view)].astype(np.float32)
        self.Ts = np.array(cams["T"])[list(training_view)].astype(np.float32) / 1000.0
        self.Ds = np.array(cams["D"])[list(training_view)].astype(np.float32)
        self.n_items = ni
        self.vertices, self.params = vertices, params

    def get_mask(self, index, nv):
        import cv2
        import imageio

        msk_cihp = imageio.imread(os.path.join(self.data_root, "mask_cihp", self.ims[index, nv])[:-4] + ".png")
        msk = (msk_cihp != 0).astype(np.uint8)
        return cv2.undistort(msk, self.Ks[nv], self.Ds[nv])

    def load(self, index):
        i = index + self.begin_ith_frame
        if self.human in ("CoreView_313", "CoreView_315"):
            i = i + 1
        xyz = np.load(os.path.join(self.data_root, self.vertices, "{}.npy".format(i))).astype(np.float32)
        params = np.load(os.path.join(self.data_root, self.params, "{}.npy".format(i)), allow_pickle=True).item()
        if self.prep is None:
            msks = np.stack([self.get_mask(index, nv) for nv in range(self.ims.shape[1])])
        else:
            paths = [os.path.join(self.data_root, "mask_cihp", im)[:-4] + ".png" for im in self.ims[index]]
            msks = self.prep.masks(paths, self.Ks, self.Ds)
        return msks, xyz, params["Rh"], params["Th"]
