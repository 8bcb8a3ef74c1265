"""test_dataset_path / train_dataset_path plugin of the mesh pass: `Dataset(data_root, human, ann_file, split)` bound to the
reference's global cfg (lib/datasets/make_dataset.py:13-23; lib/datasets/light_stage/multi_view_mesh_dataset.py reads
cfg.begin_ith_frame / num_train_frame / num_render_frame :26-29, training_view :31-43, vertices / params :52,69, big_box :60,
voxel_size :92,150).  The lattice is carved on the device (neuralbody_amd/mesh_lattice.py) and the batch carries its three axes
instead of `pts`, so it runs in the visualising process.  The reference's mesh overlay (lib/config/config.py, `mesh_cfg`) names
the dataset module for both splits; select this file for both with

    test_dataset_path /path/to/neuralbody_amd/plugins/light_stage_mesh_dataset.py \
        train_dataset_path /path/to/neuralbody_amd/plugins/light_stage_mesh_dataset.py train.num_workers 0 test.batch_size 1
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.image_prep import select_prep  # noqa: E402
from neuralbody_amd.mesh_lattice import LightStageMeshSource, MeshLatticeDataset  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time."""

    begin_ith_frame = property(lambda self: int(cfg.begin_ith_frame))
    num_train_frame = property(lambda self: int(cfg.num_train_frame))
    voxel_size = property(lambda self: tuple(cfg.voxel_size))
    big_box = property(lambda self: bool(cfg.big_box))
    # not a reference key: YAML only (the reference's command line refuses keys its config.py does not define)
    mesh_lattice_pts = property(lambda self: bool(getattr(cfg, "mesh_lattice_pts", False)))


def disk_source(data_root, human, ann_file, device="cuda:0"):
    """`image_prep` is not a reference key (YAML only): 'cv2' undistorts the masks with OpenCV on the host as the reference does,
    'device' with neuralbody_amd/image_prep.py, 'auto' (the default) with cv2 where it imports and on the device elsewhere."""
    return LightStageMeshSource(
        data_root, human, ann_file, training_view=list(cfg.training_view), begin_ith_frame=int(cfg.begin_ith_frame),
        num_train_frame=int(cfg.num_train_frame), num_render_frame=int(getattr(cfg, "num_render_frame", -1)),
        vertices=getattr(cfg, "vertices", "vertices"), params=getattr(cfg, "params", "params"),
        prep=select_prep(str(getattr(cfg, "image_prep", "auto")), device))


def _require_in_process():
    """The items are device tensors made on the current stream: no worker processes, and one lattice per batch."""
    for split in ("train", "test"):
        node = getattr(cfg, split, None)
        if node is not None and int(getattr(node, "num_workers", 0)) != 0:
            raise ValueError("light_stage_mesh_dataset: %s.num_workers must be 0 (the items are device tensors)" % split)
    node = getattr(cfg, "test", None)
    if node is not None and int(getattr(node, "batch_size", 1)) != 1:
        raise ValueError("light_stage_mesh_dataset: test.batch_size must be 1 (one lattice per batch)")


class Dataset(MeshLatticeDataset):
    def __init__(self, data_root, human, ann_file, split, source=None, device="cuda:0"):
        """`source`: a frame source to use instead of the files under `data_root` (tests)."""
        _require_in_process()
        super().__init__(source if source is not None else disk_source(data_root, human, ann_file, device), _LiveCfg(), device=device)
        self.data_root, self.human, self.split = data_root, human, split
