"""train_dataset_path / test_dataset_path plugin: `Dataset(data_root, human, ann_file, split)` bound to the reference's global
cfg (lib/datasets/make_dataset.py:13-23 builds it from cfg.train_dataset / cfg.test_dataset; lib/datasets/light_stage/
multi_view_dataset.py reads cfg.training_view :26, begin_ith_frame / frame_interval / num_train_frame :33-35, N_rand :52,
vertices / params :70,87, big_box :78, voxel_size :110, H / W :123, ratio :136, mask_bkgd / white_bkgd :139-142;
if_nerf_data_utils.py reads cfg.body_sample_ratio / face_sample_ratio :165-166).  The images and masks stay on the device and
each item's rays are drawn there (neuralbody_amd/train_rays.py), so it runs in the training process.  Select it with

    train_dataset_path /path/to/neuralbody_amd/plugins/light_stage_dataset.py \
        train_dataset_module lib.datasets.light_stage.multi_view_dataset train.num_workers 0
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.image_prep import select_prep  # noqa: E402
from neuralbody_amd.train_rays import LightStageFrameSource, TrainRayDataset  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time."""

    N_rand = property(lambda self: int(cfg.N_rand))
    body_sample_ratio = property(lambda self: float(cfg.body_sample_ratio))
    face_sample_ratio = property(lambda self: getattr(cfg, "face_sample_ratio", 0.0))
    begin_ith_frame = property(lambda self: int(cfg.begin_ith_frame))
    frame_interval = property(lambda self: int(cfg.frame_interval))
    num_train_frame = property(lambda self: int(cfg.num_train_frame))
    voxel_size = property(lambda self: tuple(cfg.voxel_size))
    big_box = property(lambda self: bool(cfg.big_box))
    test_novel_pose = property(lambda self: bool(getattr(cfg, "test_novel_pose", False)))
    mode = "h36m"  # multi_view_dataset.py:154 calls sample_ray_h36m
    n_rounds = 4
    # not a reference key: YAML only (the reference's command line refuses keys its config.py does not define)
    seed = property(lambda self: int(getattr(cfg, "train_ray_seed", 0)))
    # train_ray_mask: True adds `occupancy` to every train item (the mask loss of plugins/if_nerf_clight.py reads it)
    ray_mask = property(lambda self: bool(getattr(cfg, "train_ray_mask", False)))


def disk_source(data_root, human, ann_file, split, device="cuda:0"):
    """`image_prep` is not a reference key (YAML only): 'cv2' prepares every image with OpenCV on the host as the reference does,
    'device' with neuralbody_amd/image_prep.py, 'auto' (the default) with cv2 where it imports and on the device elsewhere."""
    return LightStageFrameSource(
        data_root, human, ann_file, split, training_view=list(cfg.training_view), begin_ith_frame=int(cfg.begin_ith_frame),
        frame_interval=int(cfg.frame_interval), num_train_frame=int(cfg.num_train_frame), H=int(cfg.H), W=int(cfg.W),
        ratio=cfg.ratio, mask_bkgd=bool(cfg.mask_bkgd), white_bkgd=bool(cfg.white_bkgd),
        vertices=getattr(cfg, "vertices", "vertices"), params=getattr(cfg, "params", "params"),
        test_novel_pose=bool(getattr(cfg, "test_novel_pose", False)),
        num_novel_pose_frame=int(getattr(cfg, "num_novel_pose_frame", 0)),
        prep=select_prep(str(getattr(cfg, "image_prep", "auto")), device))


class Dataset(TrainRayDataset):
    def __init__(self, data_root, human, ann_file, split, source=None, device="cuda:0"):
        """`source`: a frame source to use instead of the files under `data_root` (tests)."""
        super().__init__(source if source is not None else disk_source(data_root, human, ann_file, split, device), _LiveCfg(),
                         split=split, device=device)
        self.data_root, self.human = data_root, human
