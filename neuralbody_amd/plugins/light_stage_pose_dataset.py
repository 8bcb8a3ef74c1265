"""test_dataset_path plugin of pose-driven rendering: `Dataset(data_root, human, ann_file, split)` bound to the reference's
global cfg (lib/datasets/make_dataset.py:13-23).  Item i is frame begin_ith_frame + i * frame_interval, made on the device from
params/{i}.npy (poses, shapes, Rh, Th) instead of vertices/{i}.npy (neuralbody_amd/smpl_pose.py), seen by camera
cfg.test_view[0] of the annotations; the items are device tensors, so it runs in the rendering process.  Select it with

    test_dataset_path /path/to/neuralbody_amd/plugins/light_stage_pose_dataset.py train.num_workers 0

and, in the YAML (the reference's command line refuses keys its config.py does not define):

    smpl_model_path: data/zju_mocap/smplx/smpl/SMPL_NEUTRAL.pkl
    smpl_new_params: true      # default: 'new' in cfg.params, the rule of zju_smpl/extract_vertices.py:14-16
    cull_views: [0, 6, 12, 18] # default []: no culling.  Cameras of the annotations whose silhouettes of the posed body are
                               # rasterised on the device; the items then hold msks / Ks / RT for the _mmsk renderer
    cull_margin: 0.05          # metres the silhouettes are dilated by (clothing, hair); the default is the box padding
    ray_bounds: body           # default box: every ray of the SMPL box, near / far its entry and exit.  body: near / far cut to the
                               # posed body's depth range in the rendered camera, rays beside the body dropped (ray_bounds.py)
    ray_bounds_margin: 0.05    # metres kept around the body's surface, in depth and in the image
    ray_bounds_tile: 8         # pixels: the blocks that share one interval (1, 2, 4, 8, 16; 8 is the march's ray tile)
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from lib.config import cfg  # noqa: E402

from neuralbody_amd.smpl_pose import LightStagePoseSource, PoseFrameDataset, SmplModel  # noqa: E402


class _LiveCfg:
    """Reads the reference cfg at call time."""

    begin_ith_frame = property(lambda self: int(cfg.begin_ith_frame))
    frame_interval = property(lambda self: int(cfg.frame_interval))
    num_train_frame = property(lambda self: int(cfg.num_train_frame))
    voxel_size = property(lambda self: tuple(cfg.voxel_size))
    big_box = property(lambda self: bool(cfg.big_box))
    # not a reference key: YAML only
    smpl_new_params = property(lambda self: bool(getattr(cfg, "smpl_new_params", "new" in str(getattr(cfg, "params", "params")))))
    cull_views = property(lambda self: tuple(int(v) for v in getattr(cfg, "cull_views", ())))
    cull_margin = property(lambda self: float(getattr(cfg, "cull_margin", 0.05)))
    ray_bounds = property(lambda self: str(getattr(cfg, "ray_bounds", "box")))
    ray_bounds_margin = property(lambda self: float(getattr(cfg, "ray_bounds_margin", 0.05)))
    ray_bounds_tile = property(lambda self: int(getattr(cfg, "ray_bounds_tile", 8)))


def disk_source(data_root, human, ann_file):
    view = list(getattr(cfg, "test_view", [])) or [0]
    return LightStagePoseSource(
        data_root, human, ann_file, view=int(view[0]), begin_ith_frame=int(cfg.begin_ith_frame),
        frame_interval=int(cfg.frame_interval), num_train_frame=int(cfg.num_train_frame), H=int(cfg.H), W=int(cfg.W),
        ratio=cfg.ratio, num_render_frame=int(getattr(cfg, "num_render_frame", -1)), params=getattr(cfg, "params", "params"))


def _require_in_process():
    """The items are device tensors made on the current stream: no worker processes."""
    for split in ("train", "test"):
        node = getattr(cfg, split, None)
        if node is not None and int(getattr(node, "num_workers", 0)) != 0:
            raise ValueError("light_stage_pose_dataset: %s.num_workers must be 0 (the items are device tensors)" % split)


class Dataset(PoseFrameDataset):
    def __init__(self, data_root, human, ann_file, split, source=None, model=None, device="cuda:0"):
        """`source`, `model`: a frame source and an SmplModel to use instead of the files (tests)."""
        _require_in_process()
        if model is None:
            path = getattr(cfg, "smpl_model_path", None)
            if not path:
                raise ValueError("light_stage_pose_dataset: set smpl_model_path (the SMPL .pkl) in the YAML")
            model = SmplModel.from_pkl(path, device)
        super().__init__(source if source is not None else disk_source(data_root, human, ann_file), model, _LiveCfg(), device=device)
        self.data_root, self.human, self.split = data_root, human, split
