"""Generate tests/golden/mesh_lattice.npz by driving the UNMODIFIED reference mesh dataset
(lib/datasets/light_stage/multi_view_mesh_dataset.py::Dataset: __init__, prepare_input, get_mask, prepare_inside_pts and the
lattice lines of __getitem__) on CPU through oracle/ref_harness.py.  Run from the repo root, where the reference tree exists:
    python tests/golden/make_golden_mesh_lattice.py

The dataset module imports libraries that do not exist on this stack; each is seeded into sys.modules BEFORE
ref_harness.load() (which uses setdefault).  Every STAND-IN, by name:
  * cv2.dilate      — tests/lattice_ref.py::dilate (the window maximum, pixels outside the image ignored)
  * cv2.undistort   — the identity (the synthetic cameras have no distortion: D = 0)
  * cv2.Rodrigues   — neuralbody_amd.novel_view.rodrigues (the same formula; returns (R, None) like OpenCV)
  * imageio.imread  — serves the synthetic CIHP masks from memory, by path
  * plyfile.PlyData — an empty class (imported, unused)
The fixture says so in `stand_ins`.  Everything else is the reference's own: the frame and camera selection, np.arange per axis,
the 'ij' meshgrid, base_utils.project in float32, np.round, the clip, the per-view masking order and the dtypes.
The vertices, SMPL parameters and annotations the dataset np.load()s are written to a temporary directory first.
The fixture holds synthetic inputs, the axes, the dilated masks and `inside`: data only.
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from neuralbody_amd import novel_view  # noqa: E402
from tests import lattice_ref as lr  # noqa: E402
from tests import synthetic as syn  # noqa: E402
from tests.golden import scenes  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STAND_INS = ("cv2.dilate: numpy window maximum (tests/lattice_ref.py::dilate); cv2.undistort: identity; cv2.Rodrigues: "
             "neuralbody_amd.novel_view.rodrigues; imageio.imread: masks served from memory; plyfile: stub; "
             "OpenCV, imageio and plyfile were not available where this fixture was made")
BODY = scenes.MESH["body"]
N_VIEWS, H, W, STEP = 3, 64, 64, 0.02
MASKS = {}  # path -> the CIHP label image imageio.imread returns
DILATED = []  # what get_mask returned, in call order


def cv2_dilate(msk, kernel):
    assert kernel.shape[0] == kernel.shape[1] and (kernel == 1).all()
    out = lr.dilate(msk[None], kernel.shape[0])[0]
    DILATED.append(out)
    return out


def seed_modules():
    cv2 = types.ModuleType("cv2")
    cv2.dilate = cv2_dilate
    cv2.undistort = lambda img, K, D: img
    cv2.Rodrigues = lambda rvec: (novel_view.rodrigues(rvec), None)
    sys.modules["cv2"] = cv2
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: MASKS[os.path.normpath(path)]
    sys.modules["imageio"] = imageio
    plyfile = types.ModuleType("plyfile")
    plyfile.PlyData = type("PlyData", (), {})
    sys.modules["plyfile"] = plyfile


def main():
    seed_modules()
    from oracle import ref_harness as rh

    ns = rh.load()
    sys.path.insert(0, ns.root)
    import lib.datasets.light_stage.multi_view_mesh_dataset as mvm  # the reference's module, unmodified

    assert mvm.cv2.dilate is cv2_dilate
    cfg = ns.cfg
    cfg.training_view = list(range(N_VIEWS))
    cfg.begin_ith_frame, cfg.num_train_frame, cfg.num_render_frame = 0, 1, -1
    cfg.voxel_size, cfg.big_box = [STEP, STEP, STEP], False
    cfg.vertices, cfg.params = "vertices", "params"

    body = syn.make_body(**BODY)
    rh_, th_ = np.array(BODY["rh"], np.float64), np.array(BODY["th"], np.float32).reshape(1, 3)
    raw, Ks, RTs = syn.make_view_masks(body, H, W, n_views=N_VIEWS, focal_factor=1.8, distance=1.6, dilate=1)
    labels = (raw * np.array([1, 2, 14], np.uint8)[:, None, None]).astype(np.uint8)  # CIHP part labels: any non-zero is body
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "vertices"))
        os.makedirs(os.path.join(root, "params"))
        np.save(os.path.join(root, "vertices", "0.npy"), body["world_verts"])
        np.save(os.path.join(root, "params", "0.npy"), {"Rh": rh_, "Th": th_}, allow_pickle=True)
        ims = ["Camera_B%d/000000.jpg" % (v + 1) for v in range(N_VIEWS)]
        for v, im in enumerate(ims):
            MASKS[os.path.normpath(os.path.join(root, "mask_cihp", im)[:-4] + ".png")] = labels[v]
        annots = {"cams": {"K": [K.astype(np.float64).tolist() for K in Ks], "R": [RT[:, :3].astype(np.float64).tolist() for RT in RTs],
                           "T": [(RT[:, 3:].astype(np.float64) * 1000.0).tolist() for RT in RTs],
                           "D": [np.zeros((5, 1)).tolist() for _ in range(N_VIEWS)]},
                  "ims": [{"ims": ims}]}
        ann_file = os.path.join(root, "annots.npy")
        np.save(ann_file, annots, allow_pickle=True)
        ds = mvm.Dataset(root, "synthetic", ann_file, "test")
        assert len(ds) == 1
        item = ds[0]
    pts, inside = item["pts"], item["inside"]
    assert pts.dtype == np.float32 and inside.dtype == np.uint8 and tuple(pts.shape[:3]) == (24, 36, 15), pts.shape
    axes = [pts[:, 0, 0, 0].copy(), pts[0, :, 0, 1].copy(), pts[0, 0, :, 2].copy()]
    assert np.array_equal(lr.lattice_points(axes).reshape(pts.shape), pts)
    dilated = np.stack(DILATED[-N_VIEWS:])
    # the cameras as the dataset holds them (float32, T back in metres): what prepare_inside_pts projected with
    RT = np.concatenate([ds.Rs, ds.Ts], axis=2)
    band = lr.near_band(axes, dilated, ds.Ks, RT)
    f64 = lr.inside(axes, dilated, ds.Ks, RT, "f64")
    print("lattice %s, inside %d, band %d points (%.2f %%), reference != fp64: %d outside the band, %d inside it" % (
        inside.shape, int(inside.sum()), int(band.sum()), 100.0 * band.mean(), int(((inside != f64) & ~band).sum()),
        int(((inside != f64) & band).sum())))
    store = dict(stand_ins=np.array(STAND_INS), xyz=body["world_verts"], Rh=rh_, Th=th_, msks_raw=(labels != 0).astype(np.uint8),
                 Ks=ds.Ks, Rs=ds.Rs, Ts=ds.Ts, voxel_size=np.array([STEP] * 3, np.float64), axis_x=axes[0], axis_y=axes[1],
                 axis_z=axes[2], msks_dilated=dilated, inside=inside, coord=item["coord"], out_sh=item["out_sh"],
                 wbounds=item["wbounds"], bounds=item["bounds"], R=item["R"], Th_item=item["Th"],
                 latent_index=np.array(item["latent_index"]), frame_index=np.array(item["frame_index"]))
    path = os.path.join(OUT, "mesh_lattice.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
