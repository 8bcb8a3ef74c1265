"""nb_mask_band and nb_image_undistort (csrc/nb_image_prep.hip) and the disk sources above them (neuralbody_amd/image_prep.py)
against the numpy restatement of tests/image_prep_ref.py, bit for bit: the map is float64 evaluated operation by operation, the
uint8 path is integer and the float path is a fixed sequence of uncontracted float32 operations, so there is no tolerance."""
import functools
import sys
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import image_prep_cases as cases
from tests import image_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------- 1. band
@pytest.mark.parametrize("border", [1, 3, 5, 47])  # 47: a half width of 23 reaches past both sides of the image
def test_band_matches_the_restatement(border):
    from neuralbody_amd import ops

    lab = cases.band_labels()
    assert lab.shape == (3, 19, 23)
    out = ops.mask_band(_dev(lab), border)
    assert out.dtype == torch.uint8 and _same_bits(out, R.band(lab, border))
    if border == 1:
        assert _same_bits(out, (lab != 0).astype(np.uint8))
    else:
        assert int((out == 100).sum()) > 0
    for bad in (0, 2, 257):
        with pytest.raises(ValueError, match="border"):
            ops.mask_band(_dev(lab), bad)


# ---------------------------------------------------------------------------------------------------------- 2. undistort
@functools.lru_cache(maxsize=None)
def _frame_40x52():
    return cases.byte_image(40, 52, 1), cases.byte_mask(40, 52, 2)


@functools.lru_cache(maxsize=None)
def _want(name, n, fill):
    rgb, msk = _frame_40x52()
    return R.frame(rgb, msk, cases.cam(cases.K_40x52, name), n, fill)


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("name", ["strong5", "rational8", "zero"])
def test_undistort_matches_the_restatement_bit_for_bit(name, n):
    from neuralbody_amd import ops

    rgb, msk = _frame_40x52()
    cam = cases.cam(cases.K_40x52, name)
    if name == "strong5":  # the border branch is exercised
        some, all4 = R.tap_census(cam, 40, 52)
        assert some >= 0.05 and all4 >= 0.01
    img, m = ops.image_undistort(_dev(rgb), _dev(msk), cam, n)
    want_img, want_m = _want(name, n, None)
    assert tuple(img.shape) == (40 // n, 52 // n, 3) and tuple(m.shape) == (40 // n, 52 // n)
    diff = img.cpu().numpy() != want_img
    print("%s n=%d: %d of %d floats differ, %d of %d mask bytes differ" % (
        name, n, int(diff.sum()), diff.size, int((m.cpu().numpy() != want_m).sum()), want_m.size))
    assert _same_bits(m, want_m)
    assert _same_bits(img, want_img)
    if name == "zero" and n == 1:
        assert _same_bits(img, rgb.astype(np.float32) / np.float32(255.0)) and _same_bits(m, msk)


# ---------------------------------------------------------------------------------------------------------- 3. odd sizes, batches
def test_odd_frame_image_only_mask_only_and_three_cameras_in_one_call():
    from neuralbody_amd import ops

    Hh, Ww = 37, 53
    K = cases.K_37x53
    cams = []
    for v, name in enumerate(("strong5", "rational8", "zero")):
        Kv = K.copy()
        Kv[0, 0] += 3.0 * v
        Kv[1, 2] -= 1.25 * v
        cams.append(R.camera_constants(Kv, cases.DISTORTIONS[name]))
    cams = np.stack(cams)
    rgbs = np.stack([cases.byte_image(Hh, Ww, 20 + v) for v in range(3)])
    msks = np.stack([cases.byte_mask(Hh, Ww, 30 + v) for v in range(3)])
    img, none = ops.image_undistort(_dev(rgbs[0]), None, cams[0])
    assert none is None and _same_bits(img, R.frame(rgbs[0], None, cams[0])[0])
    none, m = ops.image_undistort(None, _dev(msks[0]), cams[0])
    assert none is None and _same_bits(m, R.frame(None, msks[0], cams[0])[1])
    img3, m3 = ops.image_undistort(_dev(rgbs), _dev(msks), cams)
    none, m3_only = ops.image_undistort(None, _dev(msks), cams)
    assert tuple(img3.shape) == (3, Hh, Ww, 3) and tuple(m3.shape) == (3, Hh, Ww) and torch.equal(m3, m3_only)
    for v in range(3):
        want_img, want_m = R.frame(rgbs[v], msks[v], cams[v])
        assert _same_bits(img3[v], want_img) and _same_bits(m3[v], want_m), v
    assert not np.array_equal(R.frame(None, msks[1], cams[0])[1], R.frame(None, msks[1], cams[1])[1])  # the cameras matter
    # more views than one launch holds
    reps = [0, 1, 2, 1, 0, 2, 2, 1, 0, 1, 2]
    _, m11 = ops.image_undistort(None, _dev(msks[reps]), cams[reps])
    assert torch.equal(m11, m3[reps])
    # a batch of one is a batch
    _, m1 = ops.image_undistort(None, _dev(msks[:1]), cams[:1])
    assert tuple(m1.shape) == (1, Hh, Ww) and torch.equal(m1[0], m3[0])
    for bad_n in (0, 2, 37):
        with pytest.raises(ValueError, match="divide"):
            ops.image_undistort(_dev(rgbs[0]), None, cams[0], bad_n)
    with pytest.raises(ValueError, match="shape"):
        ops.image_undistort(_dev(rgbs), _dev(msks[:2]), cams)


# ---------------------------------------------------------------------------------------------------------- 4. fill
@pytest.mark.parametrize("n", [1, 2])
def test_fill_touches_exactly_the_pixels_with_a_zero_mask(n):
    from neuralbody_amd import ops

    rgb, msk = _frame_40x52()
    cam = cases.cam(cases.K_40x52, "strong5")
    plain, m = ops.image_undistort(_dev(rgb), _dev(msk), cam, n, None)
    zero = (m == 0)
    assert 0 < int(zero.sum()) < zero.numel()
    assert float(plain[zero].max()) > 0.0  # there is something to fill
    for fill, value in (("black", 0.0), ("white", 1.0)):
        img, m2 = ops.image_undistort(_dev(rgb), _dev(msk), cam, n, fill)
        assert torch.equal(m2, m)
        assert bool((img[zero] == value).all()) and H.same_bits(img[~zero], plain[~zero])
        want_img, want_m = _want("strong5", n, fill)
        assert _same_bits(img, want_img) and _same_bits(m2, want_m)


# ---------------------------------------------------------------------------------------------------------- 5. disk to dataset
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("zju_tree"))
    return root, cases.write_tree(root)


def _frame_source(tree, split, prep):
    from neuralbody_amd.train_rays import LightStageFrameSource

    root, ann = tree
    T = cases.TREE
    return LightStageFrameSource(root, "synthetic", ann, split, training_view=T["training_view"], begin_ith_frame=0,
                                 frame_interval=1, num_train_frame=T["n_frames"], H=T["H"], W=T["W"], ratio=T["ratio"],
                                 mask_bkgd=T["mask_bkgd"], white_bkgd=T["white_bkgd"], prep=prep)


@pytest.mark.parametrize("split, index", [("train", 0), ("train", 3), ("test", 1)])
def test_disk_frames_through_the_ray_dataset_equal_reference_prepared_arrays(tree, split, index):
    from neuralbody_amd.image_prep import DeviceImagePrep
    from neuralbody_amd.train_rays import MemoryFrameSource, TrainDataConfig, TrainRayDataset

    def cfg():
        return TrainDataConfig(N_rand=64, num_train_frame=cases.TREE["n_frames"], seed=5)

    disk = TrainRayDataset(_frame_source(tree, split, DeviceImagePrep(DEV)), cfg(), split=split, device=DEV)
    mem = TrainRayDataset(MemoryFrameSource(cases.frame_items(split)), cfg(), split=split, device=DEV)
    assert len(disk) == len(mem)
    loaded = disk.source.load(index)
    want = cases.frame_items(split)[index]
    assert loaded[0].is_cuda and loaded[1].is_cuda and _same_bits(loaded[0], want[0]) and _same_bits(loaded[1], want[1])
    assert np.array_equal(loaded[2], want[2]) and loaded[5:7] == want[5:7]
    a, b = disk[index], mem[index]
    assert set(a) == set(b)
    for k in ("rgb", "ray_o", "ray_d", "near", "far", "mask_at_box"):
        assert a[k].is_cuda and a[k].numel() > 0 and a[k].dtype == b[k].dtype and tuple(a[k].shape) == tuple(b[k].shape), k
        assert H.same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k]), k
    for k in ("coord", "out_sh", "bounds", "R", "Th", "latent_index"):
        assert torch.equal(a[k], b[k]), k
    assert (a["frame_index"], a["cam_ind"]) == (b["frame_index"], b["cam_ind"])
    if split == "train":
        disk.sampler.check()
        assert float(a["rgb"].max()) > 0.0


def test_disk_masks_through_the_mesh_dataset_carve_the_same_lattice(tree):
    from neuralbody_amd.image_prep import DeviceImagePrep
    from neuralbody_amd.mesh_lattice import LightStageMeshSource, MemoryMeshSource, MeshLatticeConfig, MeshLatticeDataset

    root, ann = tree
    cfg = MeshLatticeConfig(num_train_frame=2, voxel_size=(0.02, 0.02, 0.02))
    src = LightStageMeshSource(root, "synthetic", ann, [0, 1, 2], 0, 2, prep=DeviceImagePrep(DEV))
    items, Ks, Rs, Ts = cases.mesh_items()
    assert np.array_equal(src.Ks, Ks) and np.array_equal(src.Ts, Ts)
    disk = MeshLatticeDataset(src, cfg, device=DEV)
    mem = MeshLatticeDataset(MemoryMeshSource(items, Ks, Rs, Ts), cfg, device=DEV)
    for index in (0, 1):
        msks = src.load(index)[0]
        assert msks.is_cuda and _same_bits(msks, items[index][0])
        a, b = disk[index], mem[index]
        assert a["inside"].is_cuda and tuple(a["inside"].shape) == tuple(b["inside"].shape)
        assert 0 < int(a["inside"].sum()) < a["inside"].numel()
        assert torch.equal(a["inside"], b["inside"])
        for k in ("axis_x", "axis_y", "axis_z", "coord", "out_sh"):
            assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------- 6. the plugins' choice
def _plugin_cfg(**kw):
    T = cases.TREE
    return types.SimpleNamespace(
        training_view=T["training_view"], begin_ith_frame=0, frame_interval=1, num_train_frame=T["n_frames"], num_render_frame=-1,
        H=T["H"], W=T["W"], ratio=T["ratio"], mask_bkgd=T["mask_bkgd"], white_bkgd=T["white_bkgd"], N_rand=64, body_sample_ratio=0.5,
        face_sample_ratio=0.0, voxel_size=[0.02, 0.02, 0.02], big_box=False, train_ray_seed=5, vertices="vertices", params="params",
        train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1), **kw)


def test_auto_selects_the_device_where_cv2_does_not_import(tree, monkeypatch):
    from neuralbody_amd.image_prep import DeviceImagePrep

    root, ann = tree
    monkeypatch.setitem(sys.modules, "cv2", None)  # unimportable, whatever is installed
    mod = H.load_plugin("light_stage_dataset.py", _plugin_cfg())  # no image_prep key: auto
    ds = mod.Dataset(root, "synthetic", ann, "train", device=DEV)
    assert isinstance(ds.source.prep, DeviceImagePrep) and len(ds) == 4
    item = ds[1]
    want = cases.frame_items("train")[1]
    assert _same_bits(ds._items[1]["img"], want[0]) and _same_bits(ds._items[1]["msk"], want[1])
    assert item["rgb"].is_cuda and tuple(item["rgb"].shape) == (64, 3)
    mmod = H.load_plugin("light_stage_mesh_dataset.py", _plugin_cfg())
    mds = mmod.Dataset(root, "synthetic", ann, "test", device=DEV)
    assert isinstance(mds.source.prep, DeviceImagePrep)
    assert 0 < int(mds[0]["inside"].sum())
    # `cv2` asks for the host path, which is as it was: it imports cv2 first of all
    for plugin, split in (("light_stage_dataset.py", "train"), ("light_stage_mesh_dataset.py", "test")):
        old = H.load_plugin(plugin, _plugin_cfg(image_prep="cv2")).Dataset(root, "synthetic", ann, split, device=DEV)
        assert old.source.prep is None
        with pytest.raises(ImportError):
            old.source.load(0)
    with pytest.raises(ValueError, match="image_prep"):
        H.load_plugin("light_stage_dataset.py", _plugin_cfg(image_prep="opencv")).Dataset(root, "synthetic", ann, "train", device=DEV)
