"""Host side of the device image preparation (neuralbody_amd/image_prep.py, csrc/nb_image_prep.hip): the numpy restatement the GPU
tests compare against (tests/image_prep_ref.py) checked against an independent bilinear sampler and by hand, the header, every
refusal, and the decode path on files a test writes itself.  Nothing here touches a device."""
import sys
import types

import numpy as np
import pytest

from tests import image_prep_cases as cases
from tests import image_prep_ref as R

BOUND = 1.0 / 32.0 + 1e-6  # the 1/32-pixel map moves a sample by at most 1/64 px per axis; an image in [0,1] changes by at most 1 per px


def _unquantised(S, cam, mode):
    from scipy import ndimage

    H, W = S.shape[:2]
    u, v = R.source_uv(cam, H, W)
    return np.stack([ndimage.map_coordinates(S[..., c].astype(np.float64), [v, u], order=1, mode=mode, cval=0.0)
                     for c in range(S.shape[2])], axis=-1)


def _straddling(cam, H, W):
    """Pixels with one to three of their four taps outside the image."""
    sx, sy, _, _ = R.taps(cam, H, W)
    n_in = sum(((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).astype(np.int64)
               for yy, xx in ((sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)))
    return (n_in > 0) & (n_in < 4)


@pytest.mark.parametrize("name", ["inward", "strong5", "rational8", "zero"])
def test_reference_against_map_coordinates(name):
    """The restatement against scipy.ndimage.map_coordinates(order=1) at the UNQUANTISED (v, u): swapped axes or a wrong sign in
    image_prep_ref.py would show as errors of order 1.

    mode='constant' pads with 0 but does NOT interpolate between the last pixel and the padding (scipy's documentation: "no
    interpolation is performed beyond the edges of the input"), whereas a tap outside the image READS 0 here and in cv2's
    BORDER_CONSTANT.  So with mode='constant' every pixel is compared for 'inward', whose samples all lie inside the image, and
    every pixel but those whose taps straddle the edge for the others; mode='grid-constant', which is the definition, is compared
    at every pixel of every case."""
    H, W = 40, 52
    K, D = (cases.K_INWARD, cases.D_INWARD) if name == "inward" else (cases.K_40x52, cases.DISTORTIONS[name])
    cam = R.camera_constants(K, D)
    S = np.random.RandomState(3).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    got = R.remap_f32(S, cam).astype(np.float64)
    err_grid = np.abs(got - _unquantised(S, cam, "grid-constant")).max(axis=-1)
    err_const = np.abs(got - _unquantised(S, cam, "constant")).max(axis=-1)
    edge = _straddling(cam, H, W)
    print("%s: max |ref - map_coordinates| = %.5f (grid-constant, all pixels), %.5f (constant, %d straddling pixels left out; "
          "%.5f with them)" % (name, err_grid.max(), err_const[~edge].max(), int(edge.sum()), err_const.max()))
    assert err_grid.max() <= BOUND
    assert err_const[~edge].max() <= BOUND
    if name == "inward":
        u, v = R.source_uv(cam, H, W)
        assert u.min() >= 0 and u.max() <= W - 1 and v.min() >= 0 and v.max() <= H - 1 and not edge.any()
        assert np.abs(u - np.arange(W)).max() > 1.0  # and the map is no identity
        assert err_const.max() <= BOUND


def test_strong_distortion_reaches_the_border_branch():
    some, all4 = R.tap_census(cases.cam(cases.K_40x52, "strong5"), 40, 52)
    print("strong5 at 40 x 52: %.1f %% of pixels with a tap outside, %.1f %% with all four outside" % (100 * some, 100 * all4))
    assert some >= 0.05 and all4 >= 0.01
    assert R.tap_census(cases.cam(cases.K_40x52, "rational8"), 40, 52)[1] == 0.0


def test_zero_distortion_returns_the_bytes():
    rgb, msk = cases.byte_image(40, 52, 1), cases.byte_mask(40, 52, 2)
    for D in (np.zeros(4), np.zeros(5), np.zeros(8)):
        img, m = R.frame(rgb, msk, R.camera_constants(cases.K_40x52, D), 1, None)
        want = rgb.astype(np.float32) / np.float32(255.0)
        assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(m, msk)
    img2, m2 = R.frame(rgb, msk, R.camera_constants(cases.K_40x52, np.zeros(5)), 2, None)  # INTER_AREA / INTER_NEAREST by 2
    blocks = want.reshape(20, 2, 26, 2, 3)
    assert np.array_equal(img2, (((blocks[:, 0, :, 0] + blocks[:, 0, :, 1]) + blocks[:, 1, :, 0]) + blocks[:, 1, :, 1]) * np.float32(0.25))
    assert np.array_equal(m2, msk[::2, ::2])


def test_band_on_hand_checkable_masks():
    lab = cases.band_labels()
    out = R.band(lab, 5)
    assert not out[1].any() and (out[2] == 1).all()  # nothing to erode or dilate; borders are ignored, so no band at the edge
    m = (lab[0] != 0).astype(np.uint8)
    assert out[0, 0, 0] == 1 and out[0, 5, 0] == 1 and out[0, 0, 6] == 1  # deep inside, although the body touches two borders
    assert set(np.unique(out[0])) == {0, 1, 100}
    # by hand, in row 0: the body is columns 0..13; the window reaches 2 px, so the band is columns 12..15
    assert m[0].tolist() == [1] * 14 + [0] * 9 and m[1].tolist() == [1] * 13 + [0] * 10 and m[2].tolist() == [1] * 12 + [0] * 11
    assert out[0, 0].tolist() == [1] * 10 + [100] * 6 + [0] * 7
    assert (out[0, 13:18, 18:23] == 100).all() and out[0, 15, 20] == 100 and out[0, 12, 20] == 0  # the lone pixel's 5 x 5
    assert np.array_equal(R.band(lab, 1), (lab != 0).astype(np.uint8))
    assert np.array_equal(R.band(lab, 3)[0] == 100, (R.band(lab, 3)[0] == 100) & (out[0] == 100))  # a thinner band inside


def test_header_declares_the_entry_points_and_the_version_stays():
    from neuralbody_amd import _lib

    names = _lib.header_functions()
    assert "nb_mask_band" in names and "nb_image_undistort" in names
    assert set(names) == set(_lib.SIGNATURES)
    with open(_lib.HEADER) as f:
        src = f.read()
    assert "#define NB_ABI_VERSION 20\n" in src and _lib.ABI_VERSION == 20
    assert "#define NB_CAM_DOUBLES %d\n" % _lib.CAM_DOUBLES in src
    for name, val in (("NONE", None), ("BLACK", "black"), ("WHITE", "white")):
        assert "#define NB_FILL_%s %d\n" % (name, _lib.FILL_MODES[val]) in src
    L = _lib.lib()
    assert L.nb_abi_version() == 20 and hasattr(L, "nb_mask_band") and hasattr(L, "nb_image_undistort")


def test_camera_constants_and_reduction_factor():
    from neuralbody_amd.image_prep import camera_constants, reduction_factor

    K = cases.K_40x52
    for D in (np.arange(1, 5) / 10.0, (np.arange(1, 6) / 10.0).reshape(5, 1), (np.arange(1, 9) / 10.0).reshape(1, 8)):
        c = camera_constants(K, D)
        assert c.dtype == np.float64 and np.array_equal(c, R.camera_constants(K, D))
        assert c[:4].tolist() == [60.0, 58.0, 25.3, 19.6] and c[4:4 + D.size].tolist() == D.ravel().tolist()
        assert not c[4 + D.size:].any()
    for n_bad in (0, 3, 6, 7, 12, 14):
        with pytest.raises(ValueError, match="D has %d entries" % n_bad):
            camera_constants(K, np.zeros(n_bad))
    with pytest.raises(ValueError, match="K has shape"):
        camera_constants(K[:2], np.zeros(5))
    assert [reduction_factor(r, 64, 48) for r in (1, 1.0, 0.5, 0.25, 0.125)] == [1, 1, 2, 4, 8]
    for ratio, H, W in ((0.3, 60, 60), (0.4, 40, 40), (0.5, 63, 64), (0.25, 64, 62), (2.0, 64, 64), (0.0, 64, 64), (-0.5, 64, 64)):
        with pytest.raises(ValueError, match="ratio"):
            reduction_factor(ratio, H, W)


def _png(path, arr):
    from PIL import Image

    Image.fromarray(arr).save(str(path))
    return str(path)


def test_decode_reads_what_was_written_and_frame_refuses_by_name(tmp_path, monkeypatch):
    from neuralbody_amd import ops
    from neuralbody_amd.image_prep import DeviceImagePrep, decode

    monkeypatch.setitem(sys.modules, "imageio", None)  # the PIL branch, whatever is installed
    rgb, lab = cases.byte_image(40, 52, 5), cases.band_labels(40, 52)[0]
    img_p, msk_p = _png(tmp_path / "a.png", rgb), _png(tmp_path / "m.png", lab)
    got = decode(img_p)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb) and np.array_equal(decode(msk_p), lab)
    prep = DeviceImagePrep("cpu")  # constructing touches no device
    K, D = cases.K_40x52, cases.DISTORTIONS["strong5"]
    with pytest.raises(ValueError, match=r"expected uint8 \(80, 52, 3\)"):  # the reference would resize it
        prep.frame(img_p, msk_p, K, D, 80, 52, 1.0, True, False)
    with pytest.raises(ValueError, match="expected uint8"):  # a grey image is no RGB image
        prep.frame(msk_p, msk_p, K, D, 40, 52, 1.0, True, False)
    with pytest.raises(ValueError, match="mask .* the image is"):
        prep.frame(img_p, _png(tmp_path / "small.png", lab[:20]), K, D, 40, 52, 1.0, True, False)
    with pytest.raises(ValueError, match="ratio"):
        prep.frame(img_p, msk_p, K, D, 40, 52, 0.3, True, False)
    with pytest.raises(ValueError, match="ratio"):
        prep.frame(img_p, msk_p, K, D, 40, 52, 0.125, True, False)  # 8 does not divide 52
    with pytest.raises(ValueError, match="D has 6 entries"):
        prep.frame(img_p, msk_p, K, np.zeros(6), 40, 52, 1.0, True, False)
    with pytest.raises(ValueError, match="two dimensions"):
        prep.frame(img_p, img_p, K, D, 40, 52, 1.0, True, False)  # an RGB file where the label image belongs
    with pytest.raises(ValueError, match="two dimensions"):
        prep.masks([msk_p, img_p], [K, K], [D, D])
    with pytest.raises(ValueError, match="first view"):
        prep.masks([msk_p, str(tmp_path / "small.png")], [K, K], [D, D])
    with pytest.raises(ValueError, match="D has 3 entries"):
        prep.masks([msk_p], [K], [np.zeros(3)])
    with pytest.raises(ValueError, match="paths"):
        prep.masks([msk_p], [K, K], [D, D])
    # files and arguments in order: decoded, and then there is no CPU stand-in for the kernels
    with pytest.raises(ops.NbError, match="no CPU fallback"):
        prep.frame(img_p, msk_p, K, D, 40, 52, 0.5, True, False)
    with pytest.raises(ops.NbError, match="no CPU fallback"):
        prep.masks([msk_p, msk_p], [K, K], [D, D])


def test_ops_refuse_bad_arguments_before_any_launch():
    import torch

    from neuralbody_amd import ops

    rgb, msk = torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8)
    cam = cases.cam(cases.K_40x52, "zero")
    with pytest.raises(ops.NbError):
        ops.mask_band(msk[None], 5)
    with pytest.raises(ops.NbError):
        ops.image_undistort(rgb, msk, cam)
    with pytest.raises(ValueError, match="neither"):
        ops.image_undistort(None, None, cam)
    with pytest.raises(ValueError, match="fill"):
        ops.image_undistort(rgb, msk, cam, fill="grey")
    with pytest.raises(ValueError, match="fill"):
        ops.image_undistort(rgb, None, cam, fill="black")
    with pytest.raises(ValueError, match="cam has shape"):
        ops.image_undistort(rgb, msk, cam[:11])
    with pytest.raises(ValueError, match="fx and fy"):
        ops.image_undistort(rgb, msk, np.concatenate([[0.0], cam[1:]]))
    with pytest.raises(ValueError, match="finite"):
        ops.image_undistort(rgb, msk, np.concatenate([cam[:5], [np.nan], cam[6:]]))


def test_select_prep_and_the_untouched_cv2_path(tmp_path, monkeypatch):
    from neuralbody_amd.image_prep import DeviceImagePrep, select_prep
    from neuralbody_amd.mesh_lattice import LightStageMeshSource
    from neuralbody_amd.train_rays import LightStageFrameSource

    monkeypatch.setitem(sys.modules, "cv2", None)  # unimportable, whatever is installed
    assert isinstance(select_prep("auto", "cpu"), DeviceImagePrep) and isinstance(select_prep("device", "cpu"), DeviceImagePrep)
    assert select_prep("cv2", "cpu") is None
    with pytest.raises(ValueError, match="image_prep"):
        select_prep("opencv", "cpu")
    monkeypatch.setitem(sys.modules, "cv2", types.ModuleType("cv2"))  # importable: nothing changes
    assert select_prep("auto", "cpu") is None
    monkeypatch.setitem(sys.modules, "cv2", None)
    # the disk sources over a written tree: the item lists, and prep=None still goes to cv2
    ann = cases.write_tree(str(tmp_path))
    T = cases.TREE
    kw = dict(training_view=T["training_view"], begin_ith_frame=0, frame_interval=1, num_train_frame=2, H=T["H"], W=T["W"],
              ratio=T["ratio"], mask_bkgd=T["mask_bkgd"], white_bkgd=T["white_bkgd"])
    src = LightStageFrameSource(str(tmp_path), "synthetic", ann, "train", **kw)
    assert src.prep is None and src.n_items == 4 and src.cam_inds.tolist() == [0, 1, 0, 1]
    assert LightStageFrameSource(str(tmp_path), "synthetic", ann, "test", **kw).cam_inds.tolist() == [2, 2]
    with pytest.raises(ImportError):
        src.load(0)
    msrc = LightStageMeshSource(str(tmp_path), "synthetic", ann, [0, 1, 2], 0, 2)
    assert msrc.prep is None and msrc.n_items == 2
    with pytest.raises(ImportError):
        msrc.load(0)
    # with a prep the same sources never ask for cv2: they get as far as the kernels, which have no CPU stand-in
    from neuralbody_amd import ops

    with pytest.raises(ops.NbError, match="no CPU fallback"):
        LightStageFrameSource(str(tmp_path), "synthetic", ann, "train", prep=DeviceImagePrep("cpu"), **kw).load(0)
    with pytest.raises(ops.NbError, match="no CPU fallback"):
        LightStageMeshSource(str(tmp_path), "synthetic", ann, [0, 1, 2], 0, 2, prep=DeviceImagePrep("cpu")).load(0)


def test_reference_items_of_the_tree_are_usable():
    """The arrays the GPU test feeds a MemoryFrameSource: the right shapes, a body and a band in every mask, a filled background."""
    items = cases.frame_items("train")
    assert len(items) == 4 and len(cases.frame_items("test")) == 2
    for img, msk, K, Rm, T, f, c, xyz, Rh, Th in items:
        assert img.shape == (32, 32, 3) and img.dtype == np.float32 and msk.shape == (32, 32) and msk.dtype == np.uint8
        assert (msk == 1).sum() > 20 and (msk == 100).sum() > 10 and (msk == 0).sum() > 100
        assert not img[msk == 0].any() and img[msk != 0].any()
        assert T.shape == (3, 1) and abs(float(T[2, 0])) < 10.0  # metres
    mitems, Ks, Rs, Ts = cases.mesh_items()
    assert len(mitems) == 2 and mitems[0][0].shape == (3, 64, 64) and Ks.dtype == np.float32
    assert all(0 < int((m[0] != 0).sum()) < m[0].size for m in mitems)
