"""Host-side checks of the training-ray sampler (no GPU): bound_hull, the numpy restatement tests/train_rays_ref.py against
the fixture the reference's own sample_ray_h36m / sample_ray produced (tests/golden/train_rays.npz, made by
tests/golden/make_golden_train_rays.py), the ABI surface of the two new entry points and the dataset core up to the device."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import train_rays_ref as trr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("A", "B", "C")


fixture, replayed_uniforms, case_inputs = trr.fixture, trr.replayed_uniforms, trr.case_inputs


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------- fixture
def test_fixture_is_what_the_issue_asks_for():
    g = fixture()
    assert [str(n) for n in g["names"]] == list(CASES)
    assert "stand-in" in str(g["rasteriser"])
    assert g["A/img"].shape == (48, 40, 3) and int(g["A/N"]) == 96 and str(g["A/mode"]) == "h36m"
    assert g["B/img"].shape == (64, 64, 3) and int(g["B/N"]) == 1024 and (g["B/msk"] == 100).any()
    assert g["C/img"].shape == (48, 40, 3) and str(g["C/mode"]) == "plain" and len(set(np.unique(g["C/msk"])) - {0, 1}) >= 2
    rounds = [len(g[n + "/draws_k"]) for n in CASES]
    assert max(rounds) >= 2 and max(rounds) <= 3
    for n in CASES:
        assert g[n + "/coord"].shape == (int(g[n + "/N"]), 2) and g[n + "/mask_at_box"].all()
        for k in ("rgb", "ray_o", "ray_d", "near", "far"):
            assert g[n + "/" + k].dtype == np.float32
    assert g["D/mask_at_box"].shape == (48 * 40,) and g["D/rgb"].shape[0] == int(g["D/mask_at_box"].sum())


# ------------------------------------------------------------------------------------------- bound_hull
@pytest.mark.parametrize("name", CASES)
def test_bound_hull_matches_the_fixture(name):
    from neuralbody_amd.train_rays import bound_hull

    g = fixture()
    hull = bound_hull(g[name + "/bounds"], g[name + "/K"], np.concatenate([g[name + "/R"], g[name + "/T"]], axis=1))
    assert np.array_equal(hull, g[name + "/hull"])
    # counter-clockwise and strictly convex
    nxt, nn = np.roll(hull, -1, axis=0), np.roll(hull, -2, axis=0)
    assert np.all((nxt[:, 0] - hull[:, 0]) * (nn[:, 1] - nxt[:, 1]) - (nxt[:, 1] - hull[:, 1]) * (nn[:, 0] - nxt[:, 0]) > 0)


def test_bound_hull_hand_cases():
    from neuralbody_amd.train_rays import bound_hull, convex_hull

    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]])
    RT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    # axis-aligned view: the near face (z = 2) covers the far one, the hull is its rectangle
    hull = bound_hull([[-0.2, -0.1, 2.0], [0.2, 0.3, 4.0]], K, RT)
    assert hull.tolist() == [[40, 35], [60, 35], [60, 55], [40, 55]]
    # a corner that rounds onto an edge is dropped: y = 0 projects to the principal row at every depth, so the far face's
    # corners (45, 40) and (55, 40) lie on the near face's edge (40, 40)-(60, 40)
    K1 = np.array([[1.0, 0, 50], [0, 1.0, 40], [0, 0, 1]])
    hull = bound_hull([[-20.0, 0.0, 2.0], [20.0, 30.0, 4.0]], K1, RT)
    assert hull.tolist() == [[40, 40], [60, 40], [60, 55], [40, 55]]
    assert convex_hull([[40, 35], [55, 35], [60, 35], [60, 55], [40, 55], [50, 45]]).tolist() == [[40, 35], [60, 35], [60, 55], [40, 55]]
    # half to even, like np.round: 40.5 -> 40, 61.5 -> 62
    hull = bound_hull([[-19.0, -10.0, 2.0], [23.0, 30.0, 2.0]], K1, RT)
    assert hull.tolist() == [[40, 35], [62, 35], [62, 55], [40, 55]]
    # a corner behind the camera is refused, and so is a box that projects onto a line
    with pytest.raises(ValueError, match="depth"):
        bound_hull([[-0.2, -0.1, -1.0], [0.2, 0.3, 4.0]], K, RT)
    with pytest.raises(ValueError, match="degenerate"):
        bound_hull([[0.0, -0.1, 2.0], [0.0, 0.3, 2.0]], K, RT)


# ------------------------------------------------------------------------------------------- restatement vs the reference
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = fixture()
    u = replayed_uniforms(g, name)
    out = trr.sample(u=u, body_ratio=0.5, **case_inputs(g, name))
    N = int(g[name + "/N"])
    highs = g[name + "/draws_high"]
    assert out["status"].tolist() == [N, len(g[name + "/draws_k"]), int(highs[0, 0]), int(highs[0, 1])]
    assert np.array_equal(out["pixel"], g[name + "/coord"])
    assert out["mask_at_box"].all() and np.array_equal(out["mask_at_box"], g[name + "/mask_at_box"])
    for k in ("rgb", "ray_o", "ray_d", "near", "far"):
        assert out[k].dtype == np.float32
        assert np.array_equal(bits(out[k]), bits(g[name + "/" + k])), k


def test_restatement_pads_a_short_batch():
    g = fixture()
    c = case_inputs(g, "A")
    c["msk"] = np.zeros_like(c["msk"])  # no body pixel: half of every round's draws give nothing
    u = np.random.RandomState(0).uniform(0, 1, (4, 96)).astype(np.float32)
    out = trr.sample(u=u, body_ratio=0.5, **c)
    n = int(out["status"][0])
    assert 48 <= n < 96 and out["status"][1] == 4 and out["status"][2] == 0
    assert out["mask_at_box"][:n].all() and not out["mask_at_box"][n:].any()
    assert (out["pixel"][n:] == -1).all() and (out["near"][n:] == 0).all() and (out["rgb"][n:] == 0).all()
    assert np.isfinite(out["ray_d"]).all()


# ------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    from neuralbody_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def test_header_and_signatures_name_the_new_entries(lib):
    from neuralbody_amd import _lib

    names = _lib.header_functions()
    for fn in ("nb_train_rays", "nb_train_rays_scratch_size"):
        assert fn in names and fn in _lib.SIGNATURES and hasattr(lib, fn), fn
    res, args = _lib.SIGNATURES["nb_train_rays"]
    assert res is C.c_int and len(args) == 25
    assert args[:6] == [C.c_int32, C.c_int32, C.c_double * 9, C.c_double * 9, C.c_double * 3, C.c_float * 6]
    assert args[11] is C.c_double and args[7] is C.c_int32 and args[13:15] == [C.c_int32, C.c_int32]
    assert _lib.SIGNATURES["nb_train_rays_scratch_size"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert _lib.ABI_VERSION == 20 and lib.nb_abi_version() == 20  # purely additive
    with open(_lib.HEADER) as f:
        src = f.read()
    assert "#define NB_SAMPLE_H36M 0" in src and "#define NB_SAMPLE_PLAIN 1" in src
    assert _lib.SAMPLE_MODES == {"h36m": 0, "plain": 1}


def test_scratch_size(lib):
    assert lib.nb_train_rays_scratch_size(512, 512) == 2 * lib.nb_scan_scratch_size(512 * 512)
    assert lib.nb_train_rays_scratch_size(0, 5) == 0 and lib.nb_train_rays_scratch_size(5, -1) == 0
    assert lib.nb_train_rays_scratch_size(1 << 15, 1 << 15) > 0 and lib.nb_train_rays_scratch_size(1 << 15, (1 << 15) + 1) == 0


def _call(lib, H=48, W=40, n_hull=4, hull=(10, 10, 30, 10, 30, 30, 10, 30), mode=0, ratio=0.5, n_rounds=4, n_rays=96, dev=None,
          hull_ptr=True):
    """nb_train_rays with NULL device pointers (or the fake non-NULL `dev`): every refusal comes before the first launch."""
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    h = (C.c_int32 * 16)(*(list(hull) + [0] * (16 - len(hull))))
    d = [dev] * 12
    return lib.nb_train_rays(H, W, eye, eye, (C.c_double * 3)(0, 0, 0), (C.c_float * 6)(-1, -1, 1, 1, 1, 2),
                             C.cast(h, C.c_void_p) if hull_ptr else None, n_hull, d[0], d[1], mode, ratio, d[2], n_rounds, n_rays,
                             *d[3:11], d[11], None)


@pytest.mark.parametrize("kw,word", [
    (dict(H=0), "H = 0"), (dict(W=-3), "W = -3"), (dict(H=1 << 15, W=(1 << 15) + 1), "2^30"), (dict(n_rays=0), "n_rays = 0"),
    (dict(n_rounds=0), "n_rounds = 0"), (dict(n_hull=2), "n_hull = 2"), (dict(n_hull=9), "n_hull = 9"),
    (dict(hull=(10, 10, 1 << 30, 10, 30, 30, 10, 30)), "2^30"), (dict(hull=(10, -(1 << 30), 30, 10, 30, 30, 10, 30)), "2^30"),
    (dict(ratio=-0.1), "body_ratio"), (dict(ratio=1.5), "body_ratio"), (dict(ratio=float("nan")), "body_ratio"),
    (dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"), (dict(hull_ptr=False), "NULL host pointer"),
    (dict(), "NULL device pointer")])
def test_refusals_without_touching_a_device(lib, kw, word):
    assert _call(lib, **kw) == -1  # NB_EINVAL
    msg = lib.nb_last_error().decode()
    assert msg.startswith("nb_train_rays:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_bad_modes():
    import torch

    from neuralbody_amd import _lib, ops

    img, msk, u = torch.zeros(8, 8, 3), torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(4, 16)
    eye, b, hull = np.eye(3), np.array([[-1, -1, 1], [1, 1, 2]], np.float32), [[1, 1], [6, 1], [6, 6]]
    with pytest.raises(_lib.NbError):
        ops.train_rays(img, msk, eye, eye, np.zeros(3), b, hull, "h36m", 0.5, u)
    with pytest.raises(ValueError, match="mode"):
        ops.train_rays(img, msk, eye, eye, np.zeros(3), b, hull, "face", 0.5, u)


# ------------------------------------------------------------------------------------------- multi_view_frame, dataset core
def test_multi_view_frame_matches_the_fixture_and_the_big_box_rule():
    from neuralbody_amd.train_rays import multi_view_frame

    g = fixture()
    fr = multi_view_frame(g["A/xyz"], g["A/Rh"], g["A/Th"])
    for k, v in fr.items():
        assert np.array_equal(v, g["A/frame_" + k]) and v.dtype == g["A/frame_" + k].dtype, k
    assert np.array_equal(fr["can_bounds"], g["A/bounds"])
    xyz = g["A/xyz"]
    assert np.allclose(fr["can_bounds"], [xyz.min(0) - [0, 0, 0.05], xyz.max(0) + [0, 0, 0.05]], atol=1e-6)
    big = multi_view_frame(xyz, g["A/Rh"], g["A/Th"], big_box=True)
    assert np.allclose(big["can_bounds"], [xyz.min(0) - 0.05, xyz.max(0) + 0.05], atol=1e-6)
    assert fr["coord"].dtype == np.int32 and fr["coord"].min() >= 0 and np.all(fr["coord"].max(0) < fr["out_sh"])
    assert np.all(fr["out_sh"] % 32 == 0) and fr["R"].dtype == np.float32 and fr["R"].shape == (3, 3)


def _memory_source(n_frames=3, n_views=2, first_frame=10, step=5):
    from neuralbody_amd.train_rays import MemoryFrameSource

    g = fixture()
    items = []
    for f in range(n_frames):
        for v in range(n_views):
            items.append((g["A/img"], g["A/msk"], g["A/K"], g["A/R"], g["A/T"], first_frame + step * f, v, g["A/xyz"], g["A/Rh"],
                          g["A/Th"]))
    return MemoryFrameSource(items)


def test_dataset_core_length_and_index_arithmetic():
    from neuralbody_amd.train_rays import TrainDataConfig, TrainRayDataset

    src = _memory_source()
    ds = TrainRayDataset(src, TrainDataConfig(N_rand=96, begin_ith_frame=10, frame_interval=5, num_train_frame=3))
    assert len(ds) == 6
    assert [ds.latent_index(src.items[i][5]) for i in range(6)] == [0, 0, 1, 1, 2, 2]  # (frame_index - begin) // interval
    novel = TrainRayDataset(src, TrainDataConfig(begin_ith_frame=10, frame_interval=5, num_train_frame=3, test_novel_pose=True), "test")
    assert novel.latent_index(25) == 2  # multi_view_dataset.py:170-171
    assert ds.sampler is None  # nothing touched a device yet


def test_face_sampling_is_refused_with_the_reason():
    from neuralbody_amd.train_rays import TrainDataConfig, TrainRayDataset, TrainRaySampler

    with pytest.raises(ValueError, match="face_sample_ratio.*not built"):
        TrainRayDataset(_memory_source(), TrainDataConfig(face_sample_ratio=0.1))
    with pytest.raises(ValueError, match="face_sample_ratio.*not built"):
        TrainRaySampler(48, 40, 96, face_sample_ratio=0.25)
    with pytest.raises(ValueError, match="mode"):
        TrainRaySampler(48, 40, 96, mode="face")


def test_plugin_binds_the_live_cfg():
    from tests import helpers as H
    from neuralbody_amd.train_rays import TrainRayDataset

    cfg = types.SimpleNamespace(N_rand=96, body_sample_ratio=0.5, face_sample_ratio=0.0, begin_ith_frame=10, frame_interval=5,
                                num_train_frame=3, voxel_size=[0.005, 0.005, 0.005], big_box=False, training_view=[0, 1],
                                ratio=0.5, H=1024, W=1024, mask_bkgd=True, white_bkgd=False)
    mod = H.load_plugin("light_stage_dataset.py", cfg)
    ds = mod.Dataset("nowhere", "CoreView_313", "none.npy", "train", source=_memory_source())
    assert isinstance(ds, TrainRayDataset) and len(ds) == 6
    assert (ds.cfg.N_rand, ds.cfg.mode, ds.cfg.n_rounds, ds.cfg.big_box) == (96, "h36m", 4, False)
    cfg.N_rand, cfg.big_box = 1024, True  # read at call time
    assert (ds.cfg.N_rand, ds.cfg.big_box) == (1024, True)
    cfg.face_sample_ratio = 0.1
    with pytest.raises(ValueError, match="face_sample_ratio"):
        mod.Dataset("nowhere", "CoreView_313", "none.npy", "train", source=_memory_source())
