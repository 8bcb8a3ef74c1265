"""Host side of pose-driven frames (neuralbody_amd/smpl_pose.py) against tests/golden/smpl_pose.npz, which the unmodified
reference SMPL layer wrote (tests/golden/make_golden_smpl.py): the seeded models are the fixture's, the float64 restatement the
GPU tests lean on stands where the fixture says it stands, and everything that needs a device refuses a host.  Nothing here
touches a device."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import smpl_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_pose.npz")


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _model(name):
    return sr.case_model(name)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_models_and_restatement_are_the_fixtures(name):
    g, m = _gold(), _model(name)
    assert np.allclose(sr.checksums(m), g[name + "/checksums"], rtol=1e-12, atol=0.0), "numpy's random stream moved: remake the fixture"
    poses, shapes, Rh, Th = sr.case_params(name)
    for k, v in (("poses", poses), ("shapes", shapes), ("Rh", Rh), ("Th", Th)):
        assert np.array_equal(v, g["%s/%s" % (name, k)]), k
    assert sr.parents_of(m) == g[name + "/parents"].tolist()
    new_params = bool(g[name + "/new_params"])
    assert new_params == sr.CASES[name][3]
    ref = g[name + "/verts"]
    assert ref.dtype == np.float32 and ref.shape == (sr.CASES[name][1], 3)
    r64 = sr.forward(m, poses, shapes, Rh, Th, new_params, np.float64)
    e = float(np.abs(ref.astype(np.float64) - r64).max())
    e_ref = float(g[name + "/E_ref"])
    print("%s: E_ref %.3e (fixture %.3e)" % (name, e, e_ref))
    assert 5e-8 < e_ref < 1e-6 and abs(e - e_ref) <= 1e-12
    r32 = sr.forward(m, poses, shapes, Rh, Th, new_params, np.float32)
    assert r32.dtype == np.float32 and float(np.abs(r32 - r64).max()) < 5e-6
    if new_params and not sr.CASES[name][5]:  # the pose blend is visible
        assert float(np.abs(sr.forward(m, poses, shapes, Rh, Th, False, np.float64) - r64).max()) > 1e-3


@pytest.mark.parametrize("name,pad", sr.VOXEL_CASES)
def test_voxel_cases_are_clear_of_the_out_sh_steps(name, pad):
    g = _gold()
    info = sr.voxel_case_check(g[name + "/verts"], g[name + "/Rh"], g[name + "/Th"], pad)
    assert info["ok"], info


def test_lib_exports_the_entries_and_refuses_bad_arguments():
    import ctypes as C

    from neuralbody_amd import _lib, build

    build.build(verbose=False)
    L = _lib.lib()
    assert {"nb_smpl_pose", "nb_smpl_voxelize"} <= set(_lib.header_functions()) and L.nb_abi_version() == 20
    m = _lib.NbSmplModel()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    vs = (C.c_double * 3)(0.005, 0.005, 0.005)
    assert L.nb_smpl_pose(None, one, 1, 0, one, one, None, None) == -1 and b"nb_smpl_pose" in L.nb_last_error()
    for f in ("v_template", "shapedirs", "weights", "j_template", "j_shapedirs"):
        setattr(m, f, 256)
    m.parents[:] = sr.SMPL_PARENTS
    m.n_verts = 0
    assert L.nb_smpl_pose(C.byref(m), one, 1, 0, one, one, None, None) == -1 and b"V = 0" in L.nb_last_error()
    m.n_verts = 5
    assert L.nb_smpl_pose(C.byref(m), one, 0, 0, one, one, None, None) == -1 and b"F = 0" in L.nb_last_error()
    assert L.nb_smpl_pose(C.byref(m), one, 1, 1, one, one, None, None) == -1 and b"posedirs" in L.nb_last_error()
    m.parents[7] = 7
    assert L.nb_smpl_pose(C.byref(m), one, 1, 0, one, one, None, None) == -1 and b"parents[7]" in L.nb_last_error()
    args = lambda V=5, F=1, stride=3, v=vs, pad=0: (one, V, F, one, one, stride, v, pad, one, one, one, one, one, None)  # noqa: E731
    for bad, word in ((args(V=0), b"V = 0"), (args(F=0), b"F = 0"), (args(pad=3), b"pad_mode"), (args(stride=2), b"rt_stride"),
                      (args(v=(C.c_double * 3)(0.005, 0.0, 0.005)), b"voxel_size[1]"),
                      (args(v=(C.c_double * 3)(-1.0, 0.005, 0.005)), b"voxel_size[0]")):
        assert L.nb_smpl_voxelize(*bad) == -1 and word in L.nb_last_error(), word


def test_ops_refuse_host_tensors_and_bad_shapes():
    from neuralbody_amd import _lib, ops
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    with pytest.raises(ops.NbError):
        ops.smpl_voxelize(torch.zeros(1, 5, 3), torch.zeros(1, 3), torch.zeros(1, 3), (0.005,) * 3)
    with pytest.raises(ops.NbError):
        ops.smpl_pose(_lib.NbSmplModel(), torch.zeros(1, 88))
    with pytest.raises(TypeError):
        ops.smpl_pose(object(), torch.zeros(1, 88))
    with pytest.raises(ops.NbError):
        ops.make_smpl_model({"v_template": torch.zeros(5, 3)}, sr.SMPL_PARENTS)
    model = SmplModel.from_arrays(_model("tree321_new"), device="cpu")
    assert model.n_verts == 321 and model.parents == sr.parents_of(_model("tree321_new"))
    with pytest.raises(ops.NbError):  # no CPU fallback
        PoseDriver(model, device="cpu").vertices(*sr.case_params("tree321_new"))
    with pytest.raises(ValueError, match="pad"):
        PoseDriver(model, pad="tight")
    with pytest.raises(ValueError, match="voxel_size"):
        PoseDriver(model, voxel_size=(0.005, 0.0, 0.005))


def test_smpl_model_layout_and_refusals():
    from neuralbody_amd.smpl_pose import SmplModel, pack_params

    m = _model("tree321_new")
    host, parents = SmplModel.host_arrays(m)
    V = 321
    assert {k: v.shape for k, v in host.items()} == {"v_template": (V, 3), "shapedirs": (10, 3 * V), "posedirs": (207, 3 * V),
                                                      "weights": (24, V), "j_template": (24, 3), "j_shapedirs": (24, 3, 10)}
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in host.values()) and parents[0] == -1
    assert np.array_equal(host["posedirs"][5].reshape(V, 3), m["posedirs"][:, :, 5])
    assert np.array_equal(host["shapedirs"][3].reshape(V, 3), m["shapedirs"][:, :, 3])
    assert np.array_equal(host["weights"].T, m["weights"])
    beta = sr.case_params("tree321_new")[1].astype(np.float64)
    J = m["J_regressor"].astype(np.float64) @ (m["v_template"].astype(np.float64) + m["shapedirs"].astype(np.float64) @ beta)
    assert np.abs(host["j_template"].astype(np.float64) + host["j_shapedirs"].astype(np.float64) @ beta - J).max() < 2e-7
    # the already-reshaped pose basis, a plain parents list and a matrix with .todense() are taken too
    class Sparse:
        def todense(self):
            return np.array(m["J_regressor"])

    alt = dict(m, posedirs=m["posedirs"].reshape(3 * V, 207).T, parents=sr.parents_of(m), J_regressor=Sparse())
    del alt["kintree_table"]
    host2, parents2 = SmplModel.host_arrays(alt)
    assert parents2 == parents and all(np.array_equal(host[k], host2[k]) for k in host)
    with pytest.raises(ValueError, match="24 joints"):
        SmplModel.host_arrays(dict(m, weights=np.zeros((V, 52), np.float32)))
    with pytest.raises(ValueError, match="207"):
        SmplModel.host_arrays(dict(m, posedirs=np.zeros((V, 3, 93), np.float32)))
    with pytest.raises(ValueError, match="sum to 1"):
        SmplModel.host_arrays(dict(m, weights=m["weights"] * np.float32(1.00001)))
    bad = np.array(m["kintree_table"])
    bad[0, 3] = 5
    with pytest.raises(ValueError, match="parents"):
        SmplModel.host_arrays(dict(m, kintree_table=bad))
    p = pack_params(np.zeros((3, 72)), np.ones((1, 10)), np.zeros((3, 3)), np.full((3, 3), 2.0))
    assert tuple(p.shape) == (3, 88) and p.dtype == torch.float32 and float(p[2, 81]) == 1.0 and float(p[1, 87]) == 2.0
    with pytest.raises(ValueError, match="same frames"):
        pack_params(np.zeros((3, 72)), np.ones((2, 10)), np.zeros((3, 3)), np.zeros((3, 3)))


def test_from_pkl_reads_the_references_pickle(tmp_path):
    import pickle

    from neuralbody_amd.smpl_pose import SmplModel

    m = _model("tree321_new")
    path = tmp_path / "SMPL_NEUTRAL.pkl"
    with open(path, "wb") as f:
        pickle.dump(m, f)
    a, b = SmplModel.from_pkl(str(path), device="cpu"), SmplModel.from_arrays(m, device="cpu")
    assert a.parents == b.parents and all(np.array_equal(a.host[k], b.host[k]) for k in b.host)


def test_plugin_binds_the_live_cfg():
    from tests import helpers as H
    from neuralbody_amd import ops
    from neuralbody_amd.smpl_pose import MemoryPoseSource, PoseFrameDataset, SmplModel

    cfg = types.SimpleNamespace(begin_ith_frame=3, frame_interval=2, num_train_frame=2, num_render_frame=-1, voxel_size=[0.005] * 3,
                                big_box=False, test_view=[4], H=64, W=64, ratio=0.5, params="params",
                                train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1))
    mod = H.load_plugin("light_stage_pose_dataset.py", cfg)
    poses, shapes, Rh, Th = sr.case_params("tree321_new")
    items = [dict(poses=poses[None], shapes=shapes[None], Rh=Rh[None], Th=Th[None])] * 4
    src = MemoryPoseSource(items, np.eye(3), np.eye(3), np.zeros(3), 32, 32)
    model = SmplModel.from_arrays(_model("tree321_new"), device="cpu")
    ds = mod.Dataset("nowhere", "CoreView_313", "none.npy", "test", source=src, model=model, device="cpu")
    assert isinstance(ds, PoseFrameDataset) and len(ds) == 4
    assert [ds.latent_index(i) for i in range(4)] == [0, 1, 1, 1]  # multi_view_demo_dataset.py:165
    assert (ds.cfg.begin_ith_frame, ds.cfg.frame_interval, ds.cfg.big_box, ds.cfg.smpl_new_params) == (3, 2, False, False)
    cfg.params = "new_params"  # extract_vertices.py:14-16, read at call time
    assert ds.cfg.smpl_new_params is True
    cfg.smpl_new_params = False
    assert ds.cfg.smpl_new_params is False
    with pytest.raises(ops.NbError):
        ds[0]
    with pytest.raises(ValueError, match="smpl_model_path"):
        mod.Dataset("nowhere", "CoreView_313", "none.npy", "test", source=src)
    cfg.train.num_workers = 4
    with pytest.raises(ValueError, match="num_workers"):
        mod.Dataset("nowhere", "CoreView_313", "none.npy", "test", source=src, model=model)
