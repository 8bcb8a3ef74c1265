"""Host side of the silhouette cull of pose-driven frames (csrc/nb_silhouette.hip, neuralbody_amd/smpl_pose.py): the numpy
reference of tests/silhouette_ref.py against an analytic case and against the kernel's own integer definition, the condition
on the inputs the device tests lean on (the band the reference leaves open), the dilation's border, the triangle list's
validation and the defaults that keep today's items.  Nothing here touches a device."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

from tests import silhouette_ref as sil
from tests import smpl_ref as sr


@functools.lru_cache(maxsize=None)
def _case(name):
    c = sil.path_case() if name == "paths" else sil.band_case(name)
    lo, hi = sil.lo_hi_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], c["H"], c["W"])  # computed once, shared, never written
    return c, lo, hi


def test_reference_decides_a_spheres_disc():
    """A sphere of radius r seen from distance d by a camera aimed at its centre projects onto the disc of radius
    f r / sqrt(d^2 - r^2) around the principal point.  The 5120-face icosphere lies between that sphere and the one inscribed in
    its faces (the chord error), so a pixel whose square reaches into the inner disc by more than 3 tau is set in `lo`, and one
    whose square stays out of the outer disc by more than 3 tau is clear in `hi`."""
    H = W = 96
    r, d, f = 0.4, 2.0, 1.4 * H
    verts, faces = sil.icosphere(4, (r, r, r))
    tri = verts.astype(np.float64)[faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float(np.abs(np.einsum("fk,fk->f", n, tri[:, 0]) / np.linalg.norm(n, axis=1)).min())  # the faces' inscribed sphere
    r_out = float(np.linalg.norm(verts.astype(np.float64), axis=1).max())
    assert 0.995 * r < r_in < r_out < r * (1 + 1e-6)
    K, RT = sil.look_at((0.0, 0.0, -d), (0.0, 0.0, 0.0), f, H, W, centre=(47.3, 48.6))
    lo, hi = sil.lo_hi(verts, faces, K, RT, H, W)
    rho_in, rho_out = f * r_in / math.sqrt(d * d - r_in * r_in), f * r_out / math.sqrt(d * d - r_out * r_out)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = np.maximum(np.abs(x - 47.3) - 0.5, 0.0), np.maximum(np.abs(y - 48.6) - 0.5, 0.0)
    nearest = np.hypot(dx, dy)  # from the principal point to the pixel's square
    inside, outside = nearest <= rho_in - 3 * sil.TAU, nearest >= rho_out + 3 * sil.TAU
    print("disc radius %.3f .. %.3f px; %d pixels decided set, %d decided clear, %d open; band of the reference %d" % (
        rho_in, rho_out, inside.sum(), outside.sum(), (~inside & ~outside).sum(), (hi & ~lo).sum()))
    assert inside.sum() > 2000 and outside.sum() > 2000 and (~inside & ~outside).sum() < 400
    assert lo[inside].all() and not hi[outside].any()
    assert not (lo & ~hi).any()


@pytest.mark.parametrize("name", ["ico320", "ico1280", "ico5120", "paths"])
def test_band_is_within_its_cap_and_holds_the_integer_definition(name):
    """The condition on the inputs: the band the reference leaves open is at most BAND_CAP of a mask's pixels.  And the kernel's
    definition (fp32 projection, snap, integer edge functions), evaluated on the host, lies between lo and hi."""
    c, lo, hi = _case(name)
    band = sil.band_fraction(lo, hi)
    print("%s: %d faces at %d x %d, band %s pixels, at most %.4f %%" % (name, len(c["faces"]), c["H"], c["W"],
                                                                       (hi & ~lo).sum(axis=(2, 3)).tolist(), 100 * band))
    assert band <= sil.BAND_CAP
    assert lo.any(axis=(2, 3)).sum() >= 3  # the case draws something
    if name in ("ico320", "paths"):  # the cases the device suite runs
        m = sil.snapped_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], c["H"], c["W"]).astype(bool)
        assert not (lo & ~m).any() and not (m & ~hi).any()


def test_views_that_do_not_cull_in_the_integer_definition():
    c = sil.band_case("ico320")
    v, f = c["verts"][0], c["faces"]
    near = v.copy()
    uv, depth = sil.project(v, c["Ks"][0], c["RTs"][0])
    assert depth.min() > 1.0
    fwd = c["RTs"][0][2, :3].astype(np.float64)
    k = int(np.argmin(depth))
    near[k] = (v[k].astype(np.float64) - (depth[k] - 0.005) * fwd).astype(np.float32)  # depth 0.005 m, half the threshold
    assert abs(sil.project(near, c["Ks"][0], c["RTs"][0])[1][k] - 0.005) < 1e-4 and not sil.view_culls(near, c["Ks"][0], c["RTs"][0])
    assert sil.snapped_mask(near, f, c["Ks"][0], c["RTs"][0], 45, 61).all()
    assert sil.view_culls(v, c["Ks"][0], c["RTs"][0]) and not sil.snapped_mask(v, f, c["Ks"][0], c["RTs"][0], 45, 61).all()


def test_border_formula_and_its_refusals():
    from neuralbody_amd.smpl_pose import cull_border, cull_camera_arrays

    H = W = 512
    can_bounds = np.array([[-0.4, -0.9, -0.3], [0.4, 0.9, 0.3]], np.float32)
    cams = [sil.look_at((0.0, 0.0, -3.0), (0, 0, 0), 1200.0, H, W), sil.look_at((2.5, 0.0, 0.0), (0, 0, 0), 1100.0, H, W)]
    Ks, RTs = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    # nearest corner: 3.0 - 0.3 = 2.7 m from camera 0, 2.5 - 0.4 = 2.1 m from camera 1
    want_px = math.ceil(0.05 * 1200.0 / (2.1 - 0.05)) + 1
    assert want_px == 31 and cull_border(can_bounds, Ks, RTs, 0.05) == 2 * want_px + 1
    assert cull_border(can_bounds, Ks, RTs) == 63  # the default margin is the box padding
    assert cull_border(can_bounds, Ks, RTs, 0.0) == 3  # the + 1 alone
    RT44 = np.concatenate([RTs, np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (2, 1, 1))], axis=1)
    assert cull_border(can_bounds, Ks, RT44, 0.05) == 63
    Ks2, RTs2, h, w = cull_camera_arrays((torch.from_numpy(Ks), RT44, H, W))
    assert RTs2.shape == (2, 3, 4) and Ks2.dtype == np.float64 and (h, w) == (H, W) and np.array_equal(RTs2, RTs)
    with pytest.raises(ValueError, match=r"cull_margin = 2\.2 m.*cull camera 1"):  # z_near 2.1 <= margin
        cull_border(can_bounds, Ks, RTs, 2.2)
    with pytest.raises(ValueError, match=r"cull_margin = 0\.3 m.*cull camera 1.*border"):  # ceil(0.3 * 1200 / 1.8) + 1 = 201 px
        cull_border(can_bounds, Ks, RTs, 0.3)
    inside = np.stack([cams[0][1], sil.look_at((0.3, 0.0, 0.0), (0, 0.0, 1.0), 1100.0, H, W)[1]])  # a camera inside the box
    with pytest.raises(ValueError, match="cull camera 1"):
        cull_border(can_bounds, Ks, inside, 0.05)
    with pytest.raises(ValueError, match="cull_cameras"):
        cull_camera_arrays((Ks, RTs[:, :2], H, W))
    with pytest.raises(ValueError, match="cull_cameras"):
        cull_camera_arrays((Ks, RTs, H))


def test_smpl_model_keeps_and_validates_the_triangle_list(tmp_path):
    import pickle

    from neuralbody_amd import ops
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    m = sr.case_model("tree321_new")
    V = 321
    faces = np.random.RandomState(0).randint(0, V, (500, 3)).astype(np.uint32)  # the pickle holds uint32
    model = SmplModel.from_arrays(dict(m, f=faces), device="cpu")
    assert model.faces.dtype == np.int32 and model.faces.flags.c_contiguous and np.array_equal(model.faces, faces)
    alt = {k: v for k, v in m.items() if k != "f"}
    assert np.array_equal(SmplModel.from_arrays(dict(alt, faces=faces.astype(np.int64)), device="cpu").faces, faces)
    path = tmp_path / "SMPL_NEUTRAL.pkl"
    with open(path, "wb") as fh:
        pickle.dump(dict(m, f=faces), fh)
    assert np.array_equal(SmplModel.from_pkl(str(path), device="cpu").faces, faces)
    for bad in (np.array([[0, 1, V]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError, match="triangle list"):
            SmplModel.from_arrays(dict(m, f=bad), device="cpu")
        with pytest.raises(ValueError, match="triangle list"):
            SmplModel.host_arrays(dict(m, f=bad))
    for bad in (np.zeros((4, 4), np.int64), np.zeros(6, np.int64), np.zeros((0, 3), np.int64), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError, match="triangle list"):
            SmplModel.from_arrays(dict(m, f=bad), device="cpu")
    # a model without faces is today's model: the same arrays, and it still poses (up to the device it needs)
    bare = SmplModel.from_arrays(alt, device="cpu")
    assert bare.faces is None and all(np.array_equal(bare.host[k], model.host[k]) for k in model.host) and bare.parents == model.parents
    with pytest.raises(ops.NbError, match="HIP device"):
        PoseDriver(bare, device="cpu").vertices(*sr.case_params("tree321_new"))
    # asking it for silhouettes says what is missing, before anything touches a device
    cams = (np.eye(3)[None], np.eye(4)[None, :3], 8, 8)
    with pytest.raises(ops.NbError, match="triangle list"):
        bare.faces_device()
    with pytest.raises(ops.NbError, match="HIP device|triangle list"):
        PoseDriver(bare, device="cpu").silhouettes(torch.zeros(1, V, 3), cams)
    with pytest.raises(ops.NbError, match="HIP device"):
        PoseDriver(model, device="cpu").frames(*sr.case_params("tree321_new"), latent_index=0, cull_cameras=cams)


def test_sources_and_config_default_to_no_culling():
    from tests import helpers as H
    from neuralbody_amd.smpl_pose import LightStagePoseSource, MemoryPoseSource, PoseDataConfig

    cfg = PoseDataConfig()
    assert cfg.cull_views == () and cfg.cull_margin == 0.05
    cfg = PoseDataConfig(cull_views=[3, 1], cull_margin=0.02)
    assert cfg.cull_views == (3, 1) and cfg.cull_margin == 0.02
    src = MemoryPoseSource([], np.eye(3), np.eye(3), np.zeros(3), 32, 48)
    assert src.cull is None
    with pytest.raises(ValueError, match="cull_cameras"):
        src.cull_cameras([0])
    Ks = np.stack([np.eye(3) * (i + 1) for i in range(4)])
    RTs = np.stack([np.eye(4) + i for i in range(4)])
    src = MemoryPoseSource([], np.eye(3), np.eye(3), np.zeros(3), 32, 48, cull_cameras=(Ks, RTs, 16, 24))
    k, rt, h, w = src.cull_cameras([2, 0])
    assert np.array_equal(k, Ks[[2, 0]]) and np.array_equal(rt, RTs[[2, 0], :3]) and (h, w) == (16, 24)
    # the plugin reads the two keys from the live cfg, with the same defaults
    pcfg = types.SimpleNamespace(begin_ith_frame=0, frame_interval=1, num_train_frame=1, num_render_frame=-1, voxel_size=[0.005] * 3,
                                 big_box=False, test_view=[0], H=64, W=64, ratio=1.0, params="params",
                                 train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1))
    mod = H.load_plugin("light_stage_pose_dataset.py", pcfg)
    live = mod._LiveCfg()
    assert live.cull_views == () and live.cull_margin == 0.05
    pcfg.cull_views, pcfg.cull_margin = [0, 6], 0.03
    assert live.cull_views == (0, 6) and live.cull_margin == 0.03
    # the annotation cameras as render_utils.load_cam scales them
    src = LightStagePoseSource.__new__(LightStagePoseSource)
    src._cams = {"K": [np.array([[1000.0, 0, 500], [0, 1100.0, 400], [0, 0, 1]])] * 2, "R": [np.eye(3), 2 * np.eye(3)],
                 "T": [np.array([[100.0], [200.0], [3000.0]])] * 2}
    src._ratio, src.H, src.W = 0.5, 512, 512
    k, rt, h, w = src.cull_cameras([1])
    assert k.shape == (1, 3, 3) and rt.shape == (1, 3, 4) and (h, w) == (512, 512)
    assert np.array_equal(k[0], [[500.0, 0, 250], [0, 550.0, 200], [0, 0, 1]]) and np.array_equal(rt[0, :, :3], 2 * np.eye(3))
    assert np.allclose(rt[0, :, 3], [0.1, 0.2, 3.0])


def test_lib_exports_the_entry_and_refuses_bad_arguments():
    from neuralbody_amd import _lib, build, ops

    build.build(verbose=False)
    L = _lib.lib()
    assert {"nb_smpl_silhouette", "nb_smpl_silhouette_scratch_size"} <= set(_lib.header_functions()) and L.nb_abi_version() == 20
    size = L.nb_smpl_silhouette_scratch_size
    assert size(1, 4, 4, 1) >= 4 * 5 + 8 * 4 + 4 * 4 and size(16, 6890, 13776, 4) >= 16 * 4 * (8 * 6890 + 4 * 13776)
    assert size(0, 4, 4, 1) == 0 and size(1, 0, 4, 1) == 0 and size(1, 4, 0, 1) == 0 and size(1, 4, 4, 65) == 0
    assert size(65535, 6890, 13776, 64) == 0  # F nv V beyond 2^31 - 1
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is enqueued
    args = lambda F=1, V=4, Nf=4, nv=1, Hh=8, Ww=8, scratch=one, nbytes=1 << 20: (  # noqa: E731
        one, one, one, F, V, Nf, nv, Hh, Ww, scratch, nbytes, one, None)
    for bad, word in ((args(F=0), b"F = 0"), (args(nv=65), b"nv = 65"), (args(Hh=0), b"H = 0"), (args(Ww=40000), b"W = 40000"),
                      (args(nbytes=16), b"scratch holds 16"), (args(scratch=C.c_void_p(260)), b"aligned"), (args(scratch=None), b"NULL")):
        assert L.nb_smpl_silhouette(*bad) == -1 and word in L.nb_last_error(), word
    with pytest.raises(ops.NbError):  # no CPU fallback
        ops.smpl_silhouette(torch.zeros(1, 4, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(1, 3, 4), torch.zeros(1, 3, 3), 8, 8)
