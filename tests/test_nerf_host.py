"""Host-side checks of the vanilla-NeRF baseline (neuralbody_amd/nerf.py): the float64 restatement tests/nerf_ref.py against the
fixture the unmodified reference wrote (tests/golden/nerf_baseline.npz), the state dict, the refusals, the plugins and the new ABI
entries' argument checks.  Nothing here needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import nerf_ref as ref

# fp32 forward against float64, relative to max(1, |raw|): ten layers, each a sum of up to 319 products whose rounding errors
# add like sqrt(K) u = 18 * 6e-8 = 1.1e-6 of the activation scale, carried on with gains of order one: ~1e-5; ten times that
RAW_REL_TOL = 1e-4


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(hp.GOLDEN + "/nerf_baseline.npz"))


@pytest.fixture(scope="module")
def sd(fx):
    sd = ref.make_state_dict(fx["alpha_shift"])
    assert ref.checksum(sd) == str(fx["weights_sha256"]), "the seed recipe no longer gives the fixture's weights"
    return sd


@pytest.fixture(scope="module")
def passes(fx, sd):
    """The float64 model at the fixture's own depths and directions, both passes (computed once)."""
    o, d = fx["ray_o"], fx["ray_d"]
    return (ref.render_pass(sd, "model", o, d, fx["z_coarse"], viewdirs=fx["viewdirs"]),
            ref.render_pass(sd, "model_fine", o, d, fx["z_fine"], viewdirs=fx["viewdirs"]))


def test_restatement_reproduces_the_reference_raw(fx, passes):
    for name, got, want in (("coarse", passes[0]["raw"], fx["raw_coarse"]), ("fine", passes[1]["raw"], fx["raw_fine"])):
        e_abs = float(np.abs(got - want).max())
        e_rel = hp.assert_close(want, got, RAW_REL_TOL, "raw " + name)
        print("e_ref %s: %.3e absolute, %.3e relative to max(1, |raw|); max |raw| %.1f" % (name, e_abs, e_rel, np.abs(got).max()))


def test_restatement_reproduces_the_reference_maps(fx, passes):
    coarse, fine = passes
    span = float((fx["far"] - fx["near"]).max())
    n = fx["ray_o"].shape[0]
    for key, p, mine in (("rgb0", coarse, "rgb_map"), ("acc0", coarse, "acc_map"), ("disp0", coarse, "disp_map"),
                         ("rgb_map", fine, "rgb_map"), ("acc_map", fine, "acc_map"), ("disp_map", fine, "disp_map")):
        e = hp.assert_close(fx["ref_" + key].reshape(n, -1), p[mine].reshape(n, -1), hp.RGB_TOL, key)
        print("%s: %.3e" % (key, e))
    e = hp.assert_close(fx["ref_depth_map"].reshape(n) / span, fine["depth_map"] / span, hp.RGB_TOL, "depth_map", rel=False)
    print("depth_map / (far - near): %.3e" % e)
    hp.assert_close(fx["ref_z_std"].reshape(n), fx["z_samples"].astype(np.float64).std(-1), 1e-6, "z_std")


def test_restatement_reproduces_the_reference_fine_depths(fx, passes):
    """sample_pdf in float64 on the float64 coarse weights lands on the reference's fp32 importance depths up to what the coarse
    weights' own fp32 error moves them (a sensitive function: the reason the fine pass is compared at fixed depths)."""
    zc = fx["z_coarse"].astype(np.float64)
    z = ref.sample_pdf(0.5 * (zc[:, 1:] + zc[:, :-1]), passes[0]["weights"][:, 1:-1], np.linspace(0.0, 1.0, 128))
    err = np.abs(z - fx["z_samples"])
    print("importance depths: median %.2e, max %.2e" % (np.median(err), err.max()))
    assert np.median(err) < 1e-5
    assert np.array_equal(np.sort(np.concatenate([fx["z_coarse"], fx["z_samples"]], -1), -1), fx["z_fine"])


def test_fixture_is_no_trivial_field(fx):
    acc = fx["ref_acc_map"].reshape(-1)
    assert np.mean((acc > 0.05) & (acc < 0.95)) >= 0.25
    pos = np.mean(np.concatenate([fx["raw_coarse"][..., 3].ravel(), fx["raw_fine"][..., 3].ravel()]) > 0)
    assert 0.25 <= pos <= 0.75
    shapes = {k[6:]: tuple(v) for k, v in fx.items() if k.startswith("shape_")}
    assert shapes == {"rgb_map": (1, 96, 3), "disp_map": (1, 96, 1), "acc_map": (1, 96, 1), "depth_map": (1, 96),
                      "raw": (1, 96, 192 * 4), "rgb0": (1, 96, 3), "disp0": (1, 96, 1), "acc0": (1, 96, 1), "z_std": (1, 96, 1)}


def test_lattice_weights_are_exact_in_fp32():
    """The exact GPU test's premise, checked on its own shapes: every partial sum of every layer, in any order, fits fp32."""
    sd = ref.lattice_state_dict()
    for n, S in ((1, 3), (5, 67), (3, 192)):
        o, d, z = ref.lattice_rays(n, S)
        for m in ref.MODULES:
            audit = []
            raw = ref.forward(sd, m, ref.points_f32(o, d, z), ref.viewdirs_device(d), audit=audit)
            assert max(audit) < 24, audit
            assert np.array_equal(raw, raw.astype(np.float32)) and len(np.unique(raw[..., 3])) > 1


def test_state_dict_is_the_reference_network_s(sd):
    from neuralbody_amd.nerf import NerfNetwork

    net = NerfNetwork()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert len(got) == 48 and got == ref.state_dict_shapes()
    assert list(got) == list(ref.state_dict_shapes()), "the reference's order"
    missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    # the same creation order as the reference: the same seed gives the same initialisation
    with torch.random.fork_rng():
        torch.manual_seed(0)
        fresh = NerfNetwork().state_dict()
    base = ref.make_state_dict((0.0, 0.0))
    assert np.array_equal(fresh["model_fine.views_linears.0.bias"].numpy(), base["model_fine.views_linears.0.bias"])


@pytest.mark.parametrize("key,value", [("netdepth", 4), ("netwidth", 128), ("netdepth_fine", 6), ("netwidth_fine", 512),
                                       ("use_viewdirs", False), ("xyz_res", 6), ("view_res", 2)])
def test_unsupported_configurations_are_refused_by_name(key, value):
    from neuralbody_amd.nerf import NerfNetwork

    with pytest.raises(NotImplementedError, match=key + " = "):
        NerfNetwork(**{key: value})


def test_precision_names_and_inference_only():
    from neuralbody_amd.nerf import NerfNetwork, VolumeRenderer, VolumeRendererConfig

    with pytest.raises(ValueError, match="precision"):
        NerfNetwork(precision="f16f6")
    net = NerfNetwork()
    from neuralbody_amd import nerf

    assert net.nerf_precision() == nerf.AUTO_ARITHMETIC and nerf.AUTO_ARITHMETIC in ("f32", "f16x3")
    assert NerfNetwork(precision="f32").nerf_precision() == "f32" and NerfNetwork(precision="f16x3").nerf_precision() == "f16x3"
    pts, vd = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(NotImplementedError, match="inference only"):
        net(pts, vd)  # training mode
    net.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        net(pts, vd)  # grad enabled on parameters that require it
    r = VolumeRenderer(net, VolumeRendererConfig(lindisp=True))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="lindisp"):
        r.render({"ray_o": torch.zeros(1, 2, 3), "ray_d": torch.ones(1, 2, 3), "near": torch.ones(1, 2), "far": 2 * torch.ones(1, 2)})


def test_plugins_import_against_a_stub_config():
    cfg = types.SimpleNamespace(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10,
                                view_res=4, N_samples=64, N_importance=128, perturb=1, raw_noise_std=0, white_bkgd=False,
                                lindisp=False, chunk=32768, H=1024, W=1024, ratio=0.5)
    net = hp.load_plugin("nerf.py", cfg).Network()
    assert len(net.state_dict()) == 48
    assert not net.training and not net.train().training and not net.model.training  # run.py:57,89 call train(): it stays eval
    r = hp.load_plugin("volume_renderer.py", cfg).Renderer(net)
    assert r.net is net and (r.cfg.N_samples, r.cfg.N_importance, r.cfg.chunk, r.cfg.H) == (64, 128, 32768, 512)
    cfg.N_importance, cfg.white_bkgd = 0, True  # read at call time
    assert r.cfg.N_importance == 0 and r.cfg.white_bkgd is True
    cfg.netwidth = 128
    with pytest.raises(NotImplementedError, match="netwidth"):
        hp.load_plugin("nerf.py", cfg).Network()


def test_new_entries_check_their_arguments_without_a_device():
    from neuralbody_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    # 593 920 packed weights (K padded to whole chunks) + 9 * 256 + 128 biases + alpha (256 + 4) + rgb (384 + 4)
    assert lib.nb_nerf_pack_size(0) == lib.nb_nerf_pack_size(2) == 593920 + 2432 + 260 + 388 and lib.nb_nerf_pack_size(1) == 0
    assert C.sizeof(_lib.NbNerfParams) == 24 * 8
    assert lib.nb_nerf_decode(None, None, None, None, 0, 64, None, 0, None) == 0  # n_rays == 0: at once
    for args, word in (((None, None, None, None, 4, 64, None, 0, None), b"NULL"),
                       ((None, None, None, None, 4, 0, None, 0, None), b"n_samples"),
                       ((None, None, None, None, 4, 513, None, 0, None), b"n_samples"),
                       ((None, None, None, None, 4, 64, None, 1, None), b"precision"),
                       ((16, 16, 16, 16, 4, 64, 18, 0, None), b"4-byte aligned"),
                       ((8, 16, 16, 16, 4, 64, 16, 0, None), b"16-byte aligned")):
        assert lib.nb_nerf_decode(*args) == -1 and word in lib.nb_last_error(), (args, lib.nb_last_error())
    assert lib.nb_nerf_pack(None, None, 0, None) == -1 and b"NULL" in lib.nb_last_error()
    params = _lib.NbNerfParams()
    for i in range(8):
        params.pts_w[i], params.pts_b[i] = 16, 16
    for f in ("views_w", "views_b", "feature_w", "feature_b", "alpha_w", "alpha_b", "rgb_w"):
        setattr(params, f, 16)
    params.rgb_b = 18
    assert lib.nb_nerf_pack(C.byref(params), 16, 2, None) == -1 and b"4-byte aligned" in lib.nb_last_error()
    assert lib.nb_nerf_pack(C.byref(params), 8, 0, None) == -1 and b"16-byte aligned" in lib.nb_last_error()
    assert lib.nb_nerf_pack(C.byref(params), 16, 1, None) == -1 and b"precision" in lib.nb_last_error()
    assert lib.nb_importance_merge_z(None, None, 0, 64, 128, None, None) == 0
    assert lib.nb_importance_merge_z(None, None, 4, 64, 128, None, None) == -1 and b"NULL" in lib.nb_last_error()
    assert lib.nb_importance_merge_z(None, None, 4, 64, 129, None, None) == -1 and b"n_importance" in lib.nb_last_error()
