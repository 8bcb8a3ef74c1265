"""Host-side checks of the vanilla-NeRF baseline's training step: the float64 restatement tests/nerf_train_ref.py against
torch.autograd on an independently written module, the audit that makes the exact GPU tests exact, the jitter against the
reference's statements in torch, the fixture the unmodified reference wrote (tests/golden/nerf_train_step.npz), and the API
(default refusals, trainable=True, the new entries' argument checks).  Nothing here needs a GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import helpers as hp
from tests import nerf_ref as ref
from tests import nerf_train_ref as tr


class _TorchNerf(nn.Module):
    """lib/networks/nerf.py:8-65 for D = 8, W = 256, skips = [4], use_viewdirs, written against the paper's figure (not against
    tests/nerf_ref.py): float64, embeddings passed in."""

    def __init__(self, p):
        super().__init__()
        self.p = nn.ParameterDict({k.replace(".", "/"): nn.Parameter(torch.from_numpy(np.asarray(v, np.float64))) for k, v in p.items()})

    def lin(self, name, x):
        return torch.nn.functional.linear(x, self.p[name + "/weight"], self.p[name + "/bias"])

    def forward(self, e_p, e_v):
        h = e_p
        for i in range(8):
            h = torch.relu(self.lin("pts_linears/%d" % i, h))
            if i == 4:
                h = torch.cat([e_p, h], -1)
        alpha = self.lin("alpha_linear", h)
        h = torch.cat([self.lin("feature_linear", h), e_v], -1)
        h = torch.relu(self.lin("views_linears/0", h))
        return torch.cat([self.lin("rgb_linear", h), alpha], -1)


@pytest.mark.parametrize("module", ref.MODULES)
def test_backward_restatement_equals_autograd_in_float64(module):
    sd = ref.make_state_dict((0.3, -0.2), seed=5)
    rs = np.random.RandomState(6)
    pts = rs.uniform(-1, 1, (3, 2, 3)).astype(np.float32)
    vd = ref.viewdirs_device(rs.normal(size=(3, 3)).astype(np.float32))
    d_raw = rs.normal(size=(6, 4))
    fwd = tr.forward_tap(sd, module, pts, vd)
    assert np.array_equal(fwd["raw"].reshape(3, 2, 4), ref.forward(sd, module, pts, vd))
    got = tr.backward(sd, module, fwd["tap"], d_raw)
    net = _TorchNerf({k[len(module) + 1:]: v for k, v in sd.items() if k.startswith(module + ".")})
    e_p = torch.from_numpy(fwd["tap"][:, tr.TAP_PTS:tr.TAP_PTS + 63])
    e_v = torch.from_numpy(fwd["tap"][:, tr.TAP_VIEW:tr.TAP_VIEW + 27])
    raw = net(e_p, e_v)
    assert np.allclose(raw.detach().numpy(), fwd["raw"], rtol=0, atol=1e-12)
    (raw * torch.from_numpy(d_raw)).sum().backward()
    assert list(got["grads"]) == tr.PARAM_NAMES and len(tr.PARAM_NAMES) == 24
    for name, g in got["grads"].items():
        want = net.p[name.replace(".", "/")].grad.numpy()
        assert g.shape == want.shape and tr.rel_err(g, want) < 1e-12, name
    # the tap's pad columns are zero, the d-tap has the documented width
    assert not fwd["tap"][:, tr.TAP_PTS + 63].any() and not fwd["tap"][:, tr.TAP_VIEW + 27:].any()
    assert got["dtap"].shape == (6, tr.DTAP_COLS)


# every shape of the exact GPU tests (tests/test_gpu_nerf_train.py); 3 x 192 has too many samples for exact weight gradients
@pytest.mark.parametrize("n,S,exact_w", [(1, 3, True), (5, 13, True), (1, 127, True), (3, 192, False), (1, 1, True), (1, 63, True),
                                         (1, 64, True), (1, 65, True)])
def test_lattice_backward_is_exact_in_fp32(n, S, exact_w):
    """The exact GPU tests' premise, audited on their own inputs: every partial sum of the chain, in any order, fits fp32, and so
    does every weight-gradient sum over the samples (dyadic columns) up to 127 samples.  The case must also hold pre-activations
    that are exactly 0 under a non-zero gradient: what tells the relu's `> 0` from `>= 0`."""
    sd = ref.lattice_state_dict()
    o, d, z = ref.lattice_rays(n, S)
    d_raw = tr.lattice_d_raw(n * S)
    assert set(np.unique(d_raw)) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    for m in ref.MODULES:
        fwd = tr.forward_tap(sd, m, ref.points_f32(o, d, z), ref.viewdirs_device(d))
        chain, weight = [], []
        bwd = tr.backward(sd, m, fwd["tap"], d_raw, audit=chain, audit_w=weight)
        print("%d x %d %s: chain %.1f bits, weight gradients %.1f bits" % (n, S, m, max(chain), max(weight)))
        assert max(chain) < 24
        assert (max(weight) < 24) == exact_w
        assert tr.zero_preactivations_under_gradient(fwd, bwd) > 0
        assert np.count_nonzero(bwd["dtap"][:, :256]) > 0, "the gradient reaches the first layer"
        assert np.array_equal(bwd["dtap"], bwd["dtap"].astype(np.float32))


def test_jitter_restates_the_reference_s_statements():
    """volume_renderer.py:56-70 in torch fp32 on the host (IEEE: one rounding per operation) gives jitter_f32's bits."""
    o, d, near, far = ref.fixture_rays()
    z = ref.coarse_depths_f32(near, far, 64)
    t_rand = np.random.RandomState(0).uniform(0, 1, z.shape).astype(np.float32)
    z_vals = torch.from_numpy(z)
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    want = lower + (upper - lower) * torch.from_numpy(t_rand)
    got = tr.jitter_f32(z, t_rand)
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert np.all(np.diff(got, axis=-1) >= 0) and np.all(got >= near[:, None]) and np.all(got <= far[:, None])


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(hp.GOLDEN + "/nerf_train_step.npz"))


def test_restatement_reproduces_the_reference_training_step(golden):
    """The whole step in float64 at the reference's own depths against what the unmodified reference computed in fp32: the losses
    to 1e-6, every gradient's probes and norm inside the budget, and the recorded distances are what the fixture says."""
    base = np.load(hp.GOLDEN + "/nerf_baseline.npz")
    sd = ref.make_state_dict(base["alpha_shift"])
    assert ref.checksum(sd) == str(base["weights_sha256"])
    o, d, near, far = ref.fixture_rays()
    assert np.array_equal(golden["z_coarse"], tr.jitter_f32(ref.coarse_depths_f32(near, far, 64), golden["t_rand"]))
    assert golden["t_rand"].max() < 1 and golden["u"].max() < 1 and 0 < golden["mask_at_box"].mean() < 1
    want = tr.train_step(sd, o, d, golden["z_coarse"], golden["z_fine"], golden["rgb"], golden["mask_at_box"], viewdirs=golden["viewdirs"])
    for key in ("loss", "img_loss", "img_loss0"):
        assert abs(float(golden[key]) - want[key]) <= 1e-6, key
    hp.assert_close(golden["ref_rgb_map"], want["rgb_map"], hp.RGB_TOL, "rgb_map")
    hp.assert_close(golden["ref_rgb0"], want["rgb0"], hp.RGB_TOL, "rgb0")
    names = [k[5:] for k in golden if k.startswith("norm/")]
    assert names == list(ref.state_dict_shapes()) and len(names) == 48
    assert 0 < float(golden["ref_err_worst"]) <= tr.GRAD_TOL
    for name in names:
        g = want["grads"][name]
        scale = np.abs(g).max()
        assert np.abs(g.reshape(-1)[golden["probe_idx/" + name]] - golden["probe/" + name]).max() <= tr.GRAD_TOL * scale, name
        assert abs(np.sqrt((g ** 2).sum()) - float(golden["norm/" + name])) <= tr.GRAD_TOL * np.sqrt(g.size) * scale, name
        assert float(golden["ref_err/" + name]) <= float(golden["ref_err_worst"])


def test_golden_holds_small_numeric_arrays_only():
    assert os.path.getsize(hp.GOLDEN + "/nerf_train_step.npz") < (1 << 20)
    with np.load(hp.GOLDEN + "/nerf_train_step.npz", allow_pickle=False) as g:
        assert all(g[k].dtype.kind in "fbi" for k in g.files)


# ------------------------------------------------------------------------------------------------ API
def test_default_refusals_are_unchanged_and_trainable_is_accepted():
    from neuralbody_amd.nerf import NerfNetwork, VolumeRenderer, VolumeRendererConfig

    net = NerfNetwork()
    assert net.trainable is False
    pts, vd = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(NotImplementedError, match="inference only"):
        net(pts, vd)
    net.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        net(pts, vd)
    batch = {"ray_o": torch.zeros(1, 2, 3), "ray_d": torch.ones(1, 2, 3), "near": torch.ones(1, 2), "far": 2 * torch.ones(1, 2)}
    with torch.no_grad(), pytest.raises(NotImplementedError, match="t_rand"):
        VolumeRenderer(net, VolumeRendererConfig()).render(batch, t_rand=torch.zeros(1, 2, 64))
    tnet = NerfNetwork(trainable=True, precision="f16x3")
    assert tnet.trainable and tnet.training and not tnet.eval().training and tnet.train().training
    assert tnet.nerf_precision() == "f16x3"  # governs inference only
    assert len(tnet.state_dict()) == 48
    r = VolumeRenderer(tnet, VolumeRendererConfig(perturb=1.0))
    assert r._jitters() and not VolumeRenderer(tnet.eval(), VolumeRendererConfig(perturb=1.0))._jitters()
    assert not VolumeRenderer(tnet.train(), VolumeRendererConfig(perturb=0.0))._jitters()
    assert not VolumeRenderer(net.train(), VolumeRendererConfig(perturb=1.0))._jitters()
    # the documented chunk rule: tap + d-tap of one pass below 8 GiB
    assert r.grad_chunk() == (8 << 30) // (192 * 4 * (2528 + 2432)) == 2255
    assert 1024 * 192 * 4 * (2528 + 2432) == 3900702720  # "3.9 GB, one chunk"
    assert VolumeRenderer(tnet, VolumeRendererConfig(N_samples=512, N_importance=0)).grad_chunk() >= 1
    # a host tensor is refused by the wrappers, not sent to a kernel
    with pytest.raises(Exception, match="HIP device"):
        tnet(pts, vd)


def test_param_names_are_the_module_s_parameters_in_order():
    from neuralbody_amd import nerf

    assert nerf.PARAM_NAMES == [k for k, _ in nerf.Nerf().named_parameters()] == tr.PARAM_NAMES


def test_plugins_switch_modes_only_when_trainable(monkeypatch):
    import sys

    cfg = types.SimpleNamespace(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10,
                                view_res=4, N_samples=64, N_importance=128, perturb=1, raw_noise_std=0, white_bkgd=False,
                                lindisp=False, chunk=32768, H=8, W=8, ratio=1.0)
    net = hp.load_plugin("nerf.py", cfg).Network()
    assert not net.trainable and not net.train().training
    cfg.nerf_trainable = True
    tnet = hp.load_plugin("nerf.py", cfg).Network()
    assert tnet.trainable and not tnet.training and tnet.train().training and tnet.model.training and not tnet.eval().training
    # nerf_trainer.py imports the package module volume_renderer, which binds `lib.config.cfg` on import: import it afresh against
    # the stand-in and put back whatever was there (as tests/test_mesh_host.py does for if_clight_renderer)
    monkeypatch.setitem(sys.modules, "neuralbody_amd.plugins.volume_renderer", None)
    del sys.modules["neuralbody_amd.plugins.volume_renderer"]
    mod = hp.load_plugin("nerf_trainer.py", cfg)
    wrap = mod.NetworkWrapper(net)
    assert wrap.net is net and wrap.renderer.net is net and wrap.renderer.cfg.N_importance == 128
    with pytest.raises(RuntimeError, match="nerf_trainable"):
        wrap({})
    assert mod.NetworkWrapper(tnet).renderer._jitters() is False and mod.NetworkWrapper(tnet.train()).renderer._jitters() is True


def test_new_entries_check_their_arguments_without_a_device():
    from neuralbody_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    assert lib.nb_abi_version() == 20
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nb_hip.h")) as f:
        header = f.read()
    for name in ("nb_nerf_decode_tap", "nb_nerf_pack_bwd", "nb_nerf_bwd_chain"):
        assert "int %s(" % name in header and name in _lib.SIGNATURES
    assert "#define NB_ABI_VERSION 20" in header and "#define NB_NERF_TAP_COLS 2528" in header and "#define NB_NERF_DTAP_COLS 2432" in header
    # nine transposed matrices (K = 128 once, 256 eight times, 256 features each) + rgb_linear's and alpha_linear's weights
    assert lib.nb_nerf_pack_bwd_size() == 256 * 128 + 8 * 256 * 256 + 384 + 256
    # nb_nerf_decode_tap: nb_nerf_decode's checks, plus the tap
    assert lib.nb_nerf_decode_tap(None, None, None, None, 0, 64, None, None, None) == 0  # n_rays == 0: at once
    for args, word in (((None, None, None, None, 4, 64, None, None, None), b"NULL"),
                       ((16, 16, 16, 16, 4, 64, 16, None, None), b"NULL"),
                       ((None, None, None, None, 4, 0, None, None, None), b"n_samples"),
                       ((None, None, None, None, 4, 513, None, None, None), b"n_samples"),
                       ((None, None, None, None, -1, 64, None, None, None), b"n_rays"),
                       ((16, 16, 16, 16, 4, 64, 18, 16, None), b"4-byte aligned"),
                       ((16, 16, 16, 16, 4, 64, 16, 8, None), b"16-byte aligned"),
                       ((8, 16, 16, 16, 4, 64, 16, 16, None), b"16-byte aligned")):
        assert lib.nb_nerf_decode_tap(*args) == -1 and word in lib.nb_last_error(), (args, lib.nb_last_error())
    # nb_nerf_pack_bwd
    assert lib.nb_nerf_pack_bwd(None, None, None) == -1 and b"NULL" in lib.nb_last_error()
    params = _lib.NbNerfParams()
    assert lib.nb_nerf_pack_bwd(C.byref(params), 16, None) == -1 and b"NULL weight" in lib.nb_last_error()
    for i in range(8):
        params.pts_w[i] = 16
    for f in ("views_w", "feature_w", "alpha_w"):
        setattr(params, f, 16)
    params.rgb_w = 18  # the biases stay NULL: they are not read
    assert lib.nb_nerf_pack_bwd(C.byref(params), 16, None) == -1 and b"4-byte aligned" in lib.nb_last_error()
    params.rgb_w = 16
    assert lib.nb_nerf_pack_bwd(C.byref(params), 8, None) == -1 and b"16-byte aligned" in lib.nb_last_error()
    # nb_nerf_bwd_chain
    assert lib.nb_nerf_bwd_chain(None, None, None, 0, None, None) == 0  # n_pts == 0: at once
    for args, word in (((None, None, None, 5, None, None), b"NULL"), ((16, 16, 16, 5, None, None), b"NULL"),
                       ((None, None, None, -1, None, None), b"n_pts"), ((None, None, None, 1 << 37, None, None), b"n_pts"),
                       ((16, 8, 16, 5, 16, None), b"16-byte aligned"), ((16, 16, 16, 5, 24, None), b"16-byte aligned"),
                       ((16, 16, 18, 5, 16, None), b"4-byte aligned")):
        assert lib.nb_nerf_bwd_chain(*args) == -1 and word in lib.nb_last_error(), (args, lib.nb_last_error())
