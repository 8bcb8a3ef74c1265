"""The vanilla-NeRF baseline's training step on the device (run with -m gpu on an MI355X): nb_nerf_decode_tap and
nb_nerf_bwd_chain bit for bit on the exact lattice against the float64 model of tests/nerf_train_ref.py, the 24 parameter
gradients of both modules (exact where the audit of tests/test_nerf_train_host.py says they are, inside the gradient budget
elsewhere), one whole step on the fixture against the float64 step fed the device's own depths and against the loss the
unmodified reference recorded (tests/golden/nerf_train_step.npz), and the plugins with an optimizer.

The lattice's sine and cosine embedding columns are no dyadic numbers: the device forms them with the hardware sine
(include/nb_hip.h, nb_nerf_decode: <= 4e-7 absolute), so those tap columns are held to that bound and the weight-gradient columns
that meet them to the gradient budget; every other column is compared for equality.  Those sine and cosine columns are
still held bit for bit to what nb_nerf_decode computes: they are copies of the LDS rows that the first, the skip and the view
layer read, and raw, which depends on them, must equal nb_nerf_decode(f32)'s raw bit for bit (on the fixture's weights, where
their weights are not zero: test_tapped_raw_keeps_its_bits_with_the_fixture_weights)."""
import sys
import types

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import nerf_ref as ref
from tests import nerf_train_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATTICE = [(1, 3), (5, 13), (1, 127), (3, 192)]  # 65 = one tile + 1, 127 = two tiles - 1, 576 = nine tiles
POISON = -123.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from neuralbody_amd import _lib

    _lib.lib()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _net(sd, trainable=True, precision="f32"):
    from neuralbody_amd.nerf import NerfNetwork

    net = NerfNetwork(precision=precision, trainable=trainable)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(DEV)


def _params(sd, m):
    return {k[len(m) + 1:]: _dev(v) for k, v in sd.items() if k.startswith(m + ".")}


def _sincos_columns():
    """Tap columns that hold a sine or a cosine."""
    return np.concatenate([np.arange(tr.TAP_PTS + 3, tr.TAP_PTS + 63), np.arange(tr.TAP_VIEW + 3, tr.TAP_VIEW + 27)])


_LATTICE_CACHE = {}


def _lattice(n, S, m):
    """(sd, rays, the float64 forward and backward of module m) on the lattice, once per shape and module."""
    key = (n, S, m)
    if key not in _LATTICE_CACHE:
        sd = ref.lattice_state_dict()
        o, d, z = ref.lattice_rays(n, S)
        fwd = tr.forward_tap(sd, m, ref.points_f32(o, d, z), ref.viewdirs_device(d))
        d_raw = tr.lattice_d_raw(n * S)
        chain, weight = [], []
        bwd = tr.backward(sd, m, fwd["tap"], d_raw, audit=chain, audit_w=weight)
        assert max(chain) < 24 and tr.zero_preactivations_under_gradient(fwd, bwd) > 0
        _LATTICE_CACHE[key] = (sd, (o, d, z), fwd, d_raw, bwd, max(weight))
    return _LATTICE_CACHE[key]


def _differ(got, want, what):
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %s: %r vs %r" % (what, len(bad), want.size, bad[0], got[tuple(bad[0])],
                                                                          want[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ 1: the tap
@pytest.mark.parametrize("n,S", LATTICE)
def test_tap_is_exact_on_the_lattice_and_raw_keeps_its_bits(n, S):
    from neuralbody_amd import ops

    sincos = _sincos_columns()
    exact = np.setdiff1d(np.arange(tr.TAP_COLS), sincos)
    for m in ref.MODULES:
        sd, (o, d, z), fwd, _, _, _ = _lattice(n, S, m)
        packed = ops.nerf_pack(_params(sd, m), "f32")
        raw = ops.nerf_decode(packed, _dev(o), _dev(d), _dev(z), "f32")
        # the tap sits at the head of a larger poisoned buffer: the padding samples of the last tile must store nothing
        n_pts = n * S
        buf = torch.full(((n_pts + 70) * tr.TAP_COLS,), POISON, device=DEV)
        raw_t, tap = ops.nerf_decode_tap(packed, _dev(o), _dev(d), _dev(z), tap=buf[:n_pts * tr.TAP_COLS].view(n_pts, tr.TAP_COLS))
        assert hp.same_bits(raw_t, raw), "the tapped kernel's raw is nb_nerf_decode(f32)'s, bit for bit"
        assert bool((buf[n_pts * tr.TAP_COLS:] == POISON).all()), "rows past n_pts were written"
        got = tap.cpu().numpy()
        _differ(got[:, exact], fwd["tap"][:, exact], "%s tap" % m)
        assert np.abs(got[:, sincos] - fwd["tap"][:, sincos]).max() <= tr.EMBED_TOL
        _differ(raw_t.cpu().numpy().reshape(-1, 4), fwd["raw"], "%s raw" % m)
        assert hp.same_bits(ops.nerf_decode_tap(packed, _dev(o), _dev(d), _dev(z))[1], tap)


def test_tapped_raw_keeps_its_bits_with_the_fixture_weights(sd):
    """Random weights read every embedding column, so equal raw also pins the sine and cosine rows to nb_nerf_decode's; the tap's
    copies of them are then within the encoding's bound of the float64 sine."""
    from neuralbody_amd import ops

    o, d, near, far = ref.fixture_rays()
    z = ref.coarse_depths_f32(near, far, 67)  # 96 x 67 = 6432 samples: 100 tiles and a half
    sincos = _sincos_columns()
    for m in ref.MODULES:
        packed = ops.nerf_pack(_params(sd, m), "f32")
        raw = ops.nerf_decode(packed, _dev(o), _dev(d), _dev(z), "f32")
        raw_t, tap = ops.nerf_decode_tap(packed, _dev(o), _dev(d), _dev(z))
        assert hp.same_bits(raw_t, raw)
        want = tr.forward_tap(sd, m, ref.points_f32(o, d, z), ref.viewdirs_device(d))["tap"]
        assert np.abs(tap.cpu().numpy()[:, sincos] - want[:, sincos]).max() <= tr.EMBED_TOL


# ------------------------------------------------------------------------------------------------ 2: the chain
@pytest.mark.parametrize("n,S", LATTICE + [(1, 1), (1, 63), (1, 64), (1, 65)])
def test_chain_is_exact_on_the_lattice(n, S):
    """Fed the float64 model's tap (exact in fp32 on every column the chain reads), so the chain stands on its own."""
    from neuralbody_amd import ops

    for m in ref.MODULES:
        sd, _, fwd, d_raw, bwd, _ = _lattice(n, S, m)
        n_pts = n * S
        tap = fwd["tap"].astype(np.float32)
        read = np.arange(tr.TAP_PTS)  # h0 .. h7, feature, V
        assert np.array_equal(tap[:, read].astype(np.float64), fwd["tap"][:, read])
        blob = ops.nerf_pack_bwd(_params(sd, m))
        dtap = torch.full((n_pts + 70, tr.DTAP_COLS), POISON, device=DEV)
        out = ops.nerf_bwd_chain(blob, _dev(tap), _dev(d_raw), dtap=dtap)
        assert out.data_ptr() == dtap.data_ptr()
        got = dtap.cpu().numpy()
        assert np.all(got[n_pts:] == POISON), "rows past n_pts were written"
        _differ(got[:n_pts], bwd["dtap"], "%s d-tap" % m)
        again = ops.nerf_bwd_chain(blob, _dev(tap), _dev(d_raw).view(n, S, 4))  # no atomics: the same bits; d_raw [n,S,4] as well
        assert hp.same_bits(again, dtap[:n_pts])


# ------------------------------------------------------------------------------------------------ 3: parameter gradients
def _module_grads(net, model, o, d, z, d_raw):
    net.zero_grad(set_to_none=True)
    with torch.enable_grad():
        raw = net.decode(_dev(o), _dev(d), _dev(z), model=model)
        raw.backward(_dev(d_raw).view(raw.shape))
    mod = net.model_fine if model == "fine" else net.model
    return raw.detach(), {k: p.grad.cpu().numpy() for k, p in mod.named_parameters()}


@pytest.mark.parametrize("n,S", [(1, 3), (5, 13), (1, 127)])
def test_parameter_gradients_are_exact_on_the_lattice(n, S):
    """Up to 127 samples every weight-gradient sum over the samples is exact in fp32 (audited), so the split-K atomics' order
    cannot show: all 24 tensors of both modules equal the float64 model on the dyadic columns; the columns of a sine or cosine
    are inside the budget."""
    for m, model in (("model", ""), ("model_fine", "fine")):
        sd, (o, d, z), fwd, d_raw, bwd, bits = _lattice(n, S, m)
        assert bits < 24
        net = _net(sd)
        raw, grads = _module_grads(net, model, o, d, z, d_raw)
        _differ(raw.cpu().numpy().reshape(-1, 4), fwd["raw"], "raw")
        other = net.model if model == "fine" else net.model_fine
        assert all(p.grad is None for p in other.parameters()), "only the module that was called gets gradients"
        assert list(grads) == tr.PARAM_NAMES
        for name, g in grads.items():
            want = bwd["grads"][name]
            assert g.shape == want.shape, name
            if name.endswith(".weight"):
                cols = tr.dyadic_columns(name[:-7])
                _differ(g[:, cols], want[:, cols], "%s %s" % (m, name))
                rest = np.setdiff1d(np.arange(want.shape[1]), cols)
                if rest.size:
                    assert tr.rel_err(g[:, rest], want[:, rest]) <= tr.GRAD_TOL, name
            else:
                _differ(g, want, "%s %s" % (m, name))


def test_parameter_gradients_on_the_bf16_pair_path():
    """1024 samples: the weight-gradient products of the 256-wide layers run as bf16 head + remainder pairs (~2^-16 relative)."""
    from neuralbody_amd import ops

    n, S = 8, 128
    probe = torch.empty((n * S, tr.TAP_COLS), device=DEV)
    assert ops.gemm_variant(probe[:, 256:512], probe[:, 0:256], trans_a=True) == "TN16"
    worst = 0.0
    for m, model in (("model", ""), ("model_fine", "fine")):
        sd, (o, d, z), _, d_raw, bwd, _ = _lattice(n, S, m)
        _, grads = _module_grads(_net(sd), model, o, d, z, d_raw)
        for name, g in grads.items():
            worst = max(worst, tr.rel_err(g, bwd["grads"][name]))
            assert tr.rel_err(g, bwd["grads"][name]) <= tr.GRAD_TOL, (m, name)
    print("1024 lattice samples, worst gradient error %.3e" % worst)


# ------------------------------------------------------------------------------------------------ 4: the whole step
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(hp.GOLDEN + "/nerf_train_step.npz"))


@pytest.fixture(scope="module")
def sd():
    base = np.load(hp.GOLDEN + "/nerf_baseline.npz")
    sd = ref.make_state_dict(base["alpha_shift"])
    assert ref.checksum(sd) == str(base["weights_sha256"])
    return sd


def _batch(golden):
    o, d, near, far = ref.fixture_rays()
    b = {"ray_o": _dev(o)[None], "ray_d": _dev(d)[None], "near": _dev(near)[None], "far": _dev(far)[None],
         "rgb": _dev(golden["rgb"])[None], "mask_at_box": torch.from_numpy(golden["mask_at_box"]).to(DEV)[None]}
    return b, _dev(golden["t_rand"])[None], _dev(golden["u"])[None]


def _loss(ret, batch):
    mask = batch["mask_at_box"]
    img = torch.mean((ret["rgb_map"][mask] - batch["rgb"][mask]) ** 2)
    img0 = torch.mean((ret["rgb0"] - batch["rgb"]) ** 2)
    return img + img0, img, img0


def _step(net, golden, loss_fn=_loss, **cfg):
    from neuralbody_amd.nerf import VolumeRenderer, VolumeRendererConfig

    batch, t_rand, u = _batch(golden)
    net.train()
    net.zero_grad(set_to_none=True)
    r = VolumeRenderer(net, VolumeRendererConfig(**{"N_samples": 64, "N_importance": 128, "perturb": 1.0, **cfg}))
    with torch.enable_grad():
        ret = r.render(batch, t_rand=t_rand, u=u)
        losses = loss_fn(ret, batch)
        losses[0].backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters()}
    return ret, losses, grads


@pytest.fixture(scope="module")
def step(sd, golden):
    """One step on the device and the float64 step at the device's own depths, shared by the tests below."""
    net = _net(sd)
    ret, losses, grads = _step(net, golden)
    o, d, near, far = ref.fixture_rays()
    z_coarse = tr.jitter_f32(ref.coarse_depths_f32(near, far, 64), golden["t_rand"])
    z_vals = ret["z_vals"][0].detach().cpu().numpy()
    want = tr.train_step(sd, o, d, z_coarse, z_vals, golden["rgb"], golden["mask_at_box"])
    return {"net": net, "ret": ret, "losses": [float(v.detach()) for v in losses], "grads": grads, "z_coarse": z_coarse, "z_vals": z_vals,
            "want": want}


def test_jitter_is_the_reference_s_bit_for_bit(sd, golden, step):
    from neuralbody_amd.nerf import VolumeRenderer, VolumeRendererConfig

    batch, t_rand, u = _batch(golden)
    net = step["net"].train()
    with torch.no_grad():
        coarse = VolumeRenderer(net, VolumeRendererConfig(N_importance=0, perturb=1.0)).render(batch, t_rand=t_rand)
        still = VolumeRenderer(net.eval(), VolumeRendererConfig(N_importance=0, perturb=1.0)).render(batch, t_rand=t_rand)
        drawn = VolumeRenderer(net.train(), VolumeRendererConfig(N_importance=0, perturb=1.0)).render(batch)
    o, d, near, far = ref.fixture_rays()
    z = coarse["z_vals"][0].cpu().numpy()
    assert np.array_equal(z, step["z_coarse"]) and np.array_equal(z, golden["z_coarse"])
    assert np.array_equal(still["z_vals"][0].cpu().numpy(), ref.coarse_depths_f32(near, far, 64)), "no jitter in eval mode"
    zr = drawn["z_vals"][0].cpu().numpy()  # torch.rand on the device
    assert not np.array_equal(zr, z)
    for zz in (z, zr, step["z_vals"]):
        assert np.all(np.diff(zz, axis=-1) >= 0) and np.all(zz >= near[:, None]) and np.all(zz <= far[:, None])
    # nb_importance_sample, handed the same t_rand, forms these very depths for its bins
    from neuralbody_amd import ops

    w = torch.rand((96, 64), device=DEV)
    smp = ops.importance_sample(batch["ray_o"][0], batch["ray_d"][0], batch["near"][0], batch["far"][0],
                                torch.linspace(0.0, 1.0, 64).to(DEV), t_rand[0].contiguous(), w, u[0].contiguous())
    assert hp.same_bits(smp["z_coarse"], coarse["z_vals"][0])
    # the fine pass evaluates every jittered coarse depth again (volume_renderer.py:93)
    assert all(np.isin(step["z_coarse"][i], step["z_vals"][i]).all() for i in range(z.shape[0]))


def test_step_maps_and_loss(golden, step):
    ret, want = step["ret"], step["want"]
    assert tuple(ret["weights"].shape) == (1, 96, 192) and ret["rgb_map"].requires_grad and ret["rgb0"].requires_grad
    for key in ("rgb_map", "rgb0"):
        e = hp.assert_close(ret[key][0].detach().cpu().numpy(), want[key], hp.RGB_TOL, key)
        print("%s: %.3e" % (key, e))
    print("loss %.8f, float64 at the device's depths %.8f, golden %.8f" % (step["losses"][0], want["loss"], float(golden["loss"])))
    for got, key in zip(step["losses"], ("loss", "img_loss", "img_loss0")):
        assert abs(got - float(golden[key])) <= 1e-5, key
        assert abs(got - want[key]) <= 1e-5, key


def test_step_gradients_against_float64(golden, step):
    """All 48 gradients: max |diff| / max |ref| <= 1e-4 against the float64 step at the device's depths.  Measured on the MI355X:
    see DESIGN.md 4.21 (printed here, beside the reference's own fp32 distance recorded in the fixture)."""
    errs = {k: tr.rel_err(step["grads"][k], g) for k, g in step["want"]["grads"].items()}
    assert len(errs) == 48 and all(step["grads"][k].shape == g.shape for k, g in step["want"]["grads"].items())
    worst = max(errs, key=errs.get)
    print("worst gradient error %.3e (%s); the reference's own %.3e" % (errs[worst], worst, float(golden["ref_err_worst"])))
    assert errs[worst] <= tr.GRAD_TOL, errs


def test_a_cotangent_on_the_accumulation_maps_reaches_both_modules(sd, golden, step):
    """acc_map belongs to the fine pass and acc0 to the coarse one: z_samples are detached, so a cotangent on acc_map ALONE leaves
    the coarse module without a gradient, and each module's gradient is the float64 one.

    The reference here is the float64 backward at the DEVICE's activation pattern (its tap decides the relu masks; the values of the
    tap, the composite and its backward are float64 at the float64 forward otherwise): a gradient of a relu network is a
    discontinuous function of a pre-activation at 0, and a cotangent of order 1 on a density of order 100 (alpha_linear x 20 in
    the fixture's recipe) turns ONE unit of ONE sample whose pre-activation fp32 and float64 round to different sides of 0 into
    several 1e-4 of a whole weight gradient.  Against the pure float64 pattern the figure is printed; the step's own 48 gradients
    (test_step_gradients_against_float64) are held to pure float64."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(7)
    g_acc, g_acc0 = rs.normal(size=96), rs.normal(size=96)
    net = step["net"]

    def only_acc(ret, batch):
        return ((ret["acc_map"][0, :, 0] * _dev(g_acc)).sum(),)

    def both(ret, batch):
        return ((ret["acc_map"][0, :, 0] * _dev(g_acc)).sum() + (ret["acc0"][0, :, 0] * _dev(g_acc0)).sum(),)

    ret, _, grads = _step(net, golden, only_acc)
    assert np.array_equal(ret["z_vals"][0].detach().cpu().numpy(), step["z_vals"])
    assert all(g is None for k, g in grads.items() if k.startswith("model.")), "z_samples are detached"
    _, _, grads2 = _step(net, golden, both)
    o, d, _, _ = ref.fixture_rays()
    v = ref.viewdirs_device(d)
    pure = 0.0
    for m, model, z, g_map in (("model", "", step["z_coarse"], g_acc0), ("model_fine", "fine", step["z_vals"], g_acc)):
        fwd = tr.forward_tap(sd, m, ref.points_f32(o, d, z), v)
        d_raw = tr.composite_bwd(fwd["raw"].reshape(96, -1, 4), z, d, g_acc=g_map)
        dev_tap = ops.nerf_decode_tap(ops.nerf_pack(_params(sd, m), "f32"), _dev(o), _dev(d), _dev(z))[1].cpu().numpy().astype(np.float64)
        flips = int(np.sum((dev_tap[:, :tr.TAP_PTS] > 0) != (fwd["tap"][:, :tr.TAP_PTS] > 0)))
        print("%s: %d of %d units on the other side of 0 than in float64" % (m, flips, dev_tap[:, :tr.TAP_PTS].size))
        assert flips <= 32  # of 1.5e7 / 4.5e7 units: fp32 and float64 may disagree only where a pre-activation rounds to 0
        tap = fwd["tap"].copy()
        on = dev_tap[:, :tr.TAP_PTS] > 0
        tap[:, :tr.TAP_PTS] = np.where(on, np.maximum(tap[:, :tr.TAP_PTS], np.finfo(np.float64).tiny), 0.0)  # the device's pattern
        tap[:, tr.TAP_FEATURE:tr.TAP_FEATURE + 256] = fwd["tap"][:, tr.TAP_FEATURE:tr.TAP_FEATURE + 256]  # (no activation: as it was)
        want = tr.backward(sd, m, tap, d_raw)["grads"]
        want64 = tr.backward(sd, m, fwd["tap"], d_raw)["grads"]
        for name, g in want.items():
            key = "%s.%s" % (m, name)
            pure = max(pure, tr.rel_err(grads2[key], want64[name]))
            assert tr.rel_err(grads2[key], g) <= tr.GRAD_TOL, key
            if m == "model_fine":
                assert tr.rel_err(grads[key], g) <= tr.GRAD_TOL, key
    print("against the pure float64 activation pattern: %.3e" % pure)


def test_uneven_chunks_give_the_same_gradients(golden, step):
    ret, losses, grads = _step(step["net"], golden, chunk=37)  # 96 rays: 37 + 37 + 22
    assert np.array_equal(ret["z_vals"][0].detach().cpu().numpy(), step["z_vals"])
    assert abs(float(losses[0].detach()) - step["losses"][0]) <= 1e-6
    for k, g in step["grads"].items():
        assert tr.rel_err(grads[k], g) <= tr.GRAD_TOL, k


# ------------------------------------------------------------------------------------------------ 5: plugins
_CFG = dict(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10, view_res=4, N_samples=64,
            N_importance=128, perturb=1, raw_noise_std=0, white_bkgd=False, lindisp=False, chunk=32768, H=8, W=12, ratio=1.0,
            nerf_trainable=True, nerf_precision="f32")


def test_training_through_the_plugins(sd, golden, monkeypatch):
    cfg = types.SimpleNamespace(**_CFG)
    net = hp.load_plugin("nerf.py", cfg).Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(DEV)
    # nerf_trainer.py imports the package module volume_renderer, which binds `lib.config.cfg` on import: afresh, and put back
    monkeypatch.setitem(sys.modules, "neuralbody_amd.plugins.volume_renderer", None)
    del sys.modules["neuralbody_amd.plugins.volume_renderer"]
    wrap = hp.load_plugin("nerf_trainer.py", cfg).NetworkWrapper(net)
    assert wrap.train().training and net.training
    batch, t_rand, u = _batch(golden)
    render = wrap.renderer.render
    wrap.renderer.render = lambda b: render(b, t_rand=t_rand, u=u)  # fixed randomness
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)

    ret, loss, stats, image_stats = wrap(batch)
    assert set(stats) == {"img_loss", "img_loss0", "loss"} and image_stats == {}
    assert abs(float(loss.detach()) - float(golden["loss"])) <= 1e-5
    slots = [net._memo.peek("train"), net._memo.peek("train_fine")]
    assert all(s is not None and len(s) == 2 for s in slots)
    raw_before = ret["raw"].detach().clone()
    opt.zero_grad()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    opt.step()
    # the next forward runs the new weights: both blobs of both modules are rebuilt, raw is the float64 model of the new state dict
    ret2, loss2, _, _ = wrap(batch)
    assert net._memo.peek("train") is not slots[0] and net._memo.peek("train_fine") is not slots[1]
    new_sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    o, d, _, _ = ref.fixture_rays()
    z = ret2["z_vals"][0].detach().cpu().numpy()
    want = ref.forward(new_sd, "model_fine", ref.points_f32(o, d, z), ref.viewdirs_device(d))
    hp.assert_close(ret2["raw"][0].detach().cpu().numpy().reshape(96, 192, 4), want, 1e-4, "raw after the step")  # test_nerf_host.py: RAW_REL_TOL
    assert float((ret2["raw"] - raw_before).abs().max()) > 1e-2, "the step changed nothing"
    again = net._memo.peek("train")
    wrap(batch)
    assert net._memo.peek("train") is again, "no parameter changed: no repack"
    # ten steps at the reference's learning rate lower the loss
    first = float(loss.detach())
    for _ in range(10):
        _, l, _, _ = wrap(batch)
        opt.zero_grad()
        l.backward()
        opt.step()
    with torch.no_grad():
        last = float(wrap(batch)[1])
    print("loss %.6f -> %.6f after eleven Adam steps" % (first, last))
    assert last < first
    # evaluation as run.py does it: eval mode, no gradients, no jitter, the inference kernel
    wrap.eval()
    with torch.no_grad():
        out = wrap.renderer.render(batch)
    assert "weights" not in out and not out["rgb_map"].requires_grad


def test_wrapper_refuses_gradients_on_an_inference_network(sd, golden, monkeypatch):
    cfg = types.SimpleNamespace(**{**_CFG, "nerf_trainable": False})
    net = hp.load_plugin("nerf.py", cfg).Network().to(DEV)
    monkeypatch.setitem(sys.modules, "neuralbody_amd.plugins.volume_renderer", None)
    del sys.modules["neuralbody_amd.plugins.volume_renderer"]
    wrap = hp.load_plugin("nerf_trainer.py", cfg).NetworkWrapper(net)
    batch, _, _ = _batch(golden)
    with pytest.raises(RuntimeError, match="nerf_trainable"):
        wrap(batch)
    with torch.no_grad():
        ret, loss, _, _ = wrap(batch)
    assert bool(torch.isfinite(loss)) and "weights" not in ret
