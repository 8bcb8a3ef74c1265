"""The vanilla-NeRF baseline on the device (run with -m gpu on an MI355X): nb_nerf_decode bit for bit on an exact lattice and
against the float64 model of tests/nerf_ref.py with the fixture's weights, VolumeRenderer end to end against that model fed the
device's own depths, nb_importance_merge_z against a stable sort, the checkpoint round trip and the consumers of the dict."""
import types

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import nerf_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 64  # samples per workgroup of nb_nerf_decode


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from neuralbody_amd import _lib

    _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _net(sd, precision="f32"):
    from neuralbody_amd.nerf import NerfNetwork

    net = NerfNetwork(precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(DEV).eval()


def _precisions():
    from neuralbody_amd import ops

    return sorted(ops.NERF_PRECISIONS)  # every arithmetic that is built


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(hp.GOLDEN + "/nerf_baseline.npz"))


@pytest.fixture(scope="module")
def sd(fx):
    sd = ref.make_state_dict(fx["alpha_shift"])
    assert ref.checksum(sd) == str(fx["weights_sha256"]), "the seed recipe no longer gives the fixture's weights"
    return sd


@pytest.fixture(scope="module")
def model64(fx, sd):
    """float64 passes of the fixture's rays at given fp32 depths with the device's direction, computed once per depth array."""
    cache = {}

    def run(module, z, white_bkgd=False):
        key = (module, z.tobytes())
        if key not in cache:
            cache[key] = ref.forward(sd, module, ref.points_f32(fx["ray_o"], fx["ray_d"], z), ref.viewdirs_device(fx["ray_d"]))
        raw = cache[key]
        rgb, disp, acc, weights, depth = ref.raw2outputs(raw, z, fx["ray_d"], white_bkgd)
        return {"raw": raw, "rgb_map": rgb, "disp_map": disp, "acc_map": acc, "weights": weights, "depth_map": depth}

    return run


@pytest.fixture(scope="module")
def e_ref(fx, sd):
    """The reference's own fp32 forward against the float64 model at the same points and directions (its own, fp32-normalised):
    what fp32 arithmetic costs on this field.  The device is allowed 8 x that."""
    e = 0.0
    for m, z, want in (("model", fx["z_coarse"], fx["raw_coarse"]), ("model_fine", fx["z_fine"], fx["raw_fine"])):
        got = ref.forward(sd, m, ref.points_f32(fx["ray_o"], fx["ray_d"], z), fx["viewdirs"])
        e = max(e, float(np.abs(got - want).max()))
    print("e_ref = %.3e" % e)
    assert 0.0 < e < 1e-4
    return e


# ------------------------------------------------------------------------------------------------ 1: exact lattice
@pytest.mark.parametrize("n,S", [(1, 3), (5, 67), (5, 13), (1, 2 * TILE - 1), (3, 192)])  # 5 x 13: one tile + 1; 127: two tiles - 1
def test_decode_is_exact_on_the_lattice(n, S):
    """Dyadic weights and inputs: every product and partial sum is exact in fp32, so any summation order must give the float64
    model's numbers (compared as values: a zero's sign is not part of them).  The premise is audited for these very inputs."""
    from neuralbody_amd import ops

    sd = ref.lattice_state_dict()
    o, d, z = ref.lattice_rays(n, S)
    for prec in _precisions():
        net = _net(sd, prec)
        for m, model in (("model", ""), ("model_fine", "fine")):
            audit = []
            want = ref.forward(sd, m, ref.points_f32(o, d, z), ref.viewdirs_device(d), audit=audit)
            assert max(audit) < 24
            with torch.no_grad():
                got = net.decode(_dev(o), _dev(d), _dev(z), model=model).cpu().numpy()
            assert got.shape == (n, S, 4) and got.dtype == np.float32
            bad = np.argwhere(got.astype(np.float64) != want)
            assert bad.size == 0, "%s %s: %d of %d differ, first at %s: %r vs %r" % (
                prec, m, len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
            with torch.no_grad():  # no atomics: the same bits again
                again = net.decode(_dev(o), _dev(d), _dev(z), model=model)
            assert hp.same_bits(again, _dev(got))


# ------------------------------------------------------------------------------------------------ 2: random weights
def test_decode_f32_against_float64_at_the_fixture_depths(fx, sd, model64, e_ref):
    net = _net(sd, "f32")
    worst = 0.0
    for m, model, z in (("model", "", fx["z_coarse"]), ("model_fine", "fine", fx["z_fine"])):
        with torch.no_grad():
            got = net.decode(_dev(fx["ray_o"]), _dev(fx["ray_d"]), _dev(z), model=model).cpu().numpy()
        gap = float(np.abs(got - model64(m, z)["raw"]).max())
        print("%s: device gap %.3e, e_ref %.3e, allowed %.3e" % (m, gap, e_ref, 8 * e_ref))
        worst = max(worst, gap)
    assert worst <= 8 * e_ref


# ------------------------------------------------------------------------------------------------ 3: render
def _render(net, fx, **kw):
    from neuralbody_amd.nerf import VolumeRenderer, VolumeRendererConfig

    cfg = VolumeRendererConfig(**{"N_samples": 64, "N_importance": 128, "perturb": 0.0, **kw})
    batch = {k: _dev(fx[k])[None] for k in ("ray_o", "ray_d", "near", "far")}
    with torch.no_grad():
        out = VolumeRenderer(net, cfg).render(batch)
    torch.cuda.synchronize()
    return out


def _check_render(out, fx, model64, e_ref, N, white_bkgd, tol=hp.RGB_TOL, raw_tol=True, worst=None):
    """tol: what every map is held to (None: measure only); worst: a dict that receives each map's largest error."""
    n, S = fx["ray_o"].shape[0], 64
    T = S + N
    shapes = {"rgb_map": (1, n, 3), "disp_map": (1, n, 1), "acc_map": (1, n, 1), "depth_map": (1, n), "raw": (1, n, T * 4),
              "z_vals": (1, n, T)}
    if N:
        shapes.update(rgb0=(1, n, 3), disp0=(1, n, 1), acc0=(1, n, 1), z_std=(1, n, 1))
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    got = {k: v[0].cpu().numpy() for k, v in out.items()}
    z_coarse = ref.coarse_depths_f32(fx["near"], fx["far"], S)
    z_vals = got["z_vals"]
    assert np.all(np.diff(z_vals, axis=-1) >= 0)
    coarse = model64("model", z_coarse, white_bkgd)
    last = [coarse["raw"][:, -1, 3]]
    span = (fx["far"] - fx["near"]).astype(np.float64)
    checks = []
    if N:
        fine = model64("model_fine", z_vals, white_bkgd)
        last.append(fine["raw"][:, -1, 3])
        checks += [("rgb0", coarse["rgb_map"]), ("acc0", coarse["acc_map"][:, None]), ("disp0", coarse["disp_map"][:, None])]
    else:
        fine = coarse
        assert np.array_equal(z_vals, z_coarse)
    checks += [("rgb_map", fine["rgb_map"]), ("acc_map", fine["acc_map"][:, None]), ("disp_map", fine["disp_map"][:, None])]
    # the 1e10 last interval makes the sign of the last density decide its ray: leave out the rays where it is within tolerance of 0
    keep = np.all(np.abs(np.stack(last)) > 8 * e_ref, axis=0)
    assert keep.mean() >= 0.99, "at most 1 % of rays may be left out"
    loose = np.inf if tol is None else tol
    for key, want in checks:
        e = hp.assert_close(got[key][keep], want[keep], loose, key)
        print("%s: %.3e" % (key, e))
        if worst is not None:
            worst[key] = e
    e = hp.assert_close(got["depth_map"][keep] / span[keep], fine["depth_map"][keep] / span[keep], loose, "depth_map", rel=False)
    print("depth_map / (far - near): %.3e" % e)
    if worst is not None:
        worst["depth_map"] = e
        worst["raw"] = float(np.abs(got["raw"].reshape(n, T, 4) - fine["raw"]).max())
    if raw_tol:  # the parity mode's raw: the same fp32 arithmetic as the reference's in another order
        hp.assert_close(got["raw"].reshape(n, T, 4), fine["raw"], 8 * e_ref, "raw", rel=False)
    return got, z_coarse


FAST_BUDGET = 1e-4  # README: the contract on every map (the tests of an arithmetic that serves as default hold half of it)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_render_two_passes(fx, sd, model64, e_ref, precision):
    from neuralbody_amd import nerf, ops

    net = _net(sd, precision)
    out = _render(net, fx)
    if precision == "f16x3" and nerf.AUTO_ARITHMETIC != "f16x3":
        # the fast arithmetic missed its budget and 'auto' avoids it: it still runs here, as an expected, recorded miss
        worst = {}
        _check_render(out, fx, model64, e_ref, 128, False, tol=None, raw_tol=False, worst=worst)
        pytest.xfail("f16x3 is not the default: measured %s" % worst)
    got, z_coarse = _check_render(out, fx, model64, e_ref, 128, False, raw_tol=precision == "f32")
    # z_vals = sort(coarse U fine) as a multiset, the fine depths being nb_importance_sample's of the coarse pass's weights
    with torch.no_grad():
        o, d = _dev(fx["ray_o"]), _dev(fx["ray_d"])
        raw_c = net.decode(o, d, _dev(z_coarse))
        weights = ops.composite(raw_c, _dev(z_coarse), d)[3]
        smp = ops.importance_sample(o, d, _dev(fx["near"]), _dev(fx["far"]), torch.linspace(0.0, 1.0, 64).to(DEV), None, weights,
                                    torch.linspace(0.0, 1.0, 128).to(DEV))
    assert hp.same_bits(smp["z_coarse"], _dev(z_coarse))
    z_fine = smp["z_fine"].cpu().numpy()
    assert np.array_equal(np.sort(np.concatenate([z_coarse, z_fine], -1), -1), got["z_vals"])
    hp.assert_close(got["z_std"][:, 0], z_fine.astype(np.float64).std(-1), 1e-7, "z_std", rel=False)  # float64, rounded once
    # the fine depths themselves: the float64 sample_pdf of the float64 coarse weights, up to what the weights' error moves them
    zc = z_coarse.astype(np.float64)
    z64 = ref.sample_pdf(0.5 * (zc[:, 1:] + zc[:, :-1]), model64("model", z_coarse)["weights"][:, 1:-1], np.linspace(0.0, 1.0, 128))
    print("importance depths against float64: median %.2e" % np.median(np.abs(z64 - z_fine)))
    assert np.median(np.abs(z64 - z_fine)) < 1e-5


def test_auto_follows_the_fast_arithmetic_s_measured_error(fx, sd, model64, e_ref):
    """'auto' is the fast arithmetic exactly when that holds every map of the two-pass render and of the coarse-only render to the
    1e-4 budget on this GPU; the figures are printed (and quoted in DESIGN.md 4.20)."""
    from neuralbody_amd import nerf

    net = _net(sd, "f16x3")
    worst = {}
    for N in (128, 0):
        w = {}
        _check_render(_render(net, fx, N_importance=N), fx, model64, e_ref, N, False, tol=None, raw_tol=False, worst=w)
        worst.update({"%s@%d" % (k, N): v for k, v in w.items()})
    print("f16x3 against float64:", worst)
    meets = max(v for k, v in worst.items() if not k.startswith("raw")) <= FAST_BUDGET
    assert nerf.AUTO_ARITHMETIC == ("f16x3" if meets else "f32"), worst
    assert _net(sd, "auto").nerf_precision() == nerf.AUTO_ARITHMETIC


def test_render_coarse_only(fx, sd, model64, e_ref):
    _check_render(_render(_net(sd), fx, N_importance=0), fx, model64, e_ref, 0, False)


def test_render_white_background(fx, sd, model64, e_ref):
    _check_render(_render(_net(sd), fx, white_bkgd=True), fx, model64, e_ref, 128, True)


def test_render_in_uneven_chunks_gives_the_same_bits(fx, sd, model64, e_ref):
    net = _net(sd)
    whole, parts = _render(net, fx), _render(net, fx, chunk=37)  # 96 rays: 37 + 37 + 22
    _check_render(parts, fx, model64, e_ref, 128, False)
    for k in whole:
        assert hp.same_bits(whole[k], parts[k]), k


def test_render_no_rays(fx, sd):
    empty = {k: v[:0] for k, v in fx.items() if k in ("ray_o", "ray_d", "near", "far")}
    for N in (128, 0):
        out = _render(_net(sd), empty, N_importance=N)
        T = 64 + N
        want = {"rgb_map": (1, 0, 3), "disp_map": (1, 0, 1), "acc_map": (1, 0, 1), "depth_map": (1, 0), "raw": (1, 0, T * 4),
                "z_vals": (1, 0, T)}
        if N:
            want.update(rgb0=(1, 0, 3), disp0=(1, 0, 1), acc0=(1, 0, 1), z_std=(1, 0, 1))
        assert {k: tuple(v.shape) for k, v in out.items()} == want


def test_random_u_and_raw_noise_paths(fx, sd):
    """perturb != 0 draws u on the device (a given u overrides it), raw_noise_std != 0 composites noisy densities and returns the
    clean raw."""
    from neuralbody_amd.nerf import VolumeRenderer, VolumeRendererConfig

    net = _net(sd)
    batch = {k: _dev(fx[k])[None] for k in ("ray_o", "ray_d", "near", "far")}
    u = torch.rand((1, 96, 128), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        r = VolumeRenderer(net, VolumeRendererConfig(perturb=1.0))
        a, b = r.render(batch, u=u), r.render(batch, u=u)
        c = r.render(batch)
        clean = VolumeRenderer(net, VolumeRendererConfig(perturb=0.0)).render(batch)
        noise = (torch.zeros(1, 96, 64, device=DEV), torch.ones(1, 96, 192, device=DEV))
        noisy = VolumeRenderer(net, VolumeRendererConfig(perturb=0.0, raw_noise_std=0.5)).render(batch, raw_noise=noise)
    assert all(hp.same_bits(a[k], b[k]) for k in a)
    assert not hp.same_bits(a["z_vals"], c["z_vals"]) and bool(torch.isfinite(c["rgb_map"]).all())
    assert hp.same_bits(noisy["raw"], clean["raw"]) and hp.same_bits(noisy["rgb0"], clean["rgb0"])
    assert float((noisy["acc_map"] - clean["acc_map"]).min()) >= -1e-6 and not hp.same_bits(noisy["acc_map"], clean["acc_map"])


# ------------------------------------------------------------------------------------------------ the depth-only merge
@pytest.mark.parametrize("n,S,N", [(1, 3, 1), (7, 64, 128), (5, 384, 128)])
def test_merge_z_is_a_stable_sort_of_unsorted_depths_with_ties(n, S, N):
    from neuralbody_amd import ops

    rs = np.random.RandomState(n + S)
    zc = rs.randint(0, 40, (n, S)).astype(np.float32) / 8  # many ties, no order
    zf = rs.randint(0, 40, (n, N)).astype(np.float32) / 8
    got = ops.importance_merge_z(_dev(zc), _dev(zf)).cpu().numpy()
    assert np.array_equal(got, np.sort(np.concatenate([zc, zf], -1), -1, kind="stable"))
    # nb_importance_merge's depths, bit for bit
    raw = torch.zeros((n, S, 4), device=DEV), torch.zeros((n, N, 4), device=DEV)
    assert hp.same_bits(ops.importance_merge(_dev(zc), raw[0], _dev(zf), raw[1])[0], _dev(got))


# ------------------------------------------------------------------------------------------------ 5: checkpoint, consumers
_CFG = dict(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10, view_res=4, N_samples=64,
            N_importance=128, perturb=0, raw_noise_std=0, white_bkgd=False, lindisp=False, chunk=32768, H=8, W=12, ratio=1.0)


@pytest.mark.parametrize("precision", ["f32", "auto"])
def test_checkpoint_round_trip_through_the_plugin(fx, sd, model64, e_ref, tmp_path, precision):
    net = _net(sd, precision)
    torch.save(net.state_dict(), tmp_path / "latest.pth")
    fresh = hp.load_plugin("nerf.py", types.SimpleNamespace(nerf_precision=precision, **_CFG)).Network()
    assert not fresh.train().training  # run.py:57,89: the plugin's network stays in eval mode
    fresh.load_state_dict(torch.load(tmp_path / "latest.pth", map_location="cpu"), strict=True)
    fresh = fresh.to(DEV)
    z = fx["z_coarse"]
    pts, vd = _dev(ref.points_f32(fx["ray_o"], fx["ray_d"], z)), _dev(ref.viewdirs_device(fx["ray_d"]))
    with torch.no_grad():
        for model, m in (("", "model"), ("fine", "model_fine")):
            a, b = net(pts, vd, model=model), fresh(pts, vd, model=model)
            assert a.shape == (96, 64, 4) and hp.same_bits(a, b)
            # forward takes points: the network of nerf.py:140-158 at the points the ray form decodes
            if precision == "f32":
                hp.assert_close(a.cpu().numpy(), model64(m, z)["raw"], 8 * e_ref, "forward " + m, rel=False)
        # a changed parameter is a new blob (an in-place write that counts as one: the memo keys on version counters)
        base = fresh(pts, vd)[..., :3].clone()
        fresh.model.rgb_linear.bias.add_(1.0)
        assert torch.allclose(fresh(pts, vd)[..., :3], base + 1.0, atol=1e-5)


def test_evaluator_and_novel_view_loop_take_the_dict(fx, sd):
    from neuralbody_amd.evaluator import EvalConfig, Evaluator
    from neuralbody_amd.novel_view import NovelViewRenderer
    from tests import synthetic as syn

    net = _net(sd)
    renderer = hp.load_plugin("volume_renderer.py", types.SimpleNamespace(**_CFG)).Renderer(net)
    batch = {k: _dev(fx[k])[None] for k in ("ray_o", "ray_d", "near", "far")}
    with torch.no_grad():
        out = renderer.render(batch)
    batch.update(rgb=torch.rand(1, 96, 3), mask_at_box=torch.ones(1, 8 * 12, dtype=torch.uint8))
    ev = Evaluator(EvalConfig(8, 12))
    ev.evaluate(out, batch)
    assert len(ev.mse) == 1 and np.isfinite(ev.mse[0]) and ev.mse[0] > 0.0

    body = syn.make_body(seed=0, box=(0.3, 0.5, 0.2))
    K, R, T = syn.make_camera(body, 16, 16, focal_factor=2.5, distance=1.5)
    view = NovelViewRenderer(renderer, 16, 16, device=DEV).render_view(K, np.concatenate([R, np.reshape(T, (3, 1))], 1),
                                                                      body["can_bounds"], {})
    assert view["n_rays"] > 0 and view["img"].shape == (16, 16, 3) and bool(torch.isfinite(view["img"]).all())
    assert bool(torch.isfinite(view["depth"]).all())
