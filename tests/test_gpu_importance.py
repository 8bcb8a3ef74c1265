"""Hierarchical sampling on the device (run with -m gpu on an MI355X): nb_importance_sample against the acceptance rule of
tests/importance_cases.py, nb_importance_merge against a stable argsort, and Renderer.render(batch, n_importance=N) end to end
against the oracle decoding and compositing the device's own merged depths."""
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import importance_cases as ic
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAT_RAY = 7  # the ray with near == far in every case of more than 7 rays


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from neuralbody_amd import _lib

    _lib.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ test 1
def _check_sample(n, S, N, u_mode, t_rand=None, seed=0):
    from neuralbody_amd import ops

    ray_o, ray_d, near, far = ic.make_rays(n, seed=seed + 17 * n + S, flat_ray=FLAT_RAY)
    w = ic.make_weights(n, S, seed=seed + S + N, first_kind=(S + N) % 6)
    u = ic.make_u(n, N, u_mode, seed=seed + N)
    tv = ic.t_vals(S)
    out = ops.importance_sample(_dev(ray_o), _dev(ray_d), _dev(near), _dev(far), _dev(tv), _dev(t_rand), _dev(w), _dev(u))
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    assert got["keep"] is None and got["z_fine"].shape == (n, N) and got["wpts"].shape == got["viewdir"].shape == (n, N, 3)
    # the coarse depths are the march's: bit-equal to the fp32 expression, the jitter included
    if t_rand is None:
        z_ref = ic.coarse_depths_f32(near, far, S)
    else:
        from neuralbody_amd.renderer import RenderConfig, Renderer
        import types

        rend = Renderer(types.SimpleNamespace(training=True), RenderConfig(N_samples=S, perturb=1.0))
        z_ref = rend.get_sampling_points(torch.from_numpy(ray_o)[None], torch.from_numpy(ray_d)[None], torch.from_numpy(near)[None],
                                         torch.from_numpy(far)[None], t_rand=torch.from_numpy(t_rand)[None])[1][0].numpy()
    assert np.array_equal(got["z_coarse"].view(np.int32), z_ref.view(np.int32)), "coarse depths"
    bins = ic.bins_f32(z_ref)
    z = got["z_fine"]
    assert np.isfinite(z).all()
    ok = ic.accept(z, u, bins, w)
    err = ic.cdf_error(z, u, bins, w)
    print("n=%d S=%d N=%d %s%s: %d of %d rejected, worst CDF-domain error %.3g" % (
        n, S, N, u_mode, "" if t_rand is None else " jittered", int((~ok).sum()), ok.size, float(err.max())))
    assert ok.all(), "%d of %d depths rejected, first at %s" % (int((~ok).sum()), ok.size, np.argwhere(~ok)[:4].tolist())
    if n > FLAT_RAY:  # near == far: every depth is near, exactly
        assert np.array_equal(z[FLAT_RAY], np.full(N, near[FLAT_RAY], np.float32)) and near[FLAT_RAY] == far[FLAT_RAY]
        assert got["z_std"][FLAT_RAY] == 0.0
    # wpts = fl32(o + fl32(d * z)), bit for bit
    wp = (ray_o[:, None, :] + (ray_d[:, None, :] * z[:, :, None]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got["wpts"].view(np.int32), wp.view(np.int32)), "wpts"
    # viewdir within 1 ulp of d / |d|
    vd = (ray_d.astype(np.float64) / np.linalg.norm(ray_d.astype(np.float64), axis=1, keepdims=True))[:, None, :]
    ulp = np.spacing(np.abs(vd).astype(np.float32)).astype(np.float64)
    assert (np.abs(got["viewdir"].astype(np.float64) - vd) <= ulp).all(), "viewdir"
    # z_std within 1e-6 (far - near) of the float64 population std of the returned depths
    std = z.astype(np.float64).std(axis=1)
    assert (np.abs(got["z_std"].astype(np.float64) - std) <= 1e-6 * (far - near).astype(np.float64)).all(), "z_std"


@pytest.mark.parametrize("n", [1, 65, 259])
def test_importance_sample_is_admitted_by_the_rule(n):
    """Every (S, N_imp, u) of the issue for one ray count: one ray, one ray past a wave's 64, not a multiple of the four rays of a
    workgroup.  The weights rotate through the six kinds ray by ray (and start at another kind per (S, N))."""
    for S in (3, 4, 64, 65, 130):
        for N in (1, 2, 63, 64, 65, 128):
            for u_mode in ("det", "rand"):
                _check_sample(n, S, N, u_mode)


def test_importance_sample_on_jittered_coarse_depths():
    """The coarse depths are the ones the march used: with t_rand the bins are the midpoints of the jittered depths."""
    rs = np.random.RandomState(2)
    for n, S, N in ((65, 64, 64), (5, 130, 65)):
        tr = np.minimum(rs.uniform(0, 1, (n, S)).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
        _check_sample(n, S, N, "rand", t_rand=tr)


def test_importance_sample_flags_culled_points_like_the_march():
    """With a cull the keep byte of a new point is the oracle's inside test (the reference's projection on the CPU) of that point."""
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    r, sd, batch, (Hh, Ww) = scenes.build_masked("mmsk")
    bd = H.device_batch(batch, DEV)
    n, S, N = batch["ray_o"].shape[1], r["n_samples"], 32
    w = ic.make_weights(n, S, seed=3)
    cull = ops.make_cull(bd["msks"][0], bd["RT"][0], bd["Ks"][0])
    out = ops.importance_sample(bd["ray_o"][0], bd["ray_d"][0], bd["near"][0], bd["far"][0], _dev(ic.t_vals(S)), None, _dev(w),
                                _dev(ic.make_u(n, N, "det", 0)), cull=cull)
    torch.cuda.synchronize()
    tb = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    inside = orc.inside_mmsk(out["wpts"].cpu()[None], tb, Hh, Ww).reshape(n, N).numpy()
    keep = out["keep"].cpu().numpy()
    assert set(np.unique(keep)) <= {0, 1} and 0.02 < keep.mean() < 0.98
    assert int((keep.astype(bool) != inside).sum()) == 0


def test_the_size_limits_are_refused_by_name():
    from neuralbody_amd import ops
    from neuralbody_amd._lib import NbError

    def call(S, N, n=3):
        ray_o, ray_d, near, far = ic.make_rays(n, seed=1)
        return ops.importance_sample(_dev(ray_o), _dev(ray_d), _dev(near), _dev(far), _dev(ic.t_vals(S)), None,
                                     _dev(np.zeros((n, S), np.float32)), _dev(np.zeros(N, np.float32)))

    for S, N, what in ((2, 4, "n_samples = 2"), (64, 129, "n_importance = 129"), (64, 0, "n_importance = 0"),
                       (400, 113, "n_samples + n_importance = 513")):
        with pytest.raises(NbError, match=re.escape(what)):
            call(S, N)
    with pytest.raises(NbError, match="n_samples = 2"):
        ops.importance_merge(torch.zeros((1, 2), device=DEV), torch.zeros((1, 2, 4), device=DEV), torch.zeros((1, 4), device=DEV),
                             torch.zeros((1, 4, 4), device=DEV))
    assert call(400, 112)["z_fine"].shape == (3, 112)  # the largest merged size
    assert call(64, 64, n=0)["z_fine"].shape == (0, 64)  # no rays: nothing launched


# ------------------------------------------------------------------------------------------------ test 2
@pytest.mark.parametrize("n,S,N", [(1, 3, 1), (65, 64, 64), (259, 65, 63), (6, 130, 128), (5, 384, 128)])
def test_importance_merge_is_the_stable_argsort(n, S, N):
    """z_vals and raw merged = the concatenation (coarse, then fine) under np.argsort(kind='stable'), bit for bit: fine depths in
    descending order, exact ties between coarse and fine depths and among the fine ones, keep = 0 samples (raw exactly 0)."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(n + S)
    zc = np.sort(rs.uniform(3.5, 4.5, (n, S)).astype(np.float32), axis=1)
    zf = -np.sort(-rs.uniform(3.4, 4.6, (n, N)).astype(np.float32), axis=1)  # descending
    ties = rs.randint(0, S, (n, N))
    tied = rs.uniform(0, 1, (n, N)) < 0.3
    zf = np.where(tied, np.take_along_axis(zc, ties, 1), zf).astype(np.float32)  # (repeats among the fine ones as well)
    if N > 1:
        zf[:, -1] = zc[:, -1]  # a fine depth equal to the LAST coarse one
    rc = rs.standard_normal((n, S, 4)).astype(np.float32)
    rf = rs.standard_normal((n, N, 4)).astype(np.float32)
    keep = (rs.uniform(0, 1, (n, N)) < 0.7).astype(np.uint8)
    keep[:, 0] = 0
    for kp in (None, keep):
        z, raw = ops.importance_merge(_dev(zc), _dev(rc), _dev(zf), _dev(rf), _dev(kp))
        torch.cuda.synchronize()
        cat_z = np.concatenate([zc, zf], 1)
        cat_r = np.concatenate([rc, rf if kp is None else np.where(kp[:, :, None] != 0, rf, np.float32(0.0))], 1)
        order = np.argsort(cat_z, axis=1, kind="stable")
        assert np.array_equal(z.cpu().numpy().view(np.int32), np.take_along_axis(cat_z, order, 1).view(np.int32))
        got_r = raw.cpu().numpy()
        assert np.array_equal(got_r.view(np.int32), np.take_along_axis(cat_r, order[:, :, None], 1).view(np.int32))
        if kp is not None:
            src = np.take_along_axis(np.concatenate([np.ones((n, S), np.uint8), kp], 1), order, 1)
            assert (got_r[src == 0].view(np.int32) == 0).all() and (src == 0).any()  # exactly +0


# ------------------------------------------------------------------------------------------------ tests 3 - 5
_CACHE = {}


def _scene(kind, precision):
    """(renderer, device batch, numpy batch, oracle state dict, oracle volumes, device volumes, (H, W) of the masks or None), the network
    in the fixture's mode with the ORACLE's feature volumes handed to every render: both passes and the oracle decode the same field."""
    key = (kind, precision)
    if key not in _CACHE:
        from neuralbody_amd.renderer import RenderConfig, Renderer, RendererMmsk

        if kind == "small":
            r, sd, body, batch, cam, _ = scenes.build("small")
            hw, cls = None, Renderer
        else:
            r, sd, batch, hw = scenes.build_masked("mmsk")
            cls = RendererMmsk
        sdt, vols, out_sh = H.oracle_volumes(sd, batch, True)
        net = H.make_network(sd, DEV, True, precision)
        rend = cls(net, RenderConfig(N_samples=r["n_samples"], perturb=0.0, raw_noise_std=0.0, white_bkgd=r.get("white_bkgd", False)))
        _CACHE[key] = (rend, H.device_batch(batch, DEV), batch, sdt, vols, [v.to(DEV) for v in vols], hw)
    return _CACHE[key]


def _oracle_rgb(kind, z_vals, batch, sdt, vols, hw, white_bkgd):
    """The oracle on the device's own merged depths: points o + d z, decoded on the CPU (culled ones zeroed by the oracle's cull),
    composited by the oracle's raw2outputs -> (rgb_map [n,3], raw [n,T,4], weights [n,T])."""
    from oracle import neuralbody_oracle as orc

    tb = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    n, T = z_vals.shape
    z = torch.from_numpy(z_vals)
    ray_o, ray_d = tb["ray_o"][0], tb["ray_d"][0]
    wpts = ray_o[:, None] + ray_d[:, None] * z[..., None]
    vd = (ray_d / torch.norm(ray_d, dim=1, keepdim=True))[:, None].repeat(1, T, 1)
    sp = {"bounds": tb["bounds"], "R": tb["R"], "Th": tb["Th"], "latent_index": tb["latent_index"].long(),
          "out_sh": torch.max(tb["out_sh"], dim=0)[0].tolist()}
    with torch.no_grad():
        raw = orc.calculate_density_color(sdt, wpts.reshape(1, -1, 3), vd.reshape(1, -1, 3), vols, sp)[0]
        if kind == "mmsk":
            inside = orc.inside_mmsk(wpts[None], tb, hw[0], hw[1]).reshape(-1)
            raw = raw * inside[:, None].to(raw)
        raw = raw.reshape(n, T, 4)
        rgb, _disp, _acc, weights, _depth = orc.raw2outputs(raw, z, ray_d, white_bkgd)
    return rgb.numpy(), raw.numpy(), weights.numpy()


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("kind", ["small", "mmsk"])
def test_render_with_importance_samples_matches_the_oracle(kind, N, precision):
    """render(batch, n_importance=N) against the oracle at the device's own merged depths (validated above), within helpers.RGB_TOL.
    The last sample's interval is 1e10, so its alpha is a step of the SIGN of its density: a ray whose last density the oracle itself
    puts within its fp32 rounding of zero (bench.FP32_SIGMA) is bounded by the transmittance in front of that sample instead, the
    allowance of tests/test_gpu_fullsize.py and no other.  Measured on an MI355X: 'f32' 2.7e-7 .. 7.0e-7, the default arithmetic
    2.6e-5 .. 3.0e-5 with 80 and with 128 samples per ray, no ray on the allowance."""
    import bench

    rend, bd, batch, sdt, vols, vols_dev, hw = _scene(kind, precision)
    S = rend.cfg.N_samples
    with torch.no_grad():
        off = rend.render(bd, feature_volume=vols_dev)
        out = rend.render(bd, feature_volume=vols_dev, n_importance=N)
    torch.cuda.synchronize()
    n = batch["ray_o"].shape[1]
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map", "z_vals", "rgb0", "disp0", "acc0", "z_std"}
    assert out["weights"].shape == out["z_vals"].shape == (1, n, S + N) and out["z_std"].shape == (1, n)
    assert out["rgb_map"].shape == (1, n, 3) and out["depth_map"].shape == out["acc_map"].shape == out["disp_map"].shape == (1, n)
    # the coarse maps are the n_importance = 0 render's, bit for bit
    for a, b in (("rgb0", "rgb_map"), ("acc0", "acc_map"), ("disp0", "disp_map")):
        assert H.same_bits(out[a], off[b]), a
    z = out["z_vals"][0].cpu().numpy()
    near, far = batch["near"][0], batch["far"][0]
    assert (np.diff(z, axis=1) >= 0).all() and np.array_equal(z[:, 0], near) and np.array_equal(z[:, -1], far)
    H.assert_close(out["weights"][0].sum(-1).cpu().numpy(), out["acc_map"][0].cpu().numpy(), 1e-6, "sum w == acc", rel=False)
    rgb_ref, raw_ref, w_ref = _oracle_rgb(kind, z, batch, sdt, vols, hw, rend.cfg.white_bkgd)
    sigma_last = raw_ref[:, -1, 3]
    t_last = 1.0 - w_ref[:, :-1].sum(1)
    err = np.abs(out["rgb_map"][0].cpu().numpy() - rgb_ref).max(1)
    # (a last density of exactly 0 is a culled sample, zero on both sides: no step to fall off)
    ill = (np.abs(sigma_last) <= bench.FP32_SIGMA) & (sigma_last != 0)
    bound = np.where(ill, t_last + H.RGB_TOL, H.RGB_TOL)
    print("%s N=%d %s: rgb L-inf vs the oracle at the merged depths %.3g over %d rays (%d within FP32_SIGMA of the last-sample step); "
          "fine vs coarse image differs by %.3g" % (kind, N, precision, float(err.max()), n, int(ill.sum()),
                                                    float((out["rgb_map"] - off["rgb_map"]).abs().max())))
    assert (err <= bound).all(), "rgb_map: max err %.3e over the bound at rays %s" % (float(err.max()), np.nonzero(err > bound)[0][:8].tolist())
    assert float(rgb_ref.max() - rgb_ref.min()) > 0.1, "degenerate fixture"


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
def test_off_means_off(precision, monkeypatch):
    """n_importance = 0 (argument or config): today's keys, bit-equal tensors, and neither new op is called."""
    from neuralbody_amd import ops

    rend, bd, batch, sdt, vols, vols_dev, hw = _scene("small", precision)
    with torch.no_grad():
        on = rend.render(bd, feature_volume=vols_dev, n_importance=16)  # (the ops work here; the patched ones below would raise)
        assert "z_vals" in on

        def boom(*a, **k):
            raise AssertionError("an importance op was called with n_importance = 0")

        monkeypatch.setattr(ops, "importance_sample", boom)
        monkeypatch.setattr(ops, "importance_merge", boom)
        plain = rend.render(bd, feature_volume=vols_dev)
        zero = rend.render(bd, feature_volume=vols_dev, n_importance=0)
        with pytest.raises(AssertionError, match="importance op"):
            rend.render(bd, feature_volume=vols_dev, n_importance=4)
    torch.cuda.synchronize()
    assert set(plain) == set(zero) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map"}
    for k in plain:
        assert H.same_bits(plain[k], zero[k]), k
    g = H.golden("small")
    H.assert_close(plain["rgb_map"].cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map of the plain render", rel=False)


REGROUPED_TOL = 6e-5  # what tests/test_gpu_parity.py allows the default arithmetic between two groupings of the same samples


def _assert_same(got, want, precision, regrouped):
    """Every key bit for bit.  Only where the points were GROUPED differently (a ray range shifts which 64 share a workgroup) and the
    arithmetic's rounding depends on the grouping (helpers.GROUP_DEPENDENT): the maps within REGROUPED_TOL — depths and weights of
    single samples are ill-conditioned in empty bins and are then not compared."""
    assert set(got) == set(want)
    if regrouped and precision in H.GROUP_DEPENDENT:
        for k in ("rgb_map", "acc_map", "depth_map", "rgb0", "acc0"):
            H.assert_close(got[k].cpu().numpy(), want[k].cpu().numpy(), REGROUPED_TOL, k)
        return
    for k in want:
        assert H.same_bits(got[k], want[k]), k


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
@pytest.mark.parametrize("perturb", [0.0, 1.0])
def test_ray_ranges_and_a_batch_of_two(precision, perturb):
    """Two half-range renders concatenated are the whole render, and a batch of two frames is the two single-frame renders, bit for
    bit (`_assert_same` says where the default arithmetic cannot be).  With perturb != 0 the same u_rand goes to every call."""
    from neuralbody_amd.renderer import RenderConfig

    rend0, bd, batch, sdt, vols, vols_dev, hw = _scene("small", precision)
    rend = type(rend0)(rend0.net, RenderConfig(N_samples=rend0.cfg.N_samples, perturb=perturb))
    rend.net.eval()  # (a batch of two encodes per frame: running statistics keep the two passes equal; perturb then jitters u only)
    try:
        n, N = batch["ray_o"].shape[1], 32
        u = torch.rand((1, n, N), generator=torch.Generator().manual_seed(9)).to(DEV) if perturb else None
        half = n // 2 + 3
        with torch.no_grad():
            whole = rend.render(bd, feature_volume=vols_dev, n_importance=N, u_rand=u)
            parts = [rend.render(bd, feature_volume=vols_dev, n_importance=N, u_rand=u, ray_range=rr) for rr in ((0, half), (half, n))]
            _assert_same({k: torch.cat([p[k] for p in parts], 1) for k in whole}, whole, precision, regrouped=True)
            if perturb:
                other = rend.render(bd, feature_volume=vols_dev, n_importance=N)
                assert not torch.equal(other["z_vals"], whole["z_vals"]), "torch.rand was not drawn"
            # two frames: the same frame twice, with its own rays and uniforms
            b2 = {k: torch.cat([v, v], 0) for k, v in bd.items()}
            u2 = None if u is None else torch.cat([u, u.flip(1)], 0)
            one = [rend.render(bd, n_importance=N, u_rand=None if u2 is None else u2[i:i + 1]) for i in range(2)]
            two = rend.render(b2, n_importance=N, u_rand=u2)
            assert two["rgb_map"].shape[0] == 2
            _assert_same(two, {k: torch.cat([o[k] for o in one], 0) for k in two}, precision, regrouped=False)
        torch.cuda.synchronize()
    finally:
        rend.net.train()
