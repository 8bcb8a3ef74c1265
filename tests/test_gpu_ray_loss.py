"""nb_ray_distortion and nb_composite_bwd_maps against their float64 models (tests/ray_loss_ref.py)."""
import numpy as np
import pytest
import torch

from tests import ray_loss_ref as rl
from tests.test_gpu_backward import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

WEIGHT_KINDS = ("zero", "hot_first", "hot_middle", "hot_last", "uniform", "random", "composite")
DEPTH_KINDS = ("linspace", "jittered", "equal", "runs")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _depths(kind, n, S, rs):
    near = rs.uniform(2.0, 3.0, (n, 1)).astype(np.float32)
    far = (near + rs.uniform(0.3, 1.2, (n, 1))).astype(np.float32)
    t = np.linspace(0.0, 1.0, S, dtype=np.float32)[None]
    z = (near * (1 - t) + far * t).astype(np.float32)
    if kind == "equal":  # near == far
        z = np.repeat(near, S, axis=1)
    elif kind == "jittered" and S > 1:  # get_sampling_points with perturb (if_clight_renderer.py:15-23)
        mids = 0.5 * (z[:, 1:] + z[:, :-1])
        upper, lower = np.concatenate([mids, z[:, -1:]], 1), np.concatenate([z[:, :1], mids], 1)
        z = (lower + (upper - lower) * rs.uniform(0, 1, (n, S)).astype(np.float32)).astype(np.float32)
    elif kind == "runs":  # runs of three equal neighbours, the last run possibly shorter
        z = z[:, (np.arange(S) // 3) * 3]
    assert z.dtype == np.float32 and (np.diff(z, axis=1) >= 0).all()
    return np.ascontiguousarray(z)


def _weights(kind, z, rs):
    from neuralbody_amd import ops

    n, S = z.shape
    w = np.zeros((n, S), np.float32)
    if kind.startswith("hot"):
        w[:, {"hot_first": 0, "hot_middle": S // 2, "hot_last": S - 1}[kind]] = rs.uniform(0.25, 1.0, n).astype(np.float32)
    elif kind == "uniform":
        w[:] = np.float32(1.0 / S)
    elif kind == "random":
        w = rs.uniform(0, 1, (n, S)).astype(np.float32)
    elif kind == "composite":  # nb_composite's own weights from random raw
        raw = (rs.standard_normal((n, S, 4)) * 2).astype(np.float32)
        d = rs.standard_normal((n, 3)).astype(np.float32)
        w = ops.composite(_dev(raw), _dev(z), _dev(d), False)[3].cpu().numpy()
    return w


@pytest.mark.parametrize("S", (1, 2, 3, 64, 65, 130, 512))
@pytest.mark.parametrize("n", (1, 5, 65, 259))
def test_ray_distortion_matches_the_direct_double_sums(n, S):
    """Every weight kind on every depth kind: each entry of loss and G within one fp32 rounding of the float64 model
    (2^-23 |ref| + 1e-12: the rounding on store plus float64 cancellation over at most 512 terms of magnitude <= 2)."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(1000 * n + S)
    worst = 0.0
    for dk in DEPTH_KINDS:
        z = _depths(dk, n, S, rs)
        ws = [_weights(wk, z, rs) for wk in WEIGHT_KINDS]
        refs = rl.distortion_ref_many(ws, z)
        zd = _dev(z)
        for wk, w, (L, G) in zip(WEIGHT_KINDS, ws, refs):
            wd = _dev(w)
            loss, grad = ops.ray_distortion_raw(wd, zd)
            loss_only, none = ops.ray_distortion_raw(wd, zd, want_grad=False)
            assert none is None and torch.equal(loss.view(torch.int32), loss_only.view(torch.int32)), (dk, wk)
            for name, got, ref in (("loss", loss, L), ("G", grad, G)):
                got = got.cpu().numpy().astype(np.float64)
                err = np.abs(got - ref)
                bound = 2.0 ** -23 * np.abs(ref) + 1e-12
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), "%s, depths %s, weights %s: worst |diff| / bound = %.3g" % (name, dk, wk, (err / bound).max())
            flat = torch.from_numpy(~(z[:, -1] > z[:, 0])).to(DEV)  # span = 0: S = 1, near == far, one run
            assert bool(flat.all()) == (dk == "equal" or S == 1 or (dk == "runs" and S <= 3))
            assert not loss[flat].any() and not grad[flat].any()
            if wk == "random":
                assert bool((loss[~flat] > 0).all())
    print("n = %d, S = %d: worst |diff| / (2^-23 |ref| + 1e-12) = %.3f" % (n, S, worst))


def test_ray_distortion_refuses_bad_sizes_by_name():
    from neuralbody_amd import _lib, ops

    for S in (0, 513):
        with pytest.raises(_lib.NbError, match="n_samples = %d" % S):
            ops.ray_distortion_raw(torch.zeros((3, S), device=DEV), torch.zeros((3, S), device=DEV))
    L = _lib.lib()
    buf = torch.zeros(8, device=DEV)
    assert L.nb_ray_distortion(_lib.ptr(buf), _lib.ptr(buf), -1, 4, _lib.ptr(buf), None, None) == -1  # NB_EINVAL
    assert b"n_rays = -1" in L.nb_last_error()
    assert L.nb_ray_distortion(None, None, 0, 4, None, None, None) == 0  # n_rays == 0: NB_OK at once


def test_ray_distortion_autograd():
    """ops.ray_distortion(...).sum().backward() leaves G in weights.grad; a scaled cotangent scales it; z_vals gets no gradient;
    under no_grad the result carries no graph."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(4)
    z = _dev(_depths("jittered", 37, 64, rs))
    w = _dev(rs.uniform(0, 1, (37, 64)).astype(np.float32)).requires_grad_(True)
    loss0, G = ops.ray_distortion_raw(w.detach(), z)
    zg = z.clone().requires_grad_(True)
    loss = ops.ray_distortion(w, zg)
    assert loss.requires_grad and torch.equal(loss.detach(), loss0)
    loss.sum().backward()
    assert torch.equal(w.grad, G) and zg.grad is None
    w.grad = None
    g = _dev(rs.standard_normal(37).astype(np.float32))
    (ops.ray_distortion(w, z) * g).sum().backward()
    assert torch.equal(w.grad, g[:, None] * G)
    with torch.no_grad():
        assert not ops.ray_distortion(w, z).requires_grad


# ------------------------------------------------------------------------------------------- nb_composite_bwd_maps
SHAPES = ((1, 1, False), (37, 2, True), (65, 64, False), (9, 130, True))


def _special_rays(S, rs):
    """(raw [3,S,4], z [3,S]): every density <= 0; densities of 1e4 (alpha = 1); tied depths."""
    raw = (rs.standard_normal((3, S, 4)) * 2).astype(np.float32)
    z = np.sort(rs.uniform(1, 3, (3, S)).astype(np.float32), axis=1)
    raw[0, :, 3] = -np.abs(raw[0, :, 3])
    raw[0, 0, 3] = 0.0
    raw[1, :, 3] = 1e4
    z[2, : max(S // 2, 1)] = z[2, 0]
    z[2] = np.sort(z[2])
    return raw, z


def _case(n, S, seed, min_acc=None):
    """Random raw x 2, sorted z, random ray_d (test_composite_bwd_matches_autograd) for n rays — with min_acc only rays whose float64
    acc is at least that — then the three special rays on top; cotangents for all five outputs.  -> dict of float32 arrays."""
    rs = np.random.RandomState(seed)
    m = n if min_acc is None else 16 * n + 64
    raw = (rs.standard_normal((m, S, 4)) * 2).astype(np.float32)
    z = np.sort(rs.uniform(1, 3, (m, S)).astype(np.float32), axis=1)
    d = rs.standard_normal((m + 3, 3)).astype(np.float32)
    if min_acc is not None:
        _, acc = rl.composite_maps_ref(raw, z, d[:m], False, g_acc=np.ones(m))
        keep = np.nonzero(acc >= min_acc)[0][:n]
        assert len(keep) == n, "only %d of %d candidate rays have acc >= %g" % (len(keep), m, min_acc)
        raw, z, d = raw[keep], z[keep], np.concatenate([d[keep], d[m:]])
    sraw, sz = _special_rays(S, rs)
    if min_acc is not None:
        sraw[2, -1, 3] = 5.0  # the tied ray ends opaque (its last sample's dist is 1e10 |d|): acc = 1 whatever the rest drew
    raw, z = np.concatenate([raw, sraw]), np.concatenate([z, sz])
    N = n + 3
    c = dict(raw=raw, z=z, d=d, empty=n, g_rgb=rs.standard_normal((N, 3)).astype(np.float32),
             g_acc=rs.standard_normal(N).astype(np.float32), g_depth=rs.standard_normal(N).astype(np.float32),
             g_disp=rs.standard_normal(N).astype(np.float32), g_weights=rs.standard_normal((N, S)).astype(np.float32))
    return c


def _maps(c, white, **names):
    from neuralbody_amd import ops

    return ops.composite_bwd_maps(_dev(c["raw"]), _dev(c["z"]), _dev(c["d"]), white,
                                  **{"d_" + k: _dev(c[v]) for k, v in names.items()})


@pytest.mark.parametrize("n,S,white", SHAPES)
def test_composite_bwd_maps_without_the_new_cotangents_is_composite_bwd_bit_for_bit(n, S, white):
    from neuralbody_amd import ops

    c = _case(n, S, 100 + S)
    raw, z, d = _dev(c["raw"]), _dev(c["z"]), _dev(c["d"])
    for acc, depth in ((True, True), (False, False), (True, False), (False, True)):
        kw = dict(rgb_map="g_rgb", **({"acc_map": "g_acc"} if acc else {}), **({"depth_map": "g_depth"} if depth else {}))
        want = ops.composite_bwd(raw, z, d, _dev(c["g_rgb"]), white, _dev(c["g_acc"]) if acc else None, _dev(c["g_depth"]) if depth else None)
        got = _maps(c, white, **kw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (acc, depth)


@pytest.mark.parametrize("n,S,white", SHAPES)
def test_composite_bwd_maps_with_the_weights_cotangent_matches_autograd(n, S, white):
    c = _case(n, S, 200 + S)
    ref, _ = rl.composite_maps_ref(c["raw"], c["z"], c["d"], white, c["g_rgb"], c["g_acc"], c["g_depth"], None, c["g_weights"])
    got = _maps(c, white, rgb_map="g_rgb", acc_map="g_acc", depth_map="g_depth", weights="g_weights")
    e = _rel(got.cpu().numpy(), ref, 2e-5, "d raw n=%d S=%d" % (n, S))
    # d_weights alone (no d rgb arrives)
    ref, _ = rl.composite_maps_ref(c["raw"], c["z"], c["d"], white, g_weights=c["g_weights"])
    e2 = _rel(_maps(c, white, weights="g_weights").cpu().numpy(), ref, 2e-5, "d raw from d weights alone n=%d S=%d" % (n, S))
    print("n = %d, S = %d: max |diff| / max |ref| = %.2e (four cotangents), %.2e (d weights alone)" % (n, S, e, e2))


# (c) bound: max(2e-5, 4 x the worst error measured over these cases; the factor 4 covers seeds not run)
DISP_MEASURED = 2.7e-7  # measured on an MI355X over the four shapes: 1.2e-7, 7.2e-8, 2.7e-7, 2.3e-7 (all five cotangents)
DISP_TOL = max(2e-5, 4 * DISP_MEASURED)


@pytest.mark.parametrize("n,S,white", SHAPES)
def test_composite_bwd_maps_with_the_disparity_cotangent(n, S, white):
    """Rays with acc >= 2^-6 (on the float64 reference), the empty ray on top: its d_raw is what it is without d_disp; the rest
    against float64 autograd."""
    c = _case(n, S, 300 + S, min_acc=2.0 ** -6)
    all5 = dict(rgb_map="g_rgb", acc_map="g_acc", depth_map="g_depth", weights="g_weights", disp_map="g_disp")
    ref, acc = rl.composite_maps_ref(c["raw"], c["z"], c["d"], white, c["g_rgb"], c["g_acc"], c["g_depth"], c["g_disp"], c["g_weights"])
    k = c["empty"]
    assert acc[k] == 0.0 and (np.delete(acc, k) >= 2.0 ** -6).all() and np.isfinite(ref).all()
    got = _maps(c, white, **all5)
    without = _maps(c, white, **{a: b for a, b in all5.items() if a != "disp_map"})
    assert torch.isfinite(got).all()
    assert torch.equal(got[k].view(torch.int32), without[k].view(torch.int32)), "the empty ray took something from d_disp"
    assert S == 1 or not torch.equal(got[:k], without[:k])  # (a lone sample is opaque or empty: nothing moves its alpha)
    rest = np.ones(len(acc), bool)
    rest[k] = False
    g, r = got.cpu().numpy()[rest], ref[rest]
    err = np.abs(g - r).max() / max(np.abs(r).max(), 1e-30)
    print("disparity cotangent, n = %d, S = %d: max |diff| / max |ref| = %.3e" % (n, S, err))
    _rel(g, r, DISP_TOL, "d raw with d disp n=%d S=%d" % (n, S))
    # d_disp alone
    ref1, _ = rl.composite_maps_ref(c["raw"], c["z"], c["d"], white, g_disp=c["g_disp"])
    got1 = _maps(c, white, disp_map="g_disp")
    assert not got1[k].any()
    e1 = _rel(got1.cpu().numpy()[rest], ref1[rest], DISP_TOL, "d raw from d disp alone n=%d S=%d" % (n, S))
    print("disparity cotangent alone, n = %d, S = %d: max |diff| / max |ref| = %.3e" % (n, S, e1))


def test_composite_bwd_maps_needs_a_cotangent():
    from neuralbody_amd import _lib

    c = _case(5, 8, 1)
    with pytest.raises(_lib.NbError, match="no cotangent"):
        _maps(c, False)
    assert _lib.lib().nb_composite_bwd_maps(None, None, None, 0, 8, 0, None, None, None, None, None, None, None) == 0  # n_rays == 0
