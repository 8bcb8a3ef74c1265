"""The inputs of tests/test_gpu_march_rays.py checked on the CPU (tests/march_ray_cases.py): the float32 restatement of the integrator
stays within half of tol(S) of the float64 composite on the GPU test's own rays, the depth restatement is what its formulas say,
every depth, position and trilinear weight of the lattice rays is exact and the model's quantisations are lossless on them, and the
cull cameras project every sample well inside a pixel."""
import math

import numpy as np
import pytest

from tests import f16f6_model as M
from tests import march_operand_cases as K
from tests import march_ray_cases as R


# ------------------------------------------------------------------------------------------------------------------------- A
def test_z_vals_follow_their_formulas():
    """Linear depths hit near and far; zero jitter gives the lower interval end, the largest t_rand stays below the upper one; the
    first lower and the last upper end are the linear depth itself (not the general formula)."""
    _, _, near, far = R.scene_rays()
    for S in R.SAMPLE_COUNTS:
        t = R.linear_t_vals(S)
        assert t[0] == 0 and t[-1] == 1 and (np.diff(t) > 0).all()
        zc = R.z_vals_f32(near, far, t)
        assert zc.dtype == np.float32 and (zc[:, 0] == near).all() and (zc[:, -1] == far).all() and (np.diff(zc, axis=1) > 0).all()
        mid = np.float32(0.5) * (zc[:, 1:] + zc[:, :-1])
        z0 = R.z_vals_f32(near, far, t, R.t_rand_of("zeros", R.N_RAYS, S))
        z1 = R.z_vals_f32(near, far, t, R.t_rand_of("ones", R.N_RAYS, S))
        assert (z0[:, 0] == zc[:, 0]).all() and (z0[:, 1:] == mid).all()
        assert (z1[:, -1] == zc[:, -1]).all() and (z1[:, :-1] <= mid).all() and (z1[:, :-1] > zc[:, :-1]).all()
        zr = R.z_vals_f32(near, far, t, R.t_rand_of("rand", R.N_RAYS, S))
        assert (zr >= z0).all() and (zr <= np.maximum(z1, np.nextafter(z1, np.float32(np.inf)))).all() and (np.diff(zr, axis=1) >= 0).all()
        # the general formula at the last step would lie half an interval further out: a jitter bound taken from it shows
        if S > 2:
            assert (np.abs(zr[:, -1] - zc[:, -1]) < 0.5 * (zc[:, -1] - zc[:, -2])).all()


def _seeded_raw(n, S, sigma_density, seed):
    rs = np.random.RandomState(seed)
    raw = (rs.standard_normal((n, S, 4)) * 3.0).astype(np.float32)
    raw[..., 3] = (rs.standard_normal((n, S)) * sigma_density).astype(np.float32)
    raw[0, :, 3] = -1.0  # a ray that hits nothing
    return raw


@pytest.mark.parametrize("S", R.SAMPLE_COUNTS)
def test_float32_restatement_stays_within_half_the_tolerance(S):
    """RayAccum::add's order in numpy float32 against composite_f64, on the rays, depths and jitter of the GPU test and decoder
    outputs of its magnitudes (normal logits of sigma 3; densities of sigma 20 and 1): every output within tol(S) / 2."""
    ray_o, ray_d, near, far = R.scene_rays()
    rep = 10  # 2000 rays per density scale
    worst = {}
    for jit in (None, "rand"):
        t_rand = R.t_rand_of(jit, R.N_RAYS, S)
        z = np.tile(R.z_vals_f32(near, far, R.linear_t_vals(S), t_rand), (rep, 1))
        d = np.tile(ray_d, (rep, 1))
        for k, sd in enumerate((20.0, 1.0)):
            for white in (False, True):
                raw = _seeded_raw(z.shape[0], S, sd, 100 * S + k)
                f32 = R.composite_f32_restated(raw, z, d, white)
                got = dict(weights=f32["weights"], rgb_map=f32["rgb"], acc_map=f32["acc"], depth_map=f32["depth"])
                with np.errstate(invalid="ignore", divide="ignore"):
                    q = f32["depth"] / f32["acc"]
                    got["disp_map"] = np.float32(1.0) / np.where(np.isnan(q), q, np.maximum(np.float32(1e-10), q))
                for name, r in R.integrator_ratios(got, raw, z, d, white).items():
                    worst[name] = max(worst.get(name, 0.0), r)
                assert np.isnan(got["disp_map"][0]) and f32["acc"][0] == 0
    print("S = %d: float32 restatement / tol(S): %s" % (S, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for name in ("weights", "rgb", "acc", "depth", "acc_sum"):
        assert worst[name] <= 0.5, (name, worst[name])
    assert worst["disp"] <= 1.0
    assert R.tol(64) < 1e-5


def test_composite_f64_is_raw2outputs():
    """composite_f64 against the oracle's raw2outputs in float64."""
    import torch

    from oracle import neuralbody_oracle as orc

    ray_o, ray_d, near, far = R.scene_rays()
    z = R.z_vals_f32(near, far, R.linear_t_vals(24), R.t_rand_of("rand", R.N_RAYS, 24))
    raw = _seeded_raw(R.N_RAYS, 24, 20.0, 3)
    for white in (False, True):
        mine = R.composite_f64(raw, z, ray_d, white)
        dn = R.ray_norm_f32(ray_d).astype(np.float64)
        d64 = ray_d.astype(np.float64) / np.linalg.norm(ray_d.astype(np.float64), axis=1)[:, None] * dn[:, None]
        rgb, disp, acc, w, depth = orc.raw2outputs(torch.from_numpy(raw).double(), torch.from_numpy(z).double(), torch.from_numpy(d64), white)
        for a, b in ((mine["rgb"], rgb), (mine["acc"], acc), (mine["weights"], w), (mine["depth"], depth)):
            assert np.abs(a - b.numpy()).max() < 1e-12


def test_fixture_inputs_of_the_scene_cases():
    """The cull stripes cut a good part of the samples, most rays keep some samples and lose others, and no projected sample lies
    within 2^-10 pixel of a rounding boundary in float64 (the float32 projection decides the same way)."""
    for case in R.A_CASES:
        d = R.a_inputs(case)
        assert d["z"].shape == (R.N_RAYS, d["S"]) and d["p"].dtype == np.float32
        if d["inside"] is None:
            continue
        ins = d["inside"]
        both = (ins.any(1) & ~ins.all(1)).mean()
        print("%s: %.0f%% of the samples culled, %.0f%% of the rays keep some and lose some" % (d["name"], 100 * (1 - ins.mean()), 100 * both))
        assert 0.3 < ins.mean() < 0.7 and both > (0.5 if d["S"] > 2 else 0.2)
        x, _ = R.cull_project_f64(d["p"], d["cull_RT"], d["cull_K"])
        assert x.min() > 1 and x.max() < R.STRIPE_W - 2
        x32, _ = R.cull_project_f32(d["p"], d["cull_RT"], d["cull_K"])
        assert np.abs(x32 - x).max() < 2.0 ** -12


# ------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("key", R.RAY_KEYS, ids=lambda k: k[0] + ("-colour" if k[1] else ""))
def test_lattice_ray_preconditions(key):
    """Every z, p, |d| and trilinear weight of a lattice ray case is exactly representable and what the case says; the folded planes
    are fp16 numbers; every layer of the model sums exactly; and (the colour read-out) both bf6 forms are lossless and the products
    of a (row, sample) lie on one grid below 2^24 units."""
    from tests import f16f6_phase_cases as C
    from tests import fold_stream_ref as S

    case = R.get(key)
    n, Sn = 64, case.S
    step = 1.0 if case.variant in ("whole", "cull", "narrow") else 0.5
    assert (case.z.astype(np.float64) == step * np.arange(Sn)[None, :]).all()
    axis = 1 if case.variant == "ybundle" else 0
    want_idx = case.ray_o.astype(np.float64)[:, None, :] / C.VS_HIDDEN + np.zeros((n, Sn, 3))
    want_idx[:, :, axis] += step * np.arange(Sn)[None, :]
    assert (case.idx == want_idx).all() and (case.pts.astype(np.float64) == want_idx.reshape(-1, 3) * C.VS_HIDDEN).all()
    assert (R.ray_norm_f32(case.ray_d) == np.float32(C.VS_HIDDEN)).all()
    unit = np.zeros(3)
    unit[axis] = 1.0
    assert (case.viewdir == unit).all()
    assert np.isin(case.tri_w, (0.0, 0.5, 1.0)).all() and ((case.tri_w != 0).sum(-1) <= 2).all()
    if step == 0.5:
        assert (case.tri_w == 0.5).any()
    # the 64 samples of a step read different voxels ('narrow': 32), and the voxels change from step to step
    lin = (case.idx[..., 2] * 81 + case.idx[..., 1] * 9 + case.idx[..., 0]) * 2
    for s in range(Sn):
        assert len(set(lin[:, s])) == (32 if case.variant == "narrow" else 64)
    assert all(len(set(lin[r])) == Sn for r in range(n))
    if case.variant == "leave":
        x = case.idx[..., 0]
        assert (x == 8.5).any() and (x >= 9).sum() >= 3 * n and x.max() > 10  # beyond the clamp of unnorm_s as well
        outside = (x >= 9).reshape(-1)
        assert (case.h1[:, outside] == case.params["fc0_b"][:, None]).all() and (case.params["fc0_b"] != 0).sum() == 32
    # the planes
    f = np.arange(256)
    u = case.volumes[0].reshape(-1, 32).astype(np.float64)[:, f % 32] * case.params["fc0_w"][f, f % 32]
    planes, off = K.split_planes(u)
    assert not off.any() and (K.planes_value(planes) == u).all() and (planes[:, 256:] != 0).any()
    # the model
    exp, m = R.ray_expected(case)
    assert all(m["exact"]), m["exact"]
    live = exp[:, case.inside]
    print("%s: %d x %d x %d read-outs, %.0f%% non-zero" % (case.name, exp.shape[0], n, Sn, 100.0 * (live != 0).mean()))
    assert (live != 0).mean() > (0.3 if case.colour else 0.5)
    if case.colour:
        ph = 2
        w = S.phase_weights(case.params)[ph].astype(np.float64)
        wh, q0, q1 = M.quantised_weights(S.phase_weights(case.params))[ph]
        valid = S.expected(S.phase_weights(case.params))[ph]["valid"]
        assert (q0 == wh).all() and (q1[valid] == (w - wh)[valid]).all()
        s = m["phases"][ph]["split"]
        assert not M.is_e3m2_midpoint(s["xx_scaled"]).any() and not M.is_e3m2_midpoint(s["xl_scaled"]).any()
        assert (s["xx"] == s["xh"]).all() and (s["xl"] == s["rem"]).all() and (s["rem"] >= 0).all()
        cols = np.nonzero((wh != 0).any(0))[0]
        most = 1.0
        for i in range(0, n * Sn, 7):  # every seventh sample: [R, terms]
            p = np.concatenate([wh[:, cols] * s["xh"][None, cols, i], q0[:, cols] * s["xl"][None, cols, i], q1[:, cols] * s["xx"][None, cols, i]], 1)
            mant, e = np.frexp(p)
            mi = np.abs(mant * 2.0 ** 53).astype(np.int64)
            tz = np.where(mi != 0, np.log2(np.maximum(mi & -mi, 1)).astype(np.int64), 0)
            ue = np.where(p != 0, e - 53 + tz, 10 ** 6).min(1)
            ok = ue < 10 ** 6
            most = max(most, float((np.abs(p).sum(1)[ok] / np.ldexp(1.0, ue[ok])).max(initial=0.0)))
        assert most < 2.0 ** 24, math.log2(most)


def test_lattice_cull_projection_margins():
    """Every sample of the cull case projects within 1/8 pixel of the centre of pixel (row z_r, column s) in float64, the float32
    projection rounds to that pixel, whole steps are culled (two in a row and the last), single samples of marched steps are, and
    the steps right behind a skipped one are marched."""
    case = R.get(("cull", False))
    mask, RT, Kc = case.cull
    x, y = R.cull_project_f64(case.pts, RT, Kc)
    r, s = np.divmod(np.arange(64 * case.S), case.S)
    assert np.abs(x - s).max() <= 0.01 and np.abs(y - (r >> 3)).max() <= 0.01 <= 1.0 / 8
    assert (case.inside.reshape(-1) == (mask[0][r >> 3, s] != 0)).all()
    dead = ~case.inside.any(0)
    assert tuple(np.flatnonzero(dead)) == R.CULL_DEAD_COLUMNS and dead[2] and dead[3] and not dead[4] and dead[case.S - 1]
    partial = (~case.inside).sum(0)[~dead]
    assert partial.sum() >= 6 and (partial > 0).sum() >= 4 and partial.max() < 64
