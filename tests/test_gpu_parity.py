"""GPU parity tests (run with -m gpu on an MI355X): every HIP entry point against the CPU oracle
(oracle/neuralbody_oracle.py) on the same seeded inputs, and against the committed golden fixtures
that tests/golden/make_golden.py produced by running the UNMODIFIED reference.  All calls go through
the C ABI (neuralbody_amd.ops -> libnb_hip.so).

Tolerances: RGB <= 1e-4 L-inf (BASELINE.json north_star); intermediate quantities are compared
relative to max(1, |ref|) with the budgets written next to each check."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import synthetic as syn
from tests.golden import scenes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = list(scenes.SCENES)
PRECISIONS = ["f32", "f16f6"]  # nb_march / nb_decode_points arithmetics
POINT_PRECISIONS = PRECISIONS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from neuralbody_amd import _lib

    _lib.lib()  # fail loudly if libnb_hip.so is missing


def _scene_with_oracle_volumes(name, precision="f32"):
    from neuralbody_amd import ops

    r, sd, body, batch, cam, t_rand = scenes.build(name)
    training = r["mode"] == "train"
    sdt, vols, out_sh = H.oracle_volumes(sd, batch, training)
    net = H.make_network(sd, DEV, training, precision)
    bd = H.device_batch(batch, DEV)
    vols_dev = [v.to(DEV) for v in vols]  # NCDHW; Network converts to channels-last
    sp = H.sp_input_of(bd, out_sh)
    return r, sd, sdt, batch, bd, vols, vols_dev, sp, net, t_rand


# ------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("precision", POINT_PRECISIONS)
def test_decode_points_stages_against_oracle(precision):
    """nb_decode_points with the debug tap: gathered features (K3/K4), fc_2 output (K5), the merged
    feature/latent layer, view_fc hidden (K6/K7) and raw, each against the oracle."""
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    r, sd, sdt, batch, bd, vols, vols_dev, sp, net, _ = _scene_with_oracle_volumes("small", precision)
    ns = r["n_samples"]
    ray_o, ray_d = torch.from_numpy(batch["ray_o"]), torch.from_numpy(batch["ray_d"])
    near, far = torch.from_numpy(batch["near"]), torch.from_numpy(batch["far"])
    sel = slice(0, None, 5)
    wpts, z = orc.get_sampling_points(ray_o[:, sel], ray_d[:, sel], near[:, sel], far[:, sel], ns)
    vd = ray_d[:, sel] / torch.norm(ray_d[:, sel], dim=2, keepdim=True)
    w = wpts.reshape(1, -1, 3)
    v = vd[:, :, None].repeat(1, 1, ns, 1).reshape(1, -1, 3)
    # a few points outside the volume exercise zero padding
    w[0, :7] += torch.tensor([3.0, -2.0, 1.0])
    sp_cpu = {"R": torch.from_numpy(batch["R"]), "Th": torch.from_numpy(batch["Th"]),
              "bounds": torch.from_numpy(batch["bounds"]), "latent_index": torch.from_numpy(batch["latent_index"]),
              "out_sh": sp["out_sh"]}
    with torch.no_grad():
        pp = orc.pts_to_can_pts(w, sp_cpu["R"], sp_cpu["Th"])
        g = orc.get_grid_coords(pp, sp_cpu["bounds"], sp_cpu["out_sh"], (0.005,) * 3)[:, None, None]
        feat = orc.interpolate_features(g, vols)[0].T  # [N,352]
        h = torch.relu(torch.nn.functional.conv1d(feat.T[None], sdt["fc_0.weight"], sdt["fc_0.bias"]))
        h = torch.relu(torch.nn.functional.conv1d(h, sdt["fc_1.weight"], sdt["fc_1.bias"]))
        h3 = torch.relu(torch.nn.functional.conv1d(h, sdt["fc_2.weight"], sdt["fc_2.bias"]))
        raw = orc.calculate_density_color(sdt, w, v, vols, sp_cpu)[0]
        dens = orc.calculate_density(sdt, w, vols, sp_cpu)[0]
    scene = net.make_scene(vols_dev, sp, precision)
    lb = net.latent_bias(bd["latent_index"])
    tap = precision != "f16f6"  # the f16f6 point decoder is the march kernel (every point a one-sample ray): no activation tap
    res = ops.decode_points(scene, net.packed_weights(precision), lb, w[0].to(DEV).contiguous(), v[0].to(DEV).contiguous(),
                            debug=tap, precision=precision)
    out, dbg = res if tap else (res, None)
    torch.cuda.synchronize()
    assert np.abs(feat.numpy()).max() > 0.1 and (np.abs(feat.numpy()).sum(1) == 0).any()
    # raw logits reach |20| with the synthetic alpha_fc x20 / rgb_fc x8 gains; the cross terms (four-bit weights since round 6)
    # carry ~2^-13 relative error per GEMM term, the fp32 path only summation-order noise.  (The contract is on the RGB of a
    # composited ray, 1e-4; the logits pass through a sigmoid and the weights of the ray's other samples.)
    tol_h, tol_raw = (1e-4, 2e-4) if precision == "f32" else (3e-4, 2.5e-3)
    e_h = float("nan")
    if tap:
        dbg = dbg.cpu().numpy()
        H.assert_close(dbg[:, :352], feat.numpy(), 2e-5, "trilinear features")
        e_h = H.assert_close(dbg[:, 864:1120], h3[0].T.numpy(), tol_h, "fc_2 output")
    e_raw = H.assert_close(out.cpu().numpy(), raw.numpy(), tol_raw, "raw (rgb logits, sigma)")
    print("%s: fc_2 err %.2e, raw err %.2e (rel. to max(1,|ref|))" % (precision, e_h, e_raw))
    # public API paths
    raw_api = net.calculate_density_color(w.to(DEV), v.to(DEV), vols_dev, sp)
    assert raw_api.shape == (1, w.shape[1], 4)
    assert H.same_result(raw_api[0], out, precision, 2e-4)  # ('f16f6': the API sorts the points spatially first: other groups, and
    # a six-bit quantisation step that falls differently moves a logit of |20| by ~1e-3)
    dens_api = net.calculate_density(w.to(DEV), vols_dev, sp)
    assert dens_api.shape == (1, w.shape[1], 1)
    H.assert_close(dens_api[0].cpu().numpy(), dens.numpy(), tol_raw, "calculate_density")
    # ragged size: n not a multiple of 32, and n == 0
    part = ops.decode_points(scene, net.packed_weights(precision), lb, w[0, :77].to(DEV).contiguous(), v[0, :77].to(DEV).contiguous(),
                             precision=precision)
    assert H.same_result(part, out[:77], precision, 1e-5)  # (raw logits reach |20|)
    empty = ops.decode_points(scene, net.packed_weights(precision), lb, w[0, :0].to(DEV).contiguous(), v[0, :0].to(DEV).contiguous(),
                              precision=precision)
    assert empty.shape == (0, 4)


def test_decode_matches_reference_raw_subset():
    """raw at the reference's own sample points (fixture: every 8th ray of scene 'small')."""
    r, sd, sdt, batch, bd, vols, vols_dev, sp, net, _ = _scene_with_oracle_volumes("small")
    g = H.golden("small")
    rend = H.make_renderer(net, r)
    sel = slice(0, None, scenes.RAW_RAY_STRIDE)
    wpts, z = rend.get_sampling_points(bd["ray_o"][:, sel], bd["ray_d"][:, sel], bd["near"][:, sel], bd["far"][:, sel])
    vd = bd["ray_d"][:, sel] / torch.norm(bd["ray_d"][:, sel], dim=2, keepdim=True)
    raw = rend.get_density_color(wpts, vd, lambda x, v: net.calculate_density_color(x, v, vols_dev, sp))
    H.assert_close(raw.cpu().numpy(), g["raw_subset"], 3e-4, "raw vs reference")
    dens = net.calculate_density(wpts.view(1, -1, 3), vols_dev, sp)
    H.assert_close(dens.cpu().numpy(), g["density_subset"], 3e-4, "density vs reference")


def test_network_forward_and_positional_encoding_tap():
    """Network.forward (latent_xyzc.py:128-163 signature; the reference's body is broken, ours must work) equals
    calculate_density_color on the same points, and the positional-encoding tap (TAP['PE'], the 90 view_fc inputs after the 256
    feature columns) equals the reference embedder (embedder.py:10-36) applied to viewdir / world point."""
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    r, sd, sdt, batch, bd, vols, vols_dev, sp, net, _ = _scene_with_oracle_volumes("small", "f32")
    rend = H.make_renderer(net, r)
    sel = slice(0, None, 11)
    wpts, _z = rend.get_sampling_points(bd["ray_o"][:, sel], bd["ray_d"][:, sel], bd["near"][:, sel], bd["far"][:, sel])
    vd = bd["ray_d"][:, sel] / torch.norm(bd["ray_d"][:, sel], dim=2, keepdim=True)
    w = wpts.reshape(1, -1, 3)
    v = vd[:, :, None].repeat(1, 1, r["n_samples"], 1).reshape(1, -1, 3)
    # forward() takes the ENCODED inputs (their first three entries are the raw direction / point) and encodes the frame itself
    sp_full = rend.prepare_sp_input(bd)
    raw_fwd = net.forward(sp_full, None, orc.embed(v.cpu(), 4).to(DEV), orc.embed(w.cpu(), 10).to(DEV))
    raw_ref = net.calculate_density_color(w, v, net.encode_sparse_voxels(sp_full), sp_full)
    assert raw_fwd.shape == (1, w.shape[1], 4)
    assert torch.equal(raw_fwd, raw_ref)
    with torch.no_grad():
        raw_orc = orc.calculate_density_color(sdt, w.cpu(), v.cpu(), orc.encode_sparse_voxels(
            sdt, torch.from_numpy(batch["coord"]), sp["out_sh"], training=True),
            {"R": torch.from_numpy(batch["R"]), "Th": torch.from_numpy(batch["Th"]), "bounds": torch.from_numpy(batch["bounds"]),
             "latent_index": torch.from_numpy(batch["latent_index"]), "out_sh": sp["out_sh"]})
    H.assert_close(raw_fwd.cpu().numpy(), raw_orc.numpy(), 3e-4, "Network.forward vs oracle")
    # the PE tap
    scene = net.make_scene(vols_dev, sp)
    lb = net.latent_bias(bd["latent_index"])
    _out, dbg = ops.decode_points(scene, net.packed_weights(), lb, w[0].contiguous(), v[0].contiguous(), debug=True, precision="f32")
    a, b = ops.TAP["PE"]
    pe = dbg[:, a:b].cpu().numpy()
    ref = torch.cat([orc.embed(v[0].cpu(), 4), orc.embed(w[0].cpu(), 10)], -1).numpy()  # view_fc input order (latent_xyzc.py:118)
    assert pe.shape == ref.shape == (w.shape[1], 90)
    H.assert_close(pe, ref, 1e-6, "positional-encoding tap", rel=False)


@pytest.mark.parametrize("training", [True, False])
def test_encoder_split_fp16_convolutions_match_the_fp32_kernels(training, monkeypatch):
    """Inference runs the >= 32-channel sparse convolutions on the 16-bit matrix pipe (nb_enc_conv16: head / remainder split,
    three products); the exact-fp32 MFMA kernels (NB_ENC_SPLIT=0, and what the training path always uses) are the
    reference here, the oracle comparison of the default path is test_encoder_matches_oracle_and_reference_probes."""
    import neuralbody_amd.network as nw

    r, sd, body, batch, cam, t_rand = scenes.build("full")
    net = H.make_network(sd, DEV, training, "f32")
    bd = H.device_batch(batch, DEV)
    from neuralbody_amd.renderer import Renderer

    sp = Renderer(net).prepare_sp_input(bd)
    vols = {}
    for split in (True, False):
        monkeypatch.setattr(nw, "ENC_SPLIT", split)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)  # same BN running stats
        with torch.no_grad():
            vols[split] = [v.clone() for v in net.encode_sparse_voxels(sp)]
    torch.cuda.synchronize()
    for a, b in zip(vols[True], vols[False]):
        assert a.shape == b.shape and float(b.abs().max()) > 0
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 2e-5, err


# ------------------------------------------------------------------------------------------- raw_noise_std
@pytest.mark.parametrize("precision", ["f32", "f16f6"])
def test_raw_noise_std_matches_the_reference_formula(precision):
    """cfg.raw_noise_std > 0 (nerf_net_utils.py:31-35; no shipped config sets it): sigma + randn * std before the relu.  The
    noise tensor is passed explicitly (like t_rand) so that the oracle composites the same realisation."""
    from oracle import neuralbody_oracle as orc

    r, sd, body, batch, cam, _ = scenes.build("small_dense")
    net = H.make_network(sd, DEV, True, precision)
    rend = H.make_renderer(net, r)
    rend.cfg.raw_noise_std = 0.7
    n, S = batch["ray_o"].shape[1], r["n_samples"]
    noise = torch.randn(1, n, S, generator=torch.Generator().manual_seed(5))
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        out = rend.render(bd, raw_noise=noise.to(DEV))
        clean = orc.render(orc.tensor_state_dict(sd), batch, n_samples=S, training=True, white_bkgd=r["white_bkgd"])
        tb = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
        _, z = orc.get_sampling_points(tb["ray_o"], tb["ray_d"], tb["near"], tb["far"], S)
        ref = orc.raw2outputs(clean["raw"].reshape(n, S, 4), z.reshape(n, S), tb["ray_d"].reshape(n, 3), r["white_bkgd"],
                              noise=noise[0] * 0.7)
    torch.cuda.synchronize()
    H.assert_close(out["rgb_map"][0].cpu().numpy(), ref[0].numpy(), 1e-4, "rgb_map with noise", rel=False)
    H.assert_close(out["acc_map"][0].cpu().numpy(), ref[2].numpy(), 2e-4, "acc_map with noise")
    assert float((ref[0] - clean["rgb_map"][0]).abs().max()) > 1e-2, "the noise must matter in this scene"


# ------------------------------------------------------------------------------------------- trained weights
@pytest.mark.parametrize("precision", PRECISIONS + ["auto"])
def test_render_with_trained_weights_matches_reference(precision):
    """Every other fixture uses freshly initialised weights.  scene_small_trained.npz comes from 300 Adam steps of the
    reference's own NetworkWrapper (tests/golden/make_golden.py::run_trained): the decoder, the latent codes and the vertex
    codes have an optimiser's distribution, which is what the six-bit block scales and the 'auto' fallback threshold of the
    default arithmetic must survive."""
    g = np.load(os.path.join(H.GOLDEN, "scene_small_trained.npz"))
    params = {k[len("param/"):]: g[k] for k in g.files if k.startswith("param/")}
    assert float(g["loss_history"][-10:].mean()) < 0.05 * float(g["loss_history"][0]), "the fixture did not train"
    r, sd, body, batch, cam, _ = scenes.build_trained(params)
    net = H.make_network(sd, DEV, True, precision)
    rend = H.make_renderer(net, r)
    with torch.no_grad():
        out = rend.render(H.device_batch(batch, DEV))
    torch.cuda.synchronize()
    err = H.assert_close(out["rgb_map"].cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), g["acc_map"], 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), g["weights"], 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), g["depth_map"], 2e-4, "depth_map")
    extra = ""
    if precision == "auto":
        import json
        import warnings

        from neuralbody_amd import ops
        from neuralbody_amd.network import SIX_BIT_MAX_SMALL

        frac = ops.six_bit_small_fraction(net.packed_weights("f16f6")).cpu().numpy()
        extra = " (auto -> %s, six-bit small fraction per layer [fc_1, fc_2, colour head] %s)" % (net.march_precision(), np.round(frac, 3))
        # the statistic the 'auto' policy rests on, for optimiser-shaped weights: asserted, and recorded where the round's
        # records keep it (a warning survives `pytest -q`; the JSON lands in gpurun_out/ when run through gpurun)
        assert net.march_precision() == "f16f6" and float(frac.max()) < 0.7 * SIX_BIT_MAX_SMALL, frac
        rec = {"fixture": "scene_small_trained.npz", "six_bit_small_fraction": {"fc_1": float(frac[0]), "fc_2": float(frac[1]),
               "colour_head": float(frac[2])}, "threshold": SIX_BIT_MAX_SMALL, "rgb_linf_vs_reference": err}
        warnings.warn("trained-like weights: " + json.dumps(rec))
        out_dir = os.path.join(os.path.dirname(H.GOLDEN), "..", "gpurun_out")
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, "trained_six_bit_fraction.json"), "w") as f:
                json.dump(rec, f)
    print("trained/%s: rgb L-inf vs reference %.2e%s" % (precision, err, extra))
    assert float(g["rgb_map"].max() - g["rgb_map"].min()) > 0.2, "fixture is degenerate"


# ------------------------------------------------------------------------------------------- march
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_march_on_oracle_volumes_matches_reference(name, precision):
    """nb_march fed with the oracle's feature volumes against the reference renderer's outputs."""
    r, sd, sdt, batch, bd, vols, vols_dev, sp, net, t_rand = _scene_with_oracle_volumes(name, precision)
    g = H.golden(name)
    tr = None if t_rand is None else torch.from_numpy(t_rand)[0].to(DEV).contiguous()
    out = net.render_rays(bd["ray_o"][0], bd["ray_d"][0], bd["near"][0], bd["far"][0], vols_dev, sp, r["n_samples"],
                          t_rand=tr, white_bkgd=r["white_bkgd"], want_raw=True)
    torch.cuda.synchronize()
    e = H.assert_close(out["rgb_map"].cpu().numpy()[None], g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    print("march %s/%s: rgb L-inf vs reference %.2e" % (name, precision, e))
    H.assert_close(out["acc_map"].cpu().numpy()[None], g["acc_map"], 1e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy()[None], g["weights"], 1e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy()[None], g["depth_map"], 1e-4, "depth_map")
    # disp = 1 / (depth / acc): a quotient of two sums that both vanish on rays grazing the body, so it amplifies the weights'
    # error there (the worst pixel of small_eval has acc 0.03); the six-bit cross terms get 5e-4 for it, everything else
    # keeps the common tolerances
    H.assert_close(out["disp_map"].cpu().numpy()[None], g["disp_map"], 2e-3 if precision == "f16f6" else 3e-4, "disp_map")  # (four-bit cross terms: 1.4e-3 at acc 0.03)
    assert float(g["rgb_map"].max()) > 0.1, "fixture is degenerate"


@pytest.mark.parametrize("precision", ["f16f6"])
def test_activations_beyond_fp16_range_saturate_instead_of_turning_into_nan(precision):
    """the fp16 head of an activation is the one place where the f16 arithmetics have less range than fp32.  With
    MODE.FP16_OVFL set by the kernels (nb_f6_ops.h) a layer output above 65504 saturates; without it it became inf, the
    remainder inf - inf, and the pixel NaN.  fc_0 scaled by 3e5 puts h1 far beyond the range: the render must stay finite
    (it is not accurate there: the product is formed from saturated heads)."""
    r, sd, body, batch, cam, _ = scenes.build("small")
    big = dict(sd)
    big["fc_0.weight"] = (np.array(sd["fc_0.weight"]) * 3e5).astype(np.float32)
    big["fc_0.bias"] = (np.array(sd["fc_0.bias"]) * 3e5).astype(np.float32)
    bd = H.device_batch(batch, DEV)
    outs = {}
    for prec in (precision, "f32"):
        net = H.make_network(big, DEV, True, prec)
        with torch.no_grad():
            outs[prec] = H.make_renderer(net, r).render(bd)
    for k in ("rgb_map", "acc_map", "weights", "depth_map"):  # (disp_map is 0 / 0 = nan on empty rays in the reference itself,
        v = outs[precision][k]                                  # nerf_net_utils.py:44, and WHICH rays are empty changes here)
        assert torch.isfinite(v).all(), "%s: %s has %d non-finite values" % (precision, k, int((~torch.isfinite(v)).sum()))
    assert torch.isfinite(outs["f32"]["rgb_map"]).all()
    ref, got = outs["f32"]["rgb_map"][0], outs[precision]["rgb_map"][0]
    print("%s with h1 ~ 1e5..1e7: rgb differs from fp32 by %.3g (max), %.3g (median)" % (
        precision, float((got - ref).abs().max()), float((got - ref).abs().median())))


def test_auto_precision_picks_six_bits_unless_the_weight_blocks_are_wide():
    """Network(precision='auto') = 'f16f6' for ordinary weights and the exact 'f32' kernel (with a warning) when a layer's
    (row, 32 K) blocks span a wide dynamic range (the statistic nb_mlp_pack_sections leaves behind the f16f6 stream,
    nb_mlp_six_bit_stats_offset).  A function of the weights alone: no timing, the same answer on every rank."""
    from neuralbody_amd import ops
    from neuralbody_amd.network import SIX_BIT_MAX_SMALL

    sd = syn.make_weights(3, num_train_frame=7)
    net = H.make_network(sd, DEV, True, "auto")
    assert net.march_precision() == "f16f6"
    frac = ops.six_bit_small_fraction(net.packed_weights("f16f6")).cpu().numpy()
    print("share of weights below 1/8 of their block maximum, per layer:", np.round(frac, 3))
    assert frac.shape == (3,) and (frac > 0.05).all() and (frac < 0.35).all()
    # per-column gains of 2^-6..2^6 on fc_1 (compensated on fc_0's rows: the function is unchanged)
    rs = np.random.RandomState(5)
    gain = np.exp2(rs.uniform(-6, 6, 256)).astype(np.float32)
    wide = dict(sd)
    wide["fc_0.weight"] = (np.array(sd["fc_0.weight"]) * gain[:, None, None]).astype(np.float32)
    wide["fc_0.bias"] = (np.array(sd["fc_0.bias"]) * gain).astype(np.float32)
    wide["fc_1.weight"] = (np.array(sd["fc_1.weight"]) / gain[None, :, None]).astype(np.float32)
    net2 = H.make_network(wide, DEV, True, "auto")
    with pytest.warns(UserWarning, match="exact fp32 kernel"):
        assert net2.march_precision() == "f32"
    assert float(ops.six_bit_small_fraction(net2.packed_weights("f16f6")).max()) > SIX_BIT_MAX_SMALL
    # the choice follows the weights: loading the ordinary ones back flips it
    net2.load_state_dict(net.state_dict())
    assert net2.march_precision() == "f16f6"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_march_edge_cases(precision):
    """Ragged and degenerate inputs: ray counts around the 32-ray wavefront / 128-ray workgroup granularity
    (0, 1, 31, 33, 129), sample counts that are not a multiple of 8 (scalar weight-store path) or tiny (S=2),
    rays that miss the volume completely (zero features everywhere), white background."""
    from oracle import neuralbody_oracle as orc

    r, sd, sdt, batch, bd, vols, vols_dev, sp, net, _ = _scene_with_oracle_volumes("small_dense", precision)
    n_all = batch["ray_o"].shape[1]
    ro, rd, ne, fa = bd["ray_o"][0], bd["ray_d"][0], bd["near"][0], bd["far"][0]
    full = net.render_rays(ro, rd, ne, fa, vols_dev, sp, 64, white_bkgd=True)
    for n in (0, 1, 31, 33, 129):
        part = net.render_rays(ro[:n].contiguous(), rd[:n].contiguous(), ne[:n].contiguous(), fa[:n].contiguous(),
                               vols_dev, sp, 64, white_bkgd=True)
        for k in full:
            assert part[k].shape[0] == n
            assert H.same_result(part[k], full[k][:n], precision, 1e-4 if k == "disp_map" else 2e-6), (k, n)
    # an explicit slot list (nb_hip.h ray_order: the rays reversed, padded to whole groups of 64 with padding slots that march
    # the last ray again and store nothing, plus a dead group) changes nothing
    from neuralbody_amd._lib import SLOT_DEAD

    perm = torch.arange(n_all - 1, -1, -1, dtype=torch.int32, device=DEV)
    pad = -(perm[-1:].expand((-n_all) % 64) + 1)
    dead = torch.full((64,), SLOT_DEAD, dtype=torch.int32, device=DEV)
    slots = torch.cat([dead, perm, pad]).contiguous()
    rev = net.render_rays(ro, rd, ne, fa, vols_dev, sp, 64, white_bkgd=True, ray_order=slots)
    assert H.same_result(rev["rgb_map"], full["rgb_map"], precision) and H.same_result(rev["weights"], full["weights"], precision)
    # other sample counts against the oracle
    sub = slice(0, 160)
    for S in (2, 20, 40):
        b_np = dict(batch)
        for k in ("ray_o", "ray_d", "near", "far"):
            b_np[k] = batch[k][:, sub]
        with torch.no_grad():
            ref = orc.render(sdt, b_np, n_samples=S, training=True, feature_volume=vols, white_bkgd=True)
        got = net.render_rays(ro[sub].contiguous(), rd[sub].contiguous(), ne[sub].contiguous(), fa[sub].contiguous(),
                              vols_dev, sp, S, white_bkgd=True)
        H.assert_close(got["rgb_map"].cpu().numpy()[None], ref["rgb_map"].numpy(), H.RGB_TOL, "rgb S=%d" % S, rel=False)
        H.assert_close(got["weights"].cpu().numpy()[None], ref["weights"].numpy(), 2e-4, "weights S=%d" % S)
    # rays pointing away from the body: every sample lies outside the volume -> all features are zero padding
    away = {k: torch.from_numpy(batch[k][:, :64].copy()) for k in ("ray_o", "ray_d", "near", "far")}
    away["ray_d"] = -away["ray_d"]
    b_np = dict(batch)
    b_np.update({k: v.numpy() for k, v in away.items()})
    with torch.no_grad():
        ref = orc.render(sdt, b_np, n_samples=64, training=True, feature_volume=vols, white_bkgd=True)
    got = net.render_rays(away["ray_o"][0].to(DEV), away["ray_d"][0].to(DEV), away["near"][0].to(DEV),
                          away["far"][0].to(DEV), vols_dev, sp, 64, white_bkgd=True)
    H.assert_close(got["rgb_map"].cpu().numpy()[None], ref["rgb_map"].numpy(), H.RGB_TOL, "rgb of rays that miss", rel=False)
    H.assert_close(got["acc_map"].cpu().numpy()[None], ref["acc_map"].numpy(), 1e-4, "acc of rays that miss")


def test_composite_matches_oracle():
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    rs = np.random.RandomState(5)
    for n, S, white in ((37, 64, False), (5, 128, True), (3, 40, False), (2, 2, False), (1, 200, True)):
        raw = (rs.standard_normal((n, S, 4)) * 3).astype(np.float32)
        raw[0, :, 3] = -1.0  # a ray that hits nothing: acc = 0, disp = NaN (nerf_net_utils.py:44-45)
        z = np.sort(rs.uniform(1, 3, (n, S)).astype(np.float32), axis=1)
        d = rs.standard_normal((n, 3)).astype(np.float32)
        ref = orc.raw2outputs(torch.from_numpy(raw), torch.from_numpy(z), torch.from_numpy(d), white)
        got = ops.composite(torch.from_numpy(raw).to(DEV), torch.from_numpy(z).to(DEV), torch.from_numpy(d).to(DEV), white)
        for a, b, nm in zip(got, ref, ("rgb", "disp", "acc", "weights", "depth")):
            H.assert_close(a.cpu().numpy(), b.numpy(), 2e-6, "composite %s n=%d S=%d" % (nm, n, S))
        assert np.isnan(got[1].cpu().numpy()[0])


# ------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("name", ["small", "small_eval", "full"])
def test_encoder_matches_oracle_and_reference_probes(name):
    """nb_enc_* (voxelise, 17 x [sparse conv, BN, ReLU], 4 x dense) against the oracle's dense
    stand-in and the reference-generated probe values."""
    from oracle import neuralbody_oracle as orc

    r, sd, body, batch, cam, _ = scenes.build(name)
    training = r["mode"] == "train"
    g = H.golden(name)
    sdt = orc.tensor_state_dict(sd)
    stats = {}
    with torch.no_grad():
        out_sh = batch["out_sh"].max(0).tolist()
        ref = orc.encode_sparse_voxels(sdt, torch.from_numpy(batch["coord"]), out_sh, training=training,
                                       update_stats=stats)
    net = H.make_network(sd, DEV, training)
    bd = H.device_batch(batch, DEV)
    from neuralbody_amd.renderer import Renderer

    sp = Renderer(net).prepare_sp_input(bd)
    vols = net.encode_sparse_voxels(sp)
    torch.cuda.synchronize()
    assert len(vols) == 4
    for li, (v, rv) in enumerate(zip(vols, ref)):
        assert tuple(v.shape) == tuple(rv.shape), (li, v.shape, rv.shape)
        a = v.cpu().numpy()
        b = rv.numpy()
        assert np.array_equal(np.abs(a).sum(1) > 0, np.abs(b).sum(1) > 0), "active set differs at level %d" % li
        H.assert_close(a, b, 2e-4, "volume level %d" % li)  # 17 fp32 conv+BN layers, different summation order
        flat = a[0].transpose(1, 2, 3, 0).reshape(-1, a.shape[1])
        H.assert_close(flat[g["vol%d_probe_idx" % li]], g["vol%d_probe_val" % li], 3e-4, "reference probes level %d" % li)
        assert int((np.abs(flat).sum(1) > 0).sum()) == int(g["vol%d_nonzero_voxels" % li])
    if training:
        sd_after = net.state_dict()
        for k, v in stats.items():
            H.assert_close(sd_after[k].cpu().numpy(), v.numpy(), 2e-5, k)
            H.assert_close(sd_after[k].cpu().numpy(), g["bn/" + k], 2e-5, k + " vs reference")
        assert int(sd_after["xyzc_net.conv0.1.num_batches_tracked"]) == 1
    else:
        assert torch.equal(net.state_dict()["xyzc_net.conv0.1.running_mean"].cpu(),
                           torch.from_numpy(sd["xyzc_net.conv0.1.running_mean"]))


def test_encoder_edge_cases():
    """duplicate coordinates (last vertex wins), all vertices in one voxel, voxels on the grid border."""
    from neuralbody_amd import ops

    coord = torch.tensor([[0, 0, 0], [31, 31, 31], [5, 6, 7], [5, 6, 7], [0, 0, 0]], dtype=torch.int32, device=DEV)
    grid, rows_vert, rows_lin, n_rows = ops.enc_voxelize(coord, [32, 32, 32])
    torch.cuda.synchronize()
    assert int(n_rows) == 3
    assert sorted(rows_vert[:3].tolist()) == [1, 3, 4]
    gv = grid.cpu().numpy()
    assert (gv >= 0).sum() == 3 and gv[5, 6, 7] >= 0 and gv[31, 31, 31] >= 0
    rv, rl = rows_vert[:3].tolist(), rows_lin[:3].tolist()
    for v, lin in zip(rv, rl):
        d, h, w = coord[v].tolist()
        assert lin == (d * 32 + h) * 32 + w and gv[d, h, w] == rv.index(v)
    og, ol, no, nmax, odhw = ops.enc_downsample_index(rows_lin, n_rows, 5, [32, 32, 32])
    torch.cuda.synchronize()
    ref_mask = torch.nn.functional.max_pool3d((torch.from_numpy(gv)[None, None] >= 0).float(), 3, 2, 1)[0, 0] > 0
    assert odhw == [16, 16, 16]
    assert np.array_equal(og.cpu().numpy() >= 0, ref_mask.numpy())
    assert int(no) == int(ref_mask.sum())
    lin = ol[:int(no)].cpu().numpy()
    assert np.all(np.diff(lin) > 0), "rows must be numbered in linear voxel order"
    assert np.array_equal(og.cpu().numpy().reshape(-1)[lin], np.arange(int(no)))
    # empty input
    grid, rows_vert, rows_lin, n_rows = ops.enc_voxelize(coord[:0].contiguous(), [32, 32, 32])
    torch.cuda.synchronize()
    assert int(n_rows) == 0 and int((grid >= 0).sum()) == 0


@pytest.mark.parametrize("dhw,n", [([61, 90, 47], 6890), ([32, 32, 32], 5), ([17, 9, 30], 400), ([8, 8, 8], 0), ([2, 1, 2], 3),
                                   ([40, 52, 50], 3000)])  # 13 tiles (the last partial), then 2 (likewise), 1 and 1
def test_all_levels_index_sets_equal_the_chained_per_level_ones(dhw, n):
    """nb_enc_downsample_index_all (three launches for the four strided levels) against four chained nb_enc_downsample_index calls:
    the same active cells, the same row numbers, the same out_lin and counts, bit for bit — odd and even grid sizes, voxels on the
    borders, an empty level; and the active cells against max_pool3d(k=3, s=2, p=1) of the level above."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(7)
    c = np.stack([rs.randint(0, s, size=max(n, 1)) for s in dhw], 1).astype(np.int32)
    if n:
        c[0] = [s - 1 for s in dhw]  # the far corner
        c[-1] = 0
    coord = torch.from_numpy(c[:n]).to(DEV).contiguous()
    grid, rows_vert, rows_lin, n_rows = ops.enc_voxelize(coord, dhw)
    chained, lin, cnt, cap, d = [], rows_lin, n_rows, n, list(dhw)
    for _ in range(4):
        og, ol, no, nmax, odhw = ops.enc_downsample_index(lin, cnt, cap, d)
        chained.append((og, ol, no, nmax, odhw))
        lin, cnt, cap, d = ol, no, nmax, odhw
    bufs, grids, cap, d = [], [], n, list(dhw)
    for _ in range(4):
        cap, d = ops.down_capacity(cap, d), ops.down_dhw(d)
        bufs.append(torch.zeros(cap + 1, dtype=torch.int32, device=DEV))
        grids.append(torch.full(d, -1, dtype=torch.int32, device=DEV))
    together = ops.enc_downsample_index_all(rows_lin, n_rows, n, dhw, bufs, grids)
    torch.cuda.synchronize()
    above = (grid >= 0).float().cpu()[None, None]
    for level, (a, b) in enumerate(zip(chained, together)):
        assert a[3] == b[3] and a[4] == b[4], level
        assert int(a[2]) == int(b[2]), level
        assert torch.equal(a[0], b[0]), level
        k = int(a[2])
        assert torch.equal(a[1][:k], b[1][:k]), level
        above = (torch.nn.functional.max_pool3d(above, 3, 2, 1) > 0).float()
        assert np.array_equal((b[0] >= 0).cpu().numpy(), above[0, 0].numpy() > 0), level


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_render_end_to_end_matches_reference(name, precision):
    """Renderer.render(batch) — encoder + march, all HIP — against the reference renderer's outputs."""
    r, sd, body, batch, cam, t_rand = scenes.build(name)
    g = H.golden(name)
    net = H.make_network(sd, DEV, r["mode"] == "train", precision)
    rend = H.make_renderer(net, r)
    bd = H.device_batch(batch, DEV)
    tr = None if t_rand is None else torch.from_numpy(t_rand).to(DEV)
    with torch.no_grad():
        out = rend.render(bd, t_rand=tr)
    torch.cuda.synchronize()
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map"}
    n = batch["ray_o"].shape[1]
    assert out["rgb_map"].shape == (1, n, 3) and out["weights"].shape == (1, n, r["n_samples"])
    err = H.assert_close(out["rgb_map"].cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), g["acc_map"], 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), g["weights"], 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), g["depth_map"], 2e-4, "depth_map")
    print("%s/%s: rgb L-inf vs reference %.2e over %d rays" % (name, precision, err, n))
    # unfused path of the overridable API (get_pixel_value) agrees with the fused march
    if t_rand is None:
        sp = rend.prepare_sp_input(bd)
        vols = net.encode_sparse_voxels(sp) if r["mode"] != "train" else None
        if vols is not None:
            pv = rend.get_pixel_value(bd["ray_o"], bd["ray_d"], bd["near"], bd["far"], vols, sp, bd)
            # the unfused path decodes every sample as a one-sample ray of the same kernel, in other groups (points of one
            # depth step share a workgroup there, samples of 64 rays here): the two sides differ by rounding
            H.assert_close(pv["rgb_map"].cpu().numpy(), out["rgb_map"].cpu().numpy(), 6e-5 if precision == "f16f6" else 1e-5,
                           "fused vs unfused rgb")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["mmsk", "msk"])
def test_mask_culled_renderers_match_reference(kind, precision):
    """RendererMmsk / RendererMsk (sample culling inside nb_march) against the reference's if_clight_renderer_mmsk /
    if_clight_renderer_msk outputs (tests/golden/masked_*.npz, generated by make_golden.py::run_masked)."""
    from neuralbody_amd.renderer import RenderConfig, Renderer, RendererMmsk, RendererMsk

    g = np.load(os.path.join(H.GOLDEN, "masked_%s.npz" % kind))
    r, sd, batch, (Hh, Ww) = scenes.build_masked(kind)
    net = H.make_network(sd, DEV, True, precision)
    cfg = RenderConfig(N_samples=r["n_samples"], perturb=0.0, raw_noise_std=0.0, white_bkgd=False)
    rend = (RendererMmsk if kind == "mmsk" else RendererMsk)(net, cfg)
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        out = rend.render(bd)
        base = Renderer(net, cfg).render(bd)  # the un-culled renderer on the same batch
    torch.cuda.synchronize()
    err = H.assert_close(out["rgb_map"].cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), g["acc_map"], 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), g["weights"], 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), g["depth_map"], 2e-4, "depth_map")
    # culled samples carry exactly zero weight; and the culling changes the image (the fixture exercises it)
    inside = g["inside"].reshape(out["weights"].shape)
    assert float(out["weights"].cpu().numpy()[~inside].max(initial=0.0)) == 0.0
    assert float((out["rgb_map"] - base["rgb_map"]).abs().max()) > 1e-2
    print("%s/%s: rgb L-inf vs reference %.2e, inside fraction %.2f" % (kind, precision, err, inside.mean()))


@pytest.mark.parametrize("precision", POINT_PRECISIONS)
def test_density_cube_matches_reference(precision, monkeypatch):
    """RendererMesh (encoder + nb_decode_points(density_only) over the inside lattice points) against the cube the
    reference's if_mesh_renderer hands to marching cubes (tests/golden/mesh_cube.npz)."""
    import sys
    import types

    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    g = np.load(os.path.join(H.GOLDEN, "mesh_cube.npz"))
    r, sd, batch = scenes.build_mesh()
    net = H.make_network(sd, DEV, True, precision)
    rend = RendererMesh(net, RenderConfig(mesh_th=5.0))
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        cube = rend.density_cube(bd)
    torch.cuda.synchronize()
    assert cube.is_cuda and tuple(cube.shape) == g["cube"].shape
    # densities reach |20|; 'f16f6' carries ~4e-4 of absolute density error (its measured sigma error, bench.ILL_SIGMA), the
    # exact and split-bf16 decoders stay below 2e-4
    err = H.assert_close(cube.cpu().numpy(), g["cube"], 1e-3 if precision == "f16f6" else 2e-4, "cube")
    # the iso-surface decision marching cubes makes is the same everywhere except within the tolerance of the threshold
    ours, ref = cube.cpu().numpy() > 5.0, g["cube"] > 5.0
    assert np.array_equal(ours[np.abs(g["cube"] - 5.0) > 1e-2], ref[np.abs(g["cube"] - 5.0) > 1e-2])
    # render(): same dict as the reference (cube float64 ndarray + mesh); PyMCubes/trimesh are CPU post-processing and
    # absent from the image, so they are stubbed here exactly as in make_golden.py::run_mesh
    mc, tm = types.ModuleType("mcubes"), types.ModuleType("trimesh")
    seen = {}

    def marching_cubes(c, th):
        seen["th"], seen["shape"] = th, c.shape
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)

    mc.marching_cubes = marching_cubes
    tm.Trimesh = lambda v, t: ("mesh", len(v), len(t))
    monkeypatch.setitem(sys.modules, "mcubes", mc)
    monkeypatch.setitem(sys.modules, "trimesh", tm)
    with torch.no_grad():
        out = rend.render(bd)
    assert set(out) == {"cube", "mesh"} and out["cube"].dtype == np.float64 and seen == {"th": 5.0, "shape": g["cube"].shape}
    print("mesh cube/%s: max rel err vs reference %.2e over %d lattice points" % (precision, err, int(g["n_inside"])))


# ------------------------------------------------------------------------------------------- ray generation
def test_raygen_matches_reference_golden():
    from neuralbody_amd import ops
    from tests import synthetic as syn

    g = np.load(H.GOLDEN + "/raygen.npz")
    for tag, body_kw, Hh, Ww, ff in (("a", dict(seed=3, box=(0.9, 1.7, 0.35), rh=(0.2, 0.4, 0.0), th=(0.3, 0.1, 0.2)), 40, 56, 1.1),
                                     ("b", dict(seed=4, box=(0.3, 0.5, 0.2)), 33, 17, 3.0)):
        body = syn.make_body(**body_kw)
        K, R, T = syn.make_camera(body, Hh, Ww, focal_factor=ff, distance=2.2, yaw=-0.6, pitch=0.25)
        ro, rd, near, far, mask, n = ops.raygen(Hh, Ww, K, R, T, body["can_bounds"], DEV)
        torch.cuda.synchronize()
        n = int(n)
        mask = mask.cpu().numpy().astype(bool)
        assert np.array_equal(mask, g[tag + "_mask"])
        assert n == int(mask.sum())
        # float64 ray construction + float32 slab test: identical up to the last float32 bit
        np.testing.assert_allclose(rd[:n].cpu().numpy(), g[tag + "_img_ray_d"], rtol=3e-7, atol=1e-7)
        np.testing.assert_allclose(near[:n].cpu().numpy(), g[tag + "_img_near"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(far[:n].cpu().numpy(), g[tag + "_img_far"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(ro[0].cpu().numpy(), g[tag + "_ray_o"], rtol=3e-7, atol=1e-7)
        assert torch.equal(ro[:n], ro[:1].expand(n, 3))


# ------------------------------------------------------------------------------------------- full size
@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_size_properties_512(precision):
    """BASELINE.json headline shape (512x512, 64 samples, 6890 vertices): size-independent properties —
    sharding invariance (any contiguous ray range reproduces the full render bit for bit), permutation
    equivariance, sum(weights) == acc, finite outputs, and spot parity with the oracle on a ray sample."""
    from tests import synthetic as syn
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from oracle import neuralbody_oracle as orc

    sd = syn.make_weights(0, num_train_frame=230)
    body = syn.make_body(seed=0)
    Hh = Ww = 512
    K, R, T = syn.full_coverage_camera(body, Hh, Ww)
    net = H.make_network(sd, DEV, True, precision)
    ro, rd, near, far, mask, n = [t for t in __import__("neuralbody_amd").ops.raygen(Hh, Ww, K, R, T, body["can_bounds"], DEV)]
    n = int(n)
    assert n == Hh * Ww and bool(mask.all())
    batch = syn.make_batch(body, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros(1, np.float32),
                           np.zeros(1, np.float32), np.ones(1, bool))
    bd = H.device_batch({k: v for k, v in batch.items() if k not in ("ray_o", "ray_d", "near", "far", "mask_at_box")}, DEV)
    bd.update(ray_o=ro[None, :n], ray_d=rd[None, :n], near=near[None, :n], far=far[None, :n])
    rend = Renderer(net, RenderConfig(N_samples=64))
    net.eval()  # keep BN running stats fixed so repeated encodes are identical
    with torch.no_grad():
        full = rend.render(bd)
        torch.cuda.synchronize()
        rgb = full["rgb_map"][0]
        assert torch.isfinite(rgb).all() and torch.isfinite(full["weights"]).all()
        assert float(full["acc_map"].min()) >= 0 and float(full["acc_map"].max()) <= 1 + 1e-5
        H.assert_close(full["weights"][0].sum(-1).cpu().numpy(), full["acc_map"][0].cpu().numpy(), 1e-5, "sum w == acc")
        # sharding invariance on odd boundaries
        for b, e in ((0, 1), (1000, 1037), (n - 77, n), (123457, 131072 + 33)):
            part = rend.render(bd, ray_range=(b, e))
            for k in full:
                assert H.same_result(part[k][0], full[k][0, b:e], precision, 1e-4 if k == "disp_map" else 2e-6), (k, b, e)
        # grouping rays into 8x4 pixel tiles per wavefront (ray_order) changes nothing but locality
        bd_t = dict(bd, mask_at_box=mask[None].bool())
        tiled = Renderer(net, RenderConfig(N_samples=64, H=Hh, W=Ww)).render(bd_t)
        assert Renderer(net, RenderConfig(N_samples=64, H=Hh, W=Ww))._tile_order(bd_t, n, 0, n) is not None
        for k in full:
            assert H.same_result(tiled[k], full[k], precision, 1e-4 if k == "disp_map" else 2e-6), "tiled ray order changed " + k
        part = Renderer(net, RenderConfig(N_samples=64, H=Hh, W=Ww)).render(bd_t, ray_range=(1000, 9000))
        assert H.same_result(part["rgb_map"][0], full["rgb_map"][0, 1000:9000], precision)
        # permutation equivariance
        perm = torch.randperm(4096, device=DEV)
        sub = {k: (v[:, perm] if k in ("ray_o", "ray_d", "near", "far") else v) for k, v in bd.items()}
        sub_out = rend.render(sub)
        assert H.same_result(sub_out["rgb_map"][0], full["rgb_map"][0, perm], precision)
    # spot parity against the oracle on 96 rays spread over the image
    sel = np.linspace(0, n - 1, 96).astype(np.int64)
    b_np = dict(batch)
    b_np.update(ray_o=ro[sel].cpu().numpy()[None], ray_d=rd[sel].cpu().numpy()[None], near=near[sel].cpu().numpy()[None],
                far=far[sel].cpu().numpy()[None])
    with torch.no_grad():
        ref = orc.render(orc.tensor_state_dict(sd), b_np, n_samples=64, training=False)
    H.assert_close(rgb[sel].cpu().numpy()[None], ref["rgb_map"].numpy(), H.RGB_TOL, "512x512 spot rgb", rel=False)
