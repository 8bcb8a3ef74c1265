"""The fold march's layer phases over published activations (csrc/nb_march_fold.hip, layer_s OWN): wave w walks the four K blocks
from the one it has published itself — its first block's operands come from registers, its weight pieces and scale dwords are
packed in its own block order, and the barrier behind the publish stands inside the following phase.  Every case renders with the
default arithmetic (which must resolve to 'f16f6', the folded kernel) and with the exact 'f32' kernel; the rgb of a composited ray
is held to H.RGB_TOL, the bound of the parity suite.

* rotation and pack agree: one workgroup, and a layer whose weights are zero outside ONE K block (input columns 64 b .. 64 b + 63).
  A stream piece or scale dword that meets another block than the kernel reads multiplies the live block by zeros (or by another
  block's scales): an O(1) error in one of the twelve cases;
* shapes where the moved barrier could go wrong: a partial last group, one sample per ray, the point decoder in both modes, and
  a mask-culled march whose groups skip the layers of whole depth steps in front of and behind the decoded ones;
* two renders of one batch are bit-equal."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER_KEYS = {"fc_1": "fc_1.weight", "fc_2": "fc_2.weight", "colour": "feature_fc.weight"}  # the colour head's K phase over fc_2's outputs


@pytest.fixture(scope="module")
def small():
    """Scene 'small' with the heads at nn.Conv1d's own scale and every density positive.  The suite's fixtures scale alpha_fc x20
    and rgb_fc x8 (logits up to |20|) for rays of 64 samples 1/63 of the ray apart: there a density error enters an alpha through
    an interval of a few millimetres, and a ray's colour is a mean over many samples.  A two-sample ray has neither: its interval
    is half the ray (x32), and its last sample (interval 1e10: alpha = 1 wherever sigma > 0) hands ONE colour sigmoid to the
    pixel at full weight.  With unscaled heads the logit errors of the 'f16f6' arithmetic (relative 2^-13 per cross term) shrink
    by the same x20 / x8, which puts the two-sample rays where the 64-sample rays of the suite are; a block of weights meeting the
    wrong activations still moves a logit by its own size (~0.3: 1e-2 in rgb, 200 x the bound).  alpha_fc's bias of +6 keeps
    every density well above zero, so no case hinges on the sign of a last density."""
    from tests import synthetic as syn

    r, _, body, batch, cam, _ = scenes.build("small")
    sd = syn.make_weights(r["weights_seed"], num_train_frame=r["num_train_frame"], alpha_scale=1.0, rgb_scale=1.0, alpha_bias=6.0)
    bd = H.device_batch(batch, DEV)
    n = batch["ray_o"].shape[1]
    t_rand = torch.from_numpy(np.random.RandomState(9).uniform(0.05, 0.95, (n, 2)).astype(np.float32)).to(DEV)
    return r, sd, bd, n, t_rand


def _march(sd, recipe, bd, precision, rays, n_samples, t_rand=None, cull_of=None, from_middle=False):
    """rays `rays` (a slice) of the batch through the fused march of a fresh Network -> dict of per-ray outputs (with `raw`).
    from_middle: the rays start half way through the box (their first sample lies inside the body, not on the box's face)."""
    net = H.make_network(sd, DEV, True, precision)
    rend = H.make_renderer(net, recipe)
    near, far = bd["near"][0, rays], bd["far"][0, rays]
    if from_middle:
        near = 0.5 * (near + far)
    with torch.no_grad():
        sp = rend.prepare_sp_input(bd)
        vols = net.encode_sparse_voxels(sp)
        out = net.render_rays(bd["ray_o"][0, rays].contiguous(), bd["ray_d"][0, rays].contiguous(), near.contiguous(), far.contiguous(),
                              vols, sp, n_samples, t_rand=None if t_rand is None else t_rand[rays].contiguous(), want_raw=True,
                              cull=None if cull_of is None else cull_of(net))
    torch.cuda.synchronize()
    if precision != "f32":
        assert net.march_precision() == "f16f6"  # the case must run the folded kernel
    return out


def _live(ref):
    """The exact render is not degenerate: every density clearly positive (fixture `small`), colours that differ from ray to ray."""
    return float(ref["raw"][..., 3].min()) > 0.5 and float(ref["rgb_map"].std()) > 1e-3


def _rgb_err(a, b):
    return float((a["rgb_map"] - b["rgb_map"]).abs().max())


def _one_group(n):
    b = (n // 2) // 64 * 64  # 64 consecutive rays from the middle of the image: they cross the body
    return slice(b, b + 64)


@pytest.mark.parametrize("block", [0, 1, 2, 3])
@pytest.mark.parametrize("layer", ["fc_1", "fc_2", "colour"])
def test_rotation_and_pack_agree(small, layer, block):
    r, sd, bd, n, t_rand = small
    sd = dict(sd)
    w = np.array(sd[LAYER_KEYS[layer]])
    assert w.shape[:2] == (256, 256)
    keep = np.zeros(256, bool)
    keep[64 * block:64 * block + 64] = True
    w[:, ~keep] = 0.0
    sd[LAYER_KEYS[layer]] = w
    rays = _one_group(n)
    out = _march(sd, r, bd, H.DEFAULT_PRECISION, rays, 2, t_rand)
    ref = _march(sd, r, bd, "f32", rays, 2, t_rand)
    err = _rgb_err(out, ref)
    print("%s block %d: rgb L-inf vs f32 %.2e (rgb spread %.2e, smallest density %.2f)" % (
        layer, block, err, float(ref["rgb_map"].std()), float(ref["raw"][..., 3].min())))
    assert _live(ref)
    assert err <= H.RGB_TOL


def test_partial_last_group(small):
    r, sd, bd, n, t_rand = small
    b = _one_group(n).start
    rays = slice(b, b + 65)
    ref = _march(sd, r, bd, "f32", rays, 2, t_rand)
    err = _rgb_err(_march(sd, r, bd, H.DEFAULT_PRECISION, rays, 2, t_rand), ref)
    print("65 rays: rgb L-inf vs f32 %.2e" % err)
    assert _live(ref)
    assert err <= H.RGB_TOL


def test_one_sample_per_ray(small):
    r, sd, bd, n, _ = small
    b = _one_group(n).start
    rays = slice(b, b + 96)
    ref = _march(sd, r, bd, "f32", rays, 1, from_middle=True)
    err = _rgb_err(_march(sd, r, bd, H.DEFAULT_PRECISION, rays, 1, from_middle=True), ref)
    print("one sample per ray: rgb L-inf vs f32 %.2e" % err)
    assert _live(ref)
    assert err <= H.RGB_TOL


def test_point_decoder_raw_and_density(small):
    """nb_decode_points over 70 points (the two samples of 35 rays): its raw output, and its density beside the exact colours,
    composited like a ray's samples (nb_composite on both sides)."""
    from neuralbody_amd import ops

    r, sd, bd, n, t_rand = small
    b = _one_group(n).start
    rays = slice(b, b + 35)
    res = {}
    for prec in (H.DEFAULT_PRECISION, "f32"):
        net = H.make_network(sd, DEV, True, prec)
        rend = H.make_renderer(net, dict(r, n_samples=2, perturb=True))
        with torch.no_grad():
            sp = rend.prepare_sp_input(bd)
            vols = net.encode_sparse_voxels(sp)
            ro, rd = bd["ray_o"][:, rays], bd["ray_d"][:, rays]
            wpts, z = rend.get_sampling_points(ro, rd, bd["near"][:, rays], bd["far"][:, rays], t_rand=t_rand[rays][None])
            vd = (rd / torch.norm(rd, dim=2, keepdim=True))[:, :, None].expand(-1, -1, 2, -1)
            raw = net.calculate_density_color(wpts.reshape(1, -1, 3).contiguous(), vd.reshape(1, -1, 3).contiguous(), vols, sp)
            dens = net.calculate_density(wpts.reshape(1, -1, 3).contiguous(), vols, sp)
        assert raw.shape == (1, 70, 4) and dens.shape == (1, 70, 1)
        if prec != "f32":
            assert net.march_precision() == "f16f6"
        res[prec] = (raw.reshape(35, 2, 4).contiguous(), dens.reshape(35, 2), z[0].contiguous(), rd[0].contiguous())
    raw, dens, z, rd = res[H.DEFAULT_PRECISION]
    raw_ref, dens_ref, z_ref, _ = res["f32"]
    assert torch.equal(z, z_ref)
    rgb_ref = ops.composite(raw_ref, z, rd)[0]
    err_raw = float((ops.composite(raw, z, rd)[0] - rgb_ref).abs().max())
    mixed = raw_ref.clone()
    mixed[..., 3] = dens  # the density mode's output in the place of the exact densities
    err_dens = float((ops.composite(mixed, z, rd)[0] - rgb_ref).abs().max())
    exact = raw_ref.clone()
    exact[..., 3] = dens_ref
    assert float((ops.composite(exact, z, rd)[0] - rgb_ref).abs().max()) <= 1e-6  # both f32 modes give one density
    print("70 points: composited rgb L-inf vs f32: raw mode %.2e, density mode %.2e" % (err_raw, err_dens))
    assert float(rgb_ref.std()) > 1e-3 and float(raw_ref[..., 3].min()) > 0.5
    assert err_raw <= H.RGB_TOL and err_dens <= H.RGB_TOL


def test_mask_culled_groups_skip_steps():
    """Two groups of the capsule fixture under RendererMmsk's culling, chosen where the reference's inside mask (the golden
    file's) leaves depth steps without a single surviving sample both in front of and behind the decoded ones: the march goes
    from the skipped-layers path into the publishes and back."""
    from neuralbody_amd.renderer import RenderConfig, RendererMmsk

    g = np.load(os.path.join(H.GOLDEN, "masked_mmsk.npz"))
    r, sd, batch, _ = scenes.build_masked("mmsk")
    n, S = batch["ray_o"].shape[1], r["n_samples"]
    inside = g["inside"].reshape(n, S)
    first = None
    for gi in range(n // 64):
        live = inside[64 * gi:64 * gi + 64].any(0)  # per depth step: does the group decode anything
        if live.any() and not live[0] and not live[-1]:  # skipped steps in front of AND behind the decoded ones
            first = gi
            break
    assert first is not None, "the fixture has no group that skips depth steps on both sides of its decoded ones"
    rays = slice(64 * first, min(64 * first + 128, n))
    bd = H.device_batch(batch, DEV)
    cfg = RenderConfig(N_samples=S, perturb=0.0, raw_noise_std=0.0, white_bkgd=False)
    cull_of = lambda net: RendererMmsk(net, cfg).make_cull(bd)  # noqa: E731
    recipe = dict(n_samples=S, perturb=False, white_bkgd=False)
    out = _march(sd, recipe, bd, H.DEFAULT_PRECISION, rays, S, cull_of=cull_of)
    ref = _march(sd, recipe, bd, "f32", rays, S, cull_of=cull_of)
    err = _rgb_err(out, ref)
    print("culled groups %d, %d: rgb L-inf vs f32 %.2e" % (first, first + 1, err))
    w = out["weights"].cpu().numpy()
    assert float(np.abs(w[~inside[rays]]).max(initial=0.0)) == 0.0 and float(w.max()) > 0.0
    assert err <= H.RGB_TOL


def test_two_renders_are_bit_equal(small):
    r, sd, bd, n, t_rand = small
    b = _one_group(n).start
    rays = slice(b, b + 200)
    a, c = (_march(sd, r, bd, H.DEFAULT_PRECISION, rays, 2, t_rand) for _ in range(2))
    for k in ("rgb_map", "weights", "depth_map", "acc_map"):
        assert torch.equal(a[k], c[k]), k
