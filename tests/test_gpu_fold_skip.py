"""The folded first layer walks only the LIVE 16-voxel chunks of a workgroup's voxel list (a chunk whose sixteen table entries are
all the zero row is neither fetched nor multiplied).  Dense volumes handed over as a plain list make exactly their non-zero voxels
active (nb_sparsify), so a test chooses the dead voxels by zeroing them:

  * points (64-point workgroups of nb_decode_points) with whole levels or a half-space dead against the exact-fp32 kernel on the
    same volumes — dead chunks leading, trailing, interleaved, a list without a live chunk, nothing dead, a long list in passes;
  * skipping a chunk against multiplying its zero rows: the same voxels made active with a value that the planes round to zero —
    the two decodes agree to the bit;
  * one culled ray march (RendererMmsk: the culled instance, skipped depth steps and the sequential preparation behind them)
    against the oracle."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import synthetic as syn
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2.5e-3  # raw and density: test_points_on_every_marching_tier_match_the_fp32_kernel
TINY = 1e-30  # fc_0 . V of such a voxel is ~1e-31: below half the smallest fp16 subnormal (3e-8), head and remainder round to zero

# level(s) whose voxels are dead, per variant; "half": every level, in the half-space that holds half of the workgroups
VARIANTS = {"finest": (0,), "coarsest": (3,), "interleaved": (1, 3), "half": "half", "none": (), "long": (0,)}


@pytest.fixture(scope="module")
def small():
    """The small scene: network, its dense volumes (the master copies: never written), the points, the f32 weights."""
    r, sd, body, batch, cam, _ = scenes.build("small")
    net = H.make_network(sd, DEV, True, precision="f16f6")
    bd = H.device_batch(batch, DEV)
    rend = H.make_renderer(net, r)
    with torch.no_grad():
        sp = rend.prepare_sp_input(bd)
        vols = [v.clone() for v in net.encode_sparse_voxels(sp)]
        lb = net.latent_bias(sp["latent_index"])
    verts = torch.from_numpy(body["world_verts"]).to(DEV)
    ctr = verts[torch.from_numpy(np.random.RandomState(3).choice(verts.shape[0], 24)).to(DEV)]
    lat = torch.stack(torch.meshgrid(*[torch.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3).to(DEV) * 0.003
    lattice = (ctr[:, None] + lat[None]).reshape(-1, 3).contiguous()  # 24 workgroups: a 4 x 4 x 4 lattice of 3 mm pitch each
    line = torch.arange(64.0, device=DEV)[:, None] * torch.tensor([0.0, 0.0, 0.005], device=DEV)
    lines = (ctr[:8, None] - torch.tensor([0, 0, 0.1], device=DEV) + line[None]).reshape(-1, 3).contiguous()  # passes of 128
    gen = torch.Generator(device=DEV).manual_seed(2)
    vd = torch.nn.functional.normalize(torch.randn(lattice.shape, device=DEV, generator=gen), dim=-1).contiguous()
    torch.cuda.synchronize()
    return dict(net=net, sp=sp, vols=vols, lb=lb, lattice=lattice, lines=lines, vd=vd, body=body)


def _level_rows(s, pts):
    """Index coordinate along H (the volumes' longest axis here) of `pts` in every level, as the decoder forms it: [4, n]."""
    sp, vols = s["sp"], s["vols"]
    can = (pts - sp["Th"].reshape(1, 3)) @ sp["R"].reshape(3, 3)
    y = (can[:, 1] - sp["bounds"].reshape(2, 3)[0, 1]) / 0.005 / float(sp["out_sh"][1])  # in [0, 1] over the volume
    return torch.stack([y * (v.shape[3] - 1) for v in vols])


def _variant_volumes(s, name, fill=0.0):
    """(volumes with the variant's voxels dead, dead workgroups or None).  fill: what goes into channel 0 of the voxels that were
    not zero before (0: they are dead; TINY: active, with planes that round to zero); every other channel of them is zeroed."""
    vols = [v.clone() for v in s["vols"]]
    what = VARIANTS[name]
    dead_wg = None
    if what == "half":
        iy = _level_rows(s, s["lattice"]).reshape(4, 24, 64)
        order = torch.argsort(iy[0].mean(1))
        dead_wg = order[:12]
        for l, v in enumerate(vols):
            top = int(torch.floor(iy[l][dead_wg].max()).item()) + 2  # floor + 1 is the last row a dead workgroup touches (+ 1 of margin)
            v[:, :, :, :top + 1, :] = 0.0
    else:
        for l in what:
            nz = (vols[l] != 0).any(1, keepdim=True)
            vols[l].zero_()
            if fill != 0.0:
                vols[l][:, :1][nz] = fill
    return vols, dead_wg


def _decode(s, vols, pts, vd, precision, density_only=False):
    from neuralbody_amd import ops

    net = s["net"]
    with torch.no_grad():
        scene = net.make_scene(vols, s["sp"], None if precision == "f32" else precision)
        out = ops.decode_points(scene, net.packed_weights(precision), None if density_only else s["lb"], pts,
                                None if density_only else vd, density_only=density_only, precision=precision)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(VARIANTS))
def test_dead_chunks_against_the_fp32_kernel(small, name):
    """Dead chunks leading (finest level zero), trailing (coarsest), interleaved (levels 1 and 3), a voxel list without any live
    chunk (half of the workgroups), none, and a long list marched in passes (the 5 mm lines) with its finest level dead: raw and
    density against the exact-fp32 kernel on the same volumes."""
    s = small
    vols, dead_wg = _variant_volumes(s, name)
    pts = s["lines"] if name == "long" else s["lattice"]
    vd = s["vd"][:pts.shape[0]].contiguous()
    ref = _decode(s, vols, pts, vd, "f32")
    got = _decode(s, vols, pts, vd, "f16f6")
    dref = _decode(s, vols, pts, vd, "f32", density_only=True)
    dgot = _decode(s, vols, pts, vd, "f16f6", density_only=True)
    live = torch.ones(pts.shape[0], dtype=torch.bool, device=DEV)
    clear = live  # the points whose outputs must not be degenerate
    if dead_wg is not None:
        live.view(24, 64)[dead_wg] = False
        iy0 = _level_rows(s, pts)[0]
        clear = iy0 > iy0[~live].max() + 4.0  # their finest level is untouched
        assert float(clear.float().mean()) > 0.25
        # a workgroup without a live chunk decodes the biases alone: what the all-zero volumes decode to, bit for bit, and one
        # density for every point
        zeros = [torch.zeros_like(v) for v in vols]
        bias_only = _decode(s, zeros, pts, vd, "f16f6")
        assert np.array_equal(got[~live].cpu().numpy(), bias_only[~live].cpu().numpy())
        dd = dgot.reshape(-1)[~live]
        assert bool((dd == dd[0]).all()) and bool((dref.reshape(-1)[~live] == dref.reshape(-1)[~live][0]).all())
    rl = ref[clear]
    assert float(rl.abs().max()) > 5 and float((rl[:, 3] != rl[0, 3]).float().mean()) > 0.9, "degenerate points"
    e_raw = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
    e_den = float(((dgot - dref).abs() / dref.abs().clamp_min(1.0)).max())
    print("%s: raw %.3e, density %.3e (tolerance %.1e)" % (name, e_raw, e_den, TOL))
    H.assert_close(got.cpu().numpy(), ref.cpu().numpy(), TOL, "raw %s" % name)
    H.assert_close(dgot.cpu().numpy(), dref.cpu().numpy(), TOL, "density %s" % name)


@pytest.mark.parametrize("name", ["finest", "interleaved"])
def test_skipped_chunks_equal_multiplied_zero_rows_to_the_bit(small, name):
    """The same voxels dead (their chunks are skipped) and active with planes that are zero (their chunks are fetched and
    multiplied): the decoder output is the same to the bit."""
    s = small
    net = s["net"]
    pts, vd = s["lattice"], s["vd"]
    dead, _ = _variant_volumes(s, name)
    tiny, _ = _variant_volumes(s, name, fill=TINY)
    skip = _decode(s, dead, pts, vd, "f16f6")
    dskip = _decode(s, dead, pts, vd, "f16f6", density_only=True)
    mult = _decode(s, tiny, pts, vd, "f16f6")
    # the planes of the run that multiplies: the levels' voxels are active rows, and every one of those rows is zero
    vols_cl, sparse, w, fold = net._foreign_fold
    urows = fold[1][0].view(torch.float16).float()
    for l in VARIANTS[name]:
        n = int(sparse[l][2])
        assert n == int((s["vols"][l] != 0).any(1).sum()) and n > 0, (l, n)  # (the planes of the run that skips have no such row)
        rows = urows[fold[0].row_base[l]:fold[0].row_base[l] + n]
        assert float(rows.abs().max()) == 0.0, "level %d: %g does not vanish in the planes" % (l, TINY)
    dmult = _decode(s, tiny, pts, vd, "f16f6", density_only=True)
    assert float(skip.abs().max()) > 5 and float((skip[:, 3] != skip[0, 3]).float().mean()) > 0.9, "degenerate points"
    assert np.array_equal(skip.cpu().numpy(), mult.cpu().numpy())
    assert np.array_equal(dskip.cpu().numpy(), dmult.cpu().numpy())


def test_culled_march_against_the_oracle():
    """One 64 x 64 view of the small scene through RendererMmsk (four silhouettes): the culled instance of the march, depth steps
    without a surviving sample and the sequential list preparation behind them, against the oracle's masked renderer at the
    tolerances of test_mask_culled_renderers_match_reference."""
    from neuralbody_amd.renderer import RenderConfig, RendererMmsk
    from oracle import neuralbody_oracle as orc

    r = scenes.SCENES["small"]
    sd = syn.make_weights(r["weights_seed"], num_train_frame=r["num_train_frame"])
    body = syn.make_body(**r["body"])
    Hh = Ww = 64
    K, R, T = syn.make_camera(body, Hh, Ww, focal_factor=r["cam"]["focal_factor"], distance=r["cam"]["distance"])
    ray_o, ray_d, near, far, mask = syn.host_image_rays(Hh, Ww, K, R, T, body["can_bounds"])
    batch = syn.make_batch(body, ray_o, ray_d, near, far, mask, latent_index=r["latent_index"])
    msks, Ks, RT = syn.make_view_masks(body, Hh, Ww, n_views=4, focal_factor=1.8, distance=1.6, dilate=1)
    batch.update(msks=msks[None], Ks=Ks[None], RT=RT[None])
    net = H.make_network(sd, DEV, True, precision="f16f6")
    rend = RendererMmsk(net, RenderConfig(N_samples=r["n_samples"], perturb=0.0, raw_noise_std=0.0, white_bkgd=False))
    with torch.no_grad():
        out = rend.render(H.device_batch(batch, DEV))
        ref = orc.render_masked(orc.tensor_state_dict(sd), batch, Hh, Ww, "mmsk", n_samples=r["n_samples"], training=True)
    torch.cuda.synchronize()
    inside = ref["inside"].numpy().reshape(out["weights"].shape)
    frac = float(inside.mean())
    assert 0.05 < frac < 0.95, "the silhouettes should cull a part of the samples (inside fraction %.2f)" % frac
    assert float(ref["acc_map"].max()) > 0.5, "degenerate view"
    err = H.assert_close(out["rgb_map"].cpu().numpy(), ref["rgb_map"].numpy(), H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), ref["acc_map"].numpy(), 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), ref["weights"].numpy(), 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), ref["depth_map"].numpy(), 2e-4, "depth_map")
    assert float(out["weights"].cpu().numpy()[~inside].max(initial=0.0)) == 0.0
    print("mmsk 64 x 64: rgb L-inf vs oracle %.2e, inside fraction %.2f" % (err, frac))
