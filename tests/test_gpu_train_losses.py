"""The training step with gradients through every map: the whole step against float64 autograd through the oracle for objectives
that read acc_map, depth_map and weights, the default step's launches, the trainer plugin's two opt-in losses and the dataset's
per-ray occupancy."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.golden import scenes
from tests.test_gpu_backward import ENC_TOL, _encoder_masks, _mlp_masks, _rel
from tests.test_ray_loss_host import load_trainer_plugin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USE = 96


def _small_dense_batch():
    r, sd, body, batch, cam, _ = scenes.build("small_dense")
    b_np = dict(batch)
    for k in ("ray_o", "ray_d", "near", "far"):
        b_np[k] = batch[k][:, :N_USE]
    return r, sd, b_np


@pytest.fixture(scope="module")
def step():
    """The recipe of test_full_training_step_gradients_match_autograd, once for the tests below: the HIP forward (its ReLU masks go
    to the reference) and the float64 oracle forward, both with their graphs kept."""
    from neuralbody_amd import training
    from oracle import neuralbody_oracle as orc

    r, sd, b_np = _small_dense_batch()
    net = H.make_network(sd, DEV, True, "f32")
    rend = H.make_renderer(net, dict(r, white_bkgd=True))
    training.DEBUG_CAPTURE = {}
    try:
        out = rend.render(H.device_batch(b_np, DEV))
        cap = training.DEBUG_CAPTURE
    finally:
        training.DEBUG_CAPTURE = None
    masks = {"encoder": _encoder_masks(cap["enc_ctx"]), "mlp": _mlp_masks(cap["tap"])}
    sdg = {}
    for k, v in orc.tensor_state_dict(sd).items():
        sdg[k] = v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v
    out_ref = orc.render(sdg, {k: (torch.from_numpy(v).double() if v.dtype == np.float32 else v) for k, v in b_np.items()},
                         n_samples=64, training=True, white_bkgd=True, relu_masks=masks)
    rs = np.random.RandomState(13)
    g = {k: torch.from_numpy(rs.standard_normal(tuple(out_ref[k].shape)).astype(np.float32))
         for k in ("rgb_map", "acc_map", "depth_map", "weights")}
    return dict(net=net, out=out, out_ref=out_ref, sdg=sdg, g=g)


def _compare(step, keys, what):
    """Gradients of sum_k sum(g_k . out_k) of every parameter, HIP against the float64 reference, under ENC_TOL."""
    net, out, out_ref, sdg, g = (step[k] for k in ("net", "out", "out_ref", "sdg", "g"))
    names = [n for n, _ in net.named_parameters()]
    ref = torch.autograd.grad(sum((out_ref[k] * g[k].double()).sum() for k in keys), [sdg[n] for n in names], retain_graph=True)
    got = torch.autograd.grad(sum((out[k] * g[k].to(DEV)).sum() for k in keys), [p for _, p in net.named_parameters()],
                              retain_graph=True)
    torch.cuda.synchronize()
    worst = {}
    colour = ("feature_fc", "latent_fc", "latent", "view_fc", "rgb_fc")  # behind alpha_fc's branch point: the densities never see them
    for name, a, b in zip(names, got, ref):
        assert a is not None and torch.isfinite(a).all(), name
        if "rgb_map" not in keys and name.split(".")[0] in colour:
            # acc_map, depth_map and weights are functions of the densities alone: the colour head's gradient IS zero, on both sides
            assert not b.any() and not a.any(), name
        else:
            assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0, name
        group = name.split(".")[0] if not name.startswith("xyzc_net") else ".".join(name.split(".")[:2])
        worst[group] = max(worst.get(group, 0.0), _rel(a.cpu().numpy(), b.numpy().reshape(a.shape), ENC_TOL, "grad " + name))
    print("%s: worst relative gradient error per group: %s" % (what, {k: "%.1e" % v for k, v in worst.items()}))
    print("%s: worst over all %d tensors %.2e" % (what, len(names), max(worst.values())))


def test_every_map_is_differentiable_and_the_inference_dict_is_unchanged(step):
    out = step["out"]
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map", "z_vals"}
    for k in ("rgb_map", "disp_map", "acc_map", "weights", "depth_map"):
        assert out[k].requires_grad, k
        got, ref = out[k].detach().cpu().numpy(), step["out_ref"][k].detach().numpy()
        if k == "disp_map":  # 1 / max(1e-10, 0 / 0) on a ray that met nothing: NaN on both sides
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            got, ref = got[~np.isnan(ref)], ref[~np.isnan(ref)]
        _rel(got, ref, 1e-4, "forward " + k)
    assert not out["z_vals"].requires_grad and out["z_vals"].shape == (1, N_USE, 64)
    r, sd, b_np = _small_dense_batch()
    net = H.make_network(sd, DEV, True, "f32")
    with torch.no_grad():
        inf = H.make_renderer(net, dict(r, white_bkgd=True)).render(H.device_batch(b_np, DEV))
    assert set(inf) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map"}


def test_whole_step_with_cotangents_on_four_maps_matches_autograd(step):
    """sum g_rgb . rgb + sum g_acc . acc + sum g_dep . depth + sum g_w . weights: every parameter's gradient within ENC_TOL of float64
    autograd through the whole oracle (same ReLU masks)."""
    _compare(step, ("rgb_map", "acc_map", "depth_map", "weights"), "four maps")


def test_whole_step_with_the_objective_on_acc_map_alone(step):
    """No d rgb arrives.  (On a renderer whose acc_map is marked non-differentiable there is no graph to differentiate.)"""
    assert step["out"]["acc_map"].requires_grad
    _compare(step, ("acc_map",), "acc_map alone")


def test_default_step_runs_the_launches_it_ran(monkeypatch):
    """An rgb-only loss never reaches nb_composite_bwd_maps or nb_ray_distortion, and z_vals are get_sampling_points' depths for the
    t_rand passed in, to the bit."""
    from neuralbody_amd import ops

    def refuse(*a, **k):
        raise AssertionError("the default step called a kernel of the new losses")

    calls = []
    real = ops.composite_bwd
    monkeypatch.setattr(ops, "composite_bwd_maps", refuse)
    monkeypatch.setattr(ops, "ray_distortion", refuse)
    monkeypatch.setattr(ops, "composite_bwd", lambda *a, **k: calls.append(1) or real(*a, **k))
    r, sd, b_np = _small_dense_batch()
    net = H.make_network(sd, DEV, True, "f32")
    rend = H.make_renderer(net, dict(r, perturb=True))
    bd = H.device_batch(b_np, DEV)
    t_rand = torch.rand((1, N_USE, r["n_samples"]), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    out = rend.render(bd, t_rand=t_rand)
    with torch.no_grad():
        _, z = rend.get_sampling_points(bd["ray_o"], bd["ray_d"], bd["near"], bd["far"], t_rand)
        _, z_plain = rend.get_sampling_points(bd["ray_o"], bd["ray_d"], bd["near"], bd["far"], torch.full_like(t_rand, 0.5))
    assert torch.equal(out["z_vals"], z) and not torch.equal(z, z_plain)
    (out["rgb_map"] ** 2).sum().backward()
    assert calls == [1]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def _trainer_setup():
    from tests import synthetic as syn

    sd = syn.make_weights(0, num_train_frame=5)
    body = syn.make_body(seed=0, box=(0.3, 0.5, 0.2))
    K, R, T = syn.make_camera(body, 64, 64, focal_factor=2.5, distance=1.5)
    ro, rd, near, far, mask = syn.host_image_rays(64, 64, K, R, T, body["can_bounds"])
    rs = np.random.RandomState(0)
    pick = rs.choice(ro.shape[0], 1024, replace=False)
    batch = syn.make_batch(body, ro[pick], rd[pick], near[pick], far[pick], np.ones(1024, bool), latent_index=2)
    batch["rgb"] = rs.uniform(0, 1, (1, 1024, 3)).astype(np.float32)
    bd = H.device_batch(batch, DEV)
    bd["occupancy"] = torch.from_numpy((rs.uniform(0, 1, (1, 1024)) < 0.5).astype(np.float32)).to(DEV)
    return sd, bd


def _wrapper(sd, raw_noise_std=0.0, **keys):
    from neuralbody_amd.renderer import RenderConfig

    mod, cfg = load_trainer_plugin(**keys)
    net = H.make_network(sd, DEV, True, "f32")
    wrapper = mod.NetworkWrapper(net)
    wrapper.renderer.cfg = RenderConfig(N_samples=64, perturb=1.0, raw_noise_std=raw_noise_std, white_bkgd=False)
    return net, wrapper


def _grads(net, wrapper, bd):
    torch.manual_seed(0)  # the same jitter for every step compared
    ret, loss, stats, _ = wrapper(bd)
    net.zero_grad()
    loss.mean().backward()
    return stats, {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def test_trainer_with_mask_and_distortion_losses():
    sd, bd = _trainer_setup()
    net0, plain = _wrapper(sd)
    stats0, g0 = _grads(net0, plain, bd)
    assert set(stats0) == {"img_loss", "loss"}
    mu, lam = 1.0, 0.01
    net, wrapper = _wrapper(sd, mask_loss_weight=mu, distortion_loss_weight=lam)
    stats, g = _grads(net, wrapper, bd)
    assert set(stats) == {"img_loss", "mask_loss", "distortion_loss", "loss"}
    want = stats["img_loss"] + mu * stats["mask_loss"] + lam * stats["distortion_loss"]
    assert torch.equal(stats["loss"].detach(), want.detach())
    assert float(stats["mask_loss"].detach()) > 0 and float(stats["distortion_loss"].detach()) > 0
    # acc_map and weights are functions of the densities alone, so the two terms reach every parameter in front of alpha_fc (trunk,
    # encoder, vertex codes) and none of the colour head (feature_fc, latent_fc, latent, view_fc, rgb_fc), whose gradient stays the
    # image loss's.  "Differs" is held to 1e-4 of the tensor's largest entry: two runs of the SAME step differ by the ~1e-6 of their
    # atomics' summation order, and a mask loss of weight 1 moves the density path as much as the image loss does
    colour = ("feature_fc", "latent_fc", "latent", "view_fc", "rgb_fc")
    moved = {}
    for name in g:
        assert torch.isfinite(g[name]).all(), name
        moved[name] = float((g[name] - g0[name]).abs().max()) / max(float(g0[name].abs().max()), 1e-30)
        if name.split(".")[0] not in colour:
            assert moved[name] > 1e-4, "%s: the gradient is the rgb-only step's (relative difference %.2e)" % (name, moved[name])
    print("least moved density-path gradient %.2e, most moved colour-head gradient %.2e" % (
        min(v for k, v in moved.items() if k.split(".")[0] not in colour), max(v for k, v in moved.items() if k.split(".")[0] in colour)))
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    for it in range(3):
        ret, loss, st, _ = wrapper(bd)
        opt.zero_grad()
        loss.mean().backward()
        torch.nn.utils.clip_grad_value_(net.parameters(), 40)
        opt.step()
        assert np.isfinite(float(loss))
    # under no_grad (validation) the loss is the reference's: the inference dict has no z_vals, a test item no occupancy
    with torch.no_grad():
        ret, loss, st, _ = wrapper({k: v for k, v in bd.items() if k != "occupancy"})
    assert set(st) == {"img_loss", "loss"} and set(ret) == {"rgb_map", "disp_map", "acc_map", "weights", "depth_map"}


@pytest.mark.parametrize("variant", ("raw_noise", "two_frames"))
def test_trainer_losses_with_raw_noise_and_with_a_batch_of_two_frames(variant):
    sd, bd = _trainer_setup()
    net, wrapper = _wrapper(sd, raw_noise_std=0.5 if variant == "raw_noise" else 0.0, mask_loss_weight=1.0, distortion_loss_weight=0.01)
    if variant == "two_frames":
        bd = {k: (torch.cat([v, v], 0) if isinstance(v, torch.Tensor) and v.dim() >= 1 else v) for k, v in bd.items()}
    stats, g = _grads(net, wrapper, bd)
    assert set(stats) == {"img_loss", "mask_loss", "distortion_loss", "loss"}
    for name, gr in g.items():
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0, name


@pytest.mark.parametrize("mode", ("h36m", "plain"))
def test_dataset_occupancy(mode):
    from neuralbody_amd.train_rays import TrainDataConfig, TrainRayDataset, ray_occupancy
    from tests.test_gpu_train_rays import _G, _case_a_source

    ds = TrainRayDataset(_case_a_source(), TrainDataConfig(N_rand=96, ray_mask=True, mode=mode), device=DEV)
    item = ds[0]
    pixel = ds.last_sample["pixel"].cpu().numpy()
    msk = np.asarray(_G["A/msk"])
    filled = (pixel >= 0).all(1)
    m = msk[np.maximum(pixel[:, 0], 0), np.maximum(pixel[:, 1], 0)]
    want = (((m == 1) if mode == "h36m" else (m != 0)) & filled).astype(np.float32)
    occ = item["occupancy"]
    assert occ.dtype == torch.float32 and occ.shape == (96,) and occ.is_cuda
    assert np.array_equal(occ.cpu().numpy(), want) and 0 < want.sum() < 96
    assert set(np.unique(msk)) >= {0, 1} and (mode == "plain" or not (want != 0)[m == 100].any())
    # rows the sampler left unfilled carry pixel (-1, -1): occupancy 0
    px = torch.tensor([[-1, -1], [int(pixel[0, 0]), int(pixel[0, 1])], [-1, -1]], dtype=torch.int32, device=DEV)
    assert ray_occupancy(ds._items[0]["msk"], px, mode).tolist() == [0.0, float(want[0]), 0.0]
    # without the key the item is what it was
    plain = TrainRayDataset(_case_a_source(), TrainDataConfig(N_rand=96, mode=mode), device=DEV)[0]
    assert set(item) == set(plain) | {"occupancy"} and "occupancy" not in plain
