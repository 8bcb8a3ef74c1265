"""Writes tests/golden/nerf_train_step.npz: one TRAINING step of the UNMODIFIED reference's vanilla-NeRF baseline
(lib/train/trainers/nerf.py's NetworkWrapper over lib/networks/renderer/volume_renderer.py and lib/networks/nerf.py,
configs/nerf/nerf_313.yaml with perturb 1) in train mode on the 96 rays of tests/golden/nerf_baseline.npz, on CPU in fp32.

    python tests/golden/make_golden_nerf_train.py   (where the reference tree is present; a fresh process: the harness loads once)

The two draws of torch.rand the step makes (the stratified jitter's t_rand [96,64], volume_renderer.py:62, and sample_pdf's u
[96,128], nerf_net_utils.py:70) are fixed and stored, as is the target image.  The fixture is data only: those inputs, the depths of
both passes (recovered from the points the network saw), the three losses, the two colour maps, and of each of the 48 gradients
its L2 norm, a few probe entries and its distance to the float64 restatement tests/nerf_train_ref.py (max |diff| / max |ref|, the
reference's own fp32 error), which is asserted to lie inside the gradient budget.  The weights are tests/nerf_ref.py's recipe."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import nerf_ref, nerf_train_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nerf_train_step.npz")
N_PROBES = 4


def main():
    tss = types.ModuleType("torchsearchsorted")  # nerf_net_utils.py:56 imports an extension that torch has since absorbed
    tss.searchsorted = lambda cdf, u, side="left": torch.searchsorted(cdf, u, right=(side == "right"))
    sys.modules["torchsearchsorted"] = tss
    ns = ref_harness.load(cfg_file="configs/nerf/nerf_313.yaml", opts=("perturb", "1"))
    cfg = ns.cfg
    assert (cfg.N_samples, cfg.N_importance, float(cfg.perturb), bool(cfg.lindisp), float(cfg.raw_noise_std)) == (64, 128, 1.0, False, 0.0)
    assert cfg.trainer_path == "lib/train/trainers/nerf.py"
    cwd = os.getcwd()
    os.chdir(ns.root)
    try:
        import importlib

        importlib.import_module("lib.train.trainers.make_trainer")
        mt = sys.modules["lib.train.trainers.make_trainer"]  # the package re-exports a function under the module's name
        net = ns.make_network(cfg)
        wrapper = mt._wrapper_factory(cfg, net)
    finally:
        os.chdir(cwd)
    base = np.load(os.path.join(HERE, "nerf_baseline.npz"))
    sd = nerf_ref.make_state_dict(base["alpha_shift"])
    assert nerf_ref.checksum(sd) == str(base["weights_sha256"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    wrapper.train()
    assert net.training

    o, d, near, far = nerf_ref.fixture_rays()
    n = o.shape[0]
    rs = np.random.RandomState(11)
    t_rand = rs.uniform(0.0, 1.0, (n, 64)).astype(np.float32)
    u = rs.uniform(0.0, 1.0, (n, 128)).astype(np.float32)
    u[u >= 1.0], t_rand[t_rand >= 1.0] = np.float32(0.5), np.float32(0.5)  # [0, 1) after the rounding to fp32
    rgb = rs.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    mask = rs.uniform(0.0, 1.0, n) < 0.8
    mask[:2] = (False, True)

    calls = []
    inner = net.forward

    def spy(pts, viewdirs, model=""):
        raw = inner(pts, viewdirs, model=model)
        calls.append((model, pts.detach().numpy().copy(), viewdirs.detach().numpy().copy(), raw.detach().numpy().copy()))
        return raw

    net.forward = spy
    draws = [t_rand, u]
    real_rand = torch.rand

    def fixed_rand(*shape, **kw):
        want = draws.pop(0)
        got = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        assert got == want.shape, (got, want.shape)
        return torch.from_numpy(want.copy())

    batch = {"ray_o": torch.from_numpy(o)[None], "ray_d": torch.from_numpy(d)[None], "near": torch.from_numpy(near)[None],
             "far": torch.from_numpy(far)[None], "rgb": torch.from_numpy(rgb)[None], "mask_at_box": torch.from_numpy(mask)[None]}
    torch.rand = fixed_rand
    try:
        ret, loss, stats, _ = wrapper(batch)
    finally:
        torch.rand = real_rand
    assert not draws and [c[0] for c in calls] == ["", "fine"]
    loss.backward()
    grads = {k: p.grad.detach().numpy().astype(np.float64) for k, p in net.named_parameters()}
    assert list(grads) == list(nerf_ref.state_dict_shapes()) and len(grads) == 48

    # the depths of the two passes: the jitter's restatement must give the very points the coarse module saw, the fine depths are
    # redone through the reference's own functions with the same u (as make_golden_nerf.py does)
    z_coarse = nerf_train_ref.jitter_f32(nerf_ref.coarse_depths_f32(near, far, 64), t_rand)
    assert np.array_equal(calls[0][1], nerf_ref.points_f32(o, d, z_coarse)), "jitter_f32 restates volume_renderer.py:56-70 bit for bit"
    assert np.all(np.diff(z_coarse, axis=-1) >= 0) and np.all(z_coarse >= near[:, None]) and np.all(z_coarse <= far[:, None])
    from lib.networks.renderer.nerf_net_utils import raw2outputs, sample_pdf

    draws.append(u)
    torch.rand = fixed_rand
    try:
        with torch.no_grad():
            zc = torch.from_numpy(z_coarse)
            weights = raw2outputs(torch.from_numpy(calls[0][3]), zc, torch.from_numpy(d), 0, False)[3]
            z_samples = sample_pdf(.5 * (zc[..., 1:] + zc[..., :-1]), weights[..., 1:-1], 128, det=False)
            z_fine = torch.sort(torch.cat([zc, z_samples], -1), -1)[0].numpy()
    finally:
        torch.rand = real_rand
    assert np.array_equal(calls[1][1], nerf_ref.points_f32(o, d, z_fine)), "fine depths reproduce the points the network saw"

    # the float64 restatement at the reference's own depths and (fp32-normalised) directions
    want = nerf_train_ref.train_step(sd, o, d, z_coarse, z_fine, rgb, mask, viewdirs=calls[0][2])
    out = {"t_rand": t_rand, "u": u, "rgb": rgb, "mask_at_box": mask, "z_coarse": z_coarse, "z_fine": z_fine,
           "viewdirs": calls[0][2], "loss": np.float64(float(loss.detach())), "img_loss": np.float64(float(stats["img_loss"].detach())),
           "img_loss0": np.float64(float(stats["img_loss0"].detach())), "ref_rgb_map": ret["rgb_map"].detach().numpy()[0],
           "ref_rgb0": ret["rgb0"].detach().numpy()[0]}
    for key in ("loss", "img_loss", "img_loss0"):
        out["ref_err_" + key] = np.float64(abs(float(out[key]) - want[key]))
        assert out["ref_err_" + key] <= 1e-6, (key, out[key], want[key])
    worst = 0.0
    prs = np.random.RandomState(12)
    for name, g in grads.items():
        e = nerf_train_ref.rel_err(g, want["grads"][name])
        worst = max(worst, e)
        idx = np.sort(prs.choice(g.size, min(N_PROBES, g.size), replace=False))
        out["norm/" + name] = np.float64(np.sqrt((g ** 2).sum()))
        out["probe_idx/" + name] = idx.astype(np.int64)
        out["probe/" + name] = g.reshape(-1)[idx]
        out["ref_err/" + name] = np.float64(e)
        assert np.isfinite(g).all() and out["norm/" + name] > 0, name
    out["ref_err_worst"] = np.float64(worst)
    print("loss %.6f (img %.6f, img0 %.6f); reference fp32 against float64: loss %.2e, worst gradient %.3e (budget %.0e)"
          % (out["loss"], out["img_loss"], out["img_loss0"], out["ref_err_loss"], worst, nerf_train_ref.GRAD_TOL))
    assert worst <= nerf_train_ref.GRAD_TOL, "the reference's own fp32 gradients miss the budget against float64"
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
