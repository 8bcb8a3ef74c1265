"""Training losses on acc_map and weights, the part that needs no GPU: the float64 model of the distortion loss
(tests/ray_loss_ref.py) holds its own gradient and invariants, the trainer plugin refuses a mask loss without occupancy before any
device work and leaves the default step's statements alone, and the dataset option is off by default."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import ray_loss_ref as rl


def load_trainer_plugin(**keys):
    """plugins/if_nerf_clight.py imported against a stand-in for the reference's lib.config.cfg -> (module, cfg namespace)."""
    cfgmod = types.ModuleType("lib.config")
    cfgmod.cfg = types.SimpleNamespace(N_samples=64, perturb=1.0, raw_noise_std=0.0, white_bkgd=False, H=512, W=512, ratio=1.0, **keys)
    # (the renderer plugin the trainer imports binds to the stand-in too: it must not stay behind for whoever imports it next)
    saved = {k: sys.modules.get(k) for k in ("lib", "lib.config", "neuralbody_amd.plugins.if_clight_renderer")}
    sys.modules.pop("neuralbody_amd.plugins.if_clight_renderer", None)
    sys.modules["lib"] = types.ModuleType("lib")
    sys.modules["lib.config"] = cfgmod
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("nb_plugin_trainer_losses", os.path.join(root, "neuralbody_amd", "plugins", "if_nerf_clight.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod, cfgmod.cfg


def _cases(seed=0, n=7, S=33):
    rs = np.random.RandomState(seed)
    w = rs.uniform(0, 1, (n, S))
    w[1] = 0.0
    z = np.sort(rs.uniform(2.0, 3.5, (n, S)), axis=1)
    z[2, 5:9] = z[2, 5]  # a run of equal neighbours
    return w, z


def test_gradient_of_the_model_is_the_autograd_gradient_of_its_loss():
    w, z = _cases()
    L, G = rl.distortion_ref(w, z)
    wt = torch.from_numpy(w).requires_grad_(True)
    Lt = rl.distortion_loss_torch(wt, z)
    Lt.sum().backward()
    assert np.abs(Lt.detach().numpy() - L).max() <= 1e-12
    assert np.abs(wt.grad.numpy() - G).max() <= 1e-12
    assert np.abs(G).max() > 0.1


def test_loss_is_not_negative():
    for seed in range(4):
        w, z = _cases(seed)
        L, _ = rl.distortion_ref(w, z)
        assert (L >= 0).all() and L[1] == 0.0 and L.max() > 0


def test_one_hot_weights_give_a_third_of_the_interval():
    _, z = _cases(3)
    n, S = z.shape
    _, delta, _ = rl.intervals(z)
    for k in (0, S // 2, S - 2, S - 1):
        w = np.zeros((n, S))
        w[:, k] = 1.0
        L, G = rl.distortion_ref(w, z)
        assert np.abs(L - delta[:, k] / 3).max() <= 1e-15
    assert (rl.distortion_ref(w, z)[0] == 0).all()  # the last sample is a point: delta = 0


def test_loss_ignores_a_shift_and_a_positive_scale_of_the_depths():
    w, z = _cases(5)
    L, G = rl.distortion_ref(w, z)
    for shift, scale in ((1.25, 1.0), (0.0, 3.0), (-0.5, 0.125)):
        L2, G2 = rl.distortion_ref(w, (z + shift) * scale)
        assert np.abs(L2 - L).max() <= 1e-12 * max(1.0, L.max()) and np.abs(G2 - G).max() <= 1e-12 * G.max()


def test_zero_span_gives_zeros():
    w, z = _cases(6)
    z[:] = z[:, :1]
    L, G = rl.distortion_ref(w, z)
    assert (L == 0).all() and (G == 0).all()
    L, G = rl.distortion_ref(w[:, :1], z[:, :1])  # one sample
    assert (L == 0).all() and (G == 0).all()


def _cpu_batch(n=6):
    return {"ray_o": torch.zeros(1, n, 3), "ray_d": torch.ones(1, n, 3), "near": torch.ones(1, n), "far": torch.full((1, n), 2.0),
            "mask_at_box": torch.ones(1, n, dtype=torch.bool), "rgb": torch.zeros(1, n, 3)}


class _RaisingRenderer:
    def render(self, batch):
        raise AssertionError("render() was reached")


def test_mask_loss_without_occupancy_raises_before_any_device_work():
    mod, cfg = load_trainer_plugin(mask_loss_weight=1.0)
    wrapper = mod.NetworkWrapper(torch.nn.Linear(2, 2))
    wrapper.renderer = _RaisingRenderer()
    assert torch.is_grad_enabled()
    with pytest.raises(KeyError, match="train_ray_mask"):
        wrapper(_cpu_batch())


def test_default_step_touches_neither_the_distortion_kernel_nor_occupancy(monkeypatch):
    mod, cfg = load_trainer_plugin()
    n = 6

    class Batch(dict):
        def __getitem__(self, k):
            assert k != "occupancy", "the default step read batch['occupancy']"
            return dict.__getitem__(self, k)

        def __contains__(self, k):
            assert k != "occupancy", "the default step looked for batch['occupancy']"
            return dict.__contains__(self, k)

    class Stub:
        def render(self, batch):
            return {"rgb_map": torch.full((1, n, 3), 0.5, requires_grad=True), "acc_map": torch.zeros(1, n),
                    "weights": torch.zeros(1, n, 4), "z_vals": torch.zeros(1, n, 4)}

    def refuse(*a, **k):
        raise AssertionError("ops.ray_distortion was called")

    monkeypatch.setattr(mod.ops, "ray_distortion", refuse)
    wrapper = mod.NetworkWrapper(torch.nn.Linear(2, 2))
    wrapper.renderer = Stub()
    for keys in ({}, {"mask_loss_weight": 0, "distortion_loss_weight": 0.0}):
        for k, v in keys.items():
            setattr(cfg, k, v)
        ret, loss, stats, image_stats = wrapper(Batch(_cpu_batch(n)))
        assert set(stats) == {"img_loss", "loss"} and float(loss.detach()) == 0.25 and image_stats == {}
    # and the stand-in does catch the term when it is asked for
    cfg.distortion_loss_weight = 0.01
    with pytest.raises(AssertionError, match="ray_distortion"):
        wrapper(Batch(_cpu_batch(n)))


def test_ray_mask_is_off_by_default():
    from neuralbody_amd.train_rays import TrainDataConfig

    assert TrainDataConfig().ray_mask is False
    assert TrainDataConfig(ray_mask=True).ray_mask is True


def test_new_wrappers_refuse_cpu_tensors():
    from neuralbody_amd import ops
    from neuralbody_amd._lib import NbError

    w, z = torch.zeros(3, 4), torch.zeros(3, 4)
    with pytest.raises(NbError, match="HIP device"):
        ops.ray_distortion(w, z)
    with pytest.raises(NbError, match="HIP device"):
        ops.composite_bwd_maps(torch.zeros(3, 4, 4), z, torch.zeros(3, 3), False, d_acc_map=torch.zeros(3))
