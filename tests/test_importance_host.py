"""Hierarchical sampling, the part that needs no GPU: the acceptance rule of tests/importance_cases.py admits an fp32 restatement
of the inversion (torch.searchsorted(right=True)) in two arithmetics with nothing rejected, rejects depths that are wrong, and the
new entry points are wired through the header, the ctypes table, the config and the renderer's refusals."""
import os

import numpy as np
import pytest
import torch

from tests import importance_cases as ic

N_RAYS, S, N_IMP = 192, 64, 64


def _inputs(kinds):
    """192 rays, S = 64: near 3.5..4.5, far - near 0.3..0.6; weights of the named kinds only (composited peaky densities, or the
    dyadic lattice with 70 % zeros)."""
    _o, _d, near, far = ic.make_rays(N_RAYS, seed=11)
    z = ic.coarse_depths_f32(near, far, S)
    pool = {k: ic.make_weights(N_RAYS * 6, S, seed=5)[ic.KINDS.index(k)::6][:N_RAYS] for k in kinds}
    w = np.stack([pool[kinds[r % len(kinds)]][r] for r in range(N_RAYS)])
    return ic.bins_f32(z), w


@pytest.mark.parametrize("arithmetic", ["sequential", "rounded_once"])
@pytest.mark.parametrize("u_mode", ["det", "rand"])
@pytest.mark.parametrize("kinds", [("peaky",), ("lattice",), ic.KINDS])
def test_the_rule_admits_an_fp32_restatement_in_both_arithmetics(kinds, u_mode, arithmetic):
    bins, w = _inputs(kinds)
    u = ic.make_u(N_RAYS, N_IMP, u_mode, seed=3)
    z = ic.sample_pdf_f32(bins, w, u, arithmetic)
    ok = ic.accept(z, u, bins, w)
    pdf, _ = ic.knots_f64(w)
    # the CDF-domain error, printed beside the rule's 2 tau (the rule adds the depth-rounding term of a narrow heavy bin to it)
    err = ic.cdf_error(z, u, bins, w)
    print("%s / %s / %s: %d of %d rejected, worst CDF-domain error %.3g (2 tau = %.3g), smallest pdf %.3g" % (
        "+".join(kinds), u_mode, arithmetic, int((~ok).sum()), ok.size, float(err.max()), 2 * ic.TAU, float(pdf.min())))
    assert ok.all(), "%d of %d samples rejected" % (int((~ok).sum()), ok.size)


def test_the_rule_rejects_wrong_depths():
    """The rule is not vacuous: a depth moved by a hundredth of its bin where the pdf is large, a depth of the neighbouring ray and a
    depth outside the bins are all rejected."""
    bins, w = _inputs(("peaky",))
    u = ic.make_u(N_RAYS, N_IMP, "rand", seed=4)
    z = ic.sample_pdf_f32(bins, w, u, "sequential")
    pdf, c = ic.knots_f64(w)
    assert ic.accept(z, u, bins, w).all()
    # entries whose bin holds a pdf above 0.01: a hundredth of a bin is 1e-4 in the CDF domain, more than 2 tau
    k = np.stack([np.clip(np.searchsorted(c[r], u[r], side="right") - 1, 0, pdf.shape[1] - 1) for r in range(N_RAYS)])
    heavy = np.take_along_axis(pdf, k, 1) > 0.01
    width = np.take_along_axis(np.diff(bins.astype(np.float64), axis=1), k, 1)
    assert heavy.sum() > 1000
    moved = (z + 0.01 * width).astype(np.float32)
    assert not ic.accept(moved, u, bins, w)[heavy].any()
    assert (~ic.accept(np.roll(z, 1, axis=0), u, bins, w)).mean() > 0.9
    assert not ic.accept(z + np.float32(1.0), u, bins, w).any()


def test_the_float64_model_inverts_its_own_cdf():
    """The model itself: float64 depths from the float64 knots reproduce u through the piecewise-linear CDF to 1e-12."""
    bins, w = _inputs(("peaky",))
    pdf, c = ic.knots_f64(w)
    u = np.linspace(0.0, 1.0, 33)[None].repeat(N_RAYS, 0)
    b = bins.astype(np.float64)
    z = np.stack([np.interp(u[r], c[r], b[r]) for r in range(N_RAYS)])
    back = np.stack([np.interp(z[r], b[r], c[r]) for r in range(N_RAYS)])
    assert np.abs(back - u).max() < 1e-12 and abs(float(c[:, -1].max()) - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ wiring
def test_the_entry_points_are_declared_and_bound():
    from neuralbody_amd import _lib, ops

    declared = _lib.header_functions()
    for name in ("nb_importance_sample", "nb_importance_merge"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nb_importance_sample"][1]) == 21 and len(_lib.SIGNATURES["nb_importance_merge"][1]) == 11
    assert callable(ops.importance_sample) and callable(ops.importance_merge)
    assert (ops.IMPORTANCE_MAX, ops.MERGED_MAX) == (128, 512)
    assert _lib.ABI_VERSION == 20
    with open(_lib.HEADER) as f:
        assert "#define NB_ABI_VERSION 20\n" in f.read()
    src = os.path.join(os.path.dirname(_lib.HEADER), "..", "neuralbody_amd", "csrc", "nb_importance.hip")
    assert os.path.exists(src)


def test_the_config_key_defaults_to_off():
    from neuralbody_amd.renderer import RenderConfig

    assert RenderConfig().N_importance == 0 and RenderConfig(N_importance=32).N_importance == 32


def test_the_plugin_reads_the_yaml_key():
    import types

    from tests import helpers as H

    base = dict(N_samples=64, perturb=0.0, raw_noise_std=0.0, white_bkgd=False, H=512, W=512, ratio=1.0)
    mod = H.load_plugin("if_clight_renderer.py", types.SimpleNamespace(**base))
    assert mod._LiveCfg().N_importance == 0
    mod = H.load_plugin("if_clight_renderer.py", types.SimpleNamespace(N_importance=48, **base))
    assert mod._LiveCfg().N_importance == 48


def _renderer(**cfg):
    from neuralbody_amd.network import Network
    from neuralbody_amd.renderer import RenderConfig, Renderer

    return Renderer(Network(num_train_frame=3), RenderConfig(N_samples=8, perturb=0.0, **cfg))


def _batch(n=64):
    z = lambda *sh: torch.zeros(*sh)  # noqa: E731
    return {"ray_o": z(1, n, 3), "ray_d": torch.ones(1, n, 3), "near": z(1, n), "far": torch.ones(1, n),
            "coord": torch.zeros(1, 10, 3, dtype=torch.int32), "out_sh": torch.tensor([[32, 32, 32]], dtype=torch.int32),
            "bounds": z(1, 2, 3), "R": torch.eye(3)[None], "Th": z(1, 1, 3), "latent_index": torch.zeros(1, dtype=torch.long)}


def test_the_three_refusals_raise_before_any_device_work():
    """n_importance > 0 with the differentiable path, with field normals and with raw_noise_std != 0: NotImplementedError, each with its
    reason; the cfg key counts like the argument."""
    r = _renderer()
    assert torch.is_grad_enabled() and any(p.requires_grad for p in r.net.parameters())
    with pytest.raises(NotImplementedError, match="inference-only"):
        r.render(_batch(), n_importance=16)
    with pytest.raises(NotImplementedError, match="inference-only"):
        _renderer(N_importance=16).render(_batch())
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="field normals"):
            r.render(_batch(), n_importance=16, normals=True)
        with pytest.raises(NotImplementedError, match="field normals"):
            _renderer(render_normals=True).render(_batch(), n_importance=16)
        with pytest.raises(NotImplementedError, match="raw_noise_std"):
            _renderer(raw_noise_std=0.5).render(_batch(), n_importance=16)
        with pytest.raises(ValueError, match="n_importance"):
            r.render(_batch(), n_importance=-1)
