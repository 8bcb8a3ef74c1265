"""Host-side checks of the evaluator (no GPU): the numpy restatement tests/metrics_ref.py against the fixture that the
reference's own Evaluator.evaluate produced (tests/golden/eval_metrics.npz, made by tests/golden/make_golden_eval.py), the
ABI surface of the two new entry points, and the evaluator_path plugin."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_TOL = 1e-11  # two fp64 summation orders of the same windows differ by <= 1.8e-13
MSE_RTOL = 1e-6  # the reference sums fp32 pairwise: log2(n) * 2^-24


def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))


def fixture_case(g, name):
    white, whole = (int(v) for v in g[name + "/flags"])
    return dict(mask=g[name + "/mask"], rgb_pred=g[name + "/rgb_pred"], rgb_gt=g[name + "/rgb_gt"], white_bkgd=white,
                whole_img=whole, box=tuple(int(v) for v in g[name + "/box"]), metrics=g[name + "/metrics"])


CASES = [str(n) for n in fixture()["names"]]


def test_fixture_covers_the_cases_the_protocol_needs():
    g = fixture()
    c = {n: fixture_case(g, n) for n in CASES}
    assert {v["white_bkgd"] for v in c.values()} == {0, 1}
    assert any(v["whole_img"] for v in c.values())
    assert any(v["box"][0] == 0 and v["box"][1] == 0 and not v["whole_img"] for v in c.values())  # touches two borders
    assert any(v["box"][2] == 7 for v in c.values())  # one column of windows
    assert all(max(v["mask"].shape) <= 128 for v in c.values())
    ident = c["identical"]
    assert ident["metrics"][0] == 0.0 and ident["metrics"][1] == math.inf and ident["metrics"][2] == 1.0
    holes = c["holes_two_components"]
    x, y, w, h = holes["box"]
    assert not holes["mask"][y:y + h, x:x + w].all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    c = fixture_case(fixture(), name)
    got = mr.metrics(c["mask"], c["rgb_pred"], c["rgb_gt"], c["white_bkgd"], c["whole_img"])
    mse, psnr, ssim = (float(v) for v in c["metrics"])
    print("%s: ssim err %.3e, mse rel err %.3e" % (name, abs(got["ssim"] - ssim), abs(got["mse"] - mse) / max(mse, 1e-300)))
    assert got["box"] == c["box"]
    assert got["n_windows"] == (c["box"][2] - 6) * (c["box"][3] - 6)
    if name == "identical":  # exact, not by tolerance
        assert got["mse"] == 0.0 and got["psnr"] == math.inf and got["ssim"] == 1.0
        return
    assert abs(got["ssim"] - ssim) <= SSIM_TOL
    assert abs(got["mse"] - mse) <= MSE_RTOL * mse
    assert abs(got["psnr"] - psnr) <= 10.0 / math.log(10.0) * 2.0 * MSE_RTOL


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_uniform_filter_form(name):
    ndi = pytest.importorskip("scipy.ndimage")
    c = fixture_case(fixture(), name)
    x, y, w, h = c["box"]
    imgs = [mr.scatter(c["mask"], c[k], c["white_bkgd"])[y:y + h, x:x + w] for k in ("rgb_pred", "rgb_gt")]
    n = 49.0
    cov, c1, c2 = n / (n - 1.0), (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    per_channel = []
    for ch in range(3):
        a, b = imgs[0][..., ch], imgs[1][..., ch]
        ux, uy = ndi.uniform_filter(a, size=7), ndi.uniform_filter(b, size=7)
        uxx, uyy, uxy = ndi.uniform_filter(a * a, size=7), ndi.uniform_filter(b * b, size=7), ndi.uniform_filter(a * b, size=7)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        per_channel.append(s[3:-3, 3:-3].mean())
    assert abs(mr.ssim(*imgs) - float(np.mean(per_channel))) <= SSIM_TOL


def test_restatement_degenerate_crops():
    mask = np.zeros((20, 20), bool)
    mask[3:9, 2:15] = True  # 6 high: compare_ssim raises
    rgb = np.full((int(mask.sum()), 3), 0.5, np.float32)
    got = mr.metrics(mask, rgb, rgb)
    assert math.isnan(got["ssim"]) and got["n_windows"] == 0 and got["box"] == (2, 3, 13, 6)
    with pytest.raises(ValueError):
        mr.ssim(np.zeros((6, 13, 3)), np.zeros((6, 13, 3)))
    empty = mr.metrics(np.zeros((20, 20), bool), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert empty["box"] == (0, 0, 0, 0) and math.isnan(empty["ssim"]) and math.isnan(empty["mse"])


def test_header_and_signatures_name_the_new_entries():
    from neuralbody_amd import _lib

    names = _lib.header_functions()
    for fn in ("nb_eval_metrics", "nb_eval_metrics_scratch_size"):
        assert fn in names and fn in _lib.SIGNATURES, fn
    res, args = _lib.SIGNATURES["nb_eval_metrics"]
    assert len(args) == 11  # mask, H, W, pred, gt, n_rays, white_bkgd, whole_img, out, scratch, stream
    assert _lib.ABI_VERSION == 20  # purely additive


def test_data_range_quirk_is_one_named_constant():
    with open(os.path.join(ROOT, "neuralbody_amd", "csrc", "nb_metrics.hip")) as f:
        src = f.read()
    assert "SSIM_DATA_RANGE = 2.0" in src


def _cfg(tmp_path, **kw):
    from neuralbody_amd.evaluator import EvalConfig

    return EvalConfig(H=16, W=16, result_dir=str(tmp_path), **kw)


def test_evaluator_refuses_a_host_rgb_map(tmp_path):
    from neuralbody_amd._lib import NbError
    from neuralbody_amd.evaluator import Evaluator

    ev = Evaluator(_cfg(tmp_path))
    mask = torch.ones(1, 256, dtype=torch.bool)
    batch = {"rgb": torch.zeros(1, 256, 3), "mask_at_box": mask, "frame_index": 0, "cam_ind": 0}
    with pytest.raises(NbError, match="rgb_map.*HIP device"):
        ev.evaluate({"rgb_map": torch.zeros(1, 256, 3)}, batch)
    with pytest.raises(NbError, match="rgb_map"):
        ev.evaluate({"rgb_map": np.zeros((1, 256, 3), np.float32)}, batch)
    assert ev.mse == [] and ev.psnr == [] and ev.ssim == []


def test_default_evaluator_touches_no_image_library(tmp_path):
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, %r)\n"
            "from neuralbody_amd.evaluator import Evaluator, EvalConfig\n"
            "Evaluator(EvalConfig(H=8, W=8))\n"
            "assert not {'cv2', 'skimage', 'PIL'} & set(sys.modules), sorted(sys.modules)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]


def test_save_images_needs_pil_at_construction(tmp_path, monkeypatch):
    import sys

    from neuralbody_amd.evaluator import Evaluator

    monkeypatch.setitem(sys.modules, "PIL", None)  # import PIL now raises ImportError
    with pytest.raises(ImportError):
        Evaluator(_cfg(tmp_path, eval_save_images=True))
    Evaluator(_cfg(tmp_path))  # the default path does not ask for it


def test_plugin_binds_the_live_cfg():
    from tests import helpers as H
    from neuralbody_amd.evaluator import Evaluator

    cfg = types.SimpleNamespace(H=1024, W=1000, ratio=0.5, white_bkgd=True, eval_whole_img=False, result_dir="somewhere")
    mod = H.load_plugin("if_nerf.py", cfg)
    ev = mod.Evaluator()
    assert isinstance(ev, Evaluator)
    assert (ev.cfg.H, ev.cfg.W, ev.cfg.white_bkgd, ev.cfg.eval_whole_img) == (512, 500, True, False)
    assert ev.cfg.eval_save_images is False and ev.cfg.result_dir == "somewhere"
    cfg.ratio, cfg.eval_whole_img = 1.0, True  # read at call time
    assert (ev.cfg.H, ev.cfg.eval_whole_img) == (1024, True)


def test_plugin_resolves_through_the_reference_factory():
    from oracle import ref_harness as rh

    if not rh.available():
        pytest.skip("reference tree not present")
    ns = rh.load()
    cfg = ns.cfg
    import importlib
    import sys

    importlib.import_module("lib.evaluators.make_evaluator")
    me = sys.modules["lib.evaluators.make_evaluator"]  # the package re-exports a function under the module's name
    saved = (cfg.evaluator_module, cfg.evaluator_path, cfg.skip_eval)
    cwd = os.getcwd()
    os.chdir(ns.root)
    try:
        cfg.evaluator_module = "lib.evaluators.if_nerf_hip"
        cfg.evaluator_path = os.path.join(ROOT, "neuralbody_amd", "plugins", "if_nerf.py")
        cfg.skip_eval = False
        ev = me.make_evaluator(cfg)
    finally:
        cfg.evaluator_module, cfg.evaluator_path, cfg.skip_eval = saved
        os.chdir(cwd)
    from neuralbody_amd.evaluator import Evaluator

    assert isinstance(ev, Evaluator)
    assert ev.cfg.H == int(cfg.H * cfg.ratio) and ev.cfg.W == int(cfg.W * cfg.ratio)
    assert ev.cfg.white_bkgd == bool(cfg.white_bkgd) and ev.cfg.result_dir == cfg.result_dir
    for name in ("evaluate", "summarize"):
        assert callable(getattr(ev, name))
