"""nb_eval_metrics and the Evaluator on the device: every case of the fixture the reference's own evaluator produced
(tests/golden/eval_metrics.npz), procedurally seeded views at the sizes users run against the numpy restatement
(tests/metrics_ref.py), bit-for-bit repeatability, the degenerate crops, the no-synchronisation rule of evaluate() and one
render -> evaluate -> summarize round trip."""
import math
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_TOL = 1e-11  # two fp64 summation orders of the same windows differ by <= 1.8e-13
MSE_RTOL = 1e-6  # the reference sums fp32 pairwise: log2(n) * 2^-24
PSNR_TOL = 10.0 / math.log(10.0) * 2.0 * MSE_RTOL  # psnr follows from mse

_G = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
CASES = [str(n) for n in _G["names"]]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(device=DEV, dtype=dtype)


def _run(mask, rgb_pred, rgb_gt, white_bkgd, whole_img):
    from neuralbody_amd import ops

    Hh, Ww = mask.shape
    out = ops.eval_metrics(_dev(mask.reshape(-1)), Hh, Ww, _dev(rgb_pred), _dev(rgb_gt), white_bkgd=bool(white_bkgd),
                           whole_img=bool(whole_img))
    assert out.dtype == torch.float64 and out.shape == (8,) and out.is_cuda
    return out.cpu().numpy()


def _assert_matches(name, got, mse, psnr, ssim, box, n_windows):
    print("%s: mse %.9g (rel err %.2e) psnr %.9g (err %.2e) ssim %.15g (err %.2e) box %s windows %d" % (
        name, got[0], abs(got[0] - mse) / max(abs(mse), 1e-300), got[1], abs(got[1] - psnr) if math.isfinite(psnr) else 0.0,
        got[2], abs(got[2] - ssim), tuple(int(v) for v in got[3:7]), int(got[7])))
    assert tuple(int(v) for v in got[3:7]) == tuple(box)
    assert int(got[7]) == n_windows
    assert abs(got[2] - ssim) <= SSIM_TOL
    assert abs(got[0] - mse) <= MSE_RTOL * mse
    assert abs(got[1] - psnr) <= PSNR_TOL


@pytest.mark.parametrize("name", CASES)
def test_fixture_case(name):
    white, whole = (int(v) for v in _G[name + "/flags"])
    mse, psnr, ssim = (float(v) for v in _G[name + "/metrics"])
    box = tuple(int(v) for v in _G[name + "/box"])
    got = _run(_G[name + "/mask"], _G[name + "/rgb_pred"], _G[name + "/rgb_gt"], white, whole)
    if name == "identical":  # exact, not by tolerance: the device must give +inf and 1 too
        print("identical:", got)
        assert got[0] == 0.0 and got[1] == math.inf and got[2] == 1.0
        assert tuple(int(v) for v in got[3:7]) == box and int(got[7]) == (box[2] - 6) * (box[3] - 6)
        return
    _assert_matches(name, got, mse, psnr, ssim, box, (box[2] - 6) * (box[3] - 6))


@pytest.mark.parametrize("size,white,whole", [((512, 512), False, False), ((1024, 1024), True, False), ((301, 187), False, False),
                                              ((301, 187), True, True)])
def test_procedural_view(size, white, whole):
    mask, pred, gt = mr.ellipse_case(size[0], size[1], seed=size[0] + size[1] + int(white))
    ref = mr.metrics(mask, pred, gt, white, whole)
    got = _run(mask, pred, gt, white, whole)
    _assert_matches("%dx%d white=%d whole=%d" % (size[0], size[1], white, whole), got, ref["mse"], ref["psnr"], ref["ssim"],
                    ref["box"], ref["n_windows"])


def test_second_call_is_bit_identical():
    from neuralbody_amd import ops

    mask, pred, gt = mr.ellipse_case(301, 187, seed=9)
    m, p, g = _dev(mask.reshape(-1)), _dev(pred), _dev(gt)
    a = ops.eval_metrics(m, 301, 187, p, g)
    torch.empty(1 << 22, device=DEV).normal_()  # other work in between: the scratch of the second call is not the first's
    b = ops.eval_metrics(m, 301, 187, p, g)
    c = ops.eval_metrics(m, 301, 187, p, g, whole_img=True)
    d = ops.eval_metrics(m, 301, 187, p, g, whole_img=True, out=torch.empty(8, dtype=torch.float64, device=DEV))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(c.view(torch.int64), d.view(torch.int64))


def test_background_where_the_compacted_index_runs_out():
    """Fewer rays than set mask pixels: the pixels beyond n_rays keep the background, like nb_image_assemble."""
    mask, pred, gt = mr.ellipse_case(64, 48, seed=3)
    n = int(mask.sum()) - 37
    short = mask.copy().reshape(-1)
    short[np.flatnonzero(short)[n:]] = False  # what the device must see: the last 37 pixels as background ...
    short = short.reshape(mask.shape)
    x, y, w, h = mr.bounding_rect(mask)  # ... inside the box of the WHOLE mask
    want_ssim = mr.ssim(mr.scatter(short, pred[:n], True)[y:y + h, x:x + w], mr.scatter(short, gt[:n], True)[y:y + h, x:x + w])
    want_mse = mr.metrics(short, pred[:n], gt[:n])["mse"]
    got = _run(mask, pred[:n], gt[:n], True, False)
    assert tuple(int(v) for v in got[3:7]) == (x, y, w, h) and int(got[7]) == (w - 6) * (h - 6)
    assert abs(got[2] - want_ssim) <= SSIM_TOL
    assert abs(got[0] - want_mse) <= MSE_RTOL * want_mse


def test_degenerate_crops_give_nan_and_summarize_raises(tmp_path):
    from neuralbody_amd.evaluator import EvalConfig, Evaluator

    mask = np.zeros((20, 24), bool)
    mask[3:9, 2:15] = True  # 6 high: compare_ssim raises
    rgb = np.random.RandomState(0).uniform(0, 1, (int(mask.sum()), 3)).astype(np.float32)
    got = _run(mask, rgb, rgb * 0.5, False, False)
    assert math.isnan(got[2]) and got[7] == 0 and tuple(int(v) for v in got[3:7]) == (2, 3, 13, 6)
    assert got[0] > 0 and math.isfinite(got[1])
    empty = _run(np.zeros((20, 24), bool), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), True, False)
    assert math.isnan(empty[0]) and math.isnan(empty[2]) and empty[7] == 0 and tuple(int(v) for v in empty[3:7]) == (0, 0, 0, 0)
    whole = _run(np.zeros((20, 24), bool), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), True, True)
    assert whole[0] == 0.0 and whole[2] == 1.0 and tuple(int(v) for v in whole[3:7]) == (0, 0, 24, 20)  # all background
    tiny = _run(np.ones((5, 9), bool), np.zeros((45, 3), np.float32), np.ones((45, 3), np.float32), False, True)
    assert tiny[0] == 1.0 and math.isnan(tiny[2]) and tiny[7] == 0  # whole image under 7 high: mse still counts every pixel

    ev = Evaluator(EvalConfig(H=20, W=24, result_dir=str(tmp_path)))
    batch = {"rgb": _dev(rgb * 0.5)[None], "mask_at_box": _dev(mask.reshape(1, -1)), "frame_index": torch.tensor([41]),
             "cam_ind": torch.tensor([7])}
    ev.evaluate({"rgb_map": _dev(rgb)[None]}, batch)
    assert math.isnan(ev.ssim[0])
    with pytest.raises(ValueError, match=r"frame 41, cam 7"):
        ev.summarize()
    assert ev.mse == []  # the state is cleared all the same


def test_bad_arguments_are_refused():
    from neuralbody_amd import _lib, ops

    mask, pred, gt = mr.ellipse_case(32, 32, seed=1)
    m, p, g = _dev(mask.reshape(-1)), _dev(pred), _dev(gt)
    with pytest.raises(ValueError):
        ops.eval_metrics(m, 32, 31, p, g)  # mask does not cover H * W
    with pytest.raises(ValueError):
        ops.eval_metrics(m, 32, 32, p, g[:-1])
    with pytest.raises(_lib.NbError):
        ops.eval_metrics(m, 32, 32, p.cpu(), g)
    L = _lib.lib()
    assert L.nb_eval_metrics_scratch_size(0, 5) == 0 and L.nb_eval_metrics_scratch_size(1 << 16, 1 << 16) == 0
    out = torch.zeros(8, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(L.nb_eval_metrics_scratch_size(32, 32)), dtype=torch.uint8, device=DEV)
    st = ops._stream()
    assert L.nb_eval_metrics(_lib.ptr(m), 0, 32, _lib.ptr(p), _lib.ptr(g), p.shape[0], 0, 0, _lib.ptr(out), _lib.ptr(scratch), st) == -1
    assert L.nb_eval_metrics(None, 32, 32, _lib.ptr(p), _lib.ptr(g), p.shape[0], 0, 0, _lib.ptr(out), _lib.ptr(scratch), st) == -1
    assert L.nb_eval_metrics(_lib.ptr(m), 32, 32, None, _lib.ptr(g), p.shape[0], 0, 0, _lib.ptr(out), _lib.ptr(scratch), st) == -1
    assert L.nb_eval_metrics(_lib.ptr(m), 32, 32, _lib.ptr(p), _lib.ptr(g), p.shape[0], 0, 0, _lib.ptr(out), None, st) == -1
    assert L.nb_eval_metrics(_lib.ptr(m), 1 << 16, 1 << 16, _lib.ptr(p), _lib.ptr(g), p.shape[0], 0, 0, _lib.ptr(out),
                             _lib.ptr(scratch), st) == -1
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # a refused call launches nothing


def test_evaluate_issues_no_synchronising_call(tmp_path):
    """torch.cuda.set_sync_debug_mode('error') makes every synchronising torch call raise; that this build honours it on
    ROCm is checked first with a call that must synchronise (.item()).  If it does not, one evaluate() is captured into a
    single-stream torch.cuda.graph instead (capture refuses synchronisation and allocation outside the graph's pool)."""
    from neuralbody_amd.evaluator import EvalConfig, Evaluator

    mask, pred, gt = mr.ellipse_case(96, 80, seed=2)
    ref = mr.metrics(mask, pred, gt)
    output = {"rgb_map": _dev(pred)[None]}
    batch = {"rgb": _dev(gt)[None], "mask_at_box": _dev(mask.reshape(1, -1)), "frame_index": torch.tensor([0], device=DEV),
             "cam_ind": torch.tensor([3], device=DEV)}
    ev = Evaluator(EvalConfig(H=96, W=80, result_dir=str(tmp_path)))
    ev.evaluate(output, batch)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    saved = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            ev.evaluate(output, batch)
    finally:
        torch.cuda.set_sync_debug_mode(saved)
    if honoured:
        print("no-sync check: torch.cuda.set_sync_debug_mode('error')")
    else:
        print("no-sync check: sync debug mode is not honoured by this build; capturing evaluate() in a torch.cuda.graph")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ev.evaluate(output, batch)
        g.replay()
    torch.cuda.synchronize()
    ssim = ev.ssim
    assert len(ssim) == 2 and all(abs(s - ref["ssim"]) <= SSIM_TOL for s in ssim)


def test_eval_metrics_is_capturable_in_a_graph():
    from neuralbody_amd import ops

    mask, pred, gt = mr.ellipse_case(96, 80, seed=4)
    m, p, g = _dev(mask.reshape(-1)), _dev(pred), _dev(gt)
    eager = ops.eval_metrics(m, 96, 80, p, g)
    torch.cuda.synchronize()
    out = torch.zeros(8, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.eval_metrics(m, 96, 80, p, g, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), eager.view(torch.int64))


def test_host_batch_and_saved_images(tmp_path):
    """batch['rgb'] / batch['mask_at_box'] on the host (what a DataLoader hands over) are moved by evaluate(); with
    eval_save_images the cropped comparison PNGs are written at summarize()."""
    Image = pytest.importorskip("PIL.Image")
    from neuralbody_amd.evaluator import EvalConfig, Evaluator

    mask, pred, gt = mr.ellipse_case(64, 48, seed=6)
    ref = mr.metrics(mask, pred, gt, white_bkgd=True)
    ev = Evaluator(EvalConfig(H=64, W=48, white_bkgd=True, result_dir=str(tmp_path), eval_save_images=True))
    batch = {"rgb": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(1, -1)), "frame_index": 5, "cam_ind": 2}
    ev.evaluate({"rgb_map": _dev(pred)[None]}, batch)
    means = ev.summarize()
    assert abs(means["ssim"] - ref["ssim"]) <= SSIM_TOL
    x, y, w, h = ref["box"]
    for tail, rgb in (("", pred), ("_gt", gt)):
        img = np.asarray(Image.open(str(tmp_path / "comparison" / ("frame0005_view0002%s.png" % tail))))
        assert img.shape == (h, w, 3)
        want = (mr.scatter(mask, rgb, True)[y:y + h, x:x + w] * 255.0)
        assert np.abs(img.astype(np.float64) - want).max() <= 1.0


def test_render_evaluate_summarize_round_trip(tmp_path, capsys):
    from oracle import neuralbody_oracle as orc
    from neuralbody_amd.evaluator import EvalConfig, Evaluator
    from tests.golden import scenes

    r, sd, body, batch, cam, t_rand = scenes.build("small")
    Hh, Ww = cam[3], cam[4]
    net = H.make_network(sd, DEV, True, precision=H.DEFAULT_PRECISION)
    rend = H.make_renderer(net, r)
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        out = rend.render(bd)
        ref = orc.render(orc.tensor_state_dict(sd), batch, n_samples=r["n_samples"], training=True)
    # ground truth: the oracle's RGB, perturbed
    n = ref["rgb_map"].shape[1]
    rs = np.random.RandomState(12)
    gt = np.clip(ref["rgb_map"][0].numpy() + 0.05 * rs.standard_normal((n, 3)), 0.0, 1.0).astype(np.float32)
    bd["rgb"] = _dev(gt)[None]
    bd["frame_index"], bd["cam_ind"] = torch.tensor([3]), torch.tensor([1])
    mask = batch["mask_at_box"].reshape(Hh, Ww)
    assert int(mask.sum()) == n

    ev = Evaluator(EvalConfig(H=Hh, W=Ww, white_bkgd=r["white_bkgd"], result_dir=str(tmp_path / "res")))
    ev.evaluate(out, bd)
    ev.evaluate(out, bd)
    want = mr.metrics(mask, out["rgb_map"][0].cpu().numpy(), gt, r["white_bkgd"])  # the restatement on the SAME device output
    assert want["n_windows"] > 0 and 0.0 < want["ssim"] < 1.0
    listed = (ev.mse, ev.psnr, ev.ssim)
    means = ev.summarize()
    printed = capsys.readouterr().out
    print("round trip: mse %.9g psnr %.9g ssim %.15g (restatement %.9g %.9g %.15g)" % (
        means["mse"], means["psnr"], means["ssim"], want["mse"], want["psnr"], want["ssim"]))
    assert set(means) == {"mse", "psnr", "ssim"}
    assert abs(means["ssim"] - want["ssim"]) <= SSIM_TOL
    assert abs(means["mse"] - want["mse"]) <= MSE_RTOL * want["mse"]
    assert abs(means["psnr"] - want["psnr"]) <= PSNR_TOL
    assert "mse: " in printed and "psnr: " in printed and "ssim: " in printed
    saved = np.load(str(tmp_path / "res" / "metrics.npy"), allow_pickle=True).item()  # the reference's dict layout
    assert set(saved) == {"mse", "psnr", "ssim"} and all(len(v) == 2 for v in saved.values())
    for k, lst in zip(("mse", "psnr", "ssim"), listed):
        assert saved[k] == lst and saved[k][0] == saved[k][1] and np.mean(saved[k]) == means[k]
    assert ev.mse == [] and ev.psnr == [] and ev.ssim == []  # cleared
