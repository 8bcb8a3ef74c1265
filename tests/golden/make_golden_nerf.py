"""Writes tests/golden/nerf_baseline.npz: the UNMODIFIED reference's vanilla-NeRF baseline (lib/networks/nerf.py behind
lib/networks/renderer/volume_renderer.py, configs/nerf/nerf_313.yaml with perturb 0) on 96 rays, on CPU in fp32.

    python tests/golden/make_golden_nerf.py        (where the reference tree is present; a fresh process: the harness loads once)

The fixture is data only: the rays, the reference's outputs, the depths and the raw of both passes (captured by wrapping the network
call), the two alpha_linear bias shifts of the weight recipe and a checksum of the weights.  The weights themselves are not stored:
tests/nerf_ref.py:make_state_dict rebuilds them from the seed."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import nerf_ref  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nerf_baseline.npz")
RAW_TOL = 1e-4  # the absolute tolerance on raw that the tests hold (the fixture may have no ray whose last density is within 10 x of 0)


def main():
    # nerf_net_utils.py:56 imports an extension that torch has since absorbed
    tss = types.ModuleType("torchsearchsorted")
    tss.searchsorted = lambda cdf, u, side="left": torch.searchsorted(cdf, u, right=(side == "right"))
    sys.modules["torchsearchsorted"] = tss
    ns = ref_harness.load(cfg_file="configs/nerf/nerf_313.yaml", opts=("perturb", "0"))
    cfg = ns.cfg
    assert (cfg.N_samples, cfg.N_importance, float(cfg.perturb), bool(cfg.lindisp)) == (64, 128, 0.0, False)
    cwd = os.getcwd()
    os.chdir(ns.root)
    try:
        net = ns.make_network(cfg)
        renderer = ns.make_renderer(cfg, net)
    finally:
        os.chdir(cwd)
    net.eval()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == nerf_ref.state_dict_shapes()

    o, d, near, far = nerf_ref.fixture_rays()
    z_coarse = nerf_ref.coarse_depths_f32(near, far, 64)
    # the recipe's shift: centre each module's density on the coarse points of the fixture's rays
    base = nerf_ref.make_state_dict((0.0, 0.0))
    pts = nerf_ref.points_f32(o, d, z_coarse)
    vd = nerf_ref.viewdirs_device(d)
    shift = []
    for m in nerf_ref.MODULES:
        alpha = nerf_ref.forward(base, m, pts, vd)[..., 3] / 20.0  # (make_state_dict scaled weight and bias by 20)
        shift.append(float(np.float32(-np.median(alpha))))
    sd = nerf_ref.make_state_dict(shift)
    missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys

    calls = []
    inner = net.forward

    def spy(pts, viewdirs, model=""):
        raw = inner(pts, viewdirs, model=model)
        calls.append((model, pts.detach().numpy().copy(), viewdirs.detach().numpy().copy(), raw.detach().numpy().copy()))
        return raw

    net.forward = spy
    batch = {"ray_o": torch.from_numpy(o)[None], "ray_d": torch.from_numpy(d)[None], "near": torch.from_numpy(near)[None],
             "far": torch.from_numpy(far)[None]}
    with torch.no_grad():
        ret = renderer.render(batch)
    assert [c[0] for c in calls] == ["", "fine"]
    ret = {k: v.numpy() for k, v in ret.items()}
    z_fine_pass = None
    # the depths of the two passes, recovered from the points the network saw: z = the depth whose fp32 point is that point
    raw_c, raw_f = calls[0][3], calls[1][3]
    assert np.array_equal(calls[0][1], nerf_ref.points_f32(o, d, z_coarse)), "coarse depths: near * (1 - t) + far * t in fp32"
    # volume_renderer.py:93 sorts cat(z_vals, z_samples): redo the second pass's depths through the reference's own functions
    from lib.networks.renderer.nerf_net_utils import raw2outputs, sample_pdf

    with torch.no_grad():
        zc = torch.from_numpy(z_coarse)
        _, _, _, weights, _ = raw2outputs(torch.from_numpy(raw_c), zc, torch.from_numpy(d), 0, False)
        z_samples = sample_pdf(.5 * (zc[..., 1:] + zc[..., :-1]), weights[..., 1:-1], 128, det=True)
        z_fine_pass = torch.sort(torch.cat([zc, z_samples], -1), -1)[0].numpy()
    assert np.array_equal(calls[1][1], nerf_ref.points_f32(o, d, z_fine_pass)), "fine depths reproduce the points the network saw"
    assert np.array_equal(ret["raw"].reshape(raw_f.shape), raw_f)

    # a fixture worth having: translucent rays, both signs of density, no ray decided by a last density too close to zero
    acc = ret["acc_map"].reshape(-1)
    mid = np.mean((acc > 0.05) & (acc < 0.95))
    pos = np.mean(np.concatenate([raw_c[..., 3].ravel(), raw_f[..., 3].ravel()]) > 0)
    last = min(np.abs(raw_c[:, -1, 3]).min(), np.abs(raw_f[:, -1, 3]).min())
    print("acc in (0.05, 0.95): %.2f of rays; density > 0: %.2f of samples; min |last density| %.3g; z_std %.3g .. %.3g"
          % (mid, pos, last, ret["z_std"].min(), ret["z_std"].max()))
    assert mid >= 0.25 and 0.25 <= pos <= 0.75, "trivial field"
    assert last > 10 * RAW_TOL, "a ray whose last density is within 10 x the raw tolerance of zero"

    np.savez_compressed(
        OUT, ray_o=o, ray_d=d, near=near, far=far, viewdirs=calls[0][2], alpha_shift=np.array(shift, np.float32),
        weights_sha256=np.array(nerf_ref.checksum(sd)), z_coarse=z_coarse, z_fine=z_fine_pass, z_samples=z_samples.numpy(),
        raw_coarse=raw_c, raw_fine=raw_f,
        **{"ref_" + k: v for k, v in ret.items() if k != "raw"}, **{"shape_" + k: np.array(v.shape) for k, v in ret.items()})
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
