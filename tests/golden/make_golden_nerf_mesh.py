"""Writes tests/golden/nerf_mesh.npz: the UNMODIFIED reference's mesh pass of the vanilla-NeRF baseline (lib/networks/nerf_mesh.py
behind lib/networks/renderer/volume_mesh_renderer.py, configs/nerf/nerf_313.yaml with N_importance 0) on a 16 x 14 x 12 lattice, on
CPU in fp32, and torch-CPU autograd of the reference's Nerf.forward at the first 96 inside points.

    python tests/golden/make_golden_nerf_mesh.py   (where the reference tree is present; a fresh process: the harness loads once)

The fixture is data only: the padded cubes the reference hands to marching cubes (one per module: the reference class has only
`model`, so the model_fine weights are loaded under the model names for the second), the gradients, the two scalars the tests scale
their bounds by, the iso values, the two alpha_linear bias shifts of the weight recipe and a checksum of the weights.  The weights,
the lattice and `inside` are not stored: tests/nerf_mesh_ref.py rebuilds them.  PyMCubes and trimesh are not needed: stand-ins
record what marching_cubes is handed."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import nerf_mesh_ref as mref  # noqa: E402
from tests import nerf_ref  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nerf_mesh.npz")


def main():
    handed = []
    mc = types.ModuleType("mcubes")
    mc.marching_cubes = lambda cube, th: (handed.append((np.array(cube), float(th))), (np.zeros((0, 3)), np.zeros((0, 3), int)))[1]
    sys.modules["mcubes"] = mc
    tm = types.ModuleType("trimesh")
    tm.Trimesh = lambda vertices, triangles: (vertices, triangles)
    sys.modules["trimesh"] = tm
    ns = ref_harness.load(cfg_file="configs/nerf/nerf_313.yaml", opts=("perturb", "0", "N_importance", "0"))
    cfg = ns.cfg
    assert int(cfg.N_importance) == 0 and (cfg.netdepth, cfg.netwidth, cfg.xyz_res, bool(cfg.use_viewdirs)) == (8, 256, 10, True)
    from lib.networks import nerf_mesh
    from lib.networks.renderer import volume_mesh_renderer

    pts, inside = mref.lattice()
    count = int(inside.sum())
    assert count % 64 != 0, "the last tile of the density kernel must be partial"
    pin = pts[inside]
    sd, shift = mref.centred_state_dict(pin)
    net = nerf_mesh.Network().eval()
    renderer = volume_mesh_renderer.Renderer(net)
    batch = {"pts": torch.from_numpy(pts)[None], "inside": torch.from_numpy(inside.astype(np.uint8))[None]}

    cubes, grads, isos, margins, shares, e_cube, e_grad = [], [], [], [], [], 0.0, 0.0
    for m in nerf_ref.MODULES:
        # the reference class has `model` alone: each module's weights in turn under the model.* names
        missing = net.load_state_dict({"model." + k[len(m) + 1:]: torch.from_numpy(v) for k, v in sd.items()
                                       if k.startswith(m + ".")}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        alpha64, z64 = mref.trunk(sd, m, pin)
        iso, margin = mref.pick_iso(alpha64)
        assert iso is not None and iso != 0.0 and margin >= mref.ISO_MARGIN, (m, iso, margin)
        cfg.mesh_th = iso
        del handed[:]
        with torch.no_grad():
            ret = renderer.render(batch)
        assert len(handed) == 1 and handed[0][1] == iso and ret["cube"].shape == tuple(d + 2 * mref.PAD for d in inside.shape)
        cube = handed[0][0]
        assert np.array_equal(cube, ret["cube"]) and np.array_equal(cube, cube.astype(np.float32))  # fp32 values in a float64 array
        core = cube[mref.PAD:-mref.PAD, mref.PAD:-mref.PAD, mref.PAD:-mref.PAD]
        assert np.all(core[~inside] == 0) and cube.sum() == core.sum()
        e_cube = max(e_cube, float(np.abs(core[inside] - alpha64).max()))
        assert float(np.abs(core[inside] - iso).min()) >= mref.ISO_MARGIN, "the reference's own cube is too close to the iso value"
        # the gradient: autograd through the reference's embedder and Nerf.forward, fp32 on the CPU
        x = torch.from_numpy(pin[:mref.N_GRAD]).clone().requires_grad_(True)
        hooks, acts = [], []
        for lin in net.model.pts_linears:
            hooks.append(lin.register_forward_hook(lambda mod, i, o: acts.append(o.detach().numpy() > 0)))
        net.model(net.embed_fn(x)).sum().backward()
        for h in hooks:
            h.remove()
        g = x.grad.numpy().copy()
        e_grad = max(e_grad, float(np.abs(g - mref.trunk_gradient(sd, m, pin[:mref.N_GRAD], masks=acts)).max()))
        cubes.append(cube.astype(np.float32))
        grads.append(g)
        isos.append(iso)
        margins.append(margin)
        shares.append(float(np.mean(alpha64 > iso)))
        print("%s: iso %.6f margin %.3e share above %.2f, alpha in [%.3f, %.3f]" % (m, iso, margin, shares[-1], alpha64.min(),
                                                                                    alpha64.max()))
    print("count %d (mod 64 = %d), e_ref_cube %.3e, e_ref_grad %.3e, max |grad| %.3e" % (count, count % 64, e_cube, e_grad,
                                                                                         np.abs(grads).max()))
    assert 0.0 < e_cube < 1e-4 and 0.0 < e_grad
    np.savez_compressed(OUT, alpha_shift=shift, weights_sha256=np.array(nerf_ref.checksum(sd)), count=np.array(count),
                        iso=np.array(isos, np.float64), iso_margin=np.array(margins), share_above=np.array(shares),
                        cube_ref=np.stack(cubes), grad_ref=np.stack(grads).astype(np.float32), e_ref_cube=np.array(e_cube),
                        e_ref_grad=np.array(e_grad))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
