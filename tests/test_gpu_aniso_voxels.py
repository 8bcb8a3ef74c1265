"""Every consumer of the voxel grid at a voxel size whose three entries differ (tests/aniso_cases.py: ANISO = (0.004, 0.005, 0.008)
in dhw order, out_sh (96, 128, 64)).  The order of voxel_size is decided by hand in grid_coords (csrc/nb_march_common.h: every
march, nb_decode_points, nb_trilinear_bwd, nb_trilinear_grad), the scale table of csrc/nb_field_normal.hip, nb_smpl_voxelize,
ops.make_scene and Network's backward; with the cubic voxels of every other test, reading it backwards changes nothing.  Here the
oracle renders another picture by 12 000 x RGB_TOL when it does (tests/test_aniso_cases_host.py).

Each consumer is compared with what its own test compares it with, under that test's constant; only the voxel size is new."""
import numpy as np
import pytest
import torch

from tests import aniso_cases as ac
from tests import helpers as H
from tests import smpl_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORMAL_RAYS_FROM = 512


def _network(precision):
    net = H.make_network(ac.scene()["sd"], DEV, True, precision, ac.ANISO)
    assert tuple(net.voxel_size) == ac.ANISO
    return net


# ---------------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
def test_render_matches_the_oracle(precision):
    """Renderer.render (encoder + march, all HIP) as tests/test_gpu_parity.py::test_render_end_to_end_matches_reference holds it."""
    s, ref = ac.scene(), ac.oracle_render()
    rend = H.make_renderer(_network(precision), s["recipe"])
    with torch.no_grad():
        out = rend.render(H.device_batch(s["batch"], DEV))
    torch.cuda.synchronize()
    n = s["batch"]["ray_o"].shape[1]
    assert out["rgb_map"].shape == (1, n, 3) and float(out["rgb_map"].max()) > 0.01
    err = H.assert_close(out["rgb_map"].cpu().numpy(), ref["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), ref["acc_map"], 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), ref["weights"], 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), ref["depth_map"], 2e-4, "depth_map")
    wrong = float(np.abs(out["rgb_map"].cpu().numpy() - ac.oracle_render(ac.ANISO[::-1])["rgb_map"]).max())
    print("%s: rgb L-inf vs the oracle %.2e over %d rays (vs the oracle with voxel_size reversed: %.2e)" % (precision, err, n, wrong))


# ---------------------------------------------------------------------------------------------------------- point decoder
@pytest.mark.parametrize("precision", ["f32", "f16f6"])
def test_decode_points_matches_the_oracle(precision):
    """nb_decode_points on the oracle's volumes, density and colour, under the tolerances of
    tests/test_gpu_parity.py::test_decode_points_stages_against_oracle."""
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    s = ac.scene()
    batch, ns = s["batch"], s["recipe"]["n_samples"]
    sel = slice(0, None, 5)
    ray_o, ray_d = torch.from_numpy(batch["ray_o"])[:, sel], torch.from_numpy(batch["ray_d"])[:, sel]
    wpts, _ = orc.get_sampling_points(ray_o, ray_d, torch.from_numpy(batch["near"])[:, sel], torch.from_numpy(batch["far"])[:, sel], ns)
    vd = ray_d / torch.norm(ray_d, dim=2, keepdim=True)
    w = wpts.reshape(1, -1, 3).clone()
    v = vd[:, :, None].repeat(1, 1, ns, 1).reshape(1, -1, 3)
    w[0, :7] += torch.tensor([3.0, -2.0, 1.0])  # a few points outside the volume
    sp_cpu = {k: torch.from_numpy(batch[k]) for k in ("R", "Th", "bounds", "latent_index")}
    sp_cpu["out_sh"] = s["out_sh"]
    with torch.no_grad():
        raw = orc.calculate_density_color(s["sdt"], w, v, s["vols"], sp_cpu, ac.ANISO)[0]
        dens = orc.calculate_density(s["sdt"], w, s["vols"], sp_cpu, ac.ANISO)[0]
        wrong = orc.calculate_density(s["sdt"], w, s["vols"], sp_cpu, ac.ANISO[::-1])[0]
    assert float((dens - wrong).abs().max()) > 1.0  # the points tell the order apart
    net = _network(precision)
    bd = H.device_batch(batch, DEV)
    sp = H.sp_input_of(bd, s["out_sh"])
    vols_dev = [x.to(DEV) for x in s["vols"]]
    scene = net.make_scene(vols_dev, sp, precision)
    out = ops.decode_points(scene, net.packed_weights(precision), net.latent_bias(bd["latent_index"]), w[0].to(DEV).contiguous(),
                            v[0].to(DEV).contiguous(), precision=precision)
    torch.cuda.synchronize()
    tol_raw = 2e-4 if precision == "f32" else 2.5e-3
    e_raw = H.assert_close(out.cpu().numpy(), raw.numpy(), tol_raw, "raw (rgb logits, sigma)")
    dens_api = net.calculate_density(w.to(DEV), vols_dev, sp)
    e_dens = H.assert_close(dens_api[0].cpu().numpy(), dens.numpy(), tol_raw, "calculate_density")
    print("%s: raw err %.2e, density err %.2e (rel. to max(1,|ref|)) over %d points" % (precision, e_raw, e_dens, w.shape[1]))


# ---------------------------------------------------------------------------------------------------------- training
def test_training_step_gradients_match_autograd():
    """tests/test_gpu_backward.py::test_full_training_step_gradients_match_autograd, its recipe and its ENC_TOL, at ANISO (that
    recipe is `small_dense`: the body and camera of `small` under denser weights, so that gradients flow through many samples)."""
    from tests.test_gpu_backward import training_step_gradients_match_autograd

    training_step_gradients_match_autograd(ac.ANISO)


# ---------------------------------------------------------------------------------------------------------- field normals
def test_density_gradient_matches_float64_autograd():
    """tests/test_gpu_field_normals.py::test_gradient_against_float64_autograd_of_the_oracle, its bounds, at ANISO.  The rays are
    512:768:16 of the view, not 0:256:16: with the finer grid more of the first rows' samples lie inside the volume, and 13.8 % of
    them have a pre-activation or a cell that fp32 may decide the other way -- past the suite's cap of 10 % on what a case may
    exclude.  Of these rays' samples 6.0 % do (both figures from the float64 reference alone)."""
    from tests.test_gpu_field_normals import gradient_against_float64_autograd

    gradient_against_float64_autograd(ac.SCENE, ac.ANISO, first_ray=NORMAL_RAYS_FROM)


# ---------------------------------------------------------------------------------------------------------- pose-driven frames
def test_pose_driver_frames_are_the_restatement():
    """PoseDriver(voxel_size=ANISO).frames: coord, out_sh, bounds and can_bounds of every frame equal smpl_ref.voxelize_f32 of the
    frame's own posed vertices, at every entry."""
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    model = SmplModel.from_arrays(sr.synthetic_smpl(21, 6890, sr.SMPL_PARENTS, box=(0.3, 0.5, 0.2)), DEV)
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(3)]
    stacked = [np.stack([p[k] for p in P]) for k in range(4)]
    drv = PoseDriver(model, voxel_size=ac.ANISO)
    made = drv.frames(*stacked, latent_index=[0, 1, 2], new_params=True)
    verts = drv.vertices(*stacked, new_params=True).cpu().numpy()
    assert len(made) == 3
    for f, (frame, can_bounds) in enumerate(made):
        want = sr.voxelize_f32(verts[f], frame["R"][0].cpu().numpy(), stacked[3][f], ac.ANISO, "zju")
        assert np.array_equal(frame["coord"][0].cpu().numpy(), want["coord"]), f
        assert np.array_equal(frame["out_sh"][0].cpu().numpy(), want["out_sh"]), (f, want["out_sh"].tolist())
        assert np.array_equal(frame["bounds"][0].cpu().numpy().view(np.uint32), want["bounds"].view(np.uint32)), f
        assert np.array_equal(can_bounds.reshape(-1).view(np.int32), want["summary"][:6]), f
        reversed_vs = sr.voxelize_f32(verts[f], frame["R"][0].cpu().numpy(), stacked[3][f], ac.ANISO, "zju", "vs_reversed")
        assert not np.array_equal(want["coord"], reversed_vs["coord"]) and not np.array_equal(want["out_sh"], reversed_vs["out_sh"])
