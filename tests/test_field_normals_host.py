"""The references of the field-normal tests, checked on the CPU (tests/field_normal_cases.py), and the bindings of the three entry
points of csrc/nb_field_normal.hip.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import bwd_cases as bc
from tests import decode_f32_cases as dc
from tests import field_normal_cases as fc

ENTRIES = ("nb_trilinear_grad", "nb_normal_select", "nb_normal_composite")


def test_model_equals_float64_autograd_through_grid_sample():
    """grad_f64 against torch autograd of sum_c d_feat[c] F_c(p) with F = grid_sample (align_corners, zeros) of the four levels and
    p -> normalised coordinates as latent_xyzc.py:41-60 forms them, float64, under a real rotation; on the points at least 1e-3 of a voxel
    away from every cell face (autograd's derivative at a face is a convention, the model's is the forward's cell)."""
    g, d_feat, grids = bc.random_tri_scene()
    rs = np.random.RandomState(3)
    vols = [rs.standard_normal(gr.shape + (c,)) * (np.asarray(gr) >= 0)[..., None] for gr, c in zip(grids, bc.LEVEL_CHANNELS)]
    voxel, out_sh = (0.005, 0.007, 0.004), (12, 10, 14)  # (d, h, w)
    Rm = dc._rotation((1.0, 2.0, 3.0), 0.3)
    Th, bmin = np.array([0.3, -1.2, 0.7]), np.array([-0.2, 0.1, 0.4])
    ext = np.array([voxel[2] * out_sh[2], voxel[1] * out_sh[1], voxel[0] * out_sh[0]])
    world = (bmin + (g + 1.0) / 2.0 * ext) @ Rm.T + Th
    p = torch.from_numpy(world).requires_grad_(True)
    gt = ((p - torch.from_numpy(Th)) @ torch.from_numpy(Rm) - torch.from_numpy(bmin)) / torch.from_numpy(ext) * 2.0 - 1.0
    total = 0.0
    for l, v in enumerate(vols):
        feat = torch.nn.functional.grid_sample(torch.from_numpy(v).permute(3, 0, 1, 2)[None], gt[None, None, None], padding_mode="zeros",
                                               align_corners=True)[0, :, 0, 0].t()
        total = total + (feat * torch.from_numpy(d_feat[:, bc.CHAN_BASE[l]:bc.CHAN_BASE[l] + v.shape[3]])).sum()
    total.backward()
    got, A, _ = fc.grad_f64(gt.detach().numpy(), d_feat, vols, voxel, out_sh, Rm, grids=grids)
    away = np.ones(len(g), bool)
    for gr in grids:
        D, H, W = gr.shape
        for a, s in ((0, W), (1, H), (2, D)):
            i = bc.unnormalize(gt.detach().numpy()[:, a], s)
            away &= np.abs(i - np.round(i)) >= 1e-3
    assert away.sum() > 0.9 * len(g)
    ref = p.grad.numpy()
    assert np.abs(ref[away]).max() > 1.0
    assert np.abs(got - ref)[away].max() <= 1e-12 * A[away].max()


@pytest.mark.parametrize("name", fc.E2E_SCENES)
def test_model_agrees_with_a_central_difference_of_the_oracle(name):
    """chain_f64 + grad_f64 on the oracle's volumes against (sigma(p + h e) - sigma(p - h e)) / 2h of the oracle's float64
    calculate_density, and against its autograd, on kept points: sign and axis conventions."""
    from oracle import neuralbody_oracle as orc

    e = fc.e2e_reference(name)
    pick = np.flatnonzero(e["keep"])[::37]
    assert len(pick) >= 20
    sd64 = orc.tensor_state_dict(e["sd"], dtype=torch.float64)
    vols64 = [v.double() for v in e["vols"]]
    sp = {k: torch.from_numpy(np.asarray(e["batch"][k])).double() for k in ("R", "Th", "bounds")}
    sp["out_sh"] = e["out_sh"]
    p0 = torch.from_numpy(e["wpts"][pick].astype(np.float64))
    h = 1e-7
    fd = np.zeros((len(pick), 3))
    with torch.no_grad():
        for a in range(3):
            d = torch.zeros(3, dtype=torch.float64)
            d[a] = h
            hi = orc.calculate_density(sd64, (p0 + d)[None], vols64, sp)[0, :, 0]
            lo = orc.calculate_density(sd64, (p0 - d)[None], vols64, sp)[0, :, 0]
            fd[:, a] = ((hi - lo) / (2 * h)).numpy()
    d_feat = fc.chain_f64(e["sd"], *e["h"])
    vols_cl = [v[0].permute(1, 2, 3, 0).numpy() for v in e["vols"]]
    model, _, _ = fc.grad_f64(e["gn"], d_feat, vols_cl, fc.VOXEL32, e["out_sh"], np.asarray(e["batch"]["R"], np.float64).reshape(3, 3))
    scale = np.abs(e["g64"]).max()
    assert scale > 1.0
    assert np.abs(model - e["g64"]).max() <= 1e-10 * scale          # the model is the oracle's autograd (every point: float64 has no near misses)
    assert np.abs(model[pick] - fd).max() <= 1e-5 * scale           # ... and the slope of sigma itself


@pytest.mark.parametrize("pose", list(dc.POSES))
def test_lattice_cases_are_exact_and_mutants_show(pose):
    n = max(fc.LATTICE_N)
    w, d, grad, A, touched = fc.lattice_reference(pose, n)
    fc.assert_grad_lattice(grad, A)
    assert np.array_equal(grad.astype(np.float32).astype(np.float64), grad)
    assert np.abs(grad).max() >= 1024 and (np.abs(grad) > 0).mean() > 0.5
    # the kinds of points the case is to hold: on voxel planes, in the rim, clamped, beside inactive voxels
    g = dc.case_grid(fc.lattice_q()[:n], pose)[1].astype(np.float64)
    D, H, W = dc.SHAPES[0]
    ix = bc.unnormalize(g[:, 0], W)
    assert (ix == np.round(ix)).sum() > 20 and ((ix > -1) & (ix < 0)).any() and ((ix > W - 1) & (ix < W)).any()
    assert (ix < -2).any() and (ix > W + 1).any()
    far = (ix < -20) | (ix > W + 20)  # beyond the clamp of EVERY level (level 3's voxels are eight of level 0's)
    assert far.any() and not grad[far].any()
    assert all(t.any() and not t.all() for t in touched)
    for mutate in fc.MUTANTS:
        if mutate == "R_transposed" and pose == "identity":
            continue  # (the identity cannot see it)
        bad = fc.lattice_reference(pose, n, mutate)[2]
        assert (bad != grad).any(1).sum() >= 8, mutate
    # n = 1 alone already tells the left-hand cell from the right-hand one
    assert (fc.lattice_reference(pose, 1, "left_cell")[2] != fc.lattice_reference(pose, 1)[2]).any()
    # rows no point reads with a non-zero weight pair exist on the fine levels (257 points reach all 45 voxels of the coarsest):
    # the POISON run has something to hide
    rows = fc.rows_of(dc.distinct_volumes(), fc.lattice_grids(), touched)
    assert all((r == fc.POISON).all(1).sum() >= 8 for r in rows[:2])


@pytest.mark.parametrize("name", fc.E2E_SCENES)
def test_excluded_share_stays_under_its_cap(name):
    e = fc.e2e_reference(name)
    share = 1.0 - e["keep"].mean()
    print("%s: %.1f %% of the 1024 points excluded" % (name, 100 * share))
    assert 0.0 < share <= fc.EXCLUDE_CAP
    g = np.abs(e["g64"]).max(1)
    assert (g[e["keep"]] >= fc.E2E_SIN_FROM * g.max()).sum() >= 50  # the angle check has points to look at


def test_select_and_composite_models():
    ro, rd, ne, fa, tv, tr, w = fc.select_inputs(25, 41)
    idx, pts = fc.select_model(ro, rd, ne, fa, tv, tr, w, 1.0)
    assert np.array_equal(idx, np.flatnonzero(w.reshape(-1) >= 1)) and len(idx) and not (idx // 41 == 0).any()
    g = fc.integer_gradients(len(idx))
    nm, na = fc.composite_model(idx, g, w)
    ln = np.linalg.norm(nm, axis=1)
    assert np.all((np.abs(ln - 1) < 1e-6) | (ln == 0)) and (ln == 0).any() and (ln > 0).any()
    assert np.array_equal(na, np.where(w >= 1, w, 0).sum(1))


def test_header_ctypes_and_ops_bindings():
    from neuralbody_amd import _lib, ops

    src = open(_lib.HEADER).read()
    assert "#define NB_ABI_VERSION 20\n" in src and _lib.ABI_VERSION == 20  # purely additive
    for name in ENTRIES:
        assert name in _lib.header_functions() and name in _lib.SIGNATURES
        assert src.count("replaces: nothing in the reference") >= 3
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["nb_trilinear_grad"] == (C.c_int, [C.POINTER(_lib.NbScene), P * 4, P * 4, P, P, I64, P, P])
    assert _lib.SIGNATURES["nb_normal_select"] == (C.c_int, [P, P, P, P, I64, I32, P, P, P, C.c_float, I32, P, P, P, P, P])
    assert _lib.SIGNATURES["nb_normal_composite"] == (C.c_int, [P, P, I64, P, I64, I32, P, P, P])
    for f in ("trilinear_grad", "normal_select", "normal_composite"):
        assert callable(getattr(ops, f))
    from neuralbody_amd.network import Network

    assert callable(Network.calculate_density_gradient)
    assert os.path.exists(os.path.join(os.path.dirname(_lib.HERE), "neuralbody_amd", "csrc", "nb_field_normal.hip"))


def test_refused_arguments_and_empty_calls():
    """n == 0 returns NB_OK and looks at no pointer; sizes beyond 2^31 - 256 samples and negative counts are NB_EINVAL (host checks:
    nothing is launched)."""
    from neuralbody_amd import _lib

    L = _lib.lib()
    four = (C.c_void_p * 4)()
    assert L.nb_trilinear_grad(None, four, four, None, None, 0, None, None) == 0
    assert L.nb_trilinear_grad(None, four, four, None, None, -1, None, None) == -1
    assert L.nb_trilinear_grad(None, four, four, None, None, 5, None, None) == -1 and b"NULL" in L.nb_last_error()
    assert L.nb_trilinear_grad(None, four, four, None, None, 2 ** 31 - 256, None, None) == -1 and b"2^31 - 257" in L.nb_last_error()
    assert L.nb_trilinear_grad(None, four, four, None, None, 2 ** 31 - 257, None, None) == -1 and b"NULL" in L.nb_last_error()
    assert L.nb_normal_select(None, None, None, None, 0, 64, None, None, None, 0.5, 0, None, None, None, None, None) == 0
    assert L.nb_normal_select(None, None, None, None, 7, 0, None, None, None, 0.5, 0, None, None, None, None, None) == 0
    assert L.nb_normal_select(None, None, None, None, 2 ** 25, 64, None, None, None, 0.5, 0, None, None, None, None, None) == -1
    assert b"2^31 - 256" in L.nb_last_error()
    assert L.nb_normal_select(None, None, None, None, (2 ** 31 - 256) // 64 - 1, 64, None, None, None, 0.5, 0, None, None, None, None, None) == -1
    assert b"NULL" in L.nb_last_error()  # the size passes, the pointers do not
    assert L.nb_normal_composite(None, None, 0, None, 0, 64, None, None, None) == 0
    assert L.nb_normal_composite(None, None, 5, None, 0, 64, None, None, None) == -1
    assert L.nb_normal_composite(None, None, -1, None, 4, 64, None, None, None) == -1
    assert L.nb_normal_composite(None, None, 0, None, 2 ** 25, 64, None, None, None) == -1


def test_turntable_takes_normals_from_the_projects_own_mesh_only(monkeypatch, tmp_path):
    """MeshVisualizer.render_turntable hands vertex_normals to the turntable only for this package's TriMesh; a foreign mesh object
    with a `vertex_normals` attribute (trimesh.Trimesh computes one itself) still reaches MeshTurntable.render with normals=None,
    i.e. with the triangles' own normals, as before; and never with colours."""
    import types

    from neuralbody_amd import mesh_io, mesh_render
    from neuralbody_amd.mesh import TriMesh

    seen = []

    class FakeTurntable:
        def __init__(self, H, W, dataset=None, device=None):
            self.device = torch.device("cpu")

        def render(self, mesh, triangles=None, normals=None, colors=False):
            seen.append((normals, colors))
            return "images"

        def save(self, images, directory):
            return [directory]

    monkeypatch.setattr(mesh_render, "MeshTurntable", FakeTurntable)
    vis = mesh_io.MeshVisualizer(types.SimpleNamespace(result_dir=str(tmp_path)))
    v = np.zeros((3, 3))
    f = np.array([[0, 1, 2]])
    n = np.eye(3, dtype=np.float32)
    foreign = types.SimpleNamespace(vertices=v, faces=f, vertex_normals=n.copy())
    vis.render_turntable(foreign, "a")
    vis.render_turntable(TriMesh(v, f), "b")
    vis.render_turntable(TriMesh(v, f, vertex_normals=n), "c")
    vis.render_turntable(TriMesh(v, f, vertex_normals=n, vertex_colors=np.zeros((3, 3), np.uint8)), "d", colors=True)
    assert seen[0] == (None, False) and seen[1] == (None, False) and seen[3] == (None, True)
    assert isinstance(seen[2][0], torch.Tensor) and seen[2][0].dtype == torch.float32 and np.array_equal(seen[2][0].numpy(), n)
