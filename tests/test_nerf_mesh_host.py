"""The vanilla-NeRF baseline's mesh pass without a GPU: the float64 helpers of tests/nerf_mesh_ref.py against each other and against
tests/nerf_ref.py, the integrity of tests/golden/nerf_mesh.npz, the plugin and the new entry points' declarations."""
import types

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import nerf_mesh_ref as mref
from tests import nerf_ref as ref


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(hp.GOLDEN + "/nerf_mesh.npz"))


@pytest.fixture(scope="module")
def lattice():
    pts, inside = mref.lattice()
    return pts, inside, pts[inside]


@pytest.fixture(scope="module")
def sd(fx):
    sd = ref.make_state_dict(fx["alpha_shift"])
    assert ref.checksum(sd) == str(fx["weights_sha256"]), "the seed recipe no longer gives the fixture's weights"
    return sd


def test_trunk_is_the_density_column_of_the_full_model(sd, lattice):
    pin = lattice[2]
    vd = np.tile(np.array([[0.0, 0.6, -0.8]], np.float32), (len(pin), 1))
    for m in ref.MODULES:
        alpha, z = mref.trunk(sd, m, pin)
        want = ref.forward(sd, m, pin[:, None, :], vd)[:, 0, 3]
        assert alpha.shape == (944,) and len(z) == 8 and all(v.shape == (944, 256) for v in z)
        # the same float64 operations on matrices of the same shapes; 1e-12 allows a BLAS another blocking
        assert float(np.abs(alpha - want).max()) <= 1e-12


def test_gradient_against_central_differences(sd, lattice):
    """Where no pre-activation changes sign between p - h and p + h along any axis the trunk is smooth, and the analytic chain is
    its derivative.  h = 2^-23: the truncation term h^2 / 6 |f'''| with |f'''| <= (2^9)^2 |f'| is 4e-9 |f'|, the rounding term
    eps |f| / h = 2e-9; held to 1e-6 (1 + |f'|)."""
    pin, h = lattice[2].astype(np.float64), 2.0 ** -23
    used = 0
    for m in ref.MODULES:
        z0 = mref.trunk(sd, m, pin)[1]
        grad = mref.trunk_gradient(sd, m, pin)
        smooth, cd = np.ones(len(pin), bool), np.zeros_like(grad)
        for ax in range(3):
            step = np.zeros(3)
            step[ax] = h
            (ap, zp), (am, zm) = mref.trunk(sd, m, pin + step), mref.trunk(sd, m, pin - step)
            cd[:, ax] = (ap - am) / (2 * h)
            for a, b, c in zip(z0, zp, zm):
                smooth &= np.all(((a > 0) == (b > 0)) & ((a > 0) == (c > 0)), axis=1)
        assert smooth.mean() > 0.9  # a sign change within 1e-7 of a lattice point is rare
        err = np.abs(grad - cd)[smooth] / (1.0 + np.abs(cd[smooth]))
        print("%s: %d smooth points, max |grad| %.1f, worst %.3e" % (m, smooth.sum(), np.abs(grad).max(), err.max()))
        assert err.max() <= 1e-6
        used += int(smooth.sum())
    assert used > 1000


def test_gradient_with_given_masks_is_the_default_with_its_own(sd, lattice):
    pin = lattice[2][:mref.N_GRAD]
    masks = [z > 0 for z in mref.trunk(sd, "model", pin)[1]]
    assert np.array_equal(mref.trunk_gradient(sd, "model", pin, masks), mref.trunk_gradient(sd, "model", pin))
    flipped = [m.copy() for m in masks]
    flipped[3][:, :] = ~flipped[3]
    assert not np.array_equal(mref.trunk_gradient(sd, "model", pin, flipped), mref.trunk_gradient(sd, "model", pin))


def test_fixture_integrity(fx, sd, lattice):
    pts, inside, pin = lattice
    assert pts.shape == (16, 14, 12, 3) and int(inside.sum()) == int(fx["count"]) == 944 and 944 % 64 == 48
    shift = mref.centred_state_dict(pin)[1]
    assert np.array_equal(shift, fx["alpha_shift"])
    assert fx["cube_ref"].shape == (2, 36, 34, 32) and fx["cube_ref"].dtype == np.float32
    assert fx["grad_ref"].shape == (2, mref.N_GRAD, 3) and fx["grad_ref"].dtype == np.float32
    assert 0.0 < float(fx["e_ref_cube"]) < 1e-5 and 0.0 < float(fx["e_ref_grad"]) < 1e-3
    P = mref.PAD
    for i, m in enumerate(ref.MODULES):
        alpha = mref.trunk(sd, m, pin)[0]
        iso, margin = mref.pick_iso(alpha)
        assert iso == float(fx["iso"][i]) != 0.0 and iso * 64 == round(iso * 64)
        assert margin == float(fx["iso_margin"][i]) >= mref.ISO_MARGIN
        share = float(np.mean(alpha > iso))
        assert 0.1 <= share <= 0.9 and share == float(fx["share_above"][i])
        cube = fx["cube_ref"][i].astype(np.float64)
        core = cube[P:-P, P:-P, P:-P]
        assert np.all(core[~inside] == 0) and np.count_nonzero(cube) == np.count_nonzero(core)
        assert float(np.abs(core[inside] - alpha).max()) <= float(fx["e_ref_cube"])
        assert float(np.abs(core[inside] - iso).min()) >= mref.ISO_MARGIN
        # the stored gradient against the float64 chain with the float64 model's masks: the masks can differ only at units within
        # fp32's reach of 0, which the recorded e_ref_grad (the reference's own masks) does not have to cover
        g64 = mref.trunk_gradient(sd, m, pin[:mref.N_GRAD])
        rows = np.abs(fx["grad_ref"][i] - g64).max(1) <= float(fx["e_ref_grad"])
        assert rows.mean() >= 0.9
    assert float(fx["iso"][0]) == -0.8125 and float(fx["iso"][1]) == 0.6875


def test_which_field_the_lattice_resolves(sd):
    """The premise of the GPU suite's sign check on field normals: face normals follow the lattice's differences, which side with
    the recipe field's gradient at under 0.6 of the points (its gradient lives at wavelengths of 0.012, the lattice steps by 0.08)
    and with the band-limited field's at nearly all."""
    raw = [mref.lattice_agreement(sd, m) for m in ref.MODULES]
    smooth = [mref.lattice_agreement(mref.band_limited(sd), m) for m in ref.MODULES]
    print("recipe field %s, band-limited %s" % (raw, smooth))
    assert max(raw) < 0.65 and min(smooth) > 0.99


def test_where_a_face_normal_is_the_field_s(sd):
    """The GPU suite's sign check takes its share over the vertices on lattice edges with both ends inside: the others lie on the
    cut the carving makes, and on this lattice they are most of the surface.  Emulated in float64 for that test's very case."""
    smooth = mref.band_limited(sd)
    iso = float(np.float32(np.median(mref.trunk(smooth, "model_fine", mref.lattice()[0][mref.lattice()[1]])[0])))
    inner, sides = mref.crossing_emulation(smooth, "model_fine", iso)
    print("%d crossings, %d inner; share over all %.3f, over the inner %.3f" % (len(inner), inner.sum(), sides.mean(), sides[inner].mean()))
    assert len(inner) == 658 and inner.sum() == 222 and sides.mean() < 0.6 and sides[inner].mean() >= 0.99
    inner, sides = mref.crossing_emulation(sd, "model_fine", 0.6875)  # the recipe's field: unresolved, whatever the vertices
    assert len(inner) == 420 and sides[inner].mean() < 0.6


_CFG = dict(mesh_th=0.6875, N_importance=128)


def _cpu_net():
    from neuralbody_amd.nerf import NerfNetwork

    return NerfNetwork(precision="f32").eval()


def test_plugin_loads_and_reads_the_live_cfg():
    cfg = types.SimpleNamespace(**_CFG)
    plugin = hp.load_plugin("volume_mesh_renderer.py", cfg)
    from neuralbody_amd.nerf import NerfMeshRenderer

    r = plugin.Renderer(_cpu_net())
    assert isinstance(r, NerfMeshRenderer) and r.model() == "fine" and r.cfg.mesh_th == 0.6875
    assert (r.cfg.mesh_backend, r.cfg.mesh_components, r.cfg.mesh_color, r.cfg.mesh_normals) == ("auto", "all", False, "faces")
    cfg.N_importance, cfg.mesh_th, cfg.mesh_color, cfg.mesh_normals = 0, 5, True, "field"  # read at call time
    assert r.model() == "" and r.cfg.mesh_th == 5.0 and r.cfg.mesh_color is True and r.cfg.mesh_normals == "field"


def test_plugin_refuses_a_bad_backend_and_bad_normals():
    cfg = types.SimpleNamespace(mesh_backend="host", **_CFG)
    r = hp.load_plugin("volume_mesh_renderer.py", cfg).Renderer(_cpu_net())
    with pytest.raises(ValueError, match="mesh_backend"):
        r.render({})
    with pytest.raises(ValueError, match="normals"):
        r.extract_mesh({}, cube=torch.zeros(4, 4, 4), normals="vertex")
    from neuralbody_amd.nerf import NerfMeshConfig, NerfMeshRenderer

    with pytest.raises(ValueError, match="normals"):
        NerfMeshRenderer(_cpu_net(), NerfMeshConfig()).extract_mesh({}, cube=torch.zeros(4, 4, 4), colors=True, normals="smooth")


def test_network_refuses_bad_shapes_and_training_mode():
    net = _cpu_net()
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"\[n,3\]"):
            net.density(torch.zeros(4, 1, 3))
        with pytest.raises(ValueError, match=r"\[n,3\]"):
            net.density_gradient(torch.zeros(3))
    net.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        net.density(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="inference only"):
        net.density_gradient(torch.zeros(4, 3))


def test_entry_points_are_declared_and_exported():
    from neuralbody_amd import _lib, ops

    names = {"nb_nerf_density", "nb_nerf_embed_grad"}
    assert names <= set(_lib.header_functions()) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.nb_abi_version() == _lib.ABI_VERSION  # additive: the version stays
    with open(_lib.HEADER) as f:
        assert "#define NB_NERF_TAP_PTS %d " % ops.NERF_TAP["pts"][0] in f.read()
    # the argument checks that need no device: a refused precision and sizes
    assert L.nb_nerf_density(None, None, 5, None, 1, None) != 0 and b"precision" in L.nb_last_error()
    assert L.nb_nerf_density(None, None, -1, None, 0, None) != 0
    assert L.nb_nerf_density(None, None, 0, None, 0, None) == 0 and L.nb_nerf_density(None, None, 0, None, 2, None) == 0
    assert L.nb_nerf_density(None, None, 5, None, 0, None) != 0 and b"NULL" in L.nb_last_error()
    assert L.nb_nerf_embed_grad(None, 64, None, 64, 0, None, None) == 0
    assert L.nb_nerf_embed_grad(None, 62, None, 64, 0, None, None) != 0 and b"stride" in L.nb_last_error()
    assert L.nb_nerf_embed_grad(None, 64, None, 64, 3, None, None) != 0 and b"NULL" in L.nb_last_error()


def test_gradient_chunk_rule():
    from neuralbody_amd import ops
    from neuralbody_amd.nerf import NerfNetwork

    per_point = 4 * (ops.NERF_TAP_COLS + ops.NERF_DTAP_COLS)
    assert NerfNetwork.GRADIENT_CHUNK_BYTES == 1 << 30 and NerfNetwork.GRADIENT_CHUNK_BYTES // per_point == 54120
