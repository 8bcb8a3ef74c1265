"""nb_marching_cubes on the device against its numpy restatement (tests/mc_ref.py): triangles equal as integer arrays, vertices
within one fp32 ulp (both sides evaluate the same correctly rounded fp64 expression and round once, so equality is expected),
bit-for-bit repeatability, the capacity check, and RendererMesh end to end without PyMCubes."""
import sys
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import mc_ref
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _shape_field(shape, seed):
    """Smooth-ish seeded field on a lattice whose sides are not multiples of the kernel's 4 x 4 x 64 block."""
    rng = np.random.RandomState(seed)
    return rng.rand(*shape).astype(np.float32)


CASES = dict(mc_ref.fields())
CASES.update({"33x17x70": (_shape_field((33, 17, 70), 1), 0.5), "2x2x2": (_shape_field((2, 2, 2), 2), 0.5),
              "2x65x3": (_shape_field((2, 65, 3), 3), 0.5), "5x9x131": (_shape_field((5, 9, 131), 4), 0.4)})


def _ulp_diff(a, b):
    """Largest distance in fp32 ulps between two non-negative finite fp32 arrays."""
    assert a.dtype == np.float32 and b.dtype == np.float32 and (a >= 0).all() and (b >= 0).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max(initial=0))


@pytest.mark.parametrize("name", sorted(CASES))
def test_marching_cubes_matches_restatement(name):
    from neuralbody_amd import ops

    cube, iso = CASES[name]
    rv, rt = mc_ref.marching_cubes(cube, iso)
    v, t = ops.marching_cubes(torch.from_numpy(cube).to(DEV), iso)
    torch.cuda.synchronize()
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    ulps = _ulp_diff(v, rv)
    print("%s: %d vertices, %d triangles, max vertex distance %d ulp, %d vertices differ" % (
        name, len(v), len(t), ulps, int((v != rv).any(1).sum())))
    assert np.array_equal(t, rt)
    assert ulps <= 1
    if name in mc_ref.fields():  # the surface does not reach the lattice's border there
        assert len(t) > 0 and mc_ref.is_closed_oriented_manifold(t)


def test_empty_and_equal_to_iso():
    from neuralbody_amd import ops

    cube = torch.zeros((4, 4, 4), device=DEV)
    cube[1:3, 1:3, 1:3] = 1.0
    for iso in (1.0, 2.0):  # equal counts as outside; iso above the maximum
        v, t = ops.marching_cubes(cube, iso)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.is_cuda and t.dtype == torch.int32
    nan = torch.full((3, 5, 4), float("nan"), device=DEV)
    assert tuple(ops.marching_cubes(nan, 0.0)[1].shape) == (0, 3)
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros((1, 4, 4), device=DEV), 0.5)
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros((4, 4), device=DEV), 0.5)


def test_two_calls_give_the_same_bits():
    from neuralbody_amd import ops

    cube, iso = CASES["noise"]
    cube = torch.from_numpy(cube).to(DEV)
    v0, t0 = ops.marching_cubes(cube, iso)
    v1, t1 = ops.marching_cubes(cube, iso)
    assert H.same_bits(v0, v1) and torch.equal(t0, t1)


def test_capacity_one_short_is_refused_and_writes_nothing():
    from neuralbody_amd import ops

    cube, iso = CASES["torus"]
    cube = torch.from_numpy(cube).to(DEV)
    scratch = ops.marching_cubes_scratch(cube.shape, cube.device)
    nv, nt = ops.marching_cubes_count(cube, iso, scratch).tolist()
    assert nv > 0 and nt > 0
    for dv, dt in ((1, 0), (0, 1)):
        verts = torch.full((nv - dv, 3), -7.0, device=DEV)
        tris = torch.full((nt - dt, 3), -7, dtype=torch.int32, device=DEV)
        with pytest.raises(ops.NbError):
            ops.marching_cubes_emit(cube, iso, scratch, verts, tris)
        torch.cuda.synchronize()
        assert bool((verts == -7.0).all()) and bool((tris == -7).all())
    # larger than needed is fine: the first nv / nt rows are written, the rest is left alone
    verts = torch.full((nv + 3, 3), -7.0, device=DEV)
    tris = torch.full((nt + 2, 3), -7, dtype=torch.int32, device=DEV)
    ops.marching_cubes_emit(cube, iso, scratch, verts, tris)
    rv, rt = mc_ref.marching_cubes(cube.cpu().numpy(), iso)
    assert np.array_equal(tris[:nt].cpu().numpy(), rt) and bool((tris[nt:] == -7).all()) and bool((verts[nv:] == -7.0).all())
    assert _ulp_diff(verts[:nv].cpu().numpy(), rv) <= 1


def _mesh_renderer(**cfg):
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    r, sd, batch = scenes.build_mesh()
    net = H.make_network(sd, DEV, True, "f32")
    return RendererMesh(net, RenderConfig(mesh_th=5.0, **cfg)), H.device_batch(batch, DEV), batch


def _check_render(out, rend, bd):
    from neuralbody_amd.mesh import TriMesh

    assert set(out) == {"cube", "mesh"}
    cube = out["cube"]
    with torch.no_grad():
        dev_cube = rend.density_cube(bd)
    assert isinstance(cube, np.ndarray) and cube.dtype == np.float64 and cube.shape == tuple(dev_cube.shape)
    assert np.array_equal(cube, dev_cube.double().cpu().numpy())
    mesh = out["mesh"]
    assert isinstance(mesh, TriMesh)  # trimesh is not installed where this suite runs
    rv, rt = mc_ref.marching_cubes(cube.astype(np.float32), 5.0)
    assert len(mesh.faces) > 0 and mc_ref.is_closed_oriented_manifold(mesh.faces)
    assert np.array_equal(mesh.faces, rt)
    assert mesh.vertices.dtype == np.float64 and _ulp_diff(mesh.vertices.astype(np.float32), rv) <= 1
    assert mc_ref.signed_volume(mesh.vertices, mesh.faces) > 0
    return rv, rt


def test_render_without_pymcubes_extracts_the_mesh_on_the_device(monkeypatch, tmp_path):
    rend, bd, batch = _mesh_renderer()
    monkeypatch.setitem(sys.modules, "mcubes", None)  # import mcubes raises ImportError
    monkeypatch.setitem(sys.modules, "trimesh", None)
    with torch.no_grad():
        out = rend.render(bd)
    rv, rt = _check_render(out, rend, bd)
    # world units: inside wbounds widened by the pad
    with torch.no_grad():
        wv, wt = rend.extract_mesh(bd, world=True)
        iv, it = rend.extract_mesh(bd)
    assert wv.is_cuda and wt.is_cuda and np.array_equal(wt.cpu().numpy(), rt) and torch.equal(wt, it)
    pts = batch["pts"][0]
    step = np.array([pts[1, 0, 0, 0] - pts[0, 0, 0, 0], pts[0, 1, 0, 1] - pts[0, 0, 0, 1], pts[0, 0, 1, 2] - pts[0, 0, 0, 2]])
    wb = batch["wbounds"][0]
    wv = wv.cpu().numpy()
    assert (wv >= wb[0] - 10 * step - 1e-6).all() and (wv <= wb[1] + 10 * step + 1e-6).all()
    np.testing.assert_allclose(wv, (iv.cpu().numpy() - 10.0) * step + wb[0], rtol=0, atol=1e-5)
    # and through the drop-ins of the reference's evaluator / visualizer
    from neuralbody_amd.mesh_io import MeshEvaluator, MeshVisualizer, occupied_points

    cfg = types.SimpleNamespace(mesh_th=5.0, result_dir=str(tmp_path))
    path = MeshEvaluator(cfg).evaluate(out, dict(bd, i=torch.tensor([4])))
    want = batch["pts"][0][out["cube"][10:-10, 10:-10, 10:-10] > 5.0]
    assert len(want) > 0 and np.array_equal(np.load(path), want)
    with torch.no_grad():
        assert np.array_equal(occupied_points(rend.density_cube(bd), bd["pts"][0], 5.0), want)  # selection on the device
    assert MeshVisualizer(cfg).visualize(out, bd).endswith("mesh/0000.ply")


def test_mesh_backend_device_overrides_an_importable_pymcubes(monkeypatch):
    rend, bd, _ = _mesh_renderer(mesh_backend="device")
    mc = types.ModuleType("mcubes")
    mc.marching_cubes = lambda c, th: pytest.fail("mesh_backend = 'device' must not call PyMCubes")
    monkeypatch.setitem(sys.modules, "mcubes", mc)
    monkeypatch.setitem(sys.modules, "trimesh", None)
    with torch.no_grad():
        out = rend.render(bd)
    _check_render(out, rend, bd)


def test_importable_pymcubes_is_still_what_render_calls(monkeypatch):
    """The host path of the reference survives unchanged wherever PyMCubes imports (the stub of tests/test_gpu_parity.py)."""
    rend, bd, _ = _mesh_renderer()
    mc, tm = types.ModuleType("mcubes"), types.ModuleType("trimesh")
    seen = {}

    def marching_cubes(c, th):
        seen["th"], seen["dtype"], seen["shape"] = th, c.dtype, c.shape
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)

    mc.marching_cubes = marching_cubes
    tm.Trimesh = lambda v, t: ("mesh", len(v), len(t))
    monkeypatch.setitem(sys.modules, "mcubes", mc)
    monkeypatch.setitem(sys.modules, "trimesh", tm)
    with torch.no_grad():
        out = rend.render(bd)
    assert out["mesh"] == ("mesh", 0, 0) and out["cube"].dtype == np.float64
    assert seen == {"th": 5.0, "dtype": np.float64, "shape": out["cube"].shape}
