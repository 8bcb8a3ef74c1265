"""Host side of mesh extraction: the numpy restatement of nb_marching_cubes (tests/mc_ref.py) pinned by properties that do not
involve the case table's content (a table error would be common to the restatement and the kernel), TriMesh.export, the
evaluator / visualizer drop-ins, and the ABI surface of the new entry points."""
import ctypes as C
import math
import os
import struct
import types

import numpy as np
import pytest
import torch

from tests import mc_ref

FIELDS = mc_ref.fields()


@pytest.fixture(scope="module")
def meshes():
    return {k: mc_ref.marching_cubes(c, iso) for k, (c, iso) in FIELDS.items()}


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_mesh_is_a_closed_oriented_manifold(meshes, name):
    v, t = meshes[name]
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape[1] == 3 and t.shape[1] == 3
    assert len(t) > 0 and t.min() == 0 and t.max() == len(v) - 1
    assert len(np.unique(t)) == len(v)  # every vertex is used
    assert mc_ref.is_closed_oriented_manifold(t)
    assert np.isfinite(v).all()
    cube = FIELDS[name][0]
    assert (v >= 0).all() and (v <= np.array(cube.shape, np.float32) - 1).all()


def test_noise_field_holds_every_case():
    cube, iso = FIELDS["noise"]
    seen = set(np.unique(mc_ref.case_index(cube, iso)).tolist())
    assert seen >= set(range(1, 255)), sorted(set(range(1, 255)) - seen)


def test_euler_characteristic():
    for name, chi in (("sphere", 2), ("torus", 0)):
        v, t = mc_ref.marching_cubes(*FIELDS[name])
        assert mc_ref.euler_characteristic(v, t) == chi, name


def test_sphere_vertices_lie_on_the_sphere_within_the_interpolation_bound():
    """Along a lattice edge the second derivative of |p - c| is at most 1 / |p - c|, and every point of a crossed edge is at
    least R - 1 from c, so the linear interpolant of the exact field is off by at most h^2 / 8 * 1 / (R - 1) = 1 / (8 (R - 1))
    lattice units of field value, i.e. of radius (|grad| = 1).  On top: the fp32 rounding of the two field values moves the
    interpolant by at most 2^-24 max|f| <= 2^-24 sqrt(3) M (M = the largest side), the fp32 rounding of the stored vertex moves it
    by at most 2^-24 M per coordinate, sqrt(3) 2^-24 M in all; the fp64 arithmetic in between is below 1e-12."""
    s = mc_ref.SPHERE
    v, t = mc_ref.marching_cubes(*FIELDS["sphere"])
    M = max(s["shape"])
    tol = 1.0 / (8.0 * (s["R"] - 1.0)) + 2.0 ** -24 * math.sqrt(3.0) * M + 2.0 ** -24 * math.sqrt(3.0) * M + 1e-12
    r = np.linalg.norm(v.astype(np.float64) - np.array(s["c"]), axis=1)
    err = float(np.abs(r - s["R"]).max())
    print("sphere: max | |v - c| - R | = %.3e, bound %.3e" % (err, tol))
    assert err <= tol


def test_normals_point_outwards():
    s, to = mc_ref.SPHERE, mc_ref.TORUS
    v, t = mc_ref.marching_cubes(*FIELDS["sphere"])
    vol = mc_ref.signed_volume(v, t)
    assert 0.9 * 4 / 3 * math.pi * s["R"] ** 3 < vol < 4 / 3 * math.pi * s["R"] ** 3  # inscribed-ish polyhedron, outward normals
    v, t = mc_ref.marching_cubes(*FIELDS["torus"])
    vol = mc_ref.signed_volume(v, t)
    assert 0.9 * 2 * math.pi ** 2 * to["R"] * to["r"] ** 2 < vol < 1.02 * 2 * math.pi ** 2 * to["R"] * to["r"] ** 2
    for name in ("golden", "noise"):
        v, t = mc_ref.marching_cubes(*FIELDS[name])
        assert mc_ref.signed_volume(v, t) > 0, name
    # per triangle on the sphere: the normal points away from the centre
    v, t = mc_ref.marching_cubes(*FIELDS["sphere"])
    v = v.astype(np.float64)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    g = v[t].mean(1) - np.array(s["c"])
    ok = np.einsum("ij,ij->i", n, g) > 0
    assert ok[np.linalg.norm(n, axis=1) > 1e-9].all()


def test_equal_to_iso_is_outside_and_empty_results():
    cube = np.zeros((4, 4, 4), np.float32)
    cube[1:3, 1:3, 1:3] = 1.0
    v, t = mc_ref.marching_cubes(cube, 1.0)  # nothing is > 1
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == np.float32 and t.dtype == np.int32
    v, t = mc_ref.marching_cubes(cube, 2.0)  # iso above the maximum
    assert v.shape == (0, 3) and t.shape == (0, 3)
    cube[2, 2, 2] = 1.5  # one inside point; its three lower neighbours EQUAL iso and are outside: t = 0 puts the vertices ON them
    v, t = mc_ref.marching_cubes(cube, 1.0)
    assert len(v) == 6 and len(t) == 8 and mc_ref.is_closed_oriented_manifold(t)
    third = np.float32(2.0 + (1.0 - 1.5) / (0.0 - 1.5))  # the upper neighbours are 0
    want = np.array([[1, 2, 2], [2, 1, 2], [2, 2, 1], [third, 2, 2], [2, third, 2], [2, 2, third]], np.float32)
    assert np.array_equal(v, want)  # and in (owner point, axis) order
    nan = np.full((3, 3, 3), np.nan, np.float32)  # NaN is outside
    assert mc_ref.marching_cubes(nan, 0.0)[1].shape == (0, 3)


def test_vertex_order():
    v, t = mc_ref.marching_cubes(*FIELDS["golden"])
    cube = FIELDS["golden"][0]
    # vertices: by (owner point, axis): the owner is floor(v) except on the moving axis, where t may reach 1 only by rounding
    owner = np.floor(v.astype(np.float64)).astype(np.int64)
    lin = (owner[:, 0] * cube.shape[1] + owner[:, 1]) * cube.shape[2] + owner[:, 2]
    frac = (v != np.floor(v))
    assert (frac.sum(1) <= 1).all()
    exact = frac.sum(1) == 1
    key = 3 * lin[exact] + np.argmax(frac[exact], 1)
    assert (np.diff(key) > 0).all()


def _read_ply(path):
    """Minimal reader of the binary little-endian PLY TriMesh.export writes."""
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert [ln for ln in lines if ln.startswith("property")] == ["property float x", "property float y", "property float z",
                                                                  "property list uchar int vertex_indices"]
    verts = np.frombuffer(body, "<f4", 3 * nv).reshape(nv, 3)
    faces, off = np.zeros((nf, 3), np.int64), 12 * nv
    for i in range(nf):
        n, a, b, c = struct.unpack_from("<Biii", body, off)
        assert n == 3
        faces[i], off = (a, b, c), off + 13
    assert off == len(body)
    return verts, faces


def test_trimesh_export_round_trip(tmp_path):
    from neuralbody_amd.mesh import TriMesh

    v, t = mc_ref.marching_cubes(*FIELDS["sphere"])
    mesh = TriMesh(v.astype(np.float64), t)
    assert mesh.vertices.dtype == np.float64 and mesh.faces.shape == t.shape
    path = mesh.export(str(tmp_path / "0007.ply"))
    rv, rf = _read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, t)
    empty = TriMesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    rv, rf = _read_ply(empty.export(str(tmp_path / "empty.ply")))
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.export(str(tmp_path / "mesh.obj"))


def test_evaluator_and_visualizer_drop_ins(tmp_path):
    """lib/evaluators/if_nerf_mesh.py:8-18 and lib/visualizers/if_nerf_mesh.py:26-34 on the dict RendererMesh.render returns."""
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_io import MeshEvaluator, MeshVisualizer
    from tests import helpers as H

    rng = np.random.RandomState(0)
    cube = np.pad(rng.rand(5, 6, 7) * 10.0, 10)  # the float64 ndarray of render()
    pts = rng.rand(1, 5, 6, 7, 3).astype(np.float32)
    cfg = types.SimpleNamespace(mesh_th=5.0, result_dir=str(tmp_path / "res"))
    want = pts[0][cube[10:-10, 10:-10, 10:-10] > 5.0]  # the reference's expression
    ev = MeshEvaluator(cfg)
    path = ev.evaluate({"cube": cube}, {"pts": torch.from_numpy(pts), "i": torch.tensor([3])})
    assert path == os.path.join(cfg.result_dir, "pts", "3.npy") and np.array_equal(np.load(path), want)
    assert ev.summarize() == {}
    v, t = mc_ref.marching_cubes(cube.astype(np.float32), 5.0)
    vis = MeshVisualizer(cfg)
    path = vis.visualize({"cube": cube, "mesh": TriMesh(v, t)}, {"frame_index": torch.tensor([12])})
    assert path == os.path.join(cfg.result_dir, "mesh", "0012.ply")
    rv, rf = _read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, t)
    # the plugin file binds both to the reference's cfg at call time
    live = types.SimpleNamespace(mesh_th=5.0, result_dir=str(tmp_path / "live"))
    mod = H.load_plugin("if_nerf_mesh.py", live)
    ev, vis = mod.Evaluator(), mod.Visualizer()
    live.mesh_th = 7.0
    path = ev.evaluate({"cube": cube}, {"pts": torch.from_numpy(pts), "i": torch.tensor([0])})
    assert np.array_equal(np.load(path), pts[0][cube[10:-10, 10:-10, 10:-10] > 7.0])
    assert vis.visualize({"mesh": TriMesh(v, t)}, {"frame_index": torch.tensor([1])}).endswith(os.path.join("live", "mesh", "0001.ply"))


def test_render_config_and_live_cfg_carry_mesh_backend(monkeypatch):
    import sys

    from neuralbody_amd.renderer import RenderConfig, RendererMesh
    from tests import helpers as H

    assert RenderConfig().mesh_backend == "auto" and RenderConfig(mesh_backend="device").mesh_backend == "device"
    live = types.SimpleNamespace(N_samples=64, perturb=0.0, raw_noise_std=0.0, white_bkgd=False, H=8, W=8, ratio=1.0, mesh_th=5.0)
    # if_mesh_renderer.py imports _LiveCfg from the package module if_clight_renderer, which binds `lib.config.cfg` on import:
    # import it afresh against the stand-in cfg and put back whatever was there, so no other test sees this one's cfg
    monkeypatch.setitem(sys.modules, "neuralbody_amd.plugins.if_clight_renderer", None)  # remembers what was there
    del sys.modules["neuralbody_amd.plugins.if_clight_renderer"]
    mod = H.load_plugin("if_mesh_renderer.py", live)
    rend = mod.Renderer(None)
    assert isinstance(rend, RendererMesh) and rend.cfg.mesh_backend == "auto"
    live.mesh_backend = "device"
    assert rend.cfg.mesh_backend == "device"
    with pytest.raises(ValueError):
        RendererMesh(None, RenderConfig(mesh_backend="host")).render({})


def test_abi_surface_and_refusals():
    from neuralbody_amd import _lib, build, ops

    build.build(verbose=False)
    L = _lib.lib()
    names = set(_lib.header_functions())
    assert {"nb_marching_cubes_scratch_size", "nb_marching_cubes_count", "nb_marching_cubes_emit"} <= names
    assert L.nb_abi_version() == 20  # additive entry points: the version stays
    i3 = lambda *d: (C.c_int32 * 3)(*d)  # noqa: E731
    n = 33 * 17 * 70
    size = L.nb_marching_cubes_scratch_size(i3(33, 17, 70))
    assert size >= 32 * n and size % 256 == 0
    for bad in ((1, 5, 5), (5, 0, 5), (5, 5, 1), (-3, 4, 4), (1024, 1024, 683), (65536, 65536, 2)):
        assert L.nb_marching_cubes_scratch_size(i3(*bad)) == 0, bad
    assert L.nb_marching_cubes_scratch_size(i3(1024, 1024, 682)) > 0  # 3 * 2^20 * 682 < 2^31
    # refused dims and NULL pointers return an error code before anything touches a device
    assert L.nb_marching_cubes_count(None, i3(1, 5, 5), 0.0, None, None, None) != 0
    assert b"dims" in L.nb_last_error()
    assert L.nb_marching_cubes_count(None, i3(4, 4, 4), 0.0, None, None, None) != 0
    assert L.nb_marching_cubes_emit(None, i3(4, 4, 4), 0.0, None, None, 0, 0, None, None) != 0
    assert L.nb_marching_cubes_emit(None, i3(4, 4, 1), 0.0, None, None, 0, 0, None, None) != 0
    # CPU tensors are rejected like everywhere else in ops.py
    with pytest.raises(ops.NbError):
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.5)
