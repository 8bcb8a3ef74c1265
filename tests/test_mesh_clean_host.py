"""The host side of the mesh clean-up and the vertex colours: the numpy / scipy restatement (tests/mesh_clean_ref.py) against
hand-written cases, the new entries in the header and the ctypes table, and TriMesh's colours through export / load_ply."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mesh_clean_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_mesh_clean_scratch_size", "nb_mesh_components", "nb_mesh_component_select", "nb_mesh_compact_count", "nb_mesh_compact",
           "nb_mesh_color_query", "nb_mesh_color_finish", "nb_mesh_render_attr")


# ---------------------------------------------------------------------------------------------------------- restatement
def test_labels_of_hand_written_meshes():
    faces, V = ref.cases()["two_tetrahedra"]
    assert ref.components(faces, V).tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    # a bridge face makes them one; an unused vertex is its own component
    assert ref.components(np.concatenate([faces, [[3, 4, 5]]]), 9).tolist() == [0] * 8 + [8]
    # the smallest index names the component wherever it sits
    assert ref.components([[5, 2, 7], [7, 1, 6]], 8).tolist() == [0, 1, 1, 3, 4, 1, 1, 1]
    for name in ("strip_permuted", "strip_ascending"):
        f, V = ref.cases()[name]
        assert V == 4098 and len(f) == 4096 and not ref.components(f, V).any()
    assert ref.cases()["strip_permuted"][0][-1].tolist()[-1] == 0  # vertex 0 at the far end
    f, V = ref.cases()["many_components"]
    label = ref.components(f, V)
    assert ref.n_components_with_faces(f, V) == 300 and len(np.unique(label)) == 350
    sizes = np.bincount(label[f[:, 0]])
    assert sizes[sizes > 0].min() >= 1 and sizes.max() <= 40
    f, V = ref.cases()["bad_faces"]
    assert (~ref.valid_faces(f, V)).sum() == 5 and ref.components(f, V).tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    assert ref.components(np.zeros((0, 3), np.int32), 3).tolist() == [0, 1, 2]
    assert ref.components(np.zeros((1, 3), np.int32), 1).tolist() == [0]


def test_select_rule():
    faces, V = ref.cases()["two_tetrahedra"]
    label = ref.components(faces, V)
    keep, stats = ref.select(label, faces, 1.0)  # a tie: the smaller label
    assert keep.tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and stats.tolist() == [2, 1, 4, 4]
    keep, stats = ref.select(label, faces, 0.99)  # the threshold rule keeps both
    assert keep.all() and stats.tolist() == [2, 2, 4, 8]
    f, V = ref.sized_components([100, 50, 49], gap=1)
    label = ref.components(f, V)
    keep, stats = ref.select(label, f, 0.5)
    assert stats.tolist() == [3, 2, 100, 150]
    assert keep[:102].all() and not keep[102] and keep[103:155].all() and not keep[155:].any()
    assert ref.select(label, f, 0.4875)[1].tolist() == [3, 3, 100, 199]  # ceil(48.75) = 49 (the fraction is an fp32: 0.4875 is not
    assert ref.select(label, f, 0.49)[1].tolist() == [3, 2, 100, 150]    # exact, 0.49 rounds up to 0.49000001 and asks for 50)
    assert ref.select(label, f, 1e-6)[1].tolist() == [3, 3, 100, 199]  # ceil(...) = 1: every component that has a face
    # no face, no component to keep
    keep, stats = ref.select(np.arange(4), np.zeros((0, 3), np.int32), 1.0)
    assert not keep.any() and not stats.any()


def test_compaction_keeps_the_order_and_renumbers():
    verts = np.arange(27, dtype=np.float32).reshape(9, 3)
    faces = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 7], [2, 1, 3], [0, 9, 1], [4, 0, 5]], np.int32)
    keep = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0], np.uint8)
    v, f, a = ref.compact(verts, faces, keep, attr=-verts)
    assert np.array_equal(v, verts[4:8]) and np.array_equal(a, -verts[4:8])
    assert f.tolist() == [[0, 1, 2], [2, 1, 3], [0, -1, 1]]  # in order; the index of a dropped vertex becomes -1
    v, f = ref.compact(verts, faces, np.ones(9, np.uint8))
    assert np.array_equal(v, verts) and f.tolist() == faces[[0, 1, 2, 3, 5]].tolist()  # the face with index 9 does not survive
    v, f = ref.compact(verts, faces, np.zeros(9, np.uint8))
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_lib_binds_the_new_entries():
    from neuralbody_amd import _lib

    names = _lib.header_functions()
    for fn in ENTRIES:
        assert fn in names and fn in _lib.SIGNATURES, fn
    with open(_lib.HEADER) as f:
        src = f.read()
    assert "#define NB_ABI_VERSION 20\n" in src and _lib.ABI_VERSION == 20  # purely additive
    assert "#define NB_EINTERNAL (-4)" in src and _lib.EINTERNAL == ref.EINTERNAL == -4
    assert "#define NB_MESH_HOOK_ROUNDS 4\n" in src
    assert _lib.SIGNATURES["nb_mesh_render_attr"] == _lib.SIGNATURES["nb_mesh_render"]
    assert _lib.SIGNATURES["nb_mesh_clean_scratch_size"] == (C.c_int64, [C.c_int32, C.c_int32])
    lib = _lib.lib()
    for fn in ENTRIES:
        assert hasattr(lib, fn), fn
    assert lib.nb_abi_version() == 20
    # sizes: a header, three arrays per vertex, one per face and the two scans' tile sums; refused sizes give 0
    assert lib.nb_mesh_clean_scratch_size(0, 0) == 256
    assert lib.nb_mesh_clean_scratch_size(1000, 2000) >= 256 + 4 * (3 * 1000 + 2000)
    assert lib.nb_mesh_clean_scratch_size(-1, 0) == 0 and lib.nb_mesh_clean_scratch_size(0, -1) == 0
    assert lib.nb_mesh_clean_scratch_size(2 ** 31 - 256, 0) == 0 and lib.nb_mesh_clean_scratch_size(2 ** 31 - 257, 0) > 0


def test_ops_and_interfaces_are_there():
    import inspect

    from neuralbody_amd import ops
    from neuralbody_amd.mesh_render import MeshTurntable
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    for fn in ("mesh_components", "mesh_component_select", "mesh_compact", "mesh_vertex_colors", "mesh_render_attr"):
        assert callable(getattr(ops, fn)), fn
    assert ops.mesh_components_fraction("all") is None and ops.mesh_components_fraction("largest") == 1.0
    assert ops.mesh_components_fraction(0.25) == 0.25 and ops.mesh_components_fraction(1) == 1.0
    for bad in ("biggest", 0.0, 1.5, -0.1, True):
        with pytest.raises(ValueError):
            ops.mesh_components_fraction(bad)
    p = inspect.signature(RendererMesh.extract_mesh).parameters
    assert p["components"].default == "all" and p["colors"].default is False and p["world"].default is False
    assert inspect.signature(MeshTurntable.render).parameters["colors"].default is False
    cfg = RenderConfig()
    assert cfg.mesh_components == "all" and cfg.mesh_color is False  # off unless set


def test_plugins_read_the_new_keys_at_call_time_and_default_to_off(tmp_path, monkeypatch):
    import sys
    import types

    from neuralbody_amd.mesh import TriMesh
    from tests import helpers as H

    live = types.SimpleNamespace(N_samples=64, perturb=0.0, raw_noise_std=0.0, white_bkgd=False, H=8, W=8, ratio=1.0, mesh_th=5.0,
                                 result_dir=str(tmp_path))
    # if_mesh_renderer.py imports the package module if_clight_renderer, which binds `lib.config.cfg` on import: import it afresh
    # against the stand-in and put back whatever was there, so no other test sees this one's cfg (as tests/test_mesh_host.py does)
    monkeypatch.setitem(sys.modules, "neuralbody_amd.plugins.if_clight_renderer", None)
    del sys.modules["neuralbody_amd.plugins.if_clight_renderer"]
    rend = H.load_plugin("if_mesh_renderer.py", live).Renderer(None)
    assert rend.cfg.mesh_components == "all" and rend.cfg.mesh_color is False
    live.mesh_components, live.mesh_color = 0.25, True
    assert rend.cfg.mesh_components == 0.25 and rend.cfg.mesh_color is True
    vis = H.load_plugin("if_nerf_mesh.py", live).Visualizer()
    assert vis.cfg.mesh_render_color is False and vis.cfg.mesh_render is False
    live.mesh_render_color = True
    assert vis.cfg.mesh_render_color is True
    # the colour turntable of a mesh without colours is refused before anything is drawn
    v, f, _ = _mesh()
    vis.cfg.mesh_render_device = "cpu"  # the refusal comes before any device call
    with pytest.raises(ValueError, match="vertex_colors"):
        vis.visualize({"mesh": TriMesh(v, f)}, {"frame_index": np.array([0])})


# ---------------------------------------------------------------------------------------------------------- PLY
def _mesh():
    rng = np.random.RandomState(3)
    return rng.randn(7, 3), rng.randint(0, 7, (5, 3)), rng.randint(0, 256, (7, 3)).astype(np.uint8)


def test_colours_round_trip_through_the_ply(tmp_path):
    from neuralbody_amd.mesh import TriMesh

    v, f, c = _mesh()
    path = TriMesh(v, f, vertex_colors=c).export(str(tmp_path / "c.ply"))
    with open(path, "rb") as fh:
        data = fh.read()
    header = data[:data.index(b"end_header\n")].decode("ascii")
    assert ("property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "element face 5\n") in header
    assert len(data) == len(header) + len("end_header\n") + 7 * 15 + 5 * 13
    back = TriMesh.load_ply(path)
    assert back.vertex_colors.dtype == np.uint8 and np.array_equal(back.vertex_colors, c)
    assert np.array_equal(back.vertices, v.astype(np.float32).astype(np.float64)) and np.array_equal(back.faces, f)
    # a mesh without colours comes back without; other scalars are still skipped, also around the colours
    plain = TriMesh.load_ply(TriMesh(v, f).export(str(tmp_path / "p.ply")))
    assert plain.vertex_colors is None
    vd = np.zeros(7, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                            ("alpha", "u1")])
    vd["x"], vd["y"], vd["z"], vd["nx"], vd["alpha"] = v[:, 0], v[:, 1], v[:, 2], 5.0, 255
    vd["red"], vd["green"], vd["blue"] = c[:, 0], c[:, 1], c[:, 2]
    fd = np.zeros(5, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    fd["n"], fd["v"] = 3, f
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
           "property float nx\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
           "element face 5\nproperty list uchar int vertex_indices\nend_header\n")
    with open(tmp_path / "t.ply", "wb") as fh:
        fh.write(hdr.encode("ascii") + vd.tobytes() + fd.tobytes())
    other = TriMesh.load_ply(tmp_path / "t.ply")
    assert np.array_equal(other.vertex_colors, c) and np.array_equal(other.faces, f)
    # two of the three channels are no colour
    with open(tmp_path / "g.ply", "wb") as fh:
        fh.write(hdr.replace("uchar blue", "uchar bleu").encode("ascii") + vd.tobytes() + fd.tobytes())
    assert TriMesh.load_ply(tmp_path / "g.ply").vertex_colors is None
    for bad in (c[:6], c.astype(np.float32), c[:, :2]):
        with pytest.raises(ValueError):
            TriMesh(v, f, vertex_colors=bad)


def test_a_mesh_without_colours_exports_the_bytes_it_always_did(tmp_path):
    from neuralbody_amd.mesh import TriMesh

    v, f, _ = _mesh()
    path = TriMesh(v, f).export(str(tmp_path / "p.ply"))
    # the format string of TriMesh.export's docstring
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (7, 5)).encode("ascii")
    want += v.astype("<f4").tobytes()
    for face in f:
        want += b"\x03" + face.astype("<i4").tobytes()
    with open(path, "rb") as fh:
        assert fh.read() == want
    assert '"element face %d\\nproperty list uchar int vertex_indices\\nend_header\\n" % (V, T)' in TriMesh.export.__doc__
    assert TriMesh(v, f, vertex_colors=None).vertex_colors is None
