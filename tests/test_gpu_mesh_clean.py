"""csrc/nb_mesh_clean.hip and nb_mesh_render_attr on the device, and the mesh pass above them.

Labels, flags, stats and compacted arrays are integers and copies: they must EQUAL the numpy / scipy restatement
(tests/mesh_clean_ref.py).  The colours are held to the oracle's restatement of latent_xyzc.py:91-126 at the same points
(helpers.RGB_TOL); wpts, rgb_u8 and nb_mesh_render_attr are exact and compared bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import mc_ref
from tests import mesh_clean_ref as ref
from tests import test_mesh_render_host as host
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -1414812757  # 0xABABABAB


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _clean(faces, V, components, attr=True):
    """components -> select -> compact of one mesh with made-up vertices, every output and the scratch poisoned first ->
    dict of host arrays and the give-up word."""
    from neuralbody_amd import ops

    tf = _dev(np.asarray(faces, np.int32).reshape(-1, 3))
    verts = np.arange(3 * V, dtype=np.float32).reshape(V, 3) * np.float32(0.25)
    scratch = ops.mesh_clean_scratch(V, len(tf), DEV).fill_(0xAB)
    label = ops.mesh_components(tf, V, out=torch.full((V,), POISON, dtype=torch.int32, device=DEV), scratch=scratch)
    out = {"label": _np(label), "give_up": int(ops.mesh_give_up(scratch).item())}
    if components is not None:
        keep, stats = ops.mesh_component_select(label, tf, components, keep=torch.full((V,), 0xAB, dtype=torch.uint8, device=DEV),
                                                stats=torch.full((4,), POISON, dtype=torch.int32, device=DEV), scratch=scratch)
        got = ops.mesh_compact(_dev(verts), tf, keep, attr=_dev(-verts) if attr else None, scratch=scratch)
        out.update(keep=_np(keep), stats=_np(stats), verts=_np(got[0]), faces=_np(got[1]), attr=_np(got[2]) if attr else None)
    out["verts_in"] = verts
    return out


def _check_against_restatement(faces, V, components, got):
    label = ref.components(faces, V)
    assert got["give_up"] == 0
    assert got["label"].dtype == np.int32 and np.array_equal(got["label"], label)
    if components is None:
        return
    keep, stats = ref.select(label, faces, 1.0 if components == "largest" else components)
    assert got["keep"].dtype == np.uint8 and np.array_equal(got["keep"], keep)
    assert np.array_equal(got["stats"], stats), (got["stats"], stats)
    v, f, a = ref.compact(got["verts_in"], faces, keep, attr=-got["verts_in"])
    assert _same(got["verts"], v) and _same(got["faces"], f) and _same(got["attr"], a)


# ---------------------------------------------------------------------------------------------------------- 1. components
@pytest.mark.parametrize("name", sorted(ref.cases()))
def test_components_equal_the_restatement_twice(name):
    faces, V = ref.cases()[name]
    first, again = _clean(faces, V, "largest"), _clean(faces, V, "largest")
    _check_against_restatement(faces, V, "largest", first)
    for k in ("label", "keep", "stats", "verts", "faces", "attr"):
        assert _same(first[k], again[k]), k
    n = len(np.unique(first["label"]))
    print("%s: V = %d, T = %d, %d labels, stats %s, give-up word %d" % (name, V, len(faces), n, first["stats"].tolist(), first["give_up"]))
    if name.startswith("strip"):
        assert n == 1 and first["label"][0] == 0  # one label, 0
    if name == "bad_faces":  # the 5 faces connect nothing and do not survive
        assert first["stats"].tolist() == [2, 1, 4, 4] and len(first["faces"]) == 4
    if name in ("no_faces", "one_vertex"):  # nothing has a face: nothing is kept
        assert first["stats"].tolist() == [0, 0, 0, 0] and first["verts"].shape == (0, 3) and first["faces"].shape == (0, 3)


def test_no_vertices_at_all():
    from neuralbody_amd import ops

    tf = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    label = ops.mesh_components(tf, 0)
    keep, stats = ops.mesh_component_select(label, tf, "largest")
    v, f = ops.mesh_compact(torch.zeros((0, 3), device=DEV), tf, keep)
    assert label.shape == (0,) and keep.shape == (0,) and stats.tolist() == [0, 0, 0, 0] and v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        ops.mesh_component_select(label, tf, 0.0)
    with pytest.raises(ValueError):
        ops.mesh_component_select(label, tf, "all")


# ---------------------------------------------------------------------------------------------------------- 2. select, compact
def test_equal_face_counts_the_smaller_label_wins():
    faces, V = ref.cases()["two_tetrahedra"]
    swapped = np.concatenate([faces[4:], faces[:4]])  # the larger labels' faces first: the order of the faces does not decide
    for f in (faces, swapped):
        got = _clean(f, V, "largest")
        _check_against_restatement(f, V, "largest", got)
        assert got["keep"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and got["stats"].tolist() == [2, 1, 4, 4]
    got = _clean(faces, V, 1.0)  # the float 1.0 is "largest"
    assert got["stats"].tolist() == [2, 1, 4, 4]


@pytest.mark.parametrize("fraction,kept", [(0.5, 2), (0.4875, 3), (0.51, 1)])
def test_min_fraction_on_100_50_49(fraction, kept):
    faces, V = ref.sized_components([100, 50, 49], gap=1)  # an unused vertex behind each component
    got = _clean(faces, V, fraction)
    _check_against_restatement(faces, V, fraction, got)
    assert got["stats"].tolist() == [3, kept, 100, [100, 150, 199][kept - 1]]
    # unused vertices are dropped, and the attribute travelled with its vertex
    assert len(got["verts"]) == [102, 154, 205][kept - 1] and _same(got["attr"], -got["verts"])
    assert got["faces"].min() == 0 and got["faces"].max() == len(got["verts"]) - 1


def test_flags_of_the_callers_own_and_a_dropped_second_vertex():
    from neuralbody_amd import ops

    verts = np.arange(27, dtype=np.float32).reshape(9, 3)
    faces = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 7], [2, 1, 3], [0, 9, 1], [4, 0, 5]], np.int32)
    keep = np.array([0, 0, 0, 0, 1, 1, 1, 7, 0], np.uint8)  # any non-zero flag keeps
    v, f = ops.mesh_compact(_dev(verts), _dev(faces), _dev(keep))  # a scratch of its own: the give-up word starts at 0
    rv, rf = ref.compact(verts, faces, keep)
    assert _same(_np(v), rv) and _same(_np(f), rf) and rf.tolist() == [[0, 1, 2], [2, 1, 3], [0, -1, 1]]
    v, f, a = ops.mesh_compact(_dev(verts), _dev(faces), _dev(np.ones(9, np.uint8)), attr=_dev(verts + 1))
    assert _same(_np(v), verts) and _same(_np(a), verts + 1) and _same(_np(f), faces[[0, 1, 2, 3, 5]])


def test_capacity_one_short_is_refused_and_writes_nothing():
    from neuralbody_amd import _lib, ops

    faces, V = ref.cases()["many_components"]
    tf = _dev(faces)
    verts = _dev(np.arange(3 * V, dtype=np.float32).reshape(V, 3))
    scratch = ops.mesh_clean_scratch(V, len(tf), DEV)
    label = ops.mesh_components(tf, V, scratch=scratch)
    keep, _ = ops.mesh_component_select(label, tf, 0.5, scratch=scratch)
    counts = ops.mesh_compact_count(tf, keep, scratch)
    nv, nt = counts.tolist()
    assert nv > 0 and nt > 0
    for dv, dt in ((1, 0), (0, 1)):
        vo = torch.full((nv - dv, 3), -7.0, device=DEV)
        to = torch.full((nt - dt, 3), -7, dtype=torch.int32, device=DEV)
        with pytest.raises(ops.NbError):
            ops.mesh_compact_emit(verts, tf, scratch, counts, vo, to)
        # the entry itself, handed buffers that are too small, writes nothing either: the counts are tested on the device
        rc = _lib.lib().nb_mesh_compact(_lib.ptr(verts), _lib.ptr(tf), None, V, len(tf), _lib.ptr(vo), _lib.ptr(to), None, nv - dv,
                                        nt - dt, _lib.ptr(scratch), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and bool((vo == -7.0).all()) and bool((to == -7).all())
    # larger than needed is fine: the first nv / nt rows are written, the rest is left alone
    vo = torch.full((nv + 3, 3), -7.0, device=DEV)
    to = torch.full((nt + 2, 3), -7, dtype=torch.int32, device=DEV)
    ops.mesh_compact_emit(verts, tf, scratch, counts, vo, to)
    rv, rf = ref.compact(_np(verts), faces, _np(keep))
    assert _same(_np(vo[:nv]), rv) and _same(_np(to[:nt]), rf) and bool((vo[nv:] == -7.0).all()) and bool((to[nt:] == -7).all())


def test_a_set_give_up_word_is_reported_and_nothing_is_written():
    """No input of this suite makes a hook give up, so the word is set by hand behind mesh_components: what reads it must report
    NB_EINTERNAL and write nothing."""
    from neuralbody_amd import _lib, ops

    faces, V = ref.cases()["two_tetrahedra"]
    tf = _dev(faces)
    scratch = ops.mesh_clean_scratch(V, len(tf), DEV)
    label = ops.mesh_components(tf, V, scratch=scratch)
    ops.mesh_give_up(scratch).fill_(1)
    keep = torch.full((V,), 0xAB, dtype=torch.uint8, device=DEV)
    _, stats = ops.mesh_component_select(label, tf, "largest", keep=keep, scratch=scratch)
    assert stats.tolist() == [_lib.EINTERNAL] * 4 and bool((keep == 0xAB).all())
    assert ops.mesh_compact_count(tf, keep, scratch).tolist() == [_lib.EINTERNAL] * 2
    with pytest.raises(ops.NbError, match="NB_EINTERNAL"):
        ops.mesh_compact(torch.zeros((V, 3), device=DEV), tf, keep, scratch=scratch)


# ---------------------------------------------------------------------------------------------------------- 3. marching cubes
@functools.lru_cache(maxsize=None)
def _scene():
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    _, sd, batch = scenes.build_mesh()
    rend = RendererMesh(H.make_network(sd, DEV, True, "f32"), RenderConfig(mesh_th=5.0))
    return rend, H.device_batch(batch, DEV), sd, batch


def _blobs():
    """28^3, iso 5: a sphere of radius 8, a sphere of radius 3 more than 3 cells away from it, one lattice point above the
    threshold near a corner -> (the cube with all three, the cube with the large sphere alone)."""
    g = np.stack(np.meshgrid(*[np.arange(28, dtype=np.float32)] * 3, indexing="ij"), -1)
    big = (np.float32(5 + 8) - np.linalg.norm(g - np.array([12.3, 13.1, 13.6], np.float32), axis=-1)).astype(np.float32)
    small = (np.float32(5 + 3) - np.linalg.norm(g - np.array([23.2, 5.4, 5.1], np.float32), axis=-1)).astype(np.float32)
    assert np.linalg.norm(np.array([12.3, 13.1, 13.6]) - np.array([23.2, 5.4, 5.1])) - 8 - 3 > 3
    both = np.maximum(big, small)  # within a cell of the large sphere's surface the small one's field is far below: the values there stay
    both[1, 26, 1] = 9.0
    return both.astype(np.float32), big


def test_largest_component_is_the_marching_cubes_mesh_of_the_large_sphere_alone():
    from neuralbody_amd import ops

    rend, bd, _, _ = _scene()
    both, alone = _blobs()
    tb = _dev(both)
    want_v, want_t = ops.marching_cubes(_dev(alone), 5.0)
    all_v, all_t = ops.marching_cubes(tb, 5.0)
    assert ref.n_components_with_faces(_np(all_t), len(all_v)) == 3 and ref.n_components_with_faces(_np(want_t), len(want_v)) == 1
    v, t = rend.extract_mesh(bd, cube=tb, components="largest")
    print("all: %d vertices, %d triangles; largest: %d, %d" % (len(all_v), len(all_t), len(v), len(t)))
    assert len(t) > 1000 and len(all_t) > len(t) + 8
    assert H.same_bits(v, want_v) and torch.equal(t, want_t)  # vertices, triangles and order
    assert mc_ref.is_closed_oriented_manifold(_np(t))
    # "all" is what it returns today: the same call, no further launch
    v0, t0 = rend.extract_mesh(bd, cube=tb)
    v1, t1 = rend.extract_mesh(bd, cube=tb, components="all")
    assert H.same_bits(v0, all_v) and torch.equal(t0, all_t) and H.same_bits(v1, all_v) and torch.equal(t1, all_t)
    # a fraction that lets the small sphere stay, but not the octahedron around the single point
    small_faces = np.sort(np.bincount(ref.components(_np(all_t), len(all_v))[_np(all_t)[:, 0]]))[-2]
    v2, t2 = rend.extract_mesh(bd, cube=tb, components=(small_faces - 0.5) / len(t))  # ceil(fraction * largest) = small_faces
    assert len(t2) == len(t) + small_faces and ref.n_components_with_faces(_np(t2), len(v2)) == 2
    with pytest.raises(ValueError):
        rend.extract_mesh(bd, cube=tb, components="biggest")


# ---------------------------------------------------------------------------------------------------------- 4. colours
@functools.lru_cache(maxsize=None)
def _coloured():
    rend, bd, sd, batch = _scene()
    with torch.no_grad():
        mesh = rend.extract_mesh(bd, colors=True)
        plain = rend.extract_mesh(bd)
    return mesh, plain


def test_colours_against_the_oracle_at_the_same_points():
    from oracle import neuralbody_oracle as orc

    rend, bd, sd, batch = _scene()
    mesh, plain = _coloured()
    assert H.same_bits(mesh.vertices, plain[0]) and torch.equal(mesh.triangles, plain[1]) and mesh[0] is mesh.vertices
    V = len(mesh.vertices)
    assert V > 100 and mesh.rgb_f.shape == (V, 3) and mesh.rgb_f.dtype == torch.float32 and mesh.rgb_u8.dtype == torch.uint8
    sdt, vols, out_sh = H.oracle_volumes(sd, batch, True)
    sp = {"R": torch.from_numpy(batch["R"]), "Th": torch.from_numpy(batch["Th"]), "bounds": torch.from_numpy(batch["bounds"]),
          "latent_index": torch.from_numpy(batch["latent_index"]), "out_sh": out_sh}
    with torch.no_grad():
        raw = orc.calculate_density_color(sdt, mesh.wpts.cpu()[None], mesh.viewdir.cpu()[None], vols, sp)[0]
        want = torch.sigmoid(raw[:, :3]).numpy()
    err = H.assert_close(_np(mesh.rgb_f), want, H.RGB_TOL, "rgb_f", rel=False)
    print("%d vertices: max |rgb_f - oracle| = %.3e (bound %.1e); colours span %.3f .. %.3f" % (
        V, err, H.RGB_TOL, float(mesh.rgb_f.min()), float(mesh.rgb_f.max())))
    assert float(mesh.rgb_f.max() - mesh.rgb_f.min()) > 0.05  # a constant would pass no information
    # rgb_u8 = rint(255 * rgb_f) of the device's own rgb_f, in fp32, half to even
    assert np.array_equal(_np(mesh.rgb_u8), np.rint(np.float32(255.0) * _np(mesh.rgb_f)).astype(np.uint8))


def test_wpts_and_viewdir_are_the_stated_expressions_bit_for_bit():
    from neuralbody_amd import ops

    rend, bd, _, batch = _scene()
    mesh, _ = _coloured()
    pts = batch["pts"][0]
    step = np.array([pts[1, 0, 0, 0] - pts[0, 0, 0, 0], pts[0, 1, 0, 1] - pts[0, 0, 0, 1], pts[0, 0, 1, 2] - pts[0, 0, 0, 2]], np.float32)
    origin = batch["wbounds"][0, 0].astype(np.float32)
    v = _np(mesh.vertices)
    assert pts.dtype == np.float32 and v.dtype == np.float32
    want = ((v - np.float32(10.0)) * step) + origin  # three fp32 operations per axis
    assert want.dtype == np.float32 and _same(_np(mesh.wpts), want)
    assert H.same_bits(mesh.wpts, rend._to_world(mesh.vertices, bd))  # the formula RendererMesh has for world=True
    # the normals are those of the world vertices, the direction looks at the surface from outside
    assert H.same_bits(mesh.normals, ops.mesh_vertex_normals(mesh.wpts, mesh.triangles))
    assert _same(_np(mesh.viewdir), -_np(mesh.normals)) and bool((mesh.normals.norm(dim=1) > 0.99).all())
    with torch.no_grad():
        world = rend.extract_mesh(bd, world=True, colors=True)
    assert H.same_bits(world.vertices, mesh.wpts) and H.same_bits(world.rgb_f, mesh.rgb_f)


def test_a_zero_normal_looks_down_minus_z_and_the_finish_rounds_half_to_even():
    from neuralbody_amd import ops

    verts = _dev(np.array([[10, 10, 10], [11, 10, 10], [10, 11, 10], [12, 12, 12]], np.float32))
    faces = _dev(np.array([[0, 1, 2]], np.int32))
    normals = ops.mesh_vertex_normals(verts, faces)
    step, origin = _dev(np.array([0.5, 0.25, 2.0], np.float32)), _dev(np.array([1.0, -2.0, 0.125], np.float32))
    wpts, viewdir = ops.mesh_color_query(verts, normals, step, origin, 10)
    assert _np(normals).tolist() == [[0, 0, 1]] * 3 + [[0, 0, 0]]
    assert _np(viewdir).tolist() == [[0, 0, -1]] * 4 and not np.signbit(_np(viewdir)[3, :2]).any()  # -n, and (0, 0, -1) for no normal
    assert _np(wpts).tolist() == [[1, -2, 0.125], [1.5, -2, 0.125], [1, -1.75, 0.125], [2, -1.5, 4.125]]
    raw = np.zeros((6, 4), np.float32)
    raw[:, 0] = [0.0, 40.0, -40.0, np.log(np.float32(2.5 / 252.5)), np.nan, 3.0]
    raw[:, 3] = 99.0  # the density is not looked at
    rgb_f, rgb_u8 = ops.mesh_color_finish(_dev(raw))
    f, u = _np(rgb_f), _np(rgb_u8)
    assert f[0, 0] == 0.5 and u[0, 0] == 128 and f[1, 0] == 1.0 and u[1, 0] == 255 and u[2, 0] == 0 and 0.0 <= f[2, 0] < 1e-17
    assert np.isnan(f[4, 0]) and u[4, 0] == 0 and (f[:, 1:] == 0.5).all()
    want = np.float32(1.0) / (np.float32(1.0) + np.exp(-raw[[3, 5], 0]))
    assert np.abs(f[[3, 5], 0] - want).max() <= 2 * np.finfo(np.float32).eps  # expf against numpy's: an ulp or two
    assert np.array_equal(u[[3, 5], 0], np.rint(np.float32(255.0) * f[[3, 5], 0]).astype(np.uint8))
    # (255 * 0.5 = 127.5 went to the even 128 above)
    empty = ops.mesh_color_finish(torch.zeros((0, 4), device=DEV))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------- 5. mesh_render_attr
def _two_triangles():
    """A large triangle and a smaller one in front of it, vertices shared by nothing."""
    v = np.array([[-0.3, 0.0, -0.4], [0.3, 0.05, -0.4], [0.0, -0.05, 0.45], [-0.1, 0.2, -0.1], [0.15, 0.25, -0.1], [0.0, 0.2, 0.2]], np.float32)
    return v, np.array([[0, 1, 2], [3, 5, 4]], np.int32)


@pytest.mark.parametrize("name", ["two_triangles", "ico80"])
def test_render_attr_fed_the_normal_shading_gives_mesh_renders_bits(name):
    from neuralbody_amd import ops

    v, f = _two_triangles() if name == "two_triangles" else host.mesh("ico80")
    cams = host.cams_of(v, 32, 32)[list(host.BAND_VIEWS)]
    tv, tf, tc = _dev(v), _dev(f), _dev(cams)
    normals = ops.mesh_vertex_normals(tv, tf)
    want = ops.mesh_render(tv, normals, tf, tc, 32, 32, want_face_id=True, want_depth=True)
    n = _np(normals)
    covered = 0
    for k in range(3):
        N = cams[k, 12:21].reshape(3, 3)
        # 0.5 (*) (N . n) (+) 0.5 on the host in fp32, in the order include/nb_hip.h states
        attr = np.stack([np.float32(0.5) * ((N[i, 0] * n[:, 0] + N[i, 1] * n[:, 1]) + N[i, 2] * n[:, 2]) + np.float32(0.5) for i in range(3)], 1)
        assert attr.dtype == np.float32
        got = ops.mesh_render_attr(tv, _dev(attr), tf, tc[k:k + 1], 32, 32, want_face_id=True, want_depth=True)
        for what, g, w in zip(("rgb", "face_id", "depth"), got, want):
            assert H.same_bits(g[0], w[k]), (name, k, what)
        covered += int((got[1] >= 0).sum())
    print("%s: %d covered pixels in 3 views" % (name, covered))
    assert covered > 100
    # a constant attribute gives that constant on every covered pixel and white elsewhere
    const = torch.tensor([0.25, 0.5, 0.75], device=DEV).repeat(len(v), 1).contiguous()
    dirty = torch.full((3, 32, 32, 3), float("nan"), device=DEV)
    rgb, fid = ops.mesh_render_attr(tv, const, tf, tc, 32, 32, out=dirty, want_face_id=True)
    assert rgb is dirty and torch.equal(fid, want[1])
    assert bool((rgb[fid >= 0] == const[0]).all()) and bool((rgb[fid < 0] == 1.0).all())


# ---------------------------------------------------------------------------------------------------------- 6. end to end
def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_visualizer_writes_a_clean_coloured_ply_and_both_picture_sets(tmp_path):
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_io import MeshVisualizer
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    rend0, bd, _, _ = _scene()
    rend = RendererMesh(rend0.net, RenderConfig(mesh_th=5.0, mesh_components="largest", mesh_color=True))
    with torch.no_grad():
        out = rend.render(bd)
    assert set(out) == {"cube", "mesh"} and isinstance(out["mesh"], TriMesh) and out["cube"].dtype == np.float64
    cfg = types.SimpleNamespace(result_dir=str(tmp_path), mesh_render=True, mesh_render_color=True, mesh_render_size=(48, 40))
    path = MeshVisualizer(cfg).visualize(out, bd)
    back = TriMesh.load_ply(path)
    assert back.vertex_colors is not None and back.vertex_colors.shape == (len(back.vertices), 3) and len(back.faces) > 0
    assert ref.n_components_with_faces(back.faces, len(back.vertices)) == 1 and not (ref.components(back.faces, len(back.vertices)) != 0).any()
    # the vertices are the restatement's choice among all the scene's; the colours are extract_mesh's for that mesh
    _, (all_v, all_t) = _coloured()
    label = ref.components(_np(all_t), len(all_v))
    want_v, want_t = ref.compact(_np(all_v), _np(all_t), ref.select(label, _np(all_t), 1.0)[0])
    assert np.array_equal(back.vertices, want_v.astype(np.float64)) and np.array_equal(back.faces, want_t)
    with torch.no_grad():
        mesh = rend.extract_mesh(bd, components="largest", colors=True)
    assert np.array_equal(back.vertex_colors, _np(mesh.rgb_u8)) and back.vertex_colors.std() > 1.0
    from PIL import Image

    for sub in ("mesh0_render", "mesh0_color"):
        files = sorted(p.name for p in (tmp_path / "mesh" / sub).iterdir())
        assert files == sorted("%d.jpg" % k for k in range(91)), sub
    shade = np.asarray(Image.open(tmp_path / "mesh" / "mesh0_render" / "0.jpg")).astype(np.int32)
    color = np.asarray(Image.open(tmp_path / "mesh" / "mesh0_color" / "0.jpg")).astype(np.int32)
    assert shade.shape == color.shape == (48, 40, 3) and (color[0, 0] > 235).all()  # white, up to the JPEG's ringing
    drawn = (shade < 245).any(axis=-1)
    assert drawn.sum() > 50 and np.abs(color - shade)[drawn].max() > 16  # the same silhouette, other colours
    # and the command-line tool on the file just written
    import shutil

    from tools import render_mesh

    root = tmp_path / "results"
    (root / "exp" / "mesh").mkdir(parents=True)
    shutil.copy(path, root / "exp" / "mesh" / "0000.ply")
    paths = render_mesh.main(["--exp_name", "exp", "-ww", "40", "-hh", "48", "--result_dir", str(root), "--device", DEV, "--color"])
    assert len(paths) == 91 and paths[0].endswith("exp/mesh/mesh0_color/0.jpg")
    assert _read(paths[0]) == _read(tmp_path / "mesh" / "mesh0_color" / "0.jpg")


def test_without_the_keys_the_ply_and_the_pictures_are_the_old_bytes(tmp_path):
    from neuralbody_amd import ops
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_io import MeshVisualizer
    from neuralbody_amd.mesh_render import MeshTurntable

    rend, bd, _, _ = _scene()
    with torch.no_grad():
        out = rend.render(bd)
    assert isinstance(out["mesh"], TriMesh) and out["mesh"].vertex_colors is None  # neither PyMCubes nor trimesh where this runs
    cfg = types.SimpleNamespace(result_dir=str(tmp_path / "new"), mesh_render=True, mesh_render_size=(48, 40))
    path = MeshVisualizer(cfg).visualize(out, bd)
    assert not (tmp_path / "new" / "mesh" / "mesh0_color").exists()
    # the old way: marching cubes of the cube, TriMesh(vertices, faces).export, the normal-shaded turntable
    with torch.no_grad():
        v, t = ops.marching_cubes(rend.density_cube(bd).contiguous(), 5.0)
    old = TriMesh(v.double().cpu().numpy(), t.cpu().numpy())
    (tmp_path / "old").mkdir()
    old_path = old.export(str(tmp_path / "old" / "0000.ply"))
    assert _read(path) == _read(old_path)
    tt = MeshTurntable(48, 40, device=DEV)
    old_jpg = tt.save(tt.render(old), str(tmp_path / "old" / "render"))
    for k in (0, 45, 90):
        assert _read(tmp_path / "new" / "mesh" / "mesh0_render" / ("%d.jpg" % k)) == _read(old_jpg[k]), k
