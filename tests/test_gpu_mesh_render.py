"""nb_mesh_vertex_normals and nb_mesh_render (csrc/nb_mesh_render.hip) and the turntable above them (neuralbody_amd/mesh_render.py)
on the device.

The kernels' definition is exact, so every case is compared bit for bit with its evaluation on the host
(tests/mesh_render_ref.py::snapped_*); the band test of tests/test_mesh_render_host.py is then repeated on the device's pictures
against the float64 reference on unsnapped vertices."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import mc_ref
from tests import mesh_render_ref as mr
from tests import silhouette_ref as sil
from tests import test_mesh_render_host as host
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared meshes are read-only


def _bits(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Bit for bit, NaN and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------- 1. normals
def test_normals_equal_the_host_definition_bit_for_bit():
    from neuralbody_amd import ops

    v, f = host.mesh("ico320")
    dv, df = ops.marching_cubes(_dev(mc_ref.sphere_field()), 0.0)
    for name, verts, faces in (("ico320", v, f), ("sphere", _bits(dv), _bits(df))):
        want = mr.snapped_normals(verts, faces)
        tv, tf = _dev(verts), _dev(faces)
        got = ops.mesh_vertex_normals(tv, tf)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == verts.shape
        diff = int((_bits(got).view(np.uint32) != want.view(np.uint32)).sum())
        print("%s: %d vertices, %d faces, %d of %d floats differ from the host definition" % (name, len(verts), len(faces), diff, want.size))
        assert _same(_bits(got), want)
        # a dirty accumulator and a dirty output change nothing
        acc = torch.full((len(verts), 3), -1414812757, dtype=torch.int32, device=DEV)  # 0xABABABAB
        dirty = torch.full_like(got, float("nan"))
        again = ops.mesh_vertex_normals(tv, tf, out=dirty, scratch=acc)
        assert again is dirty and H.same_bits(again, got)


def test_normals_skip_a_bad_face_and_zero_an_isolated_vertex():
    from neuralbody_amd import ops

    v, f = host.mesh("ico320")
    plain = ops.mesh_vertex_normals(_dev(v), _dev(f))
    v2 = np.concatenate([v, [[9.0, 9.0, 9.0]]]).astype(np.float32)
    f2 = np.concatenate([f[:100], [[0, 1, len(v2)], [-1, 2, 3], [5, 2 ** 31 - 1, 6]], f[100:]]).astype(np.int32)
    got = ops.mesh_vertex_normals(_dev(v2), _dev(f2))
    assert H.same_bits(got[:-1], plain) and not bool(got[-1].any())
    assert _same(_bits(got), mr.snapped_normals(v2, f2))
    empty = ops.mesh_vertex_normals(_dev(v), _dev(f[:0]))
    assert not bool(empty.any())


# ---------------------------------------------------------------------------------------------------------- 2. render
def test_three_views_equal_the_host_definition_and_lie_in_the_band():
    from neuralbody_amd import ops

    v, f = host.mesh("ico320")
    Hh, Ww = host.BAND_SIZE
    cams = host.cams_of(v, Hh, Ww)[list(host.BAND_VIEWS)]
    tv, tf, tc = _dev(v), _dev(f), _dev(cams)
    normals = ops.mesh_vertex_normals(tv, tf)
    rgb, fid, depth = ops.mesh_render(tv, normals, tf, tc, Hh, Ww, want_face_id=True, want_depth=True)
    assert tuple(rgb.shape) == (3, Hh, Ww, 3) and fid.dtype == torch.int32 and depth.dtype == torch.float32
    want = mr.snapped_stack(v, _bits(normals), f, cams, Hh, Ww)
    for name, got, ref in zip(("rgb", "face_id", "depth"), (rgb, fid, depth), want):
        diff = int((_bits(got) != ref).sum())
        print("%s: %d of %d values differ from the host definition" % (name, diff, ref.size))
        assert _same(_bits(got), ref), name
    # buffers filled with 0xAB give the same bits
    dirty = [torch.full_like(t.view(torch.int32), -1414812757).view(t.dtype) for t in (rgb, fid, depth)]
    scratch = ops.mesh_render_scratch(3, Hh, Ww, len(f), DEV).fill_(0xAB)
    again = ops.mesh_render(tv, normals, tf, tc, Hh, Ww, out=dirty[0], face_id=dirty[1], depth=dirty[2], scratch=scratch)
    assert again[0] is dirty[0] and all(H.same_bits(a, b) for a, b in zip(again, (rgb, fid, depth)))
    assert H.same_bits(ops.mesh_render(tv, normals, tf, tc, Hh, Ww), rgb)  # without the optional outputs
    # the band of the host suite, on the device's pictures
    for i, k in enumerate(host.BAND_VIEWS):
        host.check_band("ico320", k, (_bits(rgb[i]), _bits(fid[i])), host.band_case("ico320", k))


# ---------------------------------------------------------------------------------------------------------- 3. paths
PATH_H, PATH_W = 96, 128


def _view(scale, cx, cy, R):
    """An orthographic camera: x_px = scale (R v).x + cx, y_px = -scale (R v).y + cy, depth = -(R v).z."""
    M = np.concatenate([scale * R[0], [cx], -scale * R[1], [cy], -R[2], [0.0]])
    return np.concatenate([M, R.reshape(-1), np.zeros(3)]).astype(np.float32)


def _rotation(axis, ang):
    """Rodrigues: the rotation by `ang` about `axis`."""
    ax = np.array(axis) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    return np.eye(3) + math.sin(ang) * Kx + (1.0 - math.cos(ang)) * Kx @ Kx


@functools.lru_cache(maxsize=None)
def _path_case():
    """The tetrahedron of the silhouette suite in five views at 96 x 128: filling the image (boxes far beyond 16 x 16: a workgroup
    per triangle), scaled under 16 px (a thread per triangle), partly off the image, wholly off it, and 1e5 px to the right (every
    vertex beyond +-32768 px: skipped).  The faces hold both windings, a repeated-vertex face of zero area, a triangle lying behind
    the body (face 6) and a second copy of face 0 (face 7)."""
    v, faces = sil.tetrahedron(0.25)
    R = _rotation((1.0, -1.0, 0.2), 0.9)  # three faces towards the camera
    behind = np.array([[-0.05, -0.04, -1.0], [0.06, -0.03, -1.0], [0.0, 0.05, -1.0]]) @ R  # rows R^T p: view space z = -1, depth 1
    verts = np.concatenate([v, behind]).astype(np.float32)
    faces = np.concatenate([faces[:2], faces[2:, ::-1], [[1, 1, 3], [2, 0, 2], [4, 5, 6], faces[0]]]).astype(np.int32)
    cams = np.stack([_view(170.0, 64.3, 47.6, R), _view(20.0, 64.3, 47.6, R), _view(170.0, -8.2, 30.9, R), _view(170.0, 500.0, 47.6, R),
                     _view(170.0, 1e5, 47.6, R)])
    return verts, faces, cams


def test_large_small_clipped_degenerate_coincident_and_hidden_triangles():
    from neuralbody_amd import ops

    verts, faces, cams = _path_case()
    px = [mr._project64(verts[:4], c)[:, :2] for c in cams]
    assert np.ptp(px[0], axis=0).min() > 60 and np.ptp(px[1], axis=0).max() < 15     # view 0 large, view 1 small
    assert px[2][:, 0].min() < -40 and px[2][:, 0].max() > 20                          # view 2 partly off the image
    assert px[3][:, 0].min() > PATH_W + 100 and px[4][:, 0].min() > 40000            # view 3 wholly off, view 4 beyond the bound
    tv, tf, tc = _dev(verts), _dev(faces), _dev(cams)
    normals = ops.mesh_vertex_normals(tv, tf)
    rgb, fid, depth = ops.mesh_render(tv, normals, tf, tc, PATH_H, PATH_W, want_face_id=True, want_depth=True)
    want = mr.snapped_stack(verts, _bits(normals), faces, cams, PATH_H, PATH_W)
    for name, got, ref in zip(("rgb", "face_id", "depth"), (rgb, fid, depth), want):
        assert _same(_bits(got), ref), name
    ids = _bits(fid)
    covered = (ids >= 0).reshape(5, -1).sum(axis=1)
    print("covered pixels per view:", covered.tolist())
    assert covered[0] > 3000 and 20 < covered[1] < 200 and 0 < covered[2] < covered[0]
    for view in (3, 4):  # nothing drawn: white, -1, +inf
        assert covered[view] == 0 and bool((rgb[view] == 1.0).all()) and bool(torch.isinf(depth[view]).all())
    shown = set(np.unique(ids).tolist())
    assert {0, 1, 2} <= shown <= {-1, 0, 1, 2, 3}  # never the zero-area faces, the hidden triangle or the copy
    # the hidden triangle is drawable: alone, it shows; of two coincident triangles alone, the lower id wins everywhere
    for pair, want_ids in ((faces[6:7], {-1, 0}), (faces[[0, 0]], {-1, 0})):
        alone = ops.mesh_render(tv, normals, _dev(pair), tc[:1], PATH_H, PATH_W, want_face_id=True)[1]
        assert set(np.unique(_bits(alone)).tolist()) == want_ids


def test_more_listed_triangles_than_workgroups():
    """320 faces in two views at 256 x 256: more than 512 boxes of 17 or more pixel centres on a side, so the fixed grid of the
    large-triangle launch strides over its list and whole waves append to it."""
    from neuralbody_amd import ops

    v, f = sil.icosphere(2, sil.ELLIPSOID)
    cams = np.stack([_view(250.0, 127.3, 128.6, _rotation(axis, ang)) for axis, ang in (((1.0, -1.0, 0.2), 0.9), ((0.1, 1.0, 0.3), 2.1))])
    large = 0
    for cam in cams:
        px = mr._project64(v, cam)[:, :2][f]  # [T,3,2]
        lo, hi = np.ceil(px.min(axis=1) - 0.5), np.floor(px.max(axis=1) - 0.5)
        large += int(((hi - lo).max(axis=1) >= 16).sum())
    print("%d of %d (view, triangle) boxes are large" % (large, 2 * len(f)))
    assert len(f) == 320 and large > 512
    tv, tf, tc = _dev(v), _dev(f), _dev(cams)
    normals = ops.mesh_vertex_normals(tv, tf)
    got = ops.mesh_render(tv, normals, tf, tc, 256, 256, want_face_id=True, want_depth=True)
    want = mr.snapped_stack(v, _bits(normals), f, cams, 256, 256)
    for name, g, ref in zip(("rgb", "face_id", "depth"), got, want):
        assert _same(_bits(g), ref), name


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_no_triangles_is_white_and_bad_arguments_launch_nothing():
    from neuralbody_amd import _lib, ops

    verts, faces, cams = _path_case()
    tv, tf, tc = _dev(verts), _dev(faces), _dev(cams[:2])
    normals = ops.mesh_vertex_normals(tv, tf)
    rgb, fid, depth = ops.mesh_render(tv, normals, tf[:0], tc, 9, 7, want_face_id=True, want_depth=True)
    assert tuple(rgb.shape) == (2, 9, 7, 3) and bool((rgb == 1.0).all()) and bool((fid == -1).all()) and bool(torch.isinf(depth).all())
    L, p = _lib.lib(), _lib.ptr
    need = L.nb_mesh_render_scratch_size(2, 9, 7, len(faces))
    assert need > 2 * 9 * 7 * 8 and L.nb_mesh_render_scratch_size(2, 0, 7, 1) == 0 and L.nb_mesh_render_scratch_size(2, 9, -1, 1) == 0
    assert L.nb_mesh_render_scratch_size(0, 9, 7, 1) == 0 and L.nb_mesh_render_scratch_size(2, 9, 7, -1) == 0
    assert L.nb_mesh_render_scratch_size(2, 32768, 32768, 1) == 0  # n_views H W beyond 2^31
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 9, 7, 3), -7.0, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(verts=tv, faces=tf, H=9, W=7, rgb=out, scratch_bytes=need, cams=tc):
        return L.nb_mesh_render(p(verts), p(normals), p(faces), len(tv), len(tf), p(cams), 2, H, W, p(rgb), None, None, p(scratch),
                                scratch_bytes, stream)

    for kw, word in ((dict(H=0), b"H = 0"), (dict(W=-3), b"W = -3"), (dict(rgb=None), b"NULL"), (dict(cams=None), b"NULL"),
                     (dict(verts=None), b"NULL"), (dict(faces=None), b"NULL"), (dict(scratch_bytes=need - 1), b"scratch holds")):
        assert call(**kw) == -1, kw
        assert b"nb_mesh_render" in L.nb_last_error() and word in L.nb_last_error(), (kw, L.nb_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
    with pytest.raises(ValueError):
        ops.mesh_render(tv, normals, tf, tc, 0, 7)
    assert L.nb_mesh_vertex_normals(None, p(tf), len(tv), len(tf), None, None, stream) == -1
    assert L.nb_mesh_vertex_normals(p(tv), p(tf), -1, len(tf), p(scratch), p(out), stream) == -1


# ---------------------------------------------------------------------------------------------------------- 5. end to end
@functools.lru_cache(maxsize=None)
def _scene_mesh():
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    _, sd, batch = scenes.build_mesh()
    rend = RendererMesh(H.make_network(sd, DEV, True, "f32"), RenderConfig(mesh_th=5.0))
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        v, t = rend.extract_mesh(bd)
        out = rend.render(bd)
    return v, t, out, bd


def test_turntable_of_the_extracted_mesh_mirrors_after_half_a_turn():
    from neuralbody_amd.mesh_render import MeshTurntable

    v, t, _, _ = _scene_mesh()
    assert v.is_cuda and t.is_cuda and len(t) > 0
    tt = MeshTurntable(64, 64, device=DEV)
    imgs = tt.render(v, t)
    assert imgs.is_cuda and tuple(imgs.shape) == (91, 64, 64, 3) and float(imgs.min()) >= 0.0 and float(imgs.max()) <= 1.0
    cams = _bits(tt.cams(v))
    # views 0 and 45 are half a turn apart: Ry(180) maps x -> -x, z -> -z, and the camera is orthographic
    assert np.allclose(cams[45, 12:21].reshape(3, 3), np.diag([-1.0, 1.0, -1.0]) @ cams[0, 12:21].reshape(3, 3), atol=1e-6)
    cover = _bits((imgs != 1.0).any(dim=-1))
    hv, ht = _bits(v), _bits(t)
    st = mr.stable(hv, ht, cams[0], 64, 64) & mr.stable(hv, ht, cams[45], 64, 64)[:, ::-1]
    print("covered pixels: view 0 %d, view 45 %d; %d of 4096 pixels stable in both; %d stable pixels break the mirror" % (
        int(cover[0].sum()), int(cover[45].sum()), int(st.sum()), int((cover[0] != cover[45][:, ::-1])[st].sum())))
    assert cover[0].sum() > 100 and cover[45].sum() > 100 and st.sum() > 2048
    assert np.array_equal(cover[0][st], cover[45][:, ::-1][st])
    # a host mesh gives the same pictures as the device tensors it was downloaded from
    from neuralbody_amd.mesh import TriMesh

    assert H.same_bits(MeshTurntable(64, 64, device=DEV, views_per_call=7).render(TriMesh(hv, ht)), imgs)


def test_visualizer_with_mesh_render_writes_the_91_views(tmp_path):
    from neuralbody_amd.mesh_io import MeshVisualizer

    _, _, out, bd = _scene_mesh()
    cfg = types.SimpleNamespace(result_dir=str(tmp_path), mesh_render=True, mesh_render_size=(48, 40))
    path = MeshVisualizer(cfg).visualize(out, bd)
    assert path.endswith("mesh/0000.ply")
    files = sorted(p.name for p in (tmp_path / "mesh" / "mesh0_render").iterdir())
    assert files == sorted("%d.jpg" % k for k in range(91))
    from PIL import Image

    img = np.asarray(Image.open(tmp_path / "mesh" / "mesh0_render" / "0.jpg"))
    assert img.shape == (48, 40, 3) and (img[0, 0] > 250).all() and (img < 200).any()
    # and the command-line tool on the file just written
    from tools import render_mesh

    paths = render_mesh.main(["--exp_name", "exp", "--dataset", "zju_mocap", "-ww", "40", "-hh", "48", "--result_dir",
                              _exp_dir(tmp_path), "--device", DEV])
    assert len(paths) == 91 and paths[90].endswith("exp/mesh/mesh0_render/90.jpg")
    again = np.asarray(Image.open(paths[0]))
    assert np.array_equal(again, img)


def _exp_dir(tmp_path):
    """{result_dir}/{exp}/mesh/0000.ply for tools/render_mesh.py from the visualizer's mesh/0000.ply."""
    import shutil

    root = tmp_path / "results"
    (root / "exp" / "mesh").mkdir(parents=True)
    shutil.copy(tmp_path / "mesh" / "0000.ply", root / "exp" / "mesh" / "0000.ply")
    return str(root)
