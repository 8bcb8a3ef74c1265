"""Host side of the device turntable (neuralbody_amd/mesh_render.py, csrc/nb_mesh_render.hip): the camera against the reference's
chain of GL matrices, the kernels' definition (tests/mesh_render_ref.py::snapped_*) against the float64 meaning of the pictures,
and the files.  No GPU.

Measured on these inputs (float32 rounding, recorded in DESIGN 4.12):
  normals  max |snapped - reference| per component: 1.74e-7 (ico80), 3.27e-7 (ico320), 2.57e-7 (ico1280), 5.05e-7 (sphere),
           9.80e-7 (torus); the test asserts 4 x the maximum.
  band     on stable pixels the face ids agree and the colours differ by at most 3.10e-4 (ico1280, views 10 and 33) against the
           bound of half an 8-bit step, 1/510; unstable pixels are at most 1.15 % (80 faces), 1.28 % (320), 1.57 % (1280) of the
           covered ones against the cap of 2 %."""
import functools

import numpy as np
import pytest

from tests import mc_ref
from tests import mesh_render_ref as mr
from tests import silhouette_ref as sil

NORMAL_MEASURED = 9.80e-7
NORMAL_BOUND = 4.0 * NORMAL_MEASURED
COLOUR_BOUND = 1.0 / 510.0
UNSTABLE_CAP = 0.02
BAND_VIEWS = (0, 10, 33)
BAND_SIZE = (45, 61)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The meshes the host and the device suites share; computed once, never written."""
    if name.startswith("ico"):
        v, f = sil.icosphere({"ico80": 1, "ico320": 2, "ico1280": 3}[name], sil.ELLIPSOID)
    else:
        v, f = mc_ref.marching_cubes({"sphere": mc_ref.sphere_field, "torus": mc_ref.torus_field}[name](), 0.0)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def cams_of(verts, H, W, dataset="zju_mocap"):
    """float32 [91,24] as MeshTurntable uploads them, from the float64 bounding box of the turned vertices."""
    from neuralbody_amd.mesh_render import turntable_cams

    t = mr.turned(verts, dataset)
    return turntable_cams(t.min(0), t.max(0), H, W, dataset).astype(np.float32)


@functools.lru_cache(maxsize=None)
def band_case(name, k):
    """-> dict of one band case: the mesh, the view's camera, both normals, the float64 reference picture and the stable pixels."""
    H, W = BAND_SIZE
    v, f = mesh(name)
    cam = cams_of(v, H, W)[k]
    n32, n64 = mr.snapped_normals(v, f), mr.reference_normals(v, f)
    return dict(verts=v, faces=f, cam=cam, H=H, W=W, n32=n32, ref=mr.reference_render(v, n64, f, cam, H, W),
                stable=mr.stable(v, f, cam, H, W))


def check_band(name, k, got, c):
    """got = (rgb, face_id) of a renderer that follows the snapped definition; c = band_case(name, k)."""
    rgb, fid = got
    ref_rgb, ref_id, _ = c["ref"]
    st, covered = c["stable"], ref_id >= 0
    unstable = float((~st & covered).sum()) / float(covered.sum())
    err = float(np.abs(rgb.astype(np.float64) - ref_rgb)[st].max())
    print("%s view %d: %d covered pixels, %.2f %% of them unstable, %d ids differ on stable pixels (%d anywhere), colour error %.3e" % (
        name, k, int(covered.sum()), 100.0 * unstable, int(((fid != ref_id) & st).sum()), int((fid != ref_id).sum()), err))
    assert covered.sum() > 2000 and covered[0].any() and covered[-1].any()  # the body overflows the rows: clipping is exercised
    assert unstable <= UNSTABLE_CAP
    assert np.array_equal(fid[st], ref_id[st])
    assert err <= COLOUR_BOUND


# ---------------------------------------------------------------------------------------------------------- camera
@pytest.mark.parametrize("dataset", ["zju_mocap", "people_snapshot"])
@pytest.mark.parametrize("size", [(512, 512), (45, 61)])
def test_turntable_cams_are_the_reference_gl_chain(dataset, size):
    from neuralbody_amd.mesh_render import turntable_cams

    H, W = size
    t = mr.turned(mesh("ico320")[0], dataset)
    lo, hi = t.min(0), t.max(0)
    cams = turntable_cams(lo, hi, H, W, dataset)
    assert cams.shape == (91, 24) and cams.dtype == np.float64 and not cams[:, 21:].any()
    a = 1.0 / (mr.FAR - mr.NEAR)  # z_window = a depth + b with a > 0: GL_LESS keeps the smaller depth
    b = 2.0 * a - 0.5 * (mr.FAR + mr.NEAR) * a + 0.5
    for k in (0, 10, 90):
        window, normal = mr.gl_chain(lo, hi, k, H, W, dataset)
        M = cams[k, :12].reshape(3, 4)
        errs = (np.abs(M[:2] - window[:2]).max(), np.abs(a * M[2] + np.array([0.0, 0.0, 0.0, b]) - window[2]).max(),
                np.abs(cams[k, 12:21].reshape(3, 3) - normal).max())
        print(dataset, size, k, "pixel rows %.2e, depth row %.2e, normal rotation %.2e" % errs)
        assert max(errs) <= 1e-12
    # the issue's closed form of view k: Ry(-(90 + 4 (k + 1)) degrees) after the object's rotation
    from neuralbody_amd.mesh_render import _rot_y, object_rotation

    assert np.abs(cams[90, 12:21].reshape(3, 3) - _rot_y(-(90.0 + 4.0 * 91)) @ object_rotation(dataset)).max() < 1e-12
    with pytest.raises(ValueError, match="y extent"):
        turntable_cams(lo, np.array([hi[0], lo[1], hi[2]]), H, W, dataset)


# ---------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", ["ico80", "ico320", "ico1280", "sphere", "torus"])
def test_snapped_normals_against_float64(name):
    v, f = mesh(name)
    assert len(f) == {"ico80": 80, "ico320": 320, "ico1280": 1280}.get(name, len(f)) and len(f) > 0
    got, ref = mr.snapped_normals(v, f), mr.reference_normals(v, f)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: %d vertices, %d faces, max |snapped - reference| = %.3e" % (name, len(v), len(f), err))
    assert got.dtype == np.float32 and np.allclose(np.linalg.norm(ref, axis=1), 1.0)
    assert err <= NORMAL_BOUND


def test_normals_skip_bad_faces_and_leave_unused_vertices_zero():
    v, f = mesh("ico80")
    v2 = np.concatenate([v, [[9.0, 9.0, 9.0]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 1, len(v2)], [-1, 2, 3]]]).astype(np.int32)
    for fn in (mr.snapped_normals, mr.reference_normals):
        n = fn(v2, f2)
        assert np.array_equal(n[:-1], fn(v, f)) and not n[-1].any()


# ---------------------------------------------------------------------------------------------------------- band
@pytest.mark.parametrize("k", BAND_VIEWS)
@pytest.mark.parametrize("name", ["ico80", "ico320", "ico1280"])
def test_snapped_render_agrees_with_float64_on_stable_pixels(name, k):
    c = band_case(name, k)
    rgb, fid, depth = mr.snapped_render(c["verts"], c["n32"], c["faces"], c["cam"], c["H"], c["W"])
    assert rgb.dtype == np.float32 and fid.dtype == np.int32 and depth.dtype == np.float32
    assert np.array_equal(fid < 0, np.isinf(depth)) and (rgb[fid < 0] == 1.0).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0
    check_band(name, k, (rgb, fid), c)


# ---------------------------------------------------------------------------------------------------------- files
def test_ply_round_trip_and_refusals(tmp_path):
    from neuralbody_amd.mesh import TriMesh

    v, f = mesh("ico80")
    path = TriMesh(v, f).export(str(tmp_path / "m.ply"))
    back = TriMesh.load_ply(path)
    assert back.vertices.dtype == np.float64 and back.faces.dtype == np.int64
    assert np.array_equal(back.vertices, v.astype(np.float64)) and np.array_equal(back.faces, f)
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    # double coordinates, uint indices, a comment and a further vertex property
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex %d\nproperty double x\nproperty double y\n"
            "property double z\nproperty uchar flag\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (len(v), len(f)))
    vrec = np.zeros(len(v), dtype=[("p", "<f8", (3,)), ("flag", "u1")])
    vrec["p"] = v
    other = tmp_path / "d.ply"
    other.write_bytes(head.encode() + vrec.tobytes() + raw[end + 12 * len(v):])
    back = TriMesh.load_ply(other)
    assert np.array_equal(back.vertices, v.astype(np.float64)) and np.array_equal(back.faces, f)

    def refused(data, what):
        bad = tmp_path / "bad.ply"
        bad.write_bytes(data)
        with pytest.raises(ValueError, match=what):
            TriMesh.load_ply(bad)

    refused(b"solid not a ply\n", "not a PLY")
    refused(raw.replace(b"binary_little_endian", b"ascii"), "binary_little_endian")
    refused(raw.replace(b"property float x", b"property int x"), "float or double")
    refused(raw.replace(b"list uchar int", b"list uchar short"), "list uchar int")
    refused(raw.replace(b"element face", b"element edge"), "vertex, face")
    refused(raw[:-5], "bytes after the header")
    quad = bytearray(raw)
    quad[end + 12 * len(v)] = 4
    refused(bytes(quad), "only triangles")


def test_save_writes_8_bit_bgr(tmp_path):
    from neuralbody_amd import mesh_render
    from neuralbody_amd.mesh_render import MeshTurntable, to_bgr8

    patch = np.array([[[1.0, 0.5, 0.0], [-0.2, 1.7, 0.25], [0.1, 0.2, 0.3]]], np.float32)  # RGB, one row of three
    assert np.array_equal(to_bgr8(patch), np.array([[[0, 128, 255], [64, 255, 0], [77, 51, 26]]], np.uint8))  # halves go to even
    imgs = np.ones((2, 16, 16, 3), np.float32)
    imgs[1] = np.array([0.8, 0.4, 0.1], np.float32)
    paths = MeshTurntable(16, 16, device="cpu").save(imgs, str(tmp_path / "mesh0_render"))
    assert [p.split("/")[-1] for p in paths] == ["0.jpg", "1.jpg"]
    from PIL import Image

    back = [np.asarray(Image.open(p)) for p in paths]
    assert back[0].shape == (16, 16, 3) and back[0].dtype == np.uint8 and (back[0] == 255).all()
    assert np.abs(back[1].astype(int) - np.array([204, 102, 26])).max() <= 3  # the file shows RGB; JPEG is lossy
    # neither writer: the error names both
    import builtins

    real = builtins.__import__

    def no_writers(name, *a, **kw):
        if name in ("cv2", "PIL"):
            raise ImportError(name)
        return real(name, *a, **kw)

    builtins.__import__ = no_writers
    try:
        with pytest.raises(ImportError, match="cv2.*PIL"):
            mesh_render._jpeg_writer()
    finally:
        builtins.__import__ = real


def test_wrappers_refuse_host_tensors():
    import torch

    from neuralbody_amd import ops

    v, f = mesh("ico80")
    tv, tf = torch.from_numpy(v.copy()), torch.from_numpy(f.copy())
    with pytest.raises(ops.NbError):
        ops.mesh_vertex_normals(tv, tf)
    with pytest.raises(ops.NbError):
        ops.mesh_render(tv, tv, tf, torch.zeros(1, 24), 8, 8)


def test_visualizer_without_the_key_writes_the_ply_alone(tmp_path):
    import types

    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.mesh_io import MeshVisualizer

    v, f = mesh("ico80")
    cfg = types.SimpleNamespace(result_dir=str(tmp_path))
    path = MeshVisualizer(cfg).visualize({"mesh": TriMesh(v, f)}, {"frame_index": np.array([3])})
    assert path.endswith("mesh/0003.ply") and sorted(p.name for p in (tmp_path / "mesh").iterdir()) == ["0003.ply"]
