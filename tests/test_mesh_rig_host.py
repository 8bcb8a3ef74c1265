"""Host side of the animatable mesh (csrc/nb_mesh_rig.hip, neuralbody_amd/mesh_rig.py): the float32 restatements of
tests/mesh_rig_ref.py against their float64 models — what the device tolerances lean on —, the reference's own ppts_to_pts
(tests/golden/mesh_rig.npz, tools/make_golden_mesh_rig.py) against the same model, RiggedMesh's host logic, and the ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from neuralbody_amd import _lib, build, mesh_rig, ops
from neuralbody_amd.smpl_pose import PoseDriver, SmplModel
from tests import mesh_rig_ref as ref
from tests import smpl_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_rig.npz")
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------- float32 restatement vs float64 model
@pytest.mark.parametrize("level", [2, 3])
def test_closest_restatement_against_the_float64_model(level):
    """How much farther than the float64 closest point the float32 answer may lie.  v and w are quotients of differences of
    products of two dot products: each product is below (L D)^2 (L the longest edge, D the largest |p - corner| of a winning
    triangle) and the quotient's denominator is |ab x ac|^2 >= n2, so with 16 roundings of 2^-24 on the way the point moves by
    at most 16 * 2^-24 * L * (L D)^2 / n2 along the triangle — all of which is excess where the closest point sits on an edge."""
    model = ref.surface_smpl(30 + level, level)
    body = smpl_ref.forward(model, *ref.draw(130 + level)).astype(np.float32)
    faces = ref.odd_faces(model["f"], body.shape[0])
    points = np.concatenate([ref.query_points(body, faces, level), ref.lattice_points(body, 257)])
    face, bary, dist2 = ref.closest(points, body, faces, np.float32)
    finite = np.isfinite(points).all(axis=1)
    assert (face[finite] >= 2).all()  # the two faces with an index out of range never win; the zero-area ones may (a vertex region)
    assert face[~finite].tolist() == [-1] and dist2[~finite].tolist() == [np.inf] and not bary[~finite].any()
    E = ref.e_ref_closest(points, body, faces)
    print("level %d: E_ref_closest = %.3e m over %d points" % (level, E, int(finite.sum())))
    tri = body.astype(np.float64)[np.asarray(model["f"])]
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    L = max(np.linalg.norm(ab, axis=1).max(), np.linalg.norm(ac, axis=1).max(), np.linalg.norm(ab - ac, axis=1).max())
    n2 = (np.linalg.norm(np.cross(ab, ac), axis=1) ** 2).min()
    D = np.sqrt(dist2[finite].astype(np.float64).max()) + L
    assert E <= 16 * EPS32 * L * (L * D) ** 2 / n2
    # on a vertex the distance is a rounding of q, not of p - q
    on_vertex = np.flatnonzero(dist2[:40] <= (4 * EPS32) ** 2)
    assert on_vertex.size >= 35


def test_closest_restatement_edge_cases():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], np.float32)
    p = np.array([[0.25, 0.25, 1.0], [-1, -1, 0], [2, -1, 0], [0.5, -2, 3], [np.inf, 0, 0]], np.float32)
    face, bary, dist2 = ref.closest(p, v, np.array([[0, 1, 2]]), np.float32)
    assert face.tolist() == [0, 0, 0, 0, -1]
    assert np.array_equal(bary[:4], np.array([[0.5, 0.25, 0.25], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0]], np.float32))
    assert np.array_equal(dist2[:4], np.array([1, 2, 2, 13], np.float32))
    # collinear corners: the interior divides 0 by 0 for a point off the line's ends, and the face is skipped
    f2, _, d2 = ref.closest(np.array([[0.5, 1.0, 0.0]], np.float32), v, np.array([[0, 1, 3]]), np.float32)
    assert (f2.tolist(), d2.tolist()) in (([-1], [np.inf]), ([0], [1.0]))
    # nothing valid at all
    f3, b3, d3 = ref.closest(p[:2], v, np.array([[0, 1, 4], [-1, 0, 1]]), np.float32)
    assert f3.tolist() == [-1, -1] and not b3.any() and np.isinf(d3).all()
    # a tie goes to the lower index, wherever the face stands in the list
    f4, _, _ = ref.closest(p[:1], v, np.array([[0, 1, 4], [0, 1, 2], [0, 1, 2]]), np.float32)
    assert f4.tolist() == [1]


@pytest.mark.parametrize("name", sorted(ref.BIND_CASES))
@pytest.mark.parametrize("new_params", [False, True])
def test_bind_restatement_against_the_float64_model(name, new_params):
    case = ref.bind_case(name, new_params)
    model, params, points = case["model"], case["params"], case["points"]
    body = smpl_ref.forward(model, *params, new_params=new_params).astype(np.float32)
    face, bary, _ = ref.closest(points, body, model["f"], np.float32)
    E, b32, b64 = ref.e_ref_bind(model, params, points, face, bary)
    print(name, new_params, E, "min det %.4f" % b64["det"].min())
    # the cases are generic: no vertex of the float64 model under the determinant bound (a cap of zero), none unbound
    assert int((~(np.abs(b64["det"]) >= ref.DET_MIN)).sum()) == 0
    assert b64["status"].tolist() == [0, 0, 0, 0] and b32["status"].tolist() == [0, 0, 0, 0]
    # three operations per weight and shape direction; the unposed point: ~40 operations on numbers below 2 m, over det >= 1/2
    assert E["weights"] <= 3 * EPS32 and E["shapedirs"] <= 3 * EPS32 * 0.1 and E["v_template"] <= 40 * EPS32 * 2.0 / 0.5
    assert b64["det"].min() >= 0.5
    assert np.abs(b32["weights"].astype(np.float64).sum(axis=0) - 1.0).max() <= 3 * 2.0 ** -23
    # the round trip of the model itself: driving the rig with its bind parameters returns the mesh (rot(Rh) is orthonormal to
    # the 1e-8 of batch_rodrigues' shifted angle, which is what is left in float64)
    assert np.abs(ref.rig_forward(model, b64, *params, dtype=np.float64) - points).max() <= 1e-8
    assert np.abs(ref.rig_forward(model, b32, *params, dtype=np.float32) - points).max() <= 40 * EPS32 * 2.0


def test_unpose_restatement_and_the_reference_against_float64():
    """ppts_to_pts as the reference runs it (torch, float32, recorded) and the float32 restatement both sit within float32
    rounding of the float64 model."""
    y, w, A = ref.fixture_case()
    with np.load(GOLDEN) as z:
        assert np.array_equal(z["y"], y) and np.array_equal(z["w"], w) and np.array_equal(z["A"], A), \
            "fixture_case drifted from tests/golden/mesh_rig.npz: run tools/make_golden_mesh_rig.py"
        recorded = z["pts"]
    model64, det = ref.unpose(y, w, A, np.float64)
    E = ref.e_ref_unpose(y, w, A)
    E_reference = float(np.abs(recorded.astype(np.float64) - model64).max())
    print("E_ref_unpose = %.3e, the reference's ppts_to_pts: %.3e, min det %.3f" % (E, E_reference, det.min()))
    assert recorded.dtype == np.float32 and recorded.shape == y.shape == (162, 3)
    assert det.min() >= 0.5
    assert E <= 40 * EPS32 * 2.0 / 0.5 and E_reference <= 40 * EPS32 * 2.0 / 0.5


def test_degenerate_case_is_degenerate_where_constructed():
    d = ref.degenerate_case()
    model, params = d["model"], d["params"]
    body = smpl_ref.forward(model, *params).astype(np.float32)
    face, bary, _ = ref.closest(body, body, model["f"], np.float32)
    assert np.array_equal(np.sort(bary, axis=1)[:, :2], np.zeros((body.shape[0], 2), np.float32))  # one-hot
    for dtype in (np.float32, np.float64):
        b = ref.bind(model, *params, body, face, bary, dtype)
        assert b["status"].tolist() == [0, len(d["vertices"]), 0, 0]
        small = np.flatnonzero(~(np.abs(b["det"]) >= ref.DET_MIN))
        assert np.array_equal(small, d["vertices"])
        w = b["weights"][:, d["vertices"]]
        assert np.array_equal(w, np.eye(24, dtype=dtype)[:, [ref.DEGENERATE_JOINTS[0]] * len(d["vertices"])])  # the lowest j of the tie
        assert np.abs(np.delete(b["det"], d["vertices"]) - 1.0).max() <= 1e-5


# ------------------------------------------------------------------------------------------- RiggedMesh on the host
def _host_rig(with_colors=True):
    model = ref.surface_smpl(31, 2)
    body = SmplModel.from_arrays(model)
    case = ref.bind_case("ico2")
    cbody = smpl_ref.forward(model, *case["params"]).astype(np.float32)
    face, bary, _ = ref.closest(case["points"], cbody, model["f"], np.float32)
    b = ref.bind(model, *case["params"], case["points"], face, bary, np.float32)
    P = case["points"].shape[0]
    faces = np.stack([np.arange(P - 2), np.arange(1, P - 1), np.arange(2, P)], axis=1).astype(np.int32)
    colors = (np.arange(3 * P) % 251).astype(np.uint8).reshape(P, 3) if with_colors else None
    bind = {"face": face, "bary": bary, "params": np.concatenate([np.ravel(p) for p in case["params"]]).astype(np.float32), "new_params": False}
    return body, b, faces, colors, mesh_rig.RiggedMesh(body, b["v_template"], b["weights"], b["shapedirs"], faces, colors, bind)


@pytest.mark.parametrize("with_colors", [True, False])
def test_rigged_mesh_save_load_round_trip(tmp_path, with_colors):
    body, b, faces, colors, rig = _host_rig(with_colors)
    assert rig.n_verts == b["v_template"].shape[0] and rig.parents == body.parents and rig.device == body.device
    path = rig.save(tmp_path / "rig.npz")
    with np.load(path) as z:
        assert "J_regressor" not in z and "posedirs" not in z
    back = mesh_rig.RiggedMesh.load(path, body)
    for k in mesh_rig.RIG_KEYS:
        assert np.array_equal(back.host[k], b[k]) and back.host[k].dtype == np.float32
    assert np.array_equal(back.faces, faces) and back.faces.dtype == np.int32
    assert (back.vertex_colors is None) if not with_colors else np.array_equal(back.vertex_colors.numpy(), colors)
    assert np.array_equal(back.bind["face"], rig.bind["face"]) and np.array_equal(back.bind["bary"], rig.bind["bary"])
    assert np.array_equal(back.bind["params"], rig.bind["params"]) and back.bind["new_params"] is False
    assert back.body is body
    if not with_colors:
        with pytest.raises(ValueError, match="colours"):
            back.colors_device()


def test_rigged_mesh_refuses_frames_and_views():
    _, _, _, _, rig = _host_rig()
    driver = PoseDriver(rig)
    poses, shapes, Rh, Th = ref.draw(1)
    with pytest.raises(_lib.NbError, match="geometry only"):
        driver.frames(poses, shapes, Rh, Th, 0)
    with pytest.raises(_lib.NbError, match="latent code per vertex"):
        next(driver.views([(np.eye(3), np.eye(3, 4))], poses, shapes, Rh, Th, 0))


def test_rigged_mesh_shape_checks():
    body, b, faces, colors, _ = _host_rig()
    P = b["v_template"].shape[0]
    with pytest.raises(ValueError, match="weights"):
        mesh_rig.RiggedMesh(body, b["v_template"], b["weights"][:, :-1], b["shapedirs"], faces)
    with pytest.raises(ValueError, match="shapedirs"):
        mesh_rig.RiggedMesh(body, b["v_template"], b["weights"], b["shapedirs"].reshape(10, P, 3), faces)
    with pytest.raises(ValueError, match="v_template"):
        mesh_rig.RiggedMesh(body, b["v_template"].reshape(-1), b["weights"], b["shapedirs"], faces)
    with pytest.raises(ValueError, match="faces"):
        mesh_rig.RiggedMesh(body, b["v_template"], b["weights"], b["shapedirs"], faces[:0])
    with pytest.raises(ValueError, match="vertex_colors"):
        mesh_rig.RiggedMesh(body, b["v_template"], b["weights"], b["shapedirs"], faces, colors[:-1])
    with pytest.raises(ValueError, match="vertex_colors"):
        mesh_rig.RiggedMesh(body, b["v_template"], b["weights"], b["shapedirs"], faces, colors.astype(np.float32))
    with pytest.raises(TypeError):
        mesh_rig.RiggedMesh(None, b["v_template"], b["weights"], b["shapedirs"], faces)


def test_bind_mesh_refuses_a_model_without_faces_and_a_rig():
    arrays = ref.surface_smpl(31, 2)
    points, params = ref.bind_case("ico2")["points"], ref.draw(131)
    del arrays["f"]
    with pytest.raises(_lib.NbError, match="triangle list"):
        mesh_rig.bind_mesh(SmplModel.from_arrays(arrays), points, np.array([[0, 1, 2]]), *params)
    _, _, _, _, rig = _host_rig()
    with pytest.raises(TypeError):
        mesh_rig.bind_mesh(rig, points, np.array([[0, 1, 2]]), *params)
    with pytest.raises(TypeError):
        mesh_rig.animate(SmplModel.from_arrays(ref.surface_smpl(31, 2)), *params, None)


def test_wrappers_refuse_cpu_tensors():
    pts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(_lib.NbError):
        ops.mesh_closest(pts, pts, faces)
    with pytest.raises(_lib.NbError):
        ops.mesh_rig_bind(_lib.NbSmplModel(), torch.zeros(88), torch.zeros(512), faces, pts, torch.zeros(4, dtype=torch.int32), pts)


# ------------------------------------------------------------------------------------------- the cross-compiled library
@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_library_exports_the_rig_symbols(lib):
    for name in ("nb_mesh_closest_scratch_size", "nb_mesh_closest", "nb_mesh_rig_bind"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(lib, name)
    assert lib.nb_abi_version() == _lib.ABI_VERSION == 20


def test_size_limits_without_touching_a_device(lib):
    big = (2 ** 31 - 256) // 3 + 1  # 3 n >= 2^31 - 256
    ok = (2 ** 31 - 257) // 3
    assert lib.nb_mesh_closest_scratch_size(100, 0) == 0 and lib.nb_mesh_closest_scratch_size(0, 100) == 0
    assert lib.nb_mesh_closest_scratch_size(100, big) == 0 and lib.nb_mesh_closest_scratch_size(big, 100) == 0
    assert lib.nb_mesh_closest_scratch_size(ok, 100) > 0
    n = lib.nb_mesh_closest_scratch_size(162, 320)
    # header, 4096 cells, the order, one sphere and 64 triangles of 64 bytes per tile: every section a multiple of 256
    assert n == 256 + 4096 * 4 + 1280 + 256 + 5 * 64 * 64
    assert lib.nb_mesh_closest_scratch_size(162, 321) == 256 + 4096 * 4 + 1536 + 256 + 6 * 64 * 64
    one = C.c_void_p(16)  # never dereferenced: the sizes are refused first
    for P, V, Nf in ((0, 10, 10), (10, 10, 0), (10, 0, 10), (big, 10, 10), (10, big, 10), (10, 10, big), (-1, 10, 10)):
        assert lib.nb_mesh_closest(one, one, one, P, V, Nf, 0, one, 1 << 40, one, one, one, None) == -1, (P, V, Nf)
        assert b"nb_mesh_closest" in lib.nb_last_error()
    assert lib.nb_mesh_closest(None, None, None, 10, 10, 10, 0, None, 0, None, None, None, None) == -1
    assert lib.nb_mesh_closest(one, one, one, 10, 10, 10, 4, one, 1 << 40, one, one, one, None) == -1  # an unknown flag
    assert lib.nb_mesh_closest(one, one, one, 10, 10, 10, 0, one, 16, one, one, one, None) == -1       # a scratch too small
    model = _lib.NbSmplModel()
    for P, V, Nf in ((0, 10, 10), (10, 10, 0), (10, 0, 10), (big, 10, 10), (10, 10, big)):
        model.n_verts = V
        assert lib.nb_mesh_rig_bind(C.byref(model), one, one, one, Nf, one, one, one, P, one, one, one, one, None) == -1, (P, V, Nf)
        assert b"nb_mesh_rig_bind" in lib.nb_last_error()
    assert lib.nb_mesh_rig_bind(None, one, one, one, 10, one, one, one, 10, one, one, one, one, None) == -1
    model.n_verts = 10
    assert lib.nb_mesh_rig_bind(C.byref(model), None, one, one, 10, one, one, one, 10, one, one, one, one, None) == -1
