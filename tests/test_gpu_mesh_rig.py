"""Device tests of the animatable mesh: nb_mesh_closest to the bits of the exhaustive float32 restatement (tests/mesh_rig_ref.py)
and within 4 x that restatement's own error of the float64 model; nb_mesh_rig_bind, the round trip through nb_smpl_pose, driven
rigs and their consumers within 4 x the restatement's error (the factor of tests/test_gpu_smpl_pose.py).  The restatement's errors
are recomputed here per case (tests/test_mesh_rig_host.py caps them on the CPU); no tolerance is a hard-coded number."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from neuralbody_amd import _lib, mesh_rig, ops
from neuralbody_amd.mesh import TriMesh
from neuralbody_amd.mesh_render import MeshTurntable
from neuralbody_amd.smpl_pose import PoseDriver, SmplModel, pack_params
from tests import mesh_rig_ref as ref
from tests import silhouette_ref, smpl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _query(points, verts, faces, **kw):
    face, bary, dist2 = ops.mesh_closest(_dev(points), _dev(verts), _dev(np.asarray(faces, np.int32)), **kw)
    return face.cpu().numpy(), bary.cpu().numpy(), dist2.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), "face: %d of %d differ" % (int((got[0] != want[0]).sum()), len(want[0]))
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "bary bits"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), "dist2 bits"


# ------------------------------------------------------------------------------------------- 1, 2: the closest query
_SURFACES = {}


def _surface(level):
    """The posed body of `level`, a face list with invalid and zero-area faces in front, the query points (every kind, then a
    lattice in marching-cubes order) and the two references, computed once."""
    if level not in _SURFACES:
        model = ref.surface_smpl(30 + level, level)
        body = smpl_ref.forward(model, *ref.draw(130 + level)).astype(np.float32)
        faces = ref.odd_faces(model["f"], body.shape[0])
        points = np.concatenate([ref.query_points(body, faces, level), ref.lattice_points(body, 4096 if level == 2 else 1024)])
        want = ref.closest(points, body, faces, np.float32)
        d64 = np.sqrt(ref.closest(points, body, faces, np.float64)[2])
        _SURFACES[level] = dict(body=body, faces=faces, points=points, want=want, d64=d64)
    return _SURFACES[level]


@pytest.mark.parametrize("level,P", [(2, 1), (2, 63), (2, 64), (2, 65), (2, 257), (2, 4096), (3, 257), (3, 1321)])
def test_closest_equals_the_exhaustive_float32_restatement(level, P):
    s = _surface(level)
    for first in sorted({0, len(s["points"]) - P}):  # the head (vertices, edges, centroids ...) and the tail (the lattice)
        points = s["points"][first:first + P]
        want = tuple(a[first:first + P] for a in s["want"])
        _same(_query(points, s["body"], s["faces"]), want)
        _same(_query(points, s["body"], s["faces"], exhaustive=True), want)


def test_closest_answers_a_non_finite_point_and_repeats_into_dirty_buffers():
    s = _surface(2)
    points, want = s["points"][:320], tuple(a[:320] for a in s["want"])
    nan = np.flatnonzero(~np.isfinite(points).all(axis=1))
    assert nan.size == 1 and want[0][nan[0]] == -1 and np.isinf(want[2][nan[0]]) and not want[1][nan[0]].any()
    p, v, f = _dev(points), _dev(s["body"]), _dev(s["faces"])
    scratch = ops.mesh_closest_scratch(v.shape[0], f.shape[0], DEV)
    scratch.fill_(0xA5)
    face = torch.full((320,), 12345, dtype=torch.int32, device=DEV)
    bary = torch.full((320, 3), float("nan"), device=DEV)
    dist2 = torch.full((320,), -1.0, device=DEV)
    for _ in range(2):
        ops.mesh_closest(p, v, f, scratch=scratch, face=face, bary=bary, dist2=dist2)
        _same((face.cpu().numpy(), bary.cpu().numpy(), dist2.cpu().numpy()), want)
    ops.mesh_closest(p, v, f, scratch=scratch, count_tiles=True)
    skipped, met = ops.mesh_closest_tile_counts(scratch)
    n_tiles = (f.shape[0] - 2 + 63) // 64  # two faces are out of range
    assert 5 * n_tiles <= met <= 5 * (n_tiles + 16) and 0 <= skipped < met  # five workgroups; every wave also meets the start tile
    ops.mesh_closest(p, v, f, scratch=scratch, count_tiles=True, exhaustive=True)
    assert ops.mesh_closest_tile_counts(scratch) == (0, 5 * n_tiles)  # no start tile there: every tile met once per workgroup


@pytest.mark.parametrize("Nf", [1, ref.TILE - 1, ref.TILE, ref.TILE + 1])
def test_closest_on_truncated_face_lists(Nf):
    s = _surface(2)
    faces = s["faces"][4:4 + Nf]  # the icosphere's own faces
    points = s["points"][:257]
    want = ref.closest(points, s["body"], faces, np.float32)
    assert (want[0][np.isfinite(points).all(axis=1)] >= 0).all()
    _same(_query(points, s["body"], faces), want)
    _same(_query(points, s["body"], faces, exhaustive=True), want)


def test_closest_one_wave_per_workgroup():
    """Past 1024 workgroups of 64 points the query runs ONE wave per workgroup (one thread per point); below, several waves share
    the tiles of a workgroup's points.  65 faces: two tiles, the second holding one triangle."""
    s = _surface(2)
    faces = s["faces"][4:4 + ref.TILE + 1]
    points = ref.lattice_points(s["body"], 1025 * 64 + 1)
    want = ref.closest(points, s["body"], faces, np.float32)
    _same(_query(points, s["body"], faces), want)
    _same(_query(points[:513 * 64], s["body"], faces), tuple(a[:513 * 64] for a in want))  # two waves, one tile each


def test_closest_without_a_valid_face():
    s = _surface(2)
    got = _query(s["points"][:65], s["body"], s["faces"][:2])  # an index past the vertices, a negative one
    assert (got[0] == -1).all() and not got[1].any() and np.isinf(got[2]).all() and (got[2] > 0).all()
    # a zero-area face alone: whatever the arithmetic of the header gives, non-finite results skipped
    _same(_query(s["points"][:257], s["body"], s["faces"][2:4]), ref.closest(s["points"][:257], s["body"], s["faces"][2:4], np.float32))


@pytest.mark.parametrize("level", [2, 3])
def test_closest_against_float64(level):
    s = _surface(level)
    answered = s["want"][0] >= 0

    def excess(face, bary):
        q = ref.surface_point(s["body"], s["faces"], face[answered], bary[answered])
        return np.linalg.norm(s["points"][answered].astype(np.float64) - q, axis=1) - s["d64"][answered]

    E = float(np.abs(excess(s["want"][0], s["want"][1])).max())  # E_ref_closest of the case
    got = _query(s["points"], s["body"], s["faces"])
    assert np.array_equal(got[0] >= 0, answered)
    worst = float(excess(got[0], got[1]).max())
    print("level %d: distance excess %.3e m, E_ref_closest %.3e m" % (level, worst, E))
    assert worst <= FACTOR * E


# ------------------------------------------------------------------------------------------- 3: the bind
def _posed(arrays, params, new_params=False):
    """-> (SmplModel, native, params dev [1,88], ws dev [1,512], verts dev [V,3]) of one nb_smpl_pose call."""
    model = SmplModel.from_arrays(arrays, DEV)
    native, _ = model.native()
    rows = pack_params(*params).to(DEV)
    ws = torch.empty((1, _lib.SMPL_WS_FLOATS), dtype=torch.float32, device=DEV)
    verts, _ = ops.smpl_pose(native, rows, new_params, ws=ws)
    return model, native, rows, ws, verts[0]


def _bind(arrays, params, points, new_params=False, faces=None):
    model, native, rows, ws, verts = _posed(arrays, params, new_params)
    body_faces = model.faces_device() if faces is None else _dev(np.asarray(faces, np.int32))
    p = points if isinstance(points, torch.Tensor) else _dev(points)
    face, bary, _ = ops.mesh_closest(p, verts, body_faces)
    out = ops.mesh_rig_bind(native, rows[0], ws[0], body_faces, p, face, bary)
    names = ("weights", "shapedirs", "v_template", "status")
    return dict({k: v.cpu().numpy() for k, v in zip(names, out)}, face=face.cpu().numpy(), bary=bary.cpu().numpy(), model=model,
                ws=ws[0].cpu().numpy(), verts=verts)


@pytest.mark.parametrize("name", sorted(ref.BIND_CASES))
@pytest.mark.parametrize("new_params", [False, True])
def test_bind_against_float64(name, new_params):
    case = ref.bind_case(name, new_params)
    got = _bind(case["model"], case["params"], case["points"], new_params)
    E, _, b64 = ref.e_ref_bind(case["model"], case["params"], case["points"], got["face"], got["bary"])
    assert got["status"].tolist() == [0, 0, 0, 0] and b64["status"].tolist() == [0, 0, 0, 0]
    for k in ("weights", "shapedirs", "v_template"):
        err = float(np.abs(got[k].astype(np.float64) - b64[k]).max())
        print("%s new_params=%s %s: %.3e (restatement %.3e)" % (name, new_params, k, err, E[k]))
        assert err <= FACTOR * E[k], k
    sums = got["weights"].astype(np.float64).sum(axis=0)
    print("weight columns: |sum - 1| <= %.2f ulp" % (np.abs(sums - 1.0).max() / 2.0 ** -23))
    assert np.abs(sums - 1.0).max() <= 3 * 2.0 ** -23


def test_bind_degenerate_blend_goes_rigid():
    d = ref.degenerate_case()
    model, _, _, _, verts = _posed(d["model"], d["params"])
    got = _bind(d["model"], d["params"], verts.clone())  # bound exactly ON the body's vertices
    assert np.array_equal(np.sort(got["bary"], axis=1)[:, :2], np.zeros((verts.shape[0], 2), np.float32))
    assert got["status"].tolist() == [0, len(d["vertices"]), 0, 0]
    j = ref.DEGENERATE_JOINTS[0]  # the lowest joint of the 1/2, 1/2 tie
    assert np.array_equal(got["weights"][:, d["vertices"]], np.eye(24, dtype=np.float32)[:, [j] * len(d["vertices"])])
    others = np.delete(np.arange(verts.shape[0]), d["vertices"])
    onto = np.asarray(d["model"]["f"])[got["face"], np.argmax(got["bary"], axis=1)]
    assert np.array_equal(onto, np.arange(verts.shape[0]))
    assert np.array_equal(got["weights"][:, others], d["model"]["weights"].T[:, others])  # one-hot bary: the body's own weights


def test_bind_counts_an_unbound_vertex_and_bind_mesh_raises():
    case = ref.bind_case("ico2")
    V = case["model"]["v_template"].shape[0]
    invalid = np.array([[0, 1, V], [-1, 2, 3]], np.int32)
    far = np.array([[5.0, 5.0, 5.0]], np.float32)
    got = _bind(case["model"], case["params"], far, faces=invalid)
    assert got["face"].tolist() == [-1] and got["status"].tolist() == [1, 0, 0, 0]
    assert got["weights"][:, 0].tolist() == [1.0] + [0.0] * 23 and not got["shapedirs"].any() and np.isfinite(got["v_template"]).all()
    model = SmplModel.from_arrays(case["model"], DEV)
    model.faces = invalid  # past SmplModel's own validation, which refuses such a list
    with pytest.raises(_lib.NbError, match="1 of 1 mesh vertices found no face"):
        mesh_rig.bind_mesh(model, far, np.array([[0, 0, 0]]), *case["params"])
    with pytest.raises(_lib.NbError, match="found no face"):  # a non-finite mesh vertex on a sound body
        mesh_rig.bind_mesh(SmplModel.from_arrays(case["model"], DEV), np.array([[np.nan, 0, 0], [0, 0, 0.2]], np.float32),
                           np.array([[0, 1, 1]]), *case["params"])


# ------------------------------------------------------------------------------------------- 4: the round trip
@pytest.mark.parametrize("name", sorted(ref.BIND_CASES))
@pytest.mark.parametrize("new_params", [False, True])
def test_round_trip_returns_the_bound_mesh(name, new_params):
    case = ref.bind_case(name, new_params)
    arrays, params, points = case["model"], case["params"], case["points"]
    rig = mesh_rig.bind_mesh(SmplModel.from_arrays(arrays, DEV), points, arrays["f"], *params, new_params=new_params)
    assert isinstance(rig, mesh_rig.RiggedMesh) and rig.n_verts == points.shape[0] and rig.n_degenerate == 0
    back = PoseDriver(rig).vertices(*params)  # new_params = False: a rig has no pose blend shapes, they are in its template
    assert tuple(back.shape) == (1, points.shape[0], 3)
    b32 = ref.bind(arrays, *params, points, rig.bind["face"].cpu().numpy(), rig.bind["bary"].cpu().numpy(), np.float32)
    E = float(np.abs(ref.rig_forward(arrays, b32, *params, dtype=np.float32).astype(np.float64) - points).max())
    err = float(np.abs(back[0].cpu().numpy().astype(np.float64) - points).max())
    print("%s new_params=%s: round trip %.3e m (restatement %.3e m)" % (name, new_params, err, E))
    assert err <= FACTOR * E


def test_rest_pose_bind_is_exact():
    """poses = 0 (and Rh = 0, so that rot is the identity matrix to the bit): every A_j - [I|0] is 0 as nb_smpl_pose arranges, the
    blend is exactly the identity, and v_shaped IS x - Th.  So v_template carries the bits of fl((x - Th) - acc) with acc the
    float32 sum of S_l beta_l in the kernel's order: v_template + shapedirs . beta returns x - Th to the one rounding of that
    subtraction, half an ulp per coordinate."""
    case = ref.bind_case("ico2")
    poses, shapes, Rh, Th = case["params"]
    params = (np.zeros_like(poses), shapes, np.zeros_like(Rh), Th)
    got = _bind(case["model"], params, case["points"])
    assert got["status"].tolist() == [0, 0, 0, 0]
    assert not got["ws"][:24 * 12].any() and got["ws"][24 * 12 + 208:24 * 12 + 217].tolist() == np.eye(3).reshape(-1).tolist()
    P = case["points"].shape[0]
    sd, acc = got["shapedirs"].reshape(10, P, 3), np.zeros((P, 3), np.float32)
    for l in range(10):
        acc = acc + sd[l] * np.float32(shapes[l])
    y = case["points"] - Th.reshape(1, 3).astype(np.float32)
    assert acc.dtype == y.dtype == np.float32
    assert np.array_equal(_bits(got["v_template"]), _bits(y - acc))
    ulp = np.spacing(np.maximum(np.abs(y), np.maximum(np.abs(acc), np.abs(got["v_template"]))).astype(np.float32)).astype(np.float64)
    assert (np.abs((got["v_template"].astype(np.float64) + acc.astype(np.float64)) - y.astype(np.float64)) <= ulp).all()


# ------------------------------------------------------------------------------------------- 5: driven rigs
def test_points_bound_on_body_vertices_follow_the_body():
    case = ref.bind_case("ico3")
    arrays, params = case["model"], case["params"]
    model, _, _, _, verts = _posed(arrays, params)
    rig = mesh_rig.bind_mesh(model, verts.clone(), arrays["f"], *params)
    bary = rig.bind["bary"].cpu().numpy()
    assert np.array_equal(np.sort(bary, axis=1), np.tile(np.array([0, 0, 1], np.float32), (verts.shape[0], 1)))
    drive = ref.draw(232)
    got = PoseDriver(rig).vertices(*drive)[0].cpu().numpy().astype(np.float64)
    own = PoseDriver(model).vertices(*drive)[0].cpu().numpy().astype(np.float64)
    want = smpl_ref.forward(arrays, *drive)
    b32 = ref.bind(arrays, *params, verts.cpu().numpy(), rig.bind["face"].cpu().numpy(), bary, np.float32)
    E = float(np.abs(ref.rig_forward(arrays, b32, *drive, dtype=np.float32).astype(np.float64) - want).max())
    err = float(np.abs(got - want).max())
    print("rig on the body's vertices, reposed: %.3e m from float64 (restatement %.3e m; the body's own kernel %.3e m)"
          % (err, E, np.abs(own - want).max()))
    assert err <= FACTOR * E


def _shell_rig(level=3, offset=0.02):
    """The body of `level` in its rest pose with zero shape (the convex ellipsoid, moved rigidly by Rh, Th) and a shell `offset`
    off its vertices along their normals: each shell vertex's closest point is the body vertex under it."""
    arrays = ref.surface_smpl(33, level)
    _, _, Rh, Th = ref.draw(133)
    params = (np.zeros(72, np.float32), np.zeros(10, np.float32), Rh, Th)
    body = smpl_ref.forward(arrays, *params)
    shell = (body + offset * ref.vertex_normals(body, arrays["f"])).astype(np.float32)
    model = SmplModel.from_arrays(arrays, DEV)
    return arrays, params, model, mesh_rig.bind_mesh(model, shell, arrays["f"], *params), shell


def test_shell_rig_follows_a_pose_change():
    """Bound in the rest pose (T = I), shell vertex i sits at v_i + 0.02 n_i with the weights of body vertex i, so reposed it is
    M'_i (0.02 n_i) away from the reposed v_i, and |M'_i| <= sum_j w_j |R_j| = 1 (+ 2^-20 for the rounding of the weights' sum):
    within 0.02 m of the reposed surface, plus 4 x the float32 restatement's error of the shell itself."""
    arrays, params, model, rig, shell = _shell_rig()
    face, bary = rig.bind["face"].cpu().numpy(), rig.bind["bary"].cpu().numpy()
    onto = np.asarray(arrays["f"])[face, np.argmax(bary, axis=1)]
    assert np.array_equal(np.sort(bary, axis=1)[:, :2], np.zeros((len(shell), 2), np.float32)) and np.array_equal(onto, np.arange(len(shell)))
    drive = ref.draw(233)
    got = PoseDriver(rig).vertices(*drive)[0].cpu().numpy()
    b32, b64 = (ref.bind(arrays, *params, shell, face, bary, dt) for dt in (np.float32, np.float64))
    want = ref.rig_forward(arrays, b64, *drive, dtype=np.float64)
    E = float(np.abs(ref.rig_forward(arrays, b32, *drive, dtype=np.float32).astype(np.float64) - want).max())
    assert float(np.abs(got.astype(np.float64) - want).max()) <= FACTOR * E
    moved = smpl_ref.forward(arrays, *drive)
    assert np.abs(moved - smpl_ref.forward(arrays, *params)).max() > 0.05  # the pose did change
    # float64 closest of the float32 numbers: the body's reposed surface rounded, which E covers as well
    d = np.sqrt(ref.closest(got, moved.astype(np.float32), arrays["f"], np.float64)[2])
    print("shell: %.4f .. %.4f m off the reposed surface" % (d.min(), d.max()))
    bound = 0.02 * (1.0 + 2.0 ** -20) + FACTOR * E + np.abs(moved - moved.astype(np.float32)).max()
    assert d.max() <= bound
    own = np.linalg.norm(got.astype(np.float64) - moved, axis=1)  # the stronger statement: from the body vertex it was bound to
    assert own.max() <= bound and own.min() > 0.01  # (and the offsets did not collapse: a blend of mild rotations shrinks little)


# ------------------------------------------------------------------------------------------- 6: consumers
def _rigid_drive(seed):
    """A rigid motion of the whole body: the root joint turned, another Rh and Th."""
    poses, _, Rh, Th = ref.draw(seed)
    poses[3:] = 0
    return poses, np.zeros(10, np.float32), Rh, Th


def test_shell_silhouettes_contain_the_body():
    arrays, _, model, rig, _ = _shell_rig(level=2)
    H, W = 96, 128
    Ks, RTs = silhouette_ref.orbit((0.2, 1.4, 2.9, 4.4), 3.0, 1.3 * H, H, W)  # 0.02 m is 0.8 px there
    for seed in (234, 235):
        drive = _rigid_drive(seed)
        cams = (Ks, np.concatenate([RTs[:, :, :3], RTs[:, :, 3:] - RTs[:, :, :3] @ drive[3].reshape(1, 3, 1).astype(np.float32)], axis=2), H, W)
        body_driver, rig_driver = PoseDriver(model), PoseDriver(rig)
        inner = body_driver.silhouettes(body_driver.vertices(*drive), cams)
        outer = rig_driver.silhouettes(rig_driver.vertices(*drive), cams)
        assert tuple(outer.shape) == (1, 4, H, W) and outer.dtype == torch.uint8
        n_in, n_out = inner.sum(dim=(2, 3))[0].tolist(), outer.sum(dim=(2, 3))[0].tolist()
        assert all(0 < a < b < H * W for a, b in zip(n_in, n_out)), (n_in, n_out)
        assert not (inner & ~outer & 1).any()


def test_animate_draws_every_frame():
    arrays, _, model, rig, _ = _shell_rig(level=2)
    rig.vertex_colors = torch.tensor([[10, 200, 30]], dtype=torch.uint8).repeat(rig.n_verts, 1)
    F, H, W = 5, 48, 40
    drives = [_rigid_drive(240 + f) for f in range(F)]
    stack = [np.stack([d[k] for d in drives]) for k in range(4)]
    stack[3] = stack[3] * 0.1  # stay near one another: one camera set serves the clip
    table = MeshTurntable(H, W, device=DEV)
    shaded = mesh_rig.animate(rig, *stack, table, frames_per_call=2, view=3)
    flat = mesh_rig.animate(rig, *stack, table, colors=True, frames_per_call=3, view=3)
    assert tuple(shaded.shape) == tuple(flat.shape) == (F, H, W, 3) and shaded.dtype == torch.float32
    drawn = (flat != 1.0).any(dim=3)
    assert torch.equal(drawn, (shaded != 1.0).any(dim=3) | drawn)  # the same coverage (a normal-shaded pixel may be white by chance)
    share = drawn.float().mean(dim=(1, 2)).tolist()
    assert all(0.02 < s < 0.9 for s in share), share
    colour = torch.tensor([10, 200, 30], device=DEV) / 255.0
    assert torch.allclose(flat[drawn], colour.expand_as(flat[drawn]), atol=1e-6)  # the rig's own colours, where the silhouette is
    assert (flat[~drawn] == 1.0).all() and bool(torch.isfinite(shaded).all())
    assert not torch.equal(drawn[0], drawn[F - 1])
    spun = mesh_rig.animate(rig, *stack, table, colors=True, view=3, spin=True)
    assert torch.equal(spun[0], flat[0]) and not torch.equal(spun[1], flat[1])


def _writer_imports():
    try:
        from neuralbody_amd.mesh_render import _jpeg_writer

        _jpeg_writer()
        return True
    except ImportError:
        return False


@pytest.mark.skipif(not _writer_imports(), reason="neither cv2 nor PIL imports: nothing writes the JPEG files")
def test_animate_mesh_tool_writes_its_files(tmp_path):
    arrays = ref.surface_smpl(33, 2)
    _, _, Rh, Th = ref.draw(133)
    bind = dict(poses=np.zeros((1, 72), np.float32), shapes=np.zeros((1, 10), np.float32), Rh=Rh[None], Th=Th[None])
    body = smpl_ref.forward(arrays, bind["poses"][0], bind["shapes"][0], Rh, Th)
    shell = body + 0.02 * ref.vertex_normals(body, arrays["f"])
    colors = np.tile(np.array([[200, 40, 40]], np.uint8), (len(shell), 1))
    TriMesh(shell, arrays["f"], vertex_colors=colors).export(str(tmp_path / "mesh.ply"))
    with open(tmp_path / "smpl.pkl", "wb") as f:
        pickle.dump({k: v for k, v in arrays.items()}, f)
    np.save(tmp_path / "bind.npy", bind, allow_pickle=True)
    os.makedirs(tmp_path / "params")
    for i in range(3):
        poses, shapes, rh, th = _rigid_drive(250 + i)
        np.save(tmp_path / "params" / ("%d.npy" % i), dict(poses=poses[None], shapes=shapes[None], Rh=rh[None], Th=0.1 * th[None]), allow_pickle=True)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "animate_mesh.py"), str(tmp_path / "mesh.ply"), str(tmp_path / "smpl.pkl"),
           str(tmp_path / "bind.npy"), str(tmp_path / "params"), str(out), "--size", "64", "--rig", str(tmp_path / "rig.npz"), "--color",
           "--view", "2", "--spin"]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    files = sorted(os.listdir(out / "anim"))
    assert files == ["0000.jpg", "0001.jpg", "0002.jpg"]
    try:
        from PIL import Image

        img = np.asarray(Image.open(out / "anim" / "0001.jpg").convert("RGB"))
    except ImportError:
        import cv2

        img = cv2.imread(str(out / "anim" / "0001.jpg"))[..., ::-1]
    assert img.shape == (64, 64, 3)
    red = (img[..., 0] > 150) & (img[..., 1] < 100)
    white = img.min(axis=2) > 200
    assert 0.02 < red.mean() < 0.9 and white.mean() > 0.05 and (red | white).mean() > 0.9  # the rest: JPEG's ringing at the outline
    assert white[0, 0] and white[-1, -1]
    rig = mesh_rig.RiggedMesh.load(tmp_path / "rig.npz", SmplModel.from_arrays(arrays, DEV))
    assert rig.n_verts == len(shell) and np.array_equal(rig.vertex_colors.numpy(), colors)
