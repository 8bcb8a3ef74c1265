"""Pose-driven frames on the device (csrc/nb_smpl.hip, neuralbody_amd/smpl_pose.py) against the reference SMPL layer's fixture
(tests/golden/smpl_pose.npz), the float64 restatement of tests/smpl_ref.py and the package's host frames.

Vertices: max |device - float64 restatement| <= 4 x E_ref of the case (E_ref: the reference's own float32 error against the same
restatement, 1.4e-7 .. 2.7e-7 m in the fixture); device and reference are float32 evaluations of the same sums in another order.
Voxelisation: `coord` is compared at every coordinate OUTSIDE the near band (smpl_ref.BAND: the float64 coordinate within 1e-3
voxel of a half-integer), where a float32 evaluation may round to the other voxel whatever its order; inside it the difference is
at most 1, and the band may not exceed 1 % of the coordinates.  (tests/test_gpu_voxelize_exact.py holds the voxeliser to its
operation-by-operation restatement at every coordinate, the band included.)
Vertex blocks: V around the 64 vertices a workgroup skins, with guard frames behind every output; max |device - float64| <= 4 x E32,
E32 the float32 restatement's largest error over the sweep (2.9e-7 m; measured 0.50 .. 0.77 x E32)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import smpl_ref as sr
from tests import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_pose.npz")
E_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _host_model(name):
    m = sr.case_model(name)
    assert np.allclose(sr.checksums(m), _gold()[name + "/checksums"], rtol=1e-12, atol=0.0), "numpy's random stream moved"
    return m


@functools.lru_cache(maxsize=None)
def _model(name):
    """One upload per synthetic model (the two 6890 cases share theirs, the three 321 cases theirs)."""
    from neuralbody_amd.smpl_pose import SmplModel

    key = sorted(n for n in sr.CASES if sr.CASES[n][:3] == sr.CASES[name][:3])[0]
    return SmplModel.from_arrays(_host_model(key), DEV) if key == name else _model(key)


def _driver(name, **kw):
    from neuralbody_amd.smpl_pose import PoseDriver

    return PoseDriver(_model(name), **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------- 1. vertices
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_vertices_match_the_float64_restatement(name):
    g = _gold()
    poses, shapes, Rh, Th = sr.case_params(name)
    new_params = sr.CASES[name][3]
    verts = _driver(name).vertices(poses, shapes, Rh, Th, new_params)
    assert verts.is_cuda and verts.dtype == torch.float32 and tuple(verts.shape) == (1, sr.CASES[name][1], 3)
    got = verts[0].cpu().numpy().astype(np.float64)
    r64 = sr.forward(_host_model(name), poses, shapes, Rh, Th, new_params, np.float64)
    e_ref = float(g[name + "/E_ref"])
    err, err_ref = float(np.abs(got - r64).max()), float(np.abs(got - g[name + "/verts"]).max())
    print("%s: max |device - fp64| %.3e = %.2f x E_ref (%.3e); max |device - reference fp32| %.3e" % (
        name, err, err / e_ref, e_ref, err_ref))
    assert err <= E_FACTOR * e_ref


def test_posed_joints_match_the_float64_chain():
    from neuralbody_amd import ops

    name = "smpl6890_new"
    m = _host_model(name)
    poses, shapes, Rh, Th = sr.case_params(name)
    native, _ = _model(name).native()
    from neuralbody_amd.smpl_pose import pack_params

    _, joints = ops.smpl_pose(native, pack_params(poses, shapes, Rh, Th).to(DEV), True)
    # the chain's last column in float64 (lbs.py:371)
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    J = f(m["J_regressor"]) @ (f(m["v_template"]) + f(m["shapedirs"]) @ f(shapes))
    R = sr.rodrigues_lbs(f(poses).reshape(24, 3).astype(np.float32), np.float64)
    par, G = sr.parents_of(m), np.zeros((24, 4, 4))
    for j in range(24):
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = R[j], J[j] if par[j] < 0 else J[j] - J[par[j]]
        G[j] = L if par[j] < 0 else G[par[j]] @ L
    err = float(np.abs(joints[0].cpu().numpy() - G[:, :3, 3]).max())
    print("posed joints: max |device - fp64| %.3e" % err)
    assert tuple(joints.shape) == (1, 24, 3) and err <= 2e-6  # nine fp32 links of <= 1 m each


@pytest.mark.parametrize("name", ["smpl6890_new", "tree321_zero"])
@pytest.mark.parametrize("new_params", [False, True])
def test_rest_pose_is_the_shaped_body_moved_by_th(name, new_params):
    """Zero pose, Rh = 0: every rotation is the identity exactly (batch_rodrigues divides 0 by |1e-8|), the pose feature and every
    relative transform's difference from the identity are 0, so the output is fl(v_shaped + Th) with the kernel's own float32
    v_shaped, which the same call with Th = 0 returns.
      * out against fl(v_shaped + Th) of that v_shaped: at most 1 ulp apart, as float32 numbers (numpy's assert_array_max_ulp).
      * out against the float64 v_shaped + Th directly.  A float32 evaluation cannot be held to one ulp of a centimetre-sized
        coordinate here, because v_shaped is itself an eleven-term float32 sum: acc_k = acc_(k-1) + shapedirs_k beta_k for
        k = 1..10, then v_template + acc_10.  Each step rounds once at the size of its partial sum (and once at the size of
        its product where the compiler does not fuse them), so
            |v_shaped - exact| <= 2^-24 (sum_k |acc_k| + sum_k |shapedirs_k beta_k| + |v_shaped|)
        with the partial sums of THIS order taken from the float64 evaluation, and the last addition adds half an ulp of
        the output.  That bound, per coordinate, is the tolerance.  In ulps of max(|v_shaped|, |Th|, |out|) the worst
        coordinate measured 3.2 (6890 vertices) and 1.04 (321)."""
    m = _host_model(name)
    _, shapes, _, Th = sr.case_params(name)
    zero, rest = np.zeros(3, np.float32), np.zeros(72, np.float32)
    drv = _driver(name)
    v0 = drv.vertices(rest, shapes, zero, zero, new_params)[0].cpu().numpy()
    out = drv.vertices(rest, shapes, zero, Th, new_params)[0].cpu().numpy()
    want32 = (v0 + Th[None]).astype(np.float32)
    ulp = np.abs(out.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))
    same_sign = np.signbit(out) == np.signbit(want32)
    terms = m["shapedirs"].astype(np.float64) * shapes.astype(np.float64)  # [V,3,10]
    partial = np.cumsum(terms, axis=2)
    v_shaped = m["v_template"].astype(np.float64) + partial[:, :, -1]
    bound_v = 2.0 ** -24 * (np.abs(partial).sum(axis=2) + np.abs(terms).sum(axis=2) + np.abs(v_shaped))
    want = v_shaped + Th.astype(np.float64)[None]
    tol = bound_v + 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - want)
    scale = np.maximum(np.maximum(np.abs(v_shaped), np.abs(Th.astype(np.float64))[None]), np.abs(want)).astype(np.float32)
    print("%s new_params %d: out vs fl(v_shaped + Th) worst %d ulp; out vs float64 worst %.2f of its bound, %.2e m, %.2f ulp of the "
          "largest operand" % (name, new_params, int(ulp[same_sign].max()), float((err / tol).max()), float(err.max()),
                               float((err / np.spacing(scale)).max())))
    assert bool((same_sign | (np.abs(out - want32) <= np.spacing(np.abs(want32)))).all()) and int(ulp[same_sign].max()) <= 1
    assert bool((np.abs(v0.astype(np.float64) - v_shaped) <= bound_v).all())
    assert bool((err <= tol).all())


@pytest.mark.parametrize("name", ["smpl6890_new", "tree321_new"])
def test_three_frames_in_one_call_equal_three_calls(name):
    drv = _driver(name)
    P = [sr.draw_params(900 + i) for i in range(3)]
    stacked = [np.stack([p[k] for p in P]) for k in range(4)]
    for new_params in (False, True):
        together = drv.vertices(*stacked, new_params)
        assert tuple(together.shape) == (3, sr.CASES[name][1], 3)
        for i in range(3):
            alone = drv.vertices(*P[i], new_params)
            assert H.same_bits(together[i], alone[0]), (new_params, i)
        assert not H.same_bits(together[0], together[1])
    # the same inputs give the same bits
    assert H.same_bits(drv.vertices(*stacked, True), drv.vertices(*stacked, True))


def test_without_new_params_posedirs_is_never_read():
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    name = "tree321_old"
    m = _host_model(name)
    poisoned = SmplModel.from_arrays(dict(m, posedirs=np.full_like(m["posedirs"], np.nan)), DEV)
    P = sr.case_params(name)
    a = _driver(name).vertices(*P, False)
    b = PoseDriver(poisoned).vertices(*P, False)
    assert H.same_bits(a, b) and bool(torch.isfinite(b).all())
    assert bool(torch.isnan(PoseDriver(poisoned).vertices(*P, True)).all())  # and with them it is


# ---------------------------------------------------------------------------------------------------------- 1b. vertex blocks
SWEEP_V = (12, 63, 64, 65, 127, 129)  # nb_smpl_pose skins 64 vertices a workgroup; synthetic_smpl regresses a joint from 12
SWEEP_FRAMES, GUARD_FRAMES, GUARD = 3, 2, -7.0


@functools.lru_cache(maxsize=None)
def _sweep():
    """The sweep's models, parameters and float64 vertices, and E32: the largest error of the float32 restatement
    sr.forward(dtype=np.float32) against the float64 one over the sweep's cases -- what 'the same float32 sums in another order'
    costs here, computed on the host (1.0e-7 .. 2.7e-7 m a case, the size of the fixture's E_ref)."""
    cases, e32 = {}, 0.0
    for V in SWEEP_V:
        m = sr.synthetic_smpl(300 + V, V, sr.SMPL_PARENTS)
        P = [sr.draw_params(1300 + 10 * V + i) for i in range(SWEEP_FRAMES)]
        for new_params in (False, True):
            r64 = np.stack([sr.forward(m, *p, new_params, np.float64) for p in P])
            e = max(float(np.abs(sr.forward(m, *p, new_params, np.float32).astype(np.float64) - r64[i]).max()) for i, p in enumerate(P))
            e32 = max(e32, e)
            r64.setflags(write=False)
            cases[V, new_params] = dict(model=m, params=P, r64=r64, e32=e)
    return cases, e32


@functools.lru_cache(maxsize=None)
def _sweep_model(V):
    from neuralbody_amd.smpl_pose import SmplModel

    return SmplModel.from_arrays(_sweep()[0][V, False]["model"], DEV)


@pytest.mark.parametrize("new_params", [False, True])
@pytest.mark.parametrize("V", SWEEP_V)
def test_vertex_block_sweep_with_guard_rows(V, new_params):
    """V around the 64-vertex block: three frames in one call against float64 (E_FACTOR x E32), behind them guard rows of verts,
    joints and the workspace that the call must leave alone, and every frame again in a call of its own, bit for bit."""
    from neuralbody_amd import _lib, ops
    from neuralbody_amd.smpl_pose import pack_params

    cases, e32 = _sweep()
    c = cases[V, new_params]
    native, _ = _sweep_model(V).native()
    F, n = SWEEP_FRAMES, SWEEP_FRAMES + GUARD_FRAMES
    params = pack_params(*[np.stack([p[k] for p in c["params"]]) for k in range(4)]).to(DEV)
    verts = torch.full((n, V, 3), GUARD, device=DEV)
    joints = torch.full((n, _lib.SMPL_JOINTS, 3), GUARD, device=DEV)
    ws = torch.full((n, _lib.SMPL_WS_FLOATS), GUARD, device=DEV)
    ops.smpl_pose(native, params, new_params, verts=verts[:F], joints=joints[:F], ws=ws[:F])
    torch.cuda.synchronize()
    for name, t in (("verts", verts), ("joints", joints), ("ws", ws)):
        assert bool((t[F:] == GUARD).all()), "%s: written behind the %d frames" % (name, F)
    got = verts[:F].cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(joints[:F].cpu().numpy()).all()
    err = float(np.abs(got.astype(np.float64) - c["r64"]).max())
    print("V %d new_params %d: E32 %.3e (this case %.3e); max |device - fp64| %.3e = %.2f x E32" % (
        V, new_params, e32, c["e32"], err, err / e32))
    assert 5e-8 < e32 < 1e-6
    assert err <= E_FACTOR * e32
    for f in range(F):
        alone, alone_j = ops.smpl_pose(native, params[f:f + 1].contiguous(), new_params)
        assert H.same_bits(alone[0], verts[f]) and H.same_bits(alone_j[0], joints[f]), f
    assert not H.same_bits(verts[0], verts[1])


# ---------------------------------------------------------------------------------------------------------- 2. voxelisation
@functools.lru_cache(maxsize=None)
def _voxel_case(name, pad):
    g = _gold()
    verts, Rh, Th = g[name + "/verts"], g[name + "/Rh"], g[name + "/Th"]
    host = sr.host_frame(verts, Rh, Th, pad)  # computed once, shared, never written
    c64, raw = sr.coord_f64(verts, host["R"], host["Th"], pad)
    return dict(verts=verts, Rh=Rh, Th=Th, host=host, c64=c64, band=sr.near_band(c64))


def _summary(vox, f=0):
    s = vox["summary"][f].cpu().numpy()
    return s[:6].copy().view(np.float32).reshape(2, 3), s[6:9]


@pytest.mark.parametrize("name,pad", sr.VOXEL_CASES)
def test_voxelize_matches_the_host_frame(name, pad):
    from neuralbody_amd import ops

    c = _voxel_case(name, pad)
    host, V = c["host"], c["verts"].shape[0]
    vox = ops.smpl_voxelize(_dev(c["verts"][None]), _dev(c["Rh"][None]), _dev(c["Th"][None]), sr.VOXEL_SIZE, pad)
    assert {k: (tuple(v.shape), v.dtype) for k, v in vox.items()} == {
        "coord": ((1, V, 3), torch.int32), "out_sh": ((1, 3), torch.int32), "bounds": ((1, 2, 3), torch.float32),
        "R": ((1, 3, 3), torch.float32), "summary": ((1, 9), torch.int32)}
    can_bounds, sh = _summary(vox)
    # can_bounds: min and max do not depend on their order, the padding is one float32 operation
    assert np.array_equal(can_bounds.view(np.uint32), sr.padded_min_max(c["verts"], pad).view(np.uint32))
    if pad == "snapshot":
        # bit equality with rotate_smpl_frame cannot hold, whatever the kernel does: the bit-for-bit comparison above is with the
        # padded extremes of the vertices that were uploaded.
        # rotate_smpl_frame(t = 0) moves every vertex to the centroid and back through float32 (novel_view.py:103), which
        # changes a coordinate x by up to ulp(|x - centre|) / 2 + ulp(|x|) / 2 <= 2^-23 m inside a 2 m box: its can_bounds are
        # those of vertices this kernel never saw
        assert float(np.abs(can_bounds.astype(np.float64) - host["can_bounds"]).max()) <= 2.0 ** -23
    else:
        assert np.array_equal(can_bounds.view(np.uint32), host["can_bounds"].view(np.uint32))
    R = vox["R"][0].cpu().numpy()
    assert bool((np.abs(R.astype(np.float64) - host["R"]) <= np.spacing(np.abs(host["R"]))).all())
    bounds = vox["bounds"][0].cpu().numpy()
    d_bounds = float(np.abs(bounds.astype(np.float64) - host["bounds"]).max())
    assert d_bounds <= 1e-6
    out_sh = vox["out_sh"][0].cpu().numpy()
    assert np.array_equal(out_sh, host["out_sh"]) and np.array_equal(sh, out_sh) and (out_sh % 32 == 0).all()
    coord = vox["coord"][0].cpu().numpy()
    diff = coord != host["coord"]
    band = c["band"]
    print("%s %s: out_sh %s, |bounds - host| %.2e, band %.3f %% of %d, device != host at %d coordinates (%d outside the band)" % (
        name, pad, out_sh.tolist(), d_bounds, 100.0 * band.mean(), band.size, int(diff.sum()), int((diff & ~band).sum())))
    assert band.mean() <= 0.01
    assert not (diff & ~band).any()
    assert int(np.abs(coord.astype(np.int64) - host["coord"]).max()) <= 1
    # against the float64 coordinate itself, outside the band
    assert np.array_equal(coord[~band], np.round(c["c64"]).astype(np.int32)[~band])
    assert coord.min() >= 0 and (coord.max(axis=0) < out_sh).all()


def test_voxelize_two_frames_with_strided_parameters():
    from neuralbody_amd import ops

    a, b = _voxel_case("smpl6890_old", "zju"), _voxel_case("smpl6890_new", "zju")
    params = torch.zeros((2, 88), device=DEV)
    for f, c in enumerate((a, b)):
        params[f, 82:85], params[f, 85:88] = _dev(c["Rh"]), _dev(c["Th"])
    verts = _dev(np.stack([a["verts"], b["verts"]]))
    both = ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], sr.VOXEL_SIZE, "zju")
    for f, c in enumerate((a, b)):
        one = ops.smpl_voxelize(_dev(c["verts"][None]), _dev(c["Rh"][None]), _dev(c["Th"][None]), sr.VOXEL_SIZE, "zju")
        for k in one:
            assert torch.equal(both[k][f], one[k][0]), (f, k)
    assert not torch.equal(both["coord"][0], both["coord"][1])
    with pytest.raises(ValueError, match="pad"):
        ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], sr.VOXEL_SIZE, "tight")
    with pytest.raises(ValueError, match="voxel_size"):
        ops.smpl_voxelize(verts, params[:, 82:85], params[:, 85:88], (0.005, -0.005, 0.005), "zju")
    with pytest.raises(ValueError, match="strides"):
        ops.smpl_voxelize(verts, params[:, 82:85], params[:, 84:87].t().contiguous().t(), sr.VOXEL_SIZE, "zju")


# ---------------------------------------------------------------------------------------------------------- 3. driver, renderer
FRAME_SPEC = {"coord": ((1, 6890, 3), torch.int32), "out_sh": ((1, 3), torch.int32), "bounds": ((1, 2, 3), torch.float32),
              "R": ((1, 3, 3), torch.float32), "Th": ((1, 1, 3), torch.float32), "latent_index": ((1,), torch.int64)}
SIZE = 64


@functools.lru_cache(maxsize=None)
def _small_body():
    """A 6890-vertex model in the 0.3 x 0.5 x 0.2 m box of the other renderer tests, mild poses (sigma 0.1): out_sh stays small."""
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    model = SmplModel.from_arrays(sr.synthetic_smpl(21, 6890, sr.SMPL_PARENTS, box=(0.3, 0.5, 0.2)), DEV)
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(3)]
    return PoseDriver(model), [np.stack([p[k] for p in P]) for k in range(4)]


def _renderer(precision="f32"):
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer

    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, True, precision)
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=SIZE, W=SIZE))
    return rend, NovelViewRenderer(rend, SIZE, SIZE, DEV)


def _camera(can_bounds, yaw=0.35):
    K, R, T = syn.make_camera({"can_bounds": can_bounds}, SIZE, SIZE, focal_factor=2.5, distance=1.5, yaw=yaw)
    return K, np.concatenate([R, T.reshape(3, 1)], axis=1)


def test_a_driver_frame_renders_like_the_same_arrays_from_the_host():
    drv, stacked = _small_body()
    rend, nv = _renderer()
    made = drv.frames(*stacked, latent_index=[2, 3, 4], new_params=True)
    assert len(made) == 3
    frame, can_bounds = made[1]
    assert {k: (tuple(v.shape), v.dtype) for k, v in frame.items()} == FRAME_SPEC and all(v.is_cuda for v in frame.values())
    assert can_bounds.dtype == np.float32 and can_bounds.shape == (2, 3) and int(frame["latent_index"]) == 3
    K, RT = _camera(can_bounds)
    batch = nv.view_batch(K, RT, can_bounds, frame)
    # the same arrays through host numpy, in the reference's layout, as fresh tensors
    host = {k: np.ascontiguousarray(frame[k].cpu().numpy()) for k in FRAME_SPEC}
    assert [host[k].dtype for k in ("coord", "out_sh", "latent_index")] == [np.int32, np.int32, np.int64]
    batch_host = dict(batch)
    batch_host.update(H.device_batch(host, DEV))
    with torch.no_grad():
        a = rend.render(batch)
        b = rend.render(batch_host)
    assert batch["ray_o"].shape[1] > 0 and float(a["rgb_map"].max()) > 0.01
    for k in ("rgb_map", "depth_map", "acc_map"):
        assert H.same_bits(a[k], b[k]), k
    # and the frame is the host frame of the same vertices, outside the rounding band
    verts = drv.vertices(*stacked, new_params=True)[1].cpu().numpy()
    hf = sr.host_frame(verts, stacked[2][1], stacked[3][1], "zju")
    band = sr.near_band(sr.coord_f64(verts, hf["R"], hf["Th"], "zju")[0])
    assert np.array_equal(host["out_sh"][0], hf["out_sh"]) and np.array_equal(can_bounds, hf["can_bounds"])
    assert not ((host["coord"][0] != hf["coord"]) & ~band).any() and np.array_equal(host["Th"][0, 0], stacked[3][1])


def test_render_views_takes_the_drivers_views():
    drv, stacked = _small_body()
    rend, nv = _renderer()
    probe = drv.frames(*stacked, latent_index=0)
    cams = [_camera(cb, yaw=0.35 + 0.3 * f) for f, (_, cb) in enumerate(probe)]
    views = list(drv.views(cams, *stacked, latent_index=[0, 1, 2]))
    assert len(views) == 3 and all(len(v) == 4 for v in views)
    outs = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()} for o in nv.render_views(iter(views))]
    assert len(outs) == 3
    for f, (view, out) in enumerate(zip(views, outs)):
        ref = nv.render_view(*view)
        assert out["n_rays"] == ref["n_rays"] > 0 and bool(torch.isfinite(out["img"]).all())
        assert tuple(out["img"].shape) == (SIZE, SIZE, 3) and float(out["img"].max()) > 0.01
        assert H.same_result(out["img"], ref["img"], "f32"), f
    assert not torch.equal(outs[0]["img"], outs[1]["img"])
    # one camera for every frame
    K, RT = cams[0]
    assert len(list(drv.views([(K, RT)], *stacked, latent_index=0))) == 3
    with pytest.raises(ValueError, match="cameras"):
        list(drv.views(cams[:2], *stacked, latent_index=0))


# ---------------------------------------------------------------------------------------------------------- 4. plugin
def test_plugin_item_is_the_batch_dict():
    from torch.utils.data.dataloader import default_collate

    from neuralbody_amd.smpl_pose import MemoryPoseSource

    drv, stacked = _small_body()
    items = [dict(poses=stacked[0][i], shapes=stacked[1][i], Rh=stacked[2][i], Th=stacked[3][i]) for i in range(3)]
    _, can_bounds = drv.frames(*stacked, latent_index=0)[0]
    K, RT = _camera(can_bounds)
    cfg = types.SimpleNamespace(begin_ith_frame=5, frame_interval=2, num_train_frame=2, num_render_frame=-1, voxel_size=[0.005] * 3,
                                big_box=False, test_view=[0], H=SIZE, W=SIZE, ratio=1.0, params="new_params",
                                train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1))
    mod = H.load_plugin("light_stage_pose_dataset.py", cfg)
    ds = mod.Dataset("nowhere", "synthetic", "none.npy", "test", source=MemoryPoseSource(items, K, RT[:, :3], RT[:, 3], SIZE, SIZE),
                     model=drv.model, device=DEV)
    assert len(ds) == 3 and ds.cfg.smpl_new_params is True
    got = [ds[i] for i in range(3)]
    assert [int(it["latent_index"]) for it in got] == [0, 1, 1] and [it["frame_index"] for it in got] == [5, 7, 9]
    it = got[0]
    n = it["ray_o"].shape[0]
    spec = {"ray_o": ((n, 3), torch.float32), "ray_d": ((n, 3), torch.float32), "near": ((n,), torch.float32),
            "far": ((n,), torch.float32), "mask_at_box": ((SIZE * SIZE,), torch.bool), "coord": ((6890, 3), torch.int32),
            "out_sh": ((3,), torch.int32), "bounds": ((2, 3), torch.float32), "R": ((3, 3), torch.float32),
            "Th": ((1, 3), torch.float32), "latent_index": ((), torch.int64)}
    assert {k: (tuple(v.shape), v.dtype) for k, v in it.items() if k != "frame_index"} == spec
    assert all(v.is_cuda for k, v in it.items() if k != "frame_index") and n == int(it["mask_at_box"].sum()) > 0
    frame = drv.frames(*[s[:1] for s in stacked], latent_index=0, new_params=True)[0][0]
    assert torch.equal(it["coord"], frame["coord"][0]) and torch.equal(it["bounds"], frame["bounds"][0])
    rend, _ = _renderer()
    with torch.no_grad():
        out = rend.render(default_collate([it]))
    assert tuple(out["rgb_map"].shape) == (1, n, 3) and bool(torch.isfinite(out["rgb_map"]).all()) and float(out["rgb_map"].max()) > 0.01
