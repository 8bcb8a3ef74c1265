"""The vanilla-NeRF baseline's mesh pass on the device (run with -m gpu on an MI355X): nb_nerf_density exactly on a dyadic lattice
and bit for bit against nb_nerf_decode, NerfMeshRenderer's cube against the reference's (tests/golden/nerf_mesh.npz) and the
float64 trunk of tests/nerf_mesh_ref.py, the mesh behind it, nb_nerf_embed_grad alone, NerfNetwork.density_gradient against the
float64 chain under the device's own relu masks, and the options end to end through the plugins."""
import types

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import nerf_mesh_ref as mref
from tests import nerf_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAST_BUDGET = 1e-4  # README: the contract on every map; an arithmetic that serves as default is held to half of it
MODELS = (("model", "", 0), ("model_fine", "fine", 128))  # (state-dict prefix, NerfNetwork's name, an N_importance that selects it)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from neuralbody_amd import _lib

    _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _net(sd, precision="f32"):
    from neuralbody_amd.nerf import NerfNetwork

    net = NerfNetwork(precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(DEV).eval()


def _precisions():
    from neuralbody_amd import ops

    return sorted(ops.NERF_PRECISIONS)  # every arithmetic that is built


def _renderer(net, iso, N_importance, **kw):
    from neuralbody_amd.nerf import NerfMeshConfig, NerfMeshRenderer

    return NerfMeshRenderer(net, NerfMeshConfig(mesh_th=iso, N_importance=N_importance, mesh_backend="device", **kw))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(hp.GOLDEN + "/nerf_mesh.npz"))


@pytest.fixture(scope="module")
def sd(fx):
    sd = ref.make_state_dict(fx["alpha_shift"])
    assert ref.checksum(sd) == str(fx["weights_sha256"]), "the seed recipe no longer gives the fixture's weights"
    return sd


@pytest.fixture(scope="module")
def lat():
    """The fixture's lattice: host arrays, the 944 inside points and the two batch forms RendererMesh accepts, on the device."""
    pts, inside = mref.lattice()
    wbounds = np.array([[a[0] for a in mref.AXES], [a[-1] for a in mref.AXES]], np.float32)
    common = {"inside": _dev(inside.astype(np.uint8))[None], "wbounds": _dev(wbounds)[None], "frame_index": torch.tensor([7]),
              "i": torch.tensor([7])}
    b_pts = dict(common, pts=_dev(pts)[None])
    b_axes = dict(common, **{"axis_" + k: _dev(a)[None] for k, a in zip("xyz", mref.AXES)})
    return types.SimpleNamespace(pts=pts, inside=inside, pin=pts[inside], b_pts=b_pts, b_axes=b_axes)


@pytest.fixture(scope="module")
def model64(sd, lat):
    """The float64 trunk at the 944 inside points, once per module: (alpha [944], pre-activations)."""
    return {m: mref.trunk(sd, m, lat.pin) for m in ref.MODULES}


# ------------------------------------------------------------------------------------------------ 1: exact lattice
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 576])  # one point, a tile - 1, a tile, a tile + 1, two tiles - 1, nine tiles
def test_density_is_exact_on_the_lattice(n):
    """Dyadic weights and points: every product and partial sum is exact in fp32 (and in an fp16 head), so any summation order
    must give the float64 model's numbers (compared as values).  The premise is audited for these very inputs."""
    sd = ref.lattice_state_dict()
    o, d, z = ref.lattice_rays(3, 192)
    pts = ref.points_f32(o, d, z).reshape(-1, 3)[:n]
    assert pts.shape == (n, 3)
    for prec in _precisions():
        net = _net(sd, prec)
        for m, model, _ in MODELS:
            with torch.no_grad():
                got = net.density(_dev(pts), model=model)
            assert tuple(got.shape) == (n,) and got.dtype == torch.float32
            if n == 0:
                continue
            audit = []
            want = ref.forward(sd, m, pts[:, None, :], np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n, 1)), audit=audit)[:, 0, 3]
            assert max(audit) < 24
            assert np.array_equal(want, mref.trunk(sd, m, pts)[0])
            got = got.cpu().numpy()
            bad = np.argwhere(got.astype(np.float64) != want)
            assert bad.size == 0, "%s %s: %d of %d differ, first at %s: %r vs %r" % (
                prec, m, len(bad), n, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
            assert np.abs(want).max() > 0


# ------------------------------------------------------------------------------------------------ 2: the bits of nb_nerf_decode
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_density_has_the_bits_of_the_full_kernel_s_fourth_column(sd, lat, precision):
    net = _net(sd, precision)
    pts = _dev(lat.pin)
    rs = np.random.RandomState(11)
    vd = rs.normal(size=(len(lat.pin), 3))
    vd = _dev((vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32))
    with torch.no_grad():
        for _, model, _ in MODELS:
            alpha = net.density(pts, model=model)
            raw = net.forward(pts[:, None], vd, model=model)
            assert raw.shape == (944, 1, 4) and alpha.shape == (944,)
            assert hp.same_bits(alpha, raw[:, 0, 3]), "%s %r: %d of 944 differ" % (
                precision, model, int((alpha != raw[:, 0, 3]).sum()))
            assert hp.same_bits(net.density(pts, model=model), alpha)  # no atomics: the same bits again
            assert float(alpha.abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------ 3: the cube
def test_cube_against_the_reference_and_float64(fx, sd, lat, model64):
    net = _net(sd, "f32")
    P, e_ref = mref.PAD, float(fx["e_ref_cube"])
    for i, (m, _, N) in enumerate(MODELS):
        r = _renderer(net, float(fx["iso"][i]), N)
        with torch.no_grad():
            cube_axes, cube_pts = r.density_cube(lat.b_axes), r.density_cube(lat.b_pts)
        assert tuple(cube_axes.shape) == (36, 34, 32) and cube_axes.dtype == torch.float32 and cube_axes.is_cuda
        assert hp.same_bits(cube_axes, cube_pts)
        cube = cube_axes.cpu().numpy()
        core = cube[P:-P, P:-P, P:-P]
        assert np.all(core[~lat.inside] == 0) and np.count_nonzero(cube) == np.count_nonzero(core) == 944
        gap_ref = float(np.abs(core[lat.inside] - fx["cube_ref"][i][P:-P, P:-P, P:-P][lat.inside]).max())
        gap_64 = float(np.abs(core[lat.inside] - model64[m][0]).max())
        print("%s: |cube - reference| %.3e, |cube - float64| %.3e, e_ref_cube %.3e, allowed %.3e" % (m, gap_ref, gap_64, e_ref, 8 * e_ref))
        assert gap_ref <= 8 * e_ref


def test_cube_of_the_default_arithmetic_is_within_half_the_budget(fx, sd, lat, model64):
    net = _net(sd, "auto")
    P = mref.PAD
    for i, (m, _, N) in enumerate(MODELS):
        with torch.no_grad():
            cube = _renderer(net, float(fx["iso"][i]), N).density_cube(lat.b_axes).cpu().numpy()
        gap = float(np.abs(cube[P:-P, P:-P, P:-P][lat.inside] - model64[m][0]).max())
        print("%s (%s): |cube - float64| %.3e, allowed %.1e" % (m, net.nerf_precision(), gap, FAST_BUDGET / 2))
        assert gap <= FAST_BUDGET / 2


# ------------------------------------------------------------------------------------------------ 4: the mesh
def _rows(a):
    return [r.tobytes() for r in np.ascontiguousarray(a)]


def test_mesh_is_marching_cubes_of_the_cube_and_has_the_reference_s_triangles(fx, sd, lat):
    from neuralbody_amd import ops

    net = _net(sd, "f32")
    for i, (m, model, N) in enumerate(MODELS):
        iso = float(fx["iso"][i])
        r = _renderer(net, iso, N)
        with torch.no_grad():
            cube = r.density_cube(lat.b_axes)
            assert hp.same_bits(cube[10:-10, 10:-10, 10:-10][_dev(lat.inside)], net.density(_dev(lat.pin), model=model))  # N selects
            v, t = r.extract_mesh(lat.b_axes)
            v_mc, t_mc = ops.marching_cubes(cube, iso)
            v_ref, t_ref = ops.marching_cubes(_dev(fx["cube_ref"][i]), iso)
        assert v.shape[0] > 100 and t.shape[0] > 100 and t.dtype == torch.int32
        assert hp.same_bits(v, v_mc) and torch.equal(t, t_mc)
        assert torch.equal(t, t_ref), "another topology than the reference's cube gives"
        # a crossing sits at (iso - a) / (b - a) of its edge with |a - iso|, |b - iso| >= margin: values that move by at most d move it
        # by at most d / margin (plus the fp32 rounding of the position itself, 36 * 2^-24)
        assert float((v - v_ref).abs().max()) <= 8 * float(fx["e_ref_cube"]) / float(fx["iso_margin"][i]) + 1e-5
        with torch.no_grad():
            vw, tw = r.extract_mesh(lat.b_pts, world=True)
            vl, tl = r.extract_mesh(lat.b_axes, components="largest")
            out = r.render(lat.b_axes)
        assert torch.equal(tw, t) and hp.same_bits(vw, (v - 10.0) * _dev(np.array([a[1] - a[0] for a in mref.AXES])) + _dev(
            np.array([a[0] for a in mref.AXES])))
        # "largest": a sub-mesh whose vertices and triangles keep the order they have in the whole mesh
        index = {row: k for k, row in enumerate(_rows(v.cpu().numpy()))}
        kept = np.array([index[row] for row in _rows(vl.cpu().numpy())])
        assert len(index) == v.shape[0] and 0 < len(kept) <= v.shape[0] and np.all(np.diff(kept) > 0)
        whole = _rows(t.cpu().numpy())
        sub = _rows(kept[tl.cpu().numpy()].astype(np.int32))
        it = iter(whole)
        assert 0 < len(sub) <= len(whole) and all(row in it for row in sub)  # a subsequence, in order
        print("%s: %d vertices, %d triangles; largest component %d, %d" % (m, v.shape[0], t.shape[0], vl.shape[0], tl.shape[0]))
        # render(): the dict of RendererMesh.render
        assert set(out) == {"cube", "mesh"} and out["cube"].dtype == np.float64 and out["cube"].shape == (36, 34, 32)
        assert np.array_equal(out["cube"], cube.double().cpu().numpy())
        assert np.array_equal(np.asarray(out["mesh"].vertices), v.double().cpu().numpy())
        assert np.array_equal(np.asarray(out["mesh"].faces), t.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 5: nb_nerf_embed_grad alone
@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("wide", [False, True])
def test_embed_grad_is_the_float64_formula_rounded_once(n, wide):
    from neuralbody_amd import ops

    rs = np.random.RandomState(100 + n)
    cols, first = (ops.NERF_TAP_COLS, ops.NERF_TAP["pts"][0]) if wide else (64, 0)  # strides 2528 and 64
    emb_w, d_w = rs.uniform(-1, 1, (n, cols)).astype(np.float32), rs.normal(size=(n, cols)).astype(np.float32)
    emb, d_emb = _dev(emb_w)[:, first:first + 64], _dev(d_w)[:, first:first + 64]
    assert emb.stride(0) == cols
    got = ops.nerf_embed_grad(emb, d_emb).cpu().numpy()
    want64 = mref.embed_gradient(emb_w[:, first:first + 63], d_w[:, first:first + 63])
    want = want64.astype(np.float32)
    # float64 sums in another order differ by 1e-16 relative: after the one rounding, the same fp32 or its neighbour
    near = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    assert got.shape == (n, 3) and near.all(), "%d of %d beyond the adjacent fp32" % ((~near).sum(), near.size)
    print("n %d stride %d: %d of %d equal, the rest adjacent" % (n, cols, (got == want).sum(), got.size))


# ------------------------------------------------------------------------------------------------ 6: the gradient
def _device_masks(net, pts, model):
    """The relu masks of the device's own f32 forward at these points (h > 0, the rule the chain uses)."""
    from neuralbody_amd import ops

    n = pts.shape[0]
    d = torch.zeros_like(pts)
    d[:, 2] = 1.0
    with torch.no_grad():
        _, tap = ops.nerf_decode_tap(net.packed(model), pts, d, torch.zeros((n, 1), device=DEV))
    tap = tap.cpu().numpy()
    return [tap[:, 256 * i:256 * i + 256] > 0 for i in range(8)]


def test_density_gradient_against_float64_under_the_device_s_masks(fx, sd, lat, model64):
    net = _net(sd, "f32")
    e_ref = float(fx["e_ref_grad"])
    pts = _dev(lat.pin[:mref.N_GRAD])
    for i, (m, model, _) in enumerate(MODELS):
        masks = _device_masks(net, pts, model)
        z64 = [z[:mref.N_GRAD] for z in model64[m][1]]
        differ = [(a != (z > 0)) for a, z in zip(masks, z64)]
        assert all(np.all(np.abs(z[f]) < 1e-4) for f, z in zip(differ, z64)), "a mask differs at a unit far from 0"
        want = mref.trunk_gradient(sd, m, lat.pin[:mref.N_GRAD], masks=masks)
        with torch.no_grad():
            alpha, grad = net.density_gradient(pts, model=model)
            assert hp.same_bits(alpha, net.density(pts, model=model))
        gap = float(np.abs(grad.cpu().numpy() - want).max())
        gap_ref = float(np.abs(grad.cpu().numpy() - fx["grad_ref"][i]).max())
        print("%s: |grad - float64| %.3e (e_ref_grad %.3e, allowed %.3e), max |grad| %.1f, %d masks differ from float64's, "
              "|grad - reference autograd| %.3e" % (m, gap, e_ref, 8 * e_ref, np.abs(want).max(), sum(f.sum() for f in differ), gap_ref))
        assert grad.shape == (mref.N_GRAD, 3) and gap <= 8 * e_ref
        # 32 points per chunk: three chunks
        small = _net(sd, "f32")
        small.GRADIENT_CHUNK_BYTES = 32 * 4 * (2528 + 2432)
        with torch.no_grad():
            alpha_c, grad_c = small.density_gradient(pts, model=model)
        print("%s: in chunks of 32 the gradient is %sbit-equal" % (m, "" if hp.same_bits(grad_c, grad) else "NOT "))
        assert hp.same_bits(alpha_c, alpha) and float(np.abs(grad_c.cpu().numpy() - want).max()) <= 8 * e_ref


def test_density_gradient_of_the_auto_network_is_the_f32_one(sd, lat):
    """The gradient's forward is always f32, whatever the inference precision."""
    pts = _dev(lat.pin[:mref.N_GRAD])
    with torch.no_grad():
        a, g = _net(sd, "f32").density_gradient(pts, model="fine")
        b, h = _net(sd, "f16x3").density_gradient(pts, model="fine")
    assert hp.same_bits(a, b) and hp.same_bits(g, h)


def test_density_gradient_beyond_the_exact_gemm_s_size(fx, sd, lat):
    """1888 points (the 944 twice) cross into nb_sgemm's bf16-pair kernel: 2^-16 relative per product (include/nb_hip.h), with a
    sixteen-fold margin for nine chained products whose intermediates may exceed the result."""
    net = _net(sd, "f32")
    host = np.concatenate([lat.pin, lat.pin])
    pts = _dev(host)
    assert len(host) >= 1024
    for m, model, _ in MODELS:
        want = mref.trunk_gradient(sd, m, host, masks=_device_masks(net, pts, model))
        with torch.no_grad():
            alpha, grad = net.density_gradient(pts, model=model)
            assert hp.same_bits(alpha, net.density(pts, model=model))
        grad = grad.cpu().numpy()
        gap, bound = float(np.abs(grad - want).max()), 8 * float(fx["e_ref_grad"]) + 2.0 ** -12 * float(np.abs(want).max())
        print("%s: n = %d, |grad - float64| %.3e, allowed %.3e (max |grad| %.1f)" % (m, len(host), gap, bound, np.abs(want).max()))
        assert gap <= bound
        assert np.array_equal(grad[:944], grad[944:])  # a row's result does not depend on where it stands


def test_no_points(sd):
    net = _net(sd, "f32")
    with torch.no_grad():
        alpha, grad = net.density_gradient(torch.zeros((0, 3), device=DEV))
    assert tuple(alpha.shape) == (0,) and tuple(grad.shape) == (0, 3)


# ------------------------------------------------------------------------------------------------ 7: options, through the plugins
_CFG = dict(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10, view_res=4, nerf_precision="f32")


def _plugin_mesh(sd, lat, iso, result_dir):
    """render() and extract_mesh() of the fine module through the plugins with every option on -> what the checks below look at."""
    from neuralbody_amd import ops

    cfg = types.SimpleNamespace(mesh_th=iso, N_importance=128, mesh_color=True, mesh_normals="field", mesh_components="largest",
                                result_dir=str(result_dir), **_CFG)
    net = hp.load_plugin("nerf.py", cfg).Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(DEV)
    renderer = hp.load_plugin("volume_mesh_renderer.py", cfg).Renderer(net)
    with torch.no_grad():
        out = renderer.render(lat.b_axes)
        mesh = renderer.extract_mesh(lat.b_axes, components="largest", colors=True, normals="field")
        face = ops.mesh_vertex_normals(mesh.wpts, mesh.triangles)
        grad = net.density_gradient(mesh.wpts, model="fine")[1]
    fallback = (mesh.normals == face).all(1)
    # unit (or the face normal where the gradient vanishes), and always against the gradient
    assert bool(((mesh.normals.norm(dim=1) - 1).abs() < 1e-5)[~fallback].all())
    assert bool(((mesh.normals * grad).sum(1) < 0)[~fallback].all())
    sides = ((mesh.normals * face).sum(1) > 0).cpu().numpy()
    # a vertex sits on a lattice edge; where one end of that edge is outside `inside` the cube's 0 there is no value of the field: the
    # vertex belongs to the cut the carving makes, and its face normal is the cut's
    v = mesh.vertices.cpu().numpy().astype(np.float64) - mref.PAD
    lo, hi = np.floor(v).astype(int), np.ceil(v).astype(int)
    shape = np.array(lat.inside.shape)
    inner = np.ones(len(v), bool)
    for end in (lo, hi):
        ok = np.all((end >= 0) & (end < shape), axis=1)
        inner &= ok & lat.inside[tuple(np.clip(end, 0, shape - 1).T)]
    print("%d vertices, %d keep their face normal, %d on edges inside the carved region; within 90 degrees of the face normal: %.3f "
          "of all, %.3f of those" % (len(v), int(fallback.sum()), inner.sum(), sides.mean(), sides[inner].mean() if inner.any() else -1))
    return types.SimpleNamespace(cfg=cfg, net=net, out=out, mesh=mesh, sides=sides, inner=inner)


def test_options_end_to_end_through_the_plugins(fx, sd, lat, tmp_path):
    from neuralbody_amd import ops
    from neuralbody_amd.mesh import TriMesh

    iso = float(fx["iso"][1])
    run = _plugin_mesh(sd, lat, iso, tmp_path)
    cfg, net, out, mesh = run.cfg, run.net, run.out, run.mesh
    with torch.no_grad():
        raw = net(mesh.wpts[:, None].contiguous(), mesh.viewdir, model="fine")
        rgb_f, rgb_u8 = ops.mesh_color_finish(raw.reshape(-1, 4).contiguous())
    tm = out["mesh"]
    assert isinstance(tm, TriMesh) and tm.vertex_colors is not None and tm.vertex_normals is not None
    V = len(tm.vertices)
    assert V > 100 and V == mesh.vertices.shape[0] and np.array_equal(tm.faces, mesh.triangles.cpu().numpy())
    assert np.array_equal(tm.vertex_colors, rgb_u8.cpu().numpy()) and hp.same_bits(mesh.rgb_f, rgb_f)
    assert len(np.unique(tm.vertex_colors, axis=0)) > 10
    # the colour head was asked at the world vertices, looking along -normal
    assert torch.equal(mesh.viewdir, -mesh.normals) and np.array_equal(tm.vertex_normals, mesh.normals.cpu().numpy())
    wv = (mesh.vertices - 10.0) * _dev(np.array([a[1] - a[0] for a in mref.AXES])) + _dev(np.array([a[0] for a in mref.AXES]))
    assert hp.same_bits(mesh.wpts, wv)
    # the visualizer writes what TriMesh.load_ply reads back
    vis = hp.load_plugin("if_nerf_mesh.py", cfg).Visualizer()
    path = vis.visualize(out, lat.b_axes)
    assert path.endswith("0007.ply")
    back = TriMesh.load_ply(path)
    assert np.array_equal(back.vertices, tm.vertices.astype(np.float32).astype(np.float64)) and np.array_equal(back.faces, tm.faces)
    assert np.array_equal(back.vertex_colors, tm.vertex_colors) and np.array_equal(back.vertex_normals, tm.vertex_normals)
    # the evaluator takes the dict as well
    ev = hp.load_plugin("if_nerf_mesh.py", cfg).Evaluator()
    saved = np.load(ev.evaluate(out, lat.b_pts))
    assert saved.shape == (int((out["cube"][10:-10, 10:-10, 10:-10] > iso).sum()), 3)


def test_field_normals_side_with_the_face_normals(sd, lat, tmp_path):
    """mesh_normals: field through the plugins on the 16 x 14 x 12 lattice: every normal is unit (or the face normal where the
    gradient vanishes) and opposes the device's gradient (both asserted for every vertex in _plugin_mesh), and it is within 90
    degrees of its face normal for at least 90 % of the vertices whose face normal is the field's: the sign check on -grad, where a
    flipped sign gives about 0.  Two things decide where a face normal is the field's; both are worked out in float64 without the
    device (tests/test_nerf_mesh_host.py holds the figures) and neither depends on the implementation.

    The weights.  A face normal is the gradient of the LATTICE's samples, so the check presupposes a field this lattice resolves.
    The recipe's field is not one: its gradient is carried by the embedding's frequencies up to 2^9 rad per unit (a wavelength of
    0.012) while the lattice steps by 0.08; its analytic gradient (median length 178 / 164) sides with the lattice's central
    differences (6.2 / 5.5) at 0.585 / 0.597 of the inside points.  The device reads 0.545 of 110 vertices there (printed by the
    end-to-end test above), where a flipped sign would read 0.455: that field cannot show the sign.  So this test switches the
    frequencies 2^3 and above off in pts_linears[0] and in the skip layer of the same weights: 2^2 x 0.08 = 0.32 rad per step, and
    the analytic gradient sides with the lattice differences at 0.998 / 1.000 of the inside points.

    The vertices.  The cube is 0 outside `inside`, so the iso-surface also runs along the cut the carving makes, wherever an
    inside value on the far side of the iso value has an outside neighbour.  On this small lattice that is half of the surface (a
    float64 emulation of the crossings: 436 of this case's 658 vertices, and between 0.3 and 0.9 of them for every iso value tried,
    also with the whole lattice inside).  A face normal there is the cut's, unrelated to the field: over all vertices the float64
    emulation expects 0.46 here and the device read 0.427, on a field where the emulation expects 1.000 on the other vertices.  So
    the share is taken over the vertices on lattice edges with both ends inside, and the share over all is printed."""
    smooth = mref.band_limited(sd)
    alpha = mref.trunk(smooth, "model_fine", lat.pin)[0]
    iso = float(np.float32(np.median(alpha)))
    assert 0.3 <= np.mean(alpha > iso) <= 0.7 and iso != 0.0
    run = _plugin_mesh(smooth, lat, iso, tmp_path)
    assert run.inner.sum() >= 100
    assert run.sides[run.inner].mean() >= 0.9
