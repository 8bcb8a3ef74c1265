"""Field normals on the device: nb_trilinear_grad, nb_normal_select, nb_normal_composite (csrc/nb_field_normal.hip), Network.
calculate_density_gradient above them, Renderer.render(normals=True) and RendererMesh.extract_mesh(normals="field").  Cases, float64
references and bounds: tests/field_normal_cases.py (checked on the CPU by tests/test_field_normals_host.py).

  1. exact lattice: bit equality with the float64 model, POISON in the rows that carry no weight, four mutants of the model fail
  2. realistic gather: |got - ref| <= GRAD_C A per component
  3. the chain under the tap's own ReLU masks, around the 1024-row kernel switch, and split into chunks
  4. end to end against float64 autograd of the oracle
  5. select / composite against their numpy restatements, bit for bit
  6. render(normals=True) against the composition done in torch
  7. the mesh with field normals
"""
import os

import numpy as np
import pytest
import torch

from tests import decode_f32_cases as dc
from tests import field_normal_cases as fc
from tests import helpers as H
from tests import march_ray_cases as R
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
_CACHE = {}


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _grad(pose, voxel, out_sh, grids, rows, pts, d_feat):
    """nb_trilinear_grad of host arrays -> numpy [n, 3]; the scene carries shapes only (its dense volumes are never read)"""
    from neuralbody_amd import ops

    sc = ops.NbScene()
    for l, g in enumerate(grids):
        for k in range(3):
            sc.vol_dhw[l][k] = int(g.shape[k])
    pose_t = ops.make_pose(pose["R"], pose["Th"], pose["bmin"], device=DEV)
    sc.pose = pose_t.data_ptr()
    for k in range(3):
        sc.voxel_size[k], sc.out_sh[k] = float(voxel[k]), int(out_sh[k])
    out = ops.trilinear_grad((sc, [pose_t]), [_dev(g) for g in grids], [_dev(r) for r in rows], _dev(pts), _dev(d_feat))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("pose", list(dc.POSES))
@pytest.mark.parametrize("n", fc.LATTICE_N)
def test_trilinear_grad_lattice_bit_for_bit(n, pose):
    """EXACT.  Points on voxel planes (the right-hand derivative), in the zero-padding rim, beyond the clamp (gradient 0) and beside
    inactive voxels, under the identity and a signed permutation.  The same bits with POISON in every row that no point reads with a
    non-zero weight pair; four mutants of the model are told apart."""
    w, d, ref, A, touched = fc.lattice_reference(pose, n)
    fc.assert_grad_lattice(ref, A)
    rows = fc.rows_of(dc.distinct_volumes(), fc.lattice_grids())
    got = _grad(dc.POSES[pose], dc.VOXEL, dc.OUT_SH, fc.lattice_grids(), rows, w, d)
    bad = np.argwhere(got != ref.astype(F32))
    assert len(bad) == 0, "%d components differ, the first at %s: got %r, want %r" % (len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    got2 = _grad(dc.POSES[pose], dc.VOXEL, dc.OUT_SH, fc.lattice_grids(), fc.rows_of(dc.distinct_volumes(), fc.lattice_grids(), touched), w, d)
    assert np.array_equal(got2.view(np.uint32), got.view(np.uint32)), "a row that carries no weight reached the gradient"
    if n == max(fc.LATTICE_N):
        for mutate in fc.MUTANTS:
            if mutate == "R_transposed" and pose == "identity":
                continue
            assert (got != fc.lattice_reference(pose, n, mutate)[2].astype(F32)).any(), mutate


# ------------------------------------------------------------------------------------------------------------------------- 2
def test_trilinear_grad_realistic_within_its_bound():
    s = fc.realistic_case()
    rows = fc.rows_of(s["vols"], s["grids"])
    got = _grad(s["pose"], s["voxel"], s["out_sh"], s["grids"], rows, s["pts"], s["d_feat"]).astype(np.float64)
    assert np.abs(s["grad"]).max() > 100.0 and (s["A"] > 0).mean() > 0.3
    live = s["A"] > 0
    ratio = float((np.abs(got - s["grad"])[live] / (fc.GRAD_C * s["A"][live])).max())
    print("realistic nb_trilinear_grad: largest |got - ref| / (GRAD_C A) = %.4f over %d components" % (ratio, int(live.sum())))
    assert not got[~live].any()
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------------- 3
def _small_dense():
    def make():
        from neuralbody_amd.renderer import RenderConfig, Renderer

        r, sd, body, batch, cam, _ = scenes.build("small_dense")
        net = H.make_network(sd, DEV, True, "f16f6")  # (the gradient is exact fp32 whatever the Network marches with)
        bd = H.device_batch(batch, DEV)
        rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, white_bkgd=True))
        with torch.no_grad():
            sp = rend.prepare_sp_input(bd)
            fv = net.encode_sparse_voxels(sp)
        rays = slice(0, 272, 16)
        z = R.z_vals_f32(batch["near"][0][rays], batch["far"][0][rays], np.linspace(0.0, 1.0, 64, dtype=F32))
        wpts = R.sample_points_f32(batch["ray_o"][0][rays], batch["ray_d"][0][rays], z)[0].reshape(-1, 3)
        vols_cl = [v[0].permute(1, 2, 3, 0).cpu().numpy() for v in fv.dense()]
        return dict(sd=sd, batch=batch, net=net, sp=sp, fv=fv, wpts=wpts, vols_cl=vols_cl)

    return _cached("small_dense", make)


@pytest.mark.parametrize("n", fc.CHAIN_N)
def test_chain_under_the_taps_own_masks(n):
    """d_feat and grad of calculate_density_gradient against the float64 chain that takes the ReLU masks from the device tap and the
    cells from the kernel's fp32 coordinates: 1e-4 of the largest reference entry, the tolerance tests/test_gpu_backward.py holds these
    GEMM kernels to."""
    s = _small_dense()
    b = s["batch"]
    p = s["wpts"][:n]
    with torch.no_grad():
        sigma, grad = s["net"].calculate_density_gradient(_dev(p)[None], s["fv"], s["sp"])
        sig0 = s["net"].calculate_density(_dev(p)[None], s["fv"], s["sp"], precision="f32")
        # the same chunk once more through the per-chunk helper, for its tap and d_feat (the public call drops them)
        raw, tap, d_feat, g_again = s["net"]._gradient_chunk(s["net"]._gradient_context(s["fv"], s["sp"]), _dev(p))
    torch.cuda.synchronize()
    assert sigma.shape == (1, n, 1) and grad.shape == (1, n, 3)
    assert H.same_bits(sigma, sig0) and H.same_bits(g_again, grad[0]) and H.same_bits(raw[:, 3:4].contiguous(), sigma[0])
    tap, d_feat = tap.cpu().numpy(), d_feat.cpu().numpy()
    from neuralbody_amd.ops import TAP

    h = [tap[:, TAP[k][0]:TAP[k][1]] for k in ("h1", "h2", "h3")]
    ref_d = fc.chain_f64(s["sd"], *h)
    err_d = float(np.abs(d_feat - ref_d).max() / np.abs(ref_d).max())
    out_sh = [int(v) for v in s["sp"]["out_sh"]]
    g32 = dc.grid_coords32(p, b["R"][0], b["Th"][0].reshape(-1)[:3], b["bounds"][0, 0], (0.005,) * 3, out_sh)
    ref_g, _, _ = fc.grad_f64(g32, ref_d, s["vols_cl"], fc.VOXEL32, out_sh, np.asarray(b["R"][0], np.float64), index_dtype=F32)
    err_g = float(np.abs(grad[0].cpu().numpy() - ref_g).max() / max(np.abs(ref_g).max(), 1e-30))
    print("chain n = %d: d_feat %.3g, grad %.3g of the largest reference entry (%.3g, %.3g)" % (n, err_d, err_g, np.abs(ref_d).max(),
                                                                                                np.abs(ref_g).max()))
    if n > 1:
        assert np.abs(ref_g).max() > 1.0
    assert err_d <= fc.CHAIN_TOL and err_g <= fc.CHAIN_TOL


def test_chunks_agree():
    s = _small_dense()
    p = _dev(s["wpts"][:1025])[None]
    with torch.no_grad():
        s0, g0 = s["net"].calculate_density_gradient(p, s["fv"], s["sp"])
        s1, g1 = s["net"].calculate_density_gradient(p, s["fv"], s["sp"], chunk=512)  # chunks of 512, 512 and 1 point
    assert H.same_bits(s0, s1)
    err = float((g0 - g1).abs().max() / g0.abs().max())
    print("chunk 512 against one chunk of 1025: %.3g of the largest entry" % err)
    assert err <= fc.CHUNK_TOL


# ------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", fc.E2E_SCENES)
def test_gradient_against_float64_autograd_of_the_oracle(name):
    """On the oracle's own volumes (a plain list: the active set comes from nb_sparsify), at the 1024 samples of rays 0:256:16 less
    the points whose ReLU pattern or cell fp32 may decide the other way (computed from the reference alone, share under 10 %)."""
    gradient_against_float64_autograd(name)


def gradient_against_float64_autograd(name, voxel_size=None, first_ray=0):
    """The check of the test above; `voxel_size` (dhw, None: the fixtures' 5 mm cube) and `first_ray` for
    tests/test_gpu_aniso_voxels.py."""
    e = fc.e2e_reference(name, voxel_size, first_ray)
    assert 1.0 - e["keep"].mean() <= fc.EXCLUDE_CAP
    net = H.make_network(e["sd"], DEV, e["recipe"]["mode"] == "train", "f32", voxel_size)
    bd = H.device_batch(e["batch"], DEV)
    sp = H.sp_input_of(bd, e["out_sh"])
    with torch.no_grad():
        sigma, grad = net.calculate_density_gradient(_dev(e["wpts"])[None], [v.to(DEV) for v in e["vols"]], sp)
    g = grad[0].cpu().numpy().astype(np.float64)
    k = e["keep"]
    scale = np.abs(e["g64"]).max()
    err = np.abs(g - e["g64"])[k].max() / scale
    H.assert_close(sigma[0, :, 0].cpu().numpy()[k], e["sigma64"][k], 1e-4, "sigma")
    n64, n32 = np.linalg.norm(e["g64"], axis=1), np.linalg.norm(g, axis=1)
    big = k & (n64 >= fc.E2E_SIN_FROM * scale)
    sin = np.linalg.norm(np.cross(g[big] / n32[big, None], e["g64"][big] / n64[big, None]), axis=1)
    print("%s: |g - g64| <= %.3g max |g64| on %d kept points; sin(angle) <= %.3g on %d" % (name, err, k.sum(), sin.max(), big.sum()))
    assert err <= fc.E2E_TOL
    assert sin.max() <= fc.E2E_SIN


# ------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("jitter", (False, True))
@pytest.mark.parametrize("shape", fc.SELECT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_select_and_composite_bit_for_bit(shape, jitter):
    from neuralbody_amd import ops

    n, S = shape
    ro, rd, ne, fa, tv, tr, w = fc.select_inputs(n, S)
    tr = tr if jitter else None
    args = [_dev(x) for x in (ro, rd, ne, fa, tv)] + [None if tr is None else _dev(tr), _dev(w)]
    w_all = w
    # some, none (m = 0), all, a handful (w_min 3); and in a view of several rays m = 1: ONE sample of the last ray raised to 50, a
    # run of one behind empty rays for the bisection
    cases = [(w, 1.0), (w, 100.0), (w, 0.0)] + ([(w, 3.0)] if n * S > 1 else [])
    if n > 1:
        one = w.copy()
        one[n - 1, S // 2] = 50.0
        cases.append((one, 50.0))
    for w, w_min in cases:
        args[6] = _dev(w)
        idx_ref, pts_ref = fc.select_model(ro, rd, ne, fa, tv, tr, w, w_min)
        m = len(idx_ref)
        if w_min == 50.0:
            assert idx_ref.tolist() == [(n - 1) * S + S // 2]
        if w_min == 0.0:
            assert m == n * S
        n_out = ops.normal_select(*args, w_min)
        assert n_out.cpu().tolist() == [0, m]
        for cap in sorted({m, m + 3, max(m - 1, 0)}):
            idx = torch.full((cap,), -77, dtype=torch.int32, device=DEV)
            pts = torch.full((cap, 3), -77.0, dtype=torch.float32, device=DEV)
            n_out = ops.normal_select(*args, w_min, idx, pts) if cap else ops.normal_select(*args, w_min)
            k = min(cap, m)
            assert n_out.cpu().tolist() == [k, m]
            assert np.array_equal(idx.cpu().numpy()[:k], idx_ref[:k]) and (idx.cpu().numpy()[k:] == -77).all()
            assert np.array_equal(pts.cpu().numpy()[:k].view(np.uint32), pts_ref[:k].view(np.uint32))
            assert (pts.cpu().numpy()[k:] == -77).all()
        # composite of the full list: integer weights, axis-aligned integer gradients -> exact sums
        g = fc.integer_gradients(m, seed=int(w_min))
        nm_ref, na_ref = fc.composite_model(idx_ref, g, w)
        outs = []
        for fill in (777.0, float("nan")):  # a dirty output buffer is fully overwritten
            nm = torch.full((n, 3), fill, dtype=torch.float32, device=DEV)
            na = torch.full((n,), fill, dtype=torch.float32, device=DEV)
            ops.normal_composite(_dev(idx_ref), _dev(g), _dev(w), nm, na)
            outs.append((nm.cpu().numpy(), na.cpu().numpy()))
        assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))  # two calls give the same bits
        assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
        assert np.array_equal(outs[0][0], nm_ref) and np.array_equal(outs[0][1], na_ref)
        if m == 0:
            assert not outs[0][0].any() and not outs[0][1].any()
        if n > 1 and w_min > 0:
            assert not outs[0][0][0].any() and outs[0][1][0] == 0  # a ray with no selected sample
    w = w_all
    if (n, S) == (25, 41):  # general gradients: every step is one IEEE operation, so the restatement still gives the bits
        idx_ref, _ = fc.select_model(ro, rd, ne, fa, tv, tr, w, 1.0)
        rs = np.random.RandomState(3)
        g = rs.standard_normal((len(idx_ref), 3)).astype(F32)
        g[3], g[5], g[7, 0] = 0.0, 1e-13, np.inf
        wr = (w * rs.uniform(0.1, 1.0, w.shape)).astype(F32)
        nm, na = ops.normal_composite(_dev(idx_ref), _dev(g), _dev(wr))
        nm_ref, na_ref = fc.composite_model(idx_ref, g, wr)
        assert np.array_equal(nm.cpu().numpy(), nm_ref) and np.array_equal(na.cpu().numpy(), na_ref)


# ------------------------------------------------------------------------------------------------------------------------- 6
def _render_case(kind):
    from neuralbody_amd.renderer import RenderConfig, Renderer, RendererMmsk

    if kind == "mmsk":
        r, sd, batch, _ = scenes.build_masked("mmsk")
        net = H.make_network(sd, DEV, True, "f16f6")
        rend = RendererMmsk(net, RenderConfig(N_samples=r["n_samples"], perturb=0.0, raw_noise_std=0.0, white_bkgd=False))
    else:
        r, sd, body, batch, cam, _ = scenes.build("small")
        net = H.make_network(sd, DEV, True, kind)
        rend = H.make_renderer(net, r)
    return rend, batch, H.device_batch(batch, DEV)


@pytest.mark.parametrize("kind", ("f32", "f16f6", "mmsk"))
def test_render_with_normals(kind):
    """normal_map against the composition done in torch from the returned weights and calculate_density_gradient at EVERY sample of
    128 rays; normal_acc <= acc_map; without the option, today's keys and bits."""
    rend, batch, bd = _render_case(kind)
    with torch.no_grad():
        plain = rend.render(bd)
        out = rend.render(bd, normals=True)
        off = rend.render(bd, normals=False)
    assert sorted(plain) == sorted(off) == ["acc_map", "depth_map", "disp_map", "rgb_map", "weights"]
    assert sorted(out) == sorted(list(plain) + ["normal_map", "normal_acc"])
    for k in plain:
        assert H.same_bits(plain[k], off[k]) and H.same_bits(plain[k], out[k]), k
    n = bd["ray_o"].shape[1]
    assert out["normal_map"].shape == (1, n, 3) and out["normal_acc"].shape == (1, n)
    assert bool((out["normal_acc"] <= out["acc_map"] + 1e-6).all())
    ln = out["normal_map"][0].norm(dim=1)
    assert bool((((ln - 1).abs() < 1e-5) | (ln == 0)).all()) and int((ln > 0).sum()) > n // 20
    # the live cfg key does what the argument does
    rend.cfg.render_normals = True
    with torch.no_grad():
        via_cfg = rend.render(bd)
    rend.cfg.render_normals = False
    assert H.same_bits(via_cfg["normal_map"], out["normal_map"]) and H.same_bits(via_cfg["normal_acc"], out["normal_acc"])
    # the composition in torch on 128 rays through the image
    _against_torch_composition(kind, rend, batch, bd, out, np.linspace(0, n - 1, 128).astype(np.int64), 8)
    # ray_range: EVERY ray of the slice against the composition from the slice's OWN returned weights (another grouping of the rays
    # moves the f16f6 weights by rounding, so a sample at the threshold may be selected in one render and not in the other)
    with torch.no_grad():
        part = rend.render(bd, normals=True, ray_range=(64, 200))
    assert part["normal_map"].shape == (1, 136, 3) and part["normal_acc"].shape == (1, 136)
    _against_torch_composition(kind + " rays 64:200", rend, batch, bd, part, np.arange(64, 200), 1, first=64)
    if kind == "f32":  # the same weights bit for bit, so the same samples: the whole view's rows
        assert float((part["normal_map"] - out["normal_map"][:, 64:200]).abs().max()) <= 1e-4


def _against_torch_composition(what, rend, batch, bd, out, rays, at_least, first=0):
    """out['normal_map'] / ['normal_acc'] (row k = ray first + k) of the rays `rays` against sum_s w_s nhat_s composed in torch float64
    from out['weights'] and calculate_density_gradient at EVERY sample of those rays: 1e-4."""
    S = out["weights"].shape[2]
    rows = torch.from_numpy(rays - first).to(DEV)
    z = R.z_vals_f32(batch["near"][0][rays], batch["far"][0][rays], np.linspace(0.0, 1.0, S, dtype=F32))
    wpts = R.sample_points_f32(batch["ray_o"][0][rays], batch["ray_d"][0][rays], z)[0].reshape(-1, 3)
    with torch.no_grad():
        sp = rend.prepare_sp_input(bd)
        grad = rend.net.calculate_density_gradient(_dev(wpts)[None], rend.net.encode_sparse_voxels(sp), sp)[1][0].double().view(len(rays), S, 3)
    w = out["weights"][0][rows].double()
    w = torch.where(w >= fc.W_MIN, w, torch.zeros_like(w))
    gl = grad.norm(dim=2, keepdim=True)
    nhat = torch.where(gl >= 1e-12, -grad / gl.clamp_min(1e-300), torch.zeros_like(grad))
    total = (w[..., None] * nhat).sum(1)
    tl = total.norm(dim=1, keepdim=True)
    ref = torch.where(tl >= 1e-6, total / tl.clamp_min(1e-300), torch.zeros_like(total))
    got = out["normal_map"][0][rows].double()
    err = float((got - ref).abs().max())
    print("%s: normal_map against the torch composition on %d rays: %.3g; %d of them carry a normal" % (what, len(rays), err, int((tl >= 1e-6).sum())))
    assert int((tl >= 1e-6).sum()) >= at_least
    assert err <= 1e-4
    assert float((out["normal_acc"][0][rows].double() - w.sum(1)).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------- 7
def test_mesh_with_field_normals(tmp_path):
    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    _, sd, batch = scenes.build_mesh()
    net = H.make_network(sd, DEV, True, "f32")
    bd = H.device_batch(batch, DEV)
    rend = RendererMesh(net, RenderConfig(mesh_th=5.0))
    with torch.no_grad():
        faces = rend.extract_mesh(bd, colors=True)
        again = rend.extract_mesh(bd, colors=True, normals="faces")
        field = rend.extract_mesh(bd, colors=True, normals="field")
    for a, b in zip(faces, again):
        assert H.same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)  # "faces" is today's result
    assert torch.equal(field.triangles, faces.triangles) and H.same_bits(field.vertices, faces.vertices)
    V = field.vertices.shape[0]
    assert V > 100
    ln = field.normals.norm(dim=1)
    fallback = (field.normals == faces.normals).all(1)
    assert bool((((ln - 1).abs() < 1e-5) | fallback).all())
    assert int((~fallback).sum()) > V // 2
    assert H.same_bits(field.viewdir, -field.normals)
    # the field normal is the gradient's direction, and it points out of the body like the face normal does
    with torch.no_grad():
        fv_sp = rend._volumes(bd)()
        grad = net.calculate_density_gradient(field.wpts[None].contiguous(), *fv_sp)[1][0]
    unit = -grad / grad.norm(dim=1, keepdim=True).clamp_min(1e-30)
    assert float((unit - field.normals)[~fallback].abs().max()) <= 1e-5
    assert float(((field.normals * faces.normals).sum(1) > 0).float().mean()) > 0.8
    # cfg.mesh_normals: field -> TriMesh.vertex_normals, written as nx ny nz
    rend2 = RendererMesh(net, RenderConfig(mesh_th=5.0, mesh_normals="field"))
    with torch.no_grad():
        mesh = rend2.render(bd)["mesh"]
    assert isinstance(mesh, TriMesh) and mesh.vertex_colors is None
    assert np.array_equal(mesh.vertex_normals, field.normals.cpu().numpy())
    path = mesh.export(os.path.join(str(tmp_path), "m.ply"))
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in open(path, "rb").read(400)
    back = TriMesh.load_ply(path)
    assert np.array_equal(back.vertex_normals, mesh.vertex_normals) and np.array_equal(back.faces, mesh.faces)


def test_novel_view_normal_picture():
    """NovelViewRenderer with cfg.render_normals: normal_img = 0.5 n + 0.5 scattered into the image by nb_image_assemble, black
    outside the box mask; without the key the returned dict has no such entry and the same img."""
    from neuralbody_amd import novel_view as nv

    r, sd, body, batch, cam, _ = scenes.build("small")
    Hh = Ww = 40
    K0, R0, T0 = scenes.syn.make_camera(body, Hh, Ww, focal_factor=1.6, distance=1.8)
    RT = np.concatenate([np.concatenate([R0, T0.reshape(3, 1)], 1), [[0, 0, 0, 1.0]]], 0)
    rend = H.make_renderer(H.make_network(sd, DEV, True, "f16f6"), r)
    frame = {k: v for k, v in H.device_batch(batch, DEV).items() if k in ("coord", "out_sh", "bounds", "R", "Th", "latent_index")}
    nvr = nv.NovelViewRenderer(rend, Hh, Ww, torch.device(DEV))
    plain = nvr.render_view(K0, RT, body["can_bounds"], frame)
    rend.cfg.render_normals = True
    out = nvr.render_view(K0, RT, body["can_bounds"], frame)
    rend.cfg.render_normals = False
    assert "normal_img" not in plain and sorted(out) == sorted(list(plain) + ["normal_img"])
    assert torch.equal(out["img"], plain["img"]) and out["normal_img"].shape == (Hh, Ww, 3)
    inside = out["mask_at_box"].bool()
    assert int(inside.sum()) == out["n_rays"] > 0 and not bool(out["normal_img"][~inside].any())
    n = 2.0 * out["normal_img"][inside] - 1.0
    ln = n.norm(dim=1)
    assert bool((((ln - 1).abs() < 1e-5) | (ln == 0)).all()) and int((ln > 0).sum()) > 20
