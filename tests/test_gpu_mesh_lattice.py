"""The mesh lattice on the device (csrc/nb_lattice.hip, neuralbody_amd/mesh_lattice.py) against the reference dataset's fixture
(tests/golden/mesh_lattice.npz) and the numpy restatements of tests/lattice_ref.py.

`inside` is compared at every point OUTSIDE the near band (lattice_ref.BAND: the float64 pixel coordinate within 1e-3 px of a
half-integer in some view), where a float32 projection may round to the other pixel whatever its summation order; the band may
not exceed 3 % of the lattice.  INSIDE the band the device is held to the float32 restatement (the FMA chains of tests/cull_cases.py,
which give the reference's own bitmap at every point of the fixture: tests/test_mesh_lattice_host.py).  Everything else (the gathered points, their order, the dilation, the cube) is compared exactly."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lattice_ref as lr
from tests import synthetic as syn
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_lattice.npz")
BAND_MAX = 0.03


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _span(lo, hi, n):
    return np.linspace(lo, hi, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(axes, msks (dilated), Ks, RT, ref (float64 restatement), band, gold (the reference's own bitmap or None))"""
    g = _gold()
    RT = np.concatenate([g["Rs"], g["Ts"]], axis=2)
    wb = g["wbounds"]
    gold = None
    if name == "fixture":
        axes, msks, Ks, gold = [g["axis_x"], g["axis_y"], g["axis_z"]], g["msks_dilated"], g["Ks"], g["inside"]
    elif name in ("5x7x3", "16x8x8"):  # under one tile of the count-and-place body / exactly one
        dims = [int(v) for v in name.split("x")]
        axes, msks, Ks = [_span(wb[0, a], wb[1, a], dims[a]) for a in range(3)], g["msks_dilated"], g["Ks"]
    elif name == "164x160x160":  # 4 198 400 points = 4100 tiles: beyond FUSED_MAX_BLOCKS, the three-launch branch
        body = syn.make_body(**scenes.MESH["body"])
        msks, Ks, RT = syn.make_view_masks(body, 64, 64, n_views=4, focal_factor=1.8, distance=1.6, dilate=2)
        axes = [_span(wb[0, a], wb[1, a], n) for a, n in enumerate((164, 160, 160))]
    else:
        raise KeyError(name)
    ref, band = lr.inside_and_band(axes, msks, Ks, RT)
    return dict(axes=axes, msks=msks, Ks=Ks, RT=RT, ref=ref, band=band, gold=gold)


def _carve(c):
    from neuralbody_amd import ops

    axes = [_dev(a) for a in c["axes"]]
    cull, keep = ops.make_cull(_dev(c["msks"]), _dev(c["RT"]), _dev(c["Ks"]))
    inside, n_inside = ops.lattice_carve(axes, cull)
    torch.cuda.synchronize()
    return axes, inside, n_inside


def _check_outside_band(name, got, c):
    band, ref = c["band"], c["ref"]
    diff = got != ref
    print("%s: %d points, %d inside, band %.2f %%, device != fp64 at %d points (%d outside the band)" % (
        name, ref.size, int(got.sum()), 100.0 * band.mean(), int(diff.sum()), int((diff & ~band).sum())))
    assert band.mean() <= BAND_MAX
    assert got.dtype == np.uint8 and got.shape == ref.shape and set(np.unique(got)) <= {0, 1}
    assert not (diff & ~band).any()
    # inside the band the float64 restatement does not decide, the float32 one (lattice_ref.project_f32: the FMA chains of
    # tests/cull_cases.py, which is what the reference's np.dot evaluates to) does: the device equals it at every band point
    pts = lr.lattice_points(c["axes"])[band.reshape(-1)]
    chain = lr.inside_f32_at(pts, c["msks"], c["Ks"], c["RT"])
    miss = int((got.reshape(-1)[band.reshape(-1)].astype(bool) != chain).sum())
    print("%s: device != float32 chain at %d of the %d band points" % (name, miss, len(pts)))
    assert miss == 0


# ---------------------------------------------------------------------------------------------------------- 1. carve
@pytest.mark.parametrize("name", ["5x7x3", "16x8x8", "fixture", "164x160x160"])
def test_carve_matches_the_reference_outside_the_band(name):
    c = _case(name)
    _, inside, n_inside = _carve(c)
    assert inside.is_cuda and inside.dtype == torch.uint8 and n_inside.dtype == torch.int32
    got = inside.cpu().numpy()
    _check_outside_band(name, got, c)
    assert 0 < got.sum() < got.size, "degenerate case"
    assert int(n_inside.item()) == int(got.sum())
    if c["gold"] is not None:  # the reference's own float32 bitmap
        assert not ((got != c["gold"]) & ~c["band"]).any()


# ---------------------------------------------------------------------------------------------------------- 2. one view
@functools.lru_cache(maxsize=None)
def _one_view():
    """One 37 x 53 view with a 255-valued mask, the camera INSIDE the lattice's box: points in front of it inside and outside
    the image, and points behind it (projected like any other, clamped to the image: cull_pixel)."""
    Hh, Ww = 37, 53
    axes = [_span(-0.5, 0.5, 11), _span(-0.4, 0.45, 13), _span(-0.3, 0.6, 9)]
    pos = np.array([0.0123, -0.0371, 0.1507])
    yaw = 0.3
    fwd = np.array([np.sin(yaw), 0.0, np.cos(yaw)])
    right = np.array([np.cos(yaw), 0.0, -np.sin(yaw)])
    R = np.stack([right, np.array([0.0, 1.0, 0.0]), fwd])
    RT = np.concatenate([R, (-R @ pos)[:, None]], axis=1).astype(np.float32)[None]
    K = np.array([[15.0, 0, Ww / 2.0], [0, 15.0, Hh / 2.0], [0, 0, 1]], np.float32)[None]
    yy, xx = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
    msk = (255 * (((yy // 5 + xx // 7) % 2 == 0) | (xx == 0) | (yy == Hh - 1))).astype(np.uint8)[None]
    ref, band = lr.inside_and_band(axes, msk, K, RT)
    cam = lr.lattice_points(axes).astype(np.float64) @ RT[0, :, :3].astype(np.float64).T + RT[0, :, 3]
    xy = lr.project_f64(lr.lattice_points(axes), K[0], RT[0])
    out = (xy[:, 0] < -1) | (xy[:, 0] > Ww) | (xy[:, 1] < -1) | (xy[:, 1] > Hh)
    assert (cam[:, 2] < 0).sum() > 100 and ((cam[:, 2] > 0) & out).sum() > 100 and ((cam[:, 2] > 0) & ~out).sum() > 100
    return dict(axes=axes, msks=msk, Ks=K, RT=RT, ref=ref, band=band, gold=None)


def test_one_view_with_points_outside_the_image_and_behind_the_camera():
    from neuralbody_amd import ops

    c = _one_view()
    axes, inside, n_inside = _carve(c)
    got = inside.cpu().numpy()
    _check_outside_band("one view", got, c)
    assert 0 < got.sum() < got.size and int(n_inside.item()) == int(got.sum())
    # the _msk variant's pre-affine has no meaning for a world-space lattice
    cull, keep = ops.make_cull(_dev(c["msks"]), _dev(c["RT"]), _dev(c["Ks"]), R0=torch.eye(3, device=DEV),
                               Th0=torch.zeros(3, device=DEV))
    assert cull.pre_affine == 1
    with pytest.raises(ops.NbError, match="pre_affine"):
        ops.lattice_carve(axes, cull)


# ---------------------------------------------------------------------------------------------------------- 3. gather
def _gather(axes, inside, cap, guard=-7):
    from neuralbody_amd import ops

    n = int(inside.numel())
    wpts = torch.full((cap, 3), float(guard), device=DEV)
    lin = torch.full((cap,), guard, dtype=torch.int32, device=DEV)
    n_out = ops.lattice_gather(axes, inside, wpts, lin)
    torch.cuda.synchronize()
    return wpts.cpu().numpy(), lin.cpu().numpy(), n_out.cpu().tolist()


def test_gather_lists_the_flagged_points_in_linear_order():
    from neuralbody_amd import ops

    g = _gold()
    axes_np = [g["axis_x"], g["axis_y"], g["axis_z"]]
    axes = [_dev(a) for a in axes_np]
    pts = lr.lattice_points(axes_np)
    bitmap = g["inside"]  # a bitmap the reference's host dataset made
    want_lin = np.flatnonzero(bitmap.reshape(-1))
    total = len(want_lin)
    wpts, lin, n_out = _gather(axes, _dev(bitmap), total)
    assert n_out == [total, total]
    assert np.array_equal(lin, want_lin)
    assert np.array_equal(wpts.view(np.uint32), pts[want_lin].view(np.uint32))
    # any non-zero byte flags a point (a 255-valued mask product)
    wpts2, lin2, n_out2 = _gather(axes, _dev(bitmap * np.uint8(255)), total + 5)
    assert n_out2 == [total, total] and np.array_equal(lin2[:total], want_lin) and (lin2[total:] == -7).all()
    assert (wpts2[total:] == -7.0).all() and np.array_equal(wpts2[:total], wpts)
    # a capacity below the count: the first `cap` entries, nothing behind them
    cap = total // 3
    wpts3 = torch.full((cap + 9, 3), -7.0, device=DEV)
    lin3 = torch.full((cap + 9,), -7, dtype=torch.int32, device=DEV)
    n_out3 = ops.lattice_gather(axes, _dev(bitmap), wpts3[:cap], lin3[:cap])
    assert n_out3.cpu().tolist() == [cap, total]
    assert np.array_equal(lin3[:cap].cpu().numpy(), want_lin[:cap]) and bool((lin3[cap:] == -7).all())
    assert np.array_equal(wpts3[:cap].cpu().numpy(), pts[want_lin[:cap]]) and bool((wpts3[cap:] == -7.0).all())
    # count only, and the empty bitmap
    assert ops.lattice_gather(axes, _dev(bitmap)).cpu().tolist() == [0, total]
    zeros = torch.zeros(bitmap.shape, dtype=torch.uint8, device=DEV)
    assert ops.lattice_gather(axes, zeros).cpu().tolist() == [0, 0]
    wpts4, lin4, n_out4 = _gather(axes, zeros, 4)
    assert n_out4 == [0, 0] and (lin4 == -7).all() and (wpts4 == -7.0).all()


def test_gather_beyond_the_fused_tile_count():
    c = _case("164x160x160")
    axes = [_dev(a) for a in c["axes"]]
    want_lin = np.flatnonzero(c["ref"].reshape(-1))
    wpts, lin, n_out = _gather(axes, _dev(c["ref"]), len(want_lin))
    assert n_out == [len(want_lin), len(want_lin)] and np.array_equal(lin, want_lin)
    i, j, k = np.unravel_index(want_lin, c["ref"].shape)
    assert np.array_equal(wpts, np.stack([c["axes"][0][i], c["axes"][1][j], c["axes"][2][k]], axis=1))


# ---------------------------------------------------------------------------------------------------------- 4. dilate
@pytest.mark.parametrize("border", [1, 3, 5, 107])  # 107: a half width of 53 reaches past both sides of the image
def test_dilate_matches_the_restatement(border):
    from neuralbody_amd import ops

    V, Hh, Ww = 3, 37, 53
    rng = np.random.RandomState(border)
    m = np.zeros((V, Hh, Ww), np.uint8)
    m[0, [0, 0, -1, -1], [0, -1, 0, -1]] = [1, 2, 3, 4]  # the four corners
    m[1, 0, 20], m[1, -1, 31], m[1, 17, 0], m[1, 9, -1] = 5, 6, 7, 8  # every edge
    ys, xs = rng.randint(0, Hh, 12), rng.randint(0, Ww, 12)
    m[2, ys, xs] = rng.randint(1, 256, 12)
    m[2, 0, :] = 1
    out = ops.mask_dilate(_dev(m), border)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == m.shape
    assert np.array_equal(out.cpu().numpy(), lr.dilate(m, border))
    if border == 1:
        assert np.array_equal(out.cpu().numpy(), m)
    for bad in (0, 2, 4, 257):
        with pytest.raises(ValueError, match="border"):
            ops.mask_dilate(_dev(m), bad)


# ---------------------------------------------------------------------------------------------------------- 5. scatter, renderer
def test_scatter_places_strided_values_in_the_padded_cube():
    from neuralbody_amd import ops

    dims, pad = (5, 7, 3), 2
    rng = np.random.RandomState(0)
    lin = np.sort(rng.choice(5 * 7 * 3, 40, replace=False)).astype(np.int32)
    raw = rng.standard_normal((40, 4)).astype(np.float32)
    want = np.zeros(dims, np.float32)
    want.reshape(-1)[lin] = raw[:, 3]
    want = np.pad(want, pad)
    raw_d = _dev(raw)
    for alpha in (raw_d[:, 3], raw_d[:, 3].contiguous()[None, :, None]):
        cube = ops.lattice_scatter(alpha, _dev(lin), dims, pad)
        assert tuple(cube.shape) == (9, 11, 7) and np.array_equal(cube.cpu().numpy(), want)
    assert not ops.lattice_scatter(raw_d[:0, 3], _dev(lin[:0]), dims, pad).any()
    with pytest.raises(ValueError):
        ops.lattice_scatter(raw_d, _dev(lin), dims, pad)


def _axis_batch(batch):
    pts = batch["pts"][0]
    out = {k: v for k, v in batch.items() if k != "pts"}
    out["axis_x"], out["axis_y"], out["axis_z"] = pts[None, :, 0, 0, 0].copy(), pts[None, 0, :, 0, 1].copy(), pts[None, 0, 0, :, 2].copy()
    return out


def test_density_cube_and_mesh_from_axes_equal_those_from_pts():
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    r, sd, batch = scenes.build_mesh()
    net = H.make_network(sd, DEV, True, "f32")
    rend = RendererMesh(net, RenderConfig(mesh_th=5.0, mesh_backend="device"))
    bd_pts, bd_axes = H.device_batch(batch, DEV), H.device_batch(_axis_batch(batch), DEV)
    assert "pts" not in bd_axes
    with torch.no_grad():
        cube_pts = rend.density_cube(bd_pts)
        cube_axes = rend.density_cube(bd_axes)
        v_pts, t_pts = rend.extract_mesh(bd_pts, world=True)
        v_axes, t_axes = rend.extract_mesh(bd_axes, world=True)
    assert cube_axes.is_cuda and float(cube_pts.max()) > 5.0
    assert H.same_bits(cube_axes, cube_pts)
    assert len(t_pts) > 0 and torch.equal(t_axes, t_pts) and H.same_bits(v_axes, v_pts)


# ---------------------------------------------------------------------------------------------------------- 6. dataset plugin
def _plugin(n_items, **cfg_kw):
    from neuralbody_amd.mesh_lattice import MemoryMeshSource

    g = _gold()
    items = []
    for f in range(n_items):  # frame f: the fixture's body under masks rolled by 6 f pixels
        items.append((np.roll(g["msks_raw"], 6 * f, axis=2), g["xyz"], g["Rh"], g["Th"]))
    cfg = types.SimpleNamespace(begin_ith_frame=0, num_train_frame=5, num_render_frame=-1, voxel_size=[0.02, 0.02, 0.02],
                                big_box=False, training_view=[0, 1, 2], train=types.SimpleNamespace(num_workers=0),
                                test=types.SimpleNamespace(batch_size=1), **cfg_kw)
    mod = H.load_plugin("light_stage_mesh_dataset.py", cfg)
    return mod.Dataset("nowhere", "synthetic", "none.npy", "test", source=MemoryMeshSource(items, g["Ks"], g["Rs"], g["Ts"]),
                       device=DEV), items


def test_dataset_item_renders_a_mesh(monkeypatch):
    from torch.utils.data.dataloader import default_collate

    from neuralbody_amd.mesh import TriMesh
    from neuralbody_amd.renderer import RenderConfig, RendererMesh

    g = _gold()
    ds, _ = _plugin(1)
    item = ds[0]
    assert set(item) == {"coord", "out_sh", "inside", "axis_x", "axis_y", "axis_z", "wbounds", "bounds", "R", "Th", "latent_index",
                         "frame_index"}
    assert all(v.is_cuda for k, v in item.items() if k != "frame_index") and item["frame_index"] == 0
    assert item["inside"].dtype == torch.uint8 and tuple(item["inside"].shape) == (24, 36, 15)
    assert item["latent_index"].dtype == torch.int64 and int(item["latent_index"]) == 0
    c = _case("fixture")
    _check_outside_band("dataset item", item["inside"].cpu().numpy(), c)  # raw masks dilated on the device
    assert not ((item["inside"].cpu().numpy() != g["inside"]) & ~c["band"]).any()
    for k in ("coord", "out_sh", "wbounds", "bounds", "R", "axis_x", "axis_y", "axis_z"):
        assert np.array_equal(item[k].cpu().numpy(), g[k]), k
    _, sd, _ = scenes.build_mesh()
    rend = RendererMesh(H.make_network(sd, DEV, True, "f32"), RenderConfig(mesh_th=5.0, mesh_backend="device"))
    monkeypatch.setitem(sys.modules, "trimesh", None)
    batch = default_collate([item])
    with torch.no_grad():
        top = float(rend.density_cube(batch).max())
        print("largest density on the item's lattice: %.3f" % top)
        assert top > 0.0
        rend.cfg.mesh_th = 0.5 * top  # a level this frame's densities cross, whatever the scene's scale
        out = rend.render(batch)
    assert set(out) == {"cube", "mesh"} and isinstance(out["mesh"], TriMesh)
    assert out["cube"].shape == (44, 56, 35) and out["cube"].dtype == np.float64 and len(out["mesh"].faces) > 0
    occupied = out["cube"][10:-10, 10:-10, 10:-10] != 0
    assert occupied.any() and not (occupied & (item["inside"].cpu().numpy() == 0)).any()


def test_mesh_lattice_pts_adds_the_meshgrid():
    g = _gold()
    ds, _ = _plugin(1, mesh_lattice_pts=True)
    item = ds[0]
    want = np.stack(np.meshgrid(g["axis_x"], g["axis_y"], g["axis_z"], indexing="ij"), axis=-1).astype(np.float32)
    assert item["pts"].is_cuda and item["pts"].dtype == torch.float32
    assert np.array_equal(item["pts"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert "axis_x" in item


def test_consecutive_items_of_different_frames_do_not_share_a_bitmap():
    ds, items = _plugin(2)
    g = _gold()
    RT = np.concatenate([g["Rs"], g["Ts"]], axis=2)
    axes = [g["axis_x"], g["axis_y"], g["axis_z"]]
    refs = [lr.inside_and_band(axes, lr.dilate(it[0], 5), g["Ks"], RT) for it in items]
    assert (refs[0][0] != refs[1][0]).sum() > 100  # the two frames differ
    a = ds[0]
    a_copy = a["inside"].clone()
    b = ds[1]
    torch.cuda.synchronize()
    assert a["inside"].data_ptr() != b["inside"].data_ptr() and a["axis_x"].data_ptr() != b["axis_x"].data_ptr()
    assert torch.equal(a["inside"], a_copy)  # item 1 wrote nothing into item 0
    b_np = b["inside"].cpu().numpy()
    assert not ((a_copy.cpu().numpy() != refs[0][0]) & ~refs[0][1]).any()
    assert not ((b_np != refs[1][0]) & ~refs[1][1]).any()
    # freed and re-made, like a DataLoader loop: the allocator may hand frame 0's addresses to frame 1
    del a, b
    again = ds[1]["inside"].cpu().numpy()
    assert np.array_equal(again, b_np)
