"""Ray bounds from the posed body on the device: nb_body_depth_range, nb_depth_range_widen and nb_raygen_body against their
restatement (tests/ray_bounds_ref.py, checked on the host by tests/test_ray_bounds_host.py), bit for bit; then the frames, the view
renderer and the dataset plugin that use them."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import ray_bounds_ref as rb
from tests import ray_cases as rc
from tests import silhouette_ref as sil
from tests import smpl_ref as sr
from tests import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = 64
EINVAL = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _range(c, **kw):
    from neuralbody_amd import ops

    return ops.body_depth_range(_dev(c["verts"]), _dev(c["faces"]), _dev(c["RTs"]), _dev(c["Ks"]), c["H"], c["W"], **kw)


# ---------------------------------------------------------------------------------------------------------- 1. nb_body_depth_range
@pytest.mark.parametrize("name", rb.CASES)
def test_depth_range_is_the_restatement_bit_for_bit(name):
    """F = 2, nv = 3: small, large (beyond 16 x 16 px) and clipped triangles, both windings, zero-area faces ('paths'); bodies that
    leave the image and a view that is too near (the band cases).  Into a NaN-filled and into a zeroed buffer."""
    from neuralbody_amd import ops

    c, want = rb.case_ranges(name)
    shape = (2, 3, c["H"], c["W"], 2)
    got = _range(c, out=torch.full(shape, float("nan"), device=DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    g = got.cpu().numpy()
    differ = (g.view(np.int32) != want.view(np.int32)).any(axis=-1)
    print("%s: %d of %d pixels covered, %d unbounded views, %d pixels differ" % (
        name, int((want[..., 0] <= want[..., 1]).sum()), differ.size, int(np.isneginf(want[..., 0]).all(axis=(2, 3)).sum()), int(differ.sum())))
    assert not differ.any(), np.argwhere(differ)[:4].tolist()
    assert torch.equal(_range(c, out=torch.zeros(shape, device=DEV)), got)
    # the emptiness mask is nb_smpl_silhouette's on the same inputs
    mask = ops.smpl_silhouette(_dev(c["verts"]), _dev(c["faces"]), _dev(c["RTs"]), _dev(c["Ks"]), c["H"], c["W"])
    assert torch.equal((got[..., 0] <= got[..., 1]).to(torch.uint8), mask)
    if name == "paths":
        uv = sil.project(c["verts"][0], c["Ks"][0], c["RTs"][0])[0]
        assert np.ptp(uv, axis=0).min() > 90  # view 0: boxes far beyond 16 x 16, the workgroup-per-triangle pass
    else:
        assert np.isneginf(want[0, 2, ..., 0]).all() and np.isposinf(want[0, 2, ..., 1]).all()  # too near: does not bound


def test_depth_range_with_more_listed_triangles_than_workgroups():
    """320 faces in two views at 256 x 256: more than 512 boxes of 17 or more pixels on a side (tests/test_gpu_silhouette.py counts
    them for the same mesh and cameras), so the fixed grid of the large pass strides over its list."""
    v, faces = sil.icosphere(2, sil.ELLIPSOID)
    Ks, RTs = sil.orbit((0.2, 1.4), 1.5, 1.3 * 256, 256, 256)
    uv = np.stack([sil.project(v, Ks[k], RTs[k])[0][faces] for k in range(2)])  # [2,Nf,3,2]
    large = int(((np.floor(uv.max(axis=2) + 0.5) - np.ceil(uv.min(axis=2) - 0.5)).max(axis=-1) >= 16).sum())
    assert large > 512
    c = dict(verts=v[None], faces=faces, Ks=Ks, RTs=RTs, H=256, W=256)
    want = rb.depth_range_stack(c["verts"], faces, Ks, RTs, 256, 256)
    got = _range(c).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and (want[..., 0] <= want[..., 1]).mean() > 0.1


def test_depth_range_refusals():
    from neuralbody_amd import _lib, ops

    c = rb.case("paths")
    with pytest.raises(ValueError):
        ops.body_depth_range_scratch(65536, 4, 6, 3, DEV)
    with pytest.raises(ValueError):
        ops.body_depth_range(_dev(c["verts"]), _dev(c["faces"]), _dev(c["RTs"]), _dev(c["Ks"]), 0, 8)
    small = torch.empty(256, dtype=torch.uint8, device=DEV)
    with pytest.raises(ops.NbError, match="scratch holds"):
        _range(c, scratch=small)
    assert _lib.lib().nb_abi_version() == 20 and {"nb_body_depth_range", "nb_depth_range_widen", "nb_raygen_body"} <= set(_lib.header_functions())


# ---------------------------------------------------------------------------------------------------------- 2. nb_depth_range_widen
@pytest.mark.parametrize("border", [1, 3, 9, 255])
def test_widen_is_the_restatement_bit_for_bit(border):
    from neuralbody_amd import ops

    _, r = rb.case_ranges("ico320")  # [2,3,45,61,2]: covered and empty pixels, and one view that does not bound
    stacks = {6: r.reshape(6, 45, 61, 2), 1: r[1, 0][None]}
    one = np.array([[[[1.5, 2.5]]], [[rb.EMPTY]], [[rb.UNBOUNDED]], [[[0.25, 0.5]]], [[[3.0, 3.0]]], [[[0.01, 9.0]]]], np.float32)  # [6,1,1,2]
    for n, stack in list(stacks.items()) + [(6, one), (1, one[:1])]:
        for tile in (1, 8, 16):
            got = ops.depth_range_widen(_dev(stack), border, tile)
            want = rb.widen(stack, border, tile)
            assert tuple(got.shape) == stack.shape
            assert np.array_equal(_bits(got), want.view(np.int32)), (n, stack.shape, border, tile)
    if border == 1:
        assert np.array_equal(_bits(ops.depth_range_widen(_dev(stacks[6]), 1, 1)), stacks[6].view(np.int32))
    src = _dev(stacks[1])
    for bad in (dict(border=2), dict(border=257), dict(tile=3), dict(tile=32), dict(out=src)):
        with pytest.raises(ValueError):
            ops.depth_range_widen(src, **dict(dict(border=3, tile=8), **bad))


# ---------------------------------------------------------------------------------------------------------- 3. nb_raygen_body
@functools.lru_cache(maxsize=None)
def _ray_case(H, W):
    """The oblique camera of tests/ray_cases.py at H x W over OBLIQUE_BOX, an ellipsoid well inside the box, and the device's own
    widened range of it (border 3, tile 8; checked above) -> (K, R, T, range [H,W,2] on the device)."""
    from neuralbody_amd import ops

    K, R, T = rc.oblique_camera(H, W)
    v, faces = sil.icosphere(2, (0.09, 0.2, 0.07))
    v = (v + rc.OBLIQUE_BOX.mean(axis=0)).astype(np.float32)
    RT = np.concatenate([R, T.reshape(3, 1)], axis=1).astype(np.float32)
    raw = ops.body_depth_range(_dev(v[None]), _dev(faces), _dev(RT[None]), _dev(K.astype(np.float32)[None]), H, W)
    return K, R, T, ops.depth_range_widen(raw[0, 0], 3, 8)


def _np_rays(rays):
    n = int(rays[5].item())
    return tuple(t[:n].cpu().numpy() for t in rays[:4]) + (rays[4].cpu().numpy(),), n


@pytest.mark.parametrize("size", [(45, 61), (96, 128)])
def test_raygen_body_is_raygen_unbounded_and_the_restatement_otherwise(size):
    from neuralbody_amd import ops

    Hh, Ww = size
    K, R, T, rng = _ray_case(Hh, Ww)
    box = ops.raygen(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, DEV)
    box_np, n_box = _np_rays(box)
    unbounded = torch.empty((Hh, Ww, 2), device=DEV)
    unbounded[..., 0], unbounded[..., 1] = -float("inf"), float("inf")
    for margin in (0.0, 0.05):
        same = ops.raygen_body(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, unbounded, margin)
        assert int(same[5].item()) == n_box and torch.equal(same[4], box[4])
        assert all(H.same_bits(same[k][:n_box], box[k][:n_box]) for k in range(4))
        got, n = _np_rays(ops.raygen_body(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, rng, margin))
        want = rb.raygen_body(box_np, rng.cpu().numpy(), margin)
        kept = want[4][box_np[4] != 0] != 0  # which of the box's rays are left
        width = float(((want[3] - want[2]) / (box_np[3] - box_np[2])[kept]).mean())
        print("%d x %d, margin %.2f: %d of %d box rays kept, mean width %.3f of the box's" % (Hh, Ww, margin, n, n_box, width))
        assert n == want[5] and 0 < n < n_box and width < 1.0  # the ellipsoid lies strictly inside the box
        for k in range(5):
            assert np.array_equal(got[k].view(np.int32 if k < 4 else np.uint8), want[k].view(np.int32 if k < 4 else np.uint8)), (margin, k)
    # an all-empty range: no ray, an all-zero mask
    empty = torch.empty((Hh, Ww, 2), device=DEV)
    empty[..., 0], empty[..., 1] = float("inf"), -float("inf")
    none = ops.raygen_body(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, empty, 0.05)
    assert int(none[5].item()) == 0 and not bool(none[4].any())


def test_raygen_body_drops_a_ray_whose_interval_is_a_point():
    from neuralbody_amd import ops

    Hh, Ww = 45, 61
    K, R, T, _ = _ray_case(Hh, Ww)
    box = ops.raygen(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, DEV)
    box_np, n_box = _np_rays(box)
    _, _, near, far, mask = box_np
    idx = np.flatnonzero(mask)
    p, q, r = idx[n_box // 3], idx[n_box // 2], idx[2 * n_box // 3]
    rng = np.empty((Hh * Ww, 2), np.float32)
    rng[:] = rb.UNBOUNDED
    rng[p] = (-np.inf, near[n_box // 3])                                      # far' == near' == near: dropped
    rng[q] = (-np.inf, np.nextafter(near[n_box // 2], np.float32(np.inf)))    # one ulp of interval: kept
    rng[r] = (far[2 * n_box // 3], np.inf)                                    # near' == far' == far: dropped
    got, n = _np_rays(ops.raygen_body(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, _dev(rng.reshape(Hh, Ww, 2)), 0.0))
    assert n == n_box - 2 and got[4][p] == 0 and got[4][q] == 1 and got[4][r] == 0
    want = rb.raygen_body(box_np, rng, 0.0)
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[2].view(np.int32), want[2].view(np.int32))
    assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32))


def test_raygen_body_refusals_by_name():
    import ctypes as C

    from neuralbody_amd import _lib, ops

    Hh, Ww = 45, 61
    K, R, T, rng = _ray_case(Hh, Ww)
    for bad_K, text in ((K + np.array([[0, 0, 0], [0, 0, 0], [1e-9, 0, 0]]), "last row"), (K + np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1e-9]]), "last row"),
                        (K * 2.0, "last row")):
        with pytest.raises(ops.NbError, match=text):
            ops.raygen_body(Hh, Ww, bad_K, R, T, rc.OBLIQUE_BOX, rng, 0.05)
    for margin in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ops.NbError, match="margin"):
            ops.raygen_body(Hh, Ww, K, R, T, rc.OBLIQUE_BOX, rng, margin)
    # the code itself, through the library
    n = Hh * Ww
    bufs = [torch.empty(n * 3, device=DEV) for _ in range(4)] + [torch.empty(n, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                                                                ops.scan_scratch(n, DEV)]
    K2 = (K * 2.0).reshape(9)
    rcode = _lib.lib().nb_raygen_body(Hh, Ww, (C.c_double * 9)(*K2), (C.c_double * 9)(*R.reshape(9)), (C.c_double * 3)(*T.reshape(3)),
                                      (C.c_float * 6)(*rc.OBLIQUE_BOX.reshape(6)), _lib.ptr(rng), 0.05, *[_lib.ptr(b) for b in bufs], None)
    assert rcode == EINVAL and b"last row" in _lib.lib().nb_last_error()


# ---------------------------------------------------------------------------------------------------------- 4. frames, renderer, plugin
FRAME_KEYS = {"coord", "out_sh", "bounds", "R", "Th", "latent_index"}


def _central_faces(v_template):
    """tests/test_gpu_silhouette.py's body: triangles over the vertices in the middle of the small body's box (an ellipsoid of half
    the box), y-neighbours joined: a body that does not fill its box."""
    inside = ((v_template / np.array([0.07, 0.15, 0.06])) ** 2).sum(axis=1) < 1.0
    idx = np.flatnonzero(inside)
    idx = idx[np.argsort(v_template[idx, 1], kind="stable")]
    return np.stack([idx[:-2], idx[1:-1], idx[2:]], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _small_body():
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    arrays = sr.synthetic_smpl(21, 6890, sr.SMPL_PARENTS, box=(0.3, 0.5, 0.2))
    arrays["f"] = _central_faces(arrays["v_template"])
    model = SmplModel.from_arrays(arrays, DEV)
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(2)]
    return PoseDriver(model), [np.stack([p[k] if k < 2 else P[0][k] for p in P]) for k in range(4)]


def _camera(can_bounds, yaw=0.35):
    K, R, T = syn.make_camera({"can_bounds": can_bounds}, SIZE, SIZE, focal_factor=2.5, distance=1.5, yaw=yaw)
    return K, np.concatenate([R, T.reshape(3, 1)], axis=1)


@functools.lru_cache(maxsize=None)
def _oracle():
    """The weights of the golden scenes (tests/golden/scenes.py: seed 0, 7 frames), to which the parity suite holds the default
    arithmetic within helpers.RGB_TOL; the frames with the body's keys; the oracle's volumes of frame 0 (computed once on the CPU)."""
    drv, stacked = _small_body()
    sd = syn.make_weights(0, num_train_frame=7)
    made = drv.frames(*stacked, latent_index=[2, 3], new_params=True, body=True)
    frame_np = {k: made[0][0][k].cpu().numpy() for k in FRAME_KEYS}
    sdt, vols, _ = H.oracle_volumes(sd, frame_np, True)
    return sd, made, frame_np, sdt, vols


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
def test_views_bounded_by_the_body_match_the_oracle_on_the_cut_rays(precision):
    """PoseDriver.frames(body=True) -> NovelViewRenderer(body_bounds=BodyBounds()): the render of the device's own cut rays against the
    oracle decoding and compositing those rays, within helpers.RGB_TOL; a ray whose last density the oracle puts within its own fp32
    rounding of zero (bench.FP32_SIGMA) is bounded by the transmittance in front of that sample instead, the allowance of
    tests/test_gpu_importance.py and no other.  Measured on an MI355X: 'f32' 3.1e-7, the default arithmetic 3.1e-5 (the box's own rays
    of the same view: 4.8e-7 and 4.3e-5), no ray on the allowance.  The cut is not what the default arithmetic's error depends on:
    with the weights of seed 3 (tests/test_gpu_silhouette.py renders them under 'f32' alone) it measured 6.7e-5 on the box's rays, as
    the parent commit does, and 6.8e-5 on the cut rays."""
    import bench
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.ray_bounds import BodyBounds
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from oracle import neuralbody_oracle as orc

    sd, made, frame_np, sdt, vols = _oracle()
    frame, can_bounds = made[0]
    assert set(frame) == FRAME_KEYS | {"body_verts", "body_faces"}
    assert tuple(frame["body_verts"].shape) == (1, 6890, 3) and frame["body_faces"].dtype == torch.int32
    net = H.make_network(sd, DEV, True, precision)
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=SIZE, W=SIZE))
    nv = NovelViewRenderer(rend, SIZE, SIZE, DEV, body_bounds=BodyBounds())
    box = NovelViewRenderer(rend, SIZE, SIZE, DEV)
    K, RT = _camera(can_bounds)
    batch = nv.view_batch(K, RT, can_bounds, frame)
    box_batch = box.view_batch(K, RT, can_bounds, {k: frame[k] for k in FRAME_KEYS})
    n, n_box = batch["ray_o"].shape[1], box_batch["ray_o"].shape[1]
    width = float((batch["far"] - batch["near"]).mean() / (box_batch["far"] - box_batch["near"]).mean())
    print("%s: %d rays bounded by the body, %d by the box; mean far - near %.3f of the box's" % (precision, n, n_box, width))
    assert "body_verts" not in batch and "body_faces" not in batch and 0 < n < n_box and width < 1.0
    mask, box_mask = batch["mask_at_box"][0].bool(), box_batch["mask_at_box"][0].bool()
    assert int(mask.sum()) == n and bool((mask <= box_mask).all())
    with torch.no_grad():
        out = rend.render(batch, feature_volume=[v.to(DEV) for v in vols])
    b_np = dict(frame_np, **{k: batch[k].cpu().numpy() for k in ("ray_o", "ray_d", "near", "far")})
    with torch.no_grad():
        ref = orc.render(sdt, b_np, n_samples=64, training=True, feature_volume=vols)
    raw, w_ref = ref["raw"].reshape(n, 64, 4).numpy(), ref["weights"][0].numpy()
    sigma_last, t_last = raw[:, -1, 3], 1.0 - w_ref[:, :-1].sum(1)
    err = np.abs(out["rgb_map"][0].cpu().numpy() - ref["rgb_map"][0].numpy()).max(1)
    ill = (np.abs(sigma_last) <= bench.FP32_SIGMA) & (sigma_last != 0)
    bound = np.where(ill, t_last + H.RGB_TOL, H.RGB_TOL)
    print("%s: rgb L-inf vs the oracle on the cut rays %.3g over %d rays (%d on the last-sample allowance)" % (precision, float(err.max()), n, int(ill.sum())))
    assert (err <= bound).all(), "rgb_map: max err %.3e over the bound at rays %s" % (float(err.max()), np.nonzero(err > bound)[0][:8].tolist())
    assert float(ref["rgb_map"].max() - ref["rgb_map"].min()) > 0.1, "degenerate fixture"
    # the finished picture: background outside the new mask, through render_views (rays one view ahead) as through render_view
    cams = [_camera(cb, yaw=0.35 + 0.3 * f) for f, (_, cb) in enumerate(made)]
    views = [(cams[f][0], cams[f][1], made[f][1], made[f][0]) for f in range(2)]
    outs = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()} for o in nv.render_views(iter(views))]
    assert len(outs) == 2 and outs[0]["n_rays"] == n
    for f, o in enumerate(outs):
        one = nv.render_view(*views[f])
        assert H.same_bits(o["img"], one["img"]) and torch.equal(o["mask_at_box"], one["mask_at_box"])
        outside = o["mask_at_box"] == 0
        assert bool((o["img"][outside] == 0).all()) and bool((o["depth"][outside] == 0).all()) and float(o["img"].max()) > 0.01
        assert 0 < o["n_rays"] == int(o["mask_at_box"].sum())
    # a frame made without the body's keys says what to do
    with pytest.raises(KeyError, match="body=True"):
        nv.view_batch(K, RT, can_bounds, {k: frame[k] for k in FRAME_KEYS})


def test_off_means_todays_frames_views_and_items():
    """body=False and body_bounds=None: the frame's keys and the image are what today's path gives, bit for bit; the plugin without
    the key yields today's item, and with ray_bounds: body the rays of BodyBounds.rays."""
    from neuralbody_amd import ops
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.ray_bounds import BodyBounds
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from neuralbody_amd.smpl_pose import MemoryPoseSource, PoseDataConfig

    drv, stacked = _small_body()
    sd, made, _, _, _ = _oracle()
    plain = drv.frames(*stacked, latent_index=[2, 3], new_params=True)
    assert all(set(frame) == FRAME_KEYS for frame, _ in plain)
    for (a, cb_a), (b, cb_b) in zip(plain, made):
        assert np.array_equal(cb_a, cb_b) and all(torch.equal(a[k], b[k]) for k in FRAME_KEYS)
    assert torch.equal(made[1][0]["body_verts"], drv.vertices(*stacked, new_params=True)[1:2])
    assert made[0][0]["body_verts"].data_ptr() + 4 * 6890 * 3 == made[1][0]["body_verts"].data_ptr()  # views of one tensor, no copy
    net = H.make_network(sd, DEV, True, "f32")
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=SIZE, W=SIZE))
    nv = NovelViewRenderer(rend, SIZE, SIZE, DEV)
    frame, can_bounds = plain[0]
    K, RT = _camera(can_bounds)
    got = nv.render_view(K, RT, can_bounds, frame)
    # today's path by hand: nb_raygen, the frame's keys, render, assemble
    ray_o, ray_d, near, far, mask, n_rays = ops.raygen(SIZE, SIZE, K, RT[:, :3], RT[:, 3], can_bounds, DEV)
    n = int(n_rays.item())
    batch = dict(frame, ray_o=ray_o[None, :n], ray_d=ray_d[None, :n], near=near[None, :n], far=far[None, :n], mask_at_box=mask[None])
    with torch.no_grad():
        out = rend.render(batch)
    img, _ = ops.image_assemble(mask, out["rgb_map"][0].contiguous(), out["depth_map"][0].contiguous())
    assert got["n_rays"] == n and H.same_bits(got["img"], img.view(SIZE, SIZE, 3))
    assert set(nv.view_batch(K, RT, can_bounds, frame)) == FRAME_KEYS | {"ray_o", "ray_d", "near", "far", "mask_at_box"}
    # the dataset plugin
    items = [dict(poses=stacked[0][i], shapes=stacked[1][i], Rh=stacked[2][i], Th=stacked[3][i]) for i in range(2)]
    cfg = types.SimpleNamespace(begin_ith_frame=5, frame_interval=2, num_train_frame=2, num_render_frame=-1, voxel_size=[0.005] * 3,
                                big_box=False, test_view=[0], H=SIZE, W=SIZE, ratio=1.0, params="new_params",
                                train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1))
    mod = H.load_plugin("light_stage_pose_dataset.py", cfg)
    ds = mod.Dataset("nowhere", "synthetic", "none.npy", "test", model=drv.model, device=DEV,
                     source=MemoryPoseSource(items, K, RT[:, :3], RT[:, 3], SIZE, SIZE))
    today = {"ray_o", "ray_d", "near", "far", "mask_at_box", "coord", "out_sh", "bounds", "R", "Th", "latent_index", "frame_index"}
    item = ds[0]
    assert set(item) == today and item["ray_o"].shape[0] == n
    for k, want in (("ray_o", ray_o[:n]), ("ray_d", ray_d[:n]), ("near", near[:n]), ("far", far[:n])):
        assert H.same_bits(item[k], want), k
    assert torch.equal(item["mask_at_box"], mask.view(torch.bool))
    cfg.ray_bounds = "box"
    assert all(torch.equal(ds[0][k], item[k]) for k in today - {"frame_index"})
    cfg.ray_bounds, cfg.ray_bounds_margin, cfg.ray_bounds_tile = "body", 0.03, 4
    cut = ds[0]
    assert set(cut) == today
    want = BodyBounds(0.03, 4).rays(SIZE, SIZE, K, RT, can_bounds, made[0][0]["body_verts"], made[0][0]["body_faces"], DEV)
    m = int(want[5].item())
    assert 0 < m < n and cut["ray_o"].shape[0] == m
    for k, w in (("ray_o", want[0]), ("ray_d", want[1]), ("near", want[2]), ("far", want[3])):
        assert H.same_bits(cut[k], w[:m]), k
    assert torch.equal(cut["mask_at_box"], want[4].view(torch.bool))
    assert all(torch.equal(cut[k], item[k]) for k in ("coord", "out_sh", "bounds", "R", "Th", "latent_index"))
    cfg.ray_bounds = "sphere"
    with pytest.raises(ValueError, match="ray_bounds"):
        ds[0]
    assert PoseDataConfig().ray_bounds == "box" and PoseDataConfig(ray_bounds="body", ray_bounds_tile=1).ray_bounds_tile == 1
    with pytest.raises(ValueError, match="ray_bounds"):
        PoseDataConfig(ray_bounds="mesh")
