"""nb_smpl_silhouette (csrc/nb_silhouette.hip) and the cull keys of pose-driven frames (neuralbody_amd/smpl_pose.py) on the device.

The masks are held to the float64 reference of tests/silhouette_ref.py, computed on UNSNAPPED vertices: with tau = 1/256 px above
the snap's reach (2.8e-3 px), union(lo) <= mask <= union(hi) for a correct kernel, whatever it does inside the band between them
(tests/test_silhouette_host.py caps that band at 0.25 % of a mask for every mesh used here).  The kernel's definition is exact, so
the same cases are also compared, bit for bit, with its evaluation on the host (silhouette_ref.snapped_mask)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import silhouette_ref as sil
from tests import smpl_ref as sr
from tests import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = 64
MARGIN = 0.01  # metres; the 0.05 default is 9 px at 64 x 64 and leaves nothing of the small body's box to cull


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = sil.path_case() if name == "paths" else sil.band_case(name)
    lo, hi = sil.lo_hi_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], c["H"], c["W"])  # computed once, shared, never written
    return c, lo, hi


def _masks(c, **kw):
    from neuralbody_amd import ops

    return ops.smpl_silhouette(_dev(c["verts"]), _dev(c["faces"]), _dev(c["RTs"]), _dev(c["Ks"]), c["H"], c["W"], **kw)


def _check_band(name, got, lo, hi):
    m = got.cpu().numpy()
    assert m.dtype == np.uint8 and set(np.unique(m).tolist()) <= {0, 1}
    m = m.astype(bool)
    missing, extra = int((lo & ~m).sum()), int((m & ~hi).sum())
    print("%s: %s set pixels per mask, band %d pixels, %d pixels of lo missing, %d outside hi" % (
        name, m.sum(axis=(2, 3)).tolist(), int((hi & ~lo).sum()), missing, extra))
    assert missing == 0 and extra == 0
    return m


# ---------------------------------------------------------------------------------------------------------- 1. band
def test_masks_lie_between_lo_and_hi_and_a_dirty_buffer_changes_nothing():
    c, lo, hi = _case("ico320")
    assert c["verts"].shape[0] == 2 and c["Ks"].shape[0] == 3 and (c["H"], c["W"]) == (45, 61)
    got = _masks(c)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 45, 61)
    m = _check_band("ico320", got, lo, hi)
    assert m.any(axis=(2, 3)).all() and not torch.equal(got[0], got[1])
    dirty = torch.full_like(got, 0xAB)
    again = _masks(c, out=dirty)
    assert again is dirty and torch.equal(again, got)
    assert np.array_equal(m, sil.snapped_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], 45, 61).astype(bool))


# ---------------------------------------------------------------------------------------------------------- 2. paths
def test_large_small_clipped_and_degenerate_triangles():
    """silhouette_ref.path_case: a tetrahedron filling most of 96 x 128 (a workgroup per triangle), the same pulled back under
    16 px (a thread per triangle), partly and wholly off the image, both windings, a repeated-vertex face."""
    c, lo, hi = _case("paths")
    uv = [[sil.project(c["verts"][f], c["Ks"][v], c["RTs"][v])[0] for v in range(3)] for f in range(2)]
    assert np.ptp(uv[0][0], axis=0).min() > 90 and np.ptp(uv[0][1], axis=0).max() < 15  # view 0 large, view 1 small
    assert uv[0][2][:, 0].min() < -40 and uv[0][2][:, 0].max() > 20                       # view 2 partly off the image
    assert uv[1][0][:, 1].max() < -100 and uv[1][2][:, 1].max() < -100                    # frame 1 wholly off views 0 and 2
    got = _masks(c)
    m = _check_band("paths", got, lo, hi)
    assert m[0, 0].mean() > 0.4 and 0 < m[0, 1].sum() < 200 and m[0, 2].any() and m[1, 1].any()
    assert not m[1, 0].any() and not m[1, 2].any()
    assert np.array_equal(m, sil.snapped_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], 96, 128).astype(bool))
    # the zero-area faces and the winding draw nothing of their own: the four faces in their first winding give the same bits
    plain = dict(c, faces=sil.tetrahedron(0.25)[1])
    assert torch.equal(_masks(plain), got)


def test_more_listed_triangles_than_workgroups():
    """320 faces in two views at 256 x 256: more than 512 boxes of 17 or more pixels on a side, so the fixed grid of the
    large-triangle launch strides over its list and whole waves append to it."""
    v, faces = sil.icosphere(2, sil.ELLIPSOID)
    Ks, RTs = sil.orbit((0.2, 1.4), 1.5, 1.3 * 256, 256, 256)
    large = 0
    for view in range(2):
        uv = sil.project(v, Ks[view], RTs[view])[0][faces]  # [Nf,3,2]
        lo, hi = np.ceil(uv.min(axis=1) - 0.5), np.floor(uv.max(axis=1) + 0.5)
        assert lo.min() >= 0 and hi.max() <= 255  # all on the image
        large += int(((hi - lo).max(axis=1) >= 16).sum())
    print("%d of %d (view, triangle) boxes are large" % (large, 2 * len(faces)))
    assert len(faces) == 320 and large > 512
    c = dict(verts=v[None], faces=faces, Ks=Ks, RTs=RTs, H=256, W=256)
    lo, hi = sil.lo_hi_stack(c["verts"], faces, Ks, RTs, 256, 256)
    assert sil.band_fraction(lo, hi) <= sil.BAND_CAP
    m = _check_band("ico320 at 256 x 256", _masks(c), lo, hi)
    assert np.array_equal(m, sil.snapped_stack(c["verts"], faces, Ks, RTs, 256, 256).astype(bool))


# ---------------------------------------------------------------------------------------------------------- 3. views that do not cull
def test_a_view_too_near_or_too_wide_is_all_ones_and_leaves_the_others_alone():
    c, _, _ = _case("ico320")
    v = c["verts"][0].astype(np.float64)
    Hh, Ww = c["H"], c["W"]
    # camera 5 mm outside vertex k of the convex body, looking in along its normal: depth 0.005 m there, more everywhere else
    k = 17
    n = v[k] / np.array(sil.ELLIPSOID) ** 2
    n /= np.linalg.norm(n)
    K_near, RT_near = sil.look_at(v[k] + 0.005 * n, v[k] - n, 1.3 * Hh, Hh, Ww)
    uv, depth = sil.project(v, K_near, RT_near)
    assert abs(depth[k] - 0.005) < 1e-6 and depth.min() > 0.004 and np.abs(uv).max() < 20000.0
    # the first camera with a focal length of 10^6 px: depths stay near 2 m, projections reach beyond 10^5 px
    K_wide = c["Ks"][0].astype(np.float64).copy()
    K_wide[0, 0] = K_wide[1, 1] = 1e6
    uv, depth = sil.project(v, K_wide, c["RTs"][0])
    assert depth.min() > 1.0 and np.abs(uv).max() > 1e5
    Ks = np.stack([c["Ks"][1], K_near.astype(np.float32), K_wide.astype(np.float32)])
    RTs = np.stack([c["RTs"][1], RT_near.astype(np.float32), c["RTs"][0]])
    assert not sil.view_culls(c["verts"][0], Ks[1], RTs[1]) and not sil.view_culls(c["verts"][0], Ks[2], RTs[2])
    both = _masks(dict(c, Ks=Ks, RTs=RTs))
    alone = _masks(dict(c, Ks=Ks[:1], RTs=RTs[:1]))
    assert tuple(both.shape) == (2, 3, Hh, Ww) and tuple(alone.shape) == (2, 1, Hh, Ww)
    assert bool((both[0, 1] == 1).all()) and bool((both[0, 2] == 1).all())
    assert torch.equal(both[:, 0], alone[:, 0]) and 0 < int(both[0, 0].sum()) < Hh * Ww // 2
    assert bool((both[1, 2] == 1).all())  # the smaller frame is too wide for the 10^6 px camera as well


# ---------------------------------------------------------------------------------------------------------- 4. nothing of the body is culled
def test_no_point_of_the_surface_misses_the_dilated_mask():
    from neuralbody_amd import ops

    c, _, _ = _case("ico320")
    raw = _masks(c)
    pts = sil.surface_points(c["verts"][0], c["faces"], 20000, seed=5)
    for view in range(3):
        mask = ops.mask_dilate(raw[0, view:view + 1], 3)[0].cpu().numpy()
        x, y = sil.cull_pixels(pts, c["Ks"][view], c["RTs"][view], c["H"], c["W"])
        hit = mask[y, x] != 0
        print("view %d: %d of %d surface points on a set pixel of the 3 x 3 dilation, %d on the raw mask" % (
            view, int(hit.sum()), hit.size, int((raw[0, view].cpu().numpy()[y, x] != 0).sum())))
        assert hit.all()


# ---------------------------------------------------------------------------------------------------------- 5. driver, renderer
def _central_faces(v_template):
    """Triangles over the vertices in the middle of the small body's box (an ellipsoid of half the box), y-neighbours joined:
    a body that does not fill its box, so that silhouettes have something to cull."""
    inside = ((v_template / np.array([0.07, 0.15, 0.06])) ** 2).sum(axis=1) < 1.0
    idx = np.flatnonzero(inside)
    idx = idx[np.argsort(v_template[idx, 1], kind="stable")]
    return np.stack([idx[:-2], idx[1:-1], idx[2:]], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _small_body():
    """The 6890-vertex small body of the pose tests (tests/test_gpu_smpl_pose.py) with a triangle list.  The three frames share
    the first one's Rh and Th: the subject stays inside one rig of cull cameras, as on a light stage."""
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    arrays = sr.synthetic_smpl(21, 6890, sr.SMPL_PARENTS, box=(0.3, 0.5, 0.2))
    arrays["f"] = _central_faces(arrays["v_template"])
    assert 300 < len(arrays["f"]) < 2000
    model = SmplModel.from_arrays(arrays, DEV)
    P = [sr.draw_params(700 + i, sigma=0.1) for i in range(3)]
    return PoseDriver(model), [np.stack([p[k] if k < 2 else P[0][k] for p in P]) for k in range(4)]


def _camera(can_bounds, yaw=0.35):
    K, R, T = syn.make_camera({"can_bounds": can_bounds}, SIZE, SIZE, focal_factor=2.5, distance=1.5, yaw=yaw)
    return K, np.concatenate([R, T.reshape(3, 1)], axis=1)


def _cull_cameras(can_bounds):
    cams = [_camera(can_bounds, yaw) for yaw in (0.35, 1.7, 3.0)]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), SIZE, SIZE


def _border(can_bounds, Ks, RTs, margin):
    """The issue's formula, restated here."""
    cb = np.asarray(can_bounds, np.float64)
    z_near = min(float(RT[2, :3] @ np.array([cb[i, 0], cb[j, 1], cb[k, 2]]) + RT[2, 3])
                 for RT in np.asarray(RTs, np.float64) for i in (0, 1) for j in (0, 1) for k in (0, 1))
    px = math.ceil(margin * max(float(Ks[:, 0, 0].max()), float(Ks[:, 1, 1].max())) / (z_near - margin)) + 1
    return 2 * px + 1


FRAME_KEYS = {"coord", "out_sh", "bounds", "R", "Th", "latent_index"}


def test_frames_carry_the_dilated_silhouettes_and_render_culled():
    from neuralbody_amd import ops
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer, RendererMmsk

    drv, stacked = _small_body()
    probe = drv.frames(*stacked, latent_index=[2, 3, 4], new_params=True)
    assert all(set(frame) == FRAME_KEYS for frame, _ in probe)  # the default: today's frames
    cull = _cull_cameras(probe[0][1])
    made = drv.frames(*stacked, latent_index=[2, 3, 4], new_params=True, cull_cameras=cull, cull_margin=MARGIN)
    raw = drv.silhouettes(drv.vertices(*stacked, new_params=True), cull)
    assert tuple(raw.shape) == (3, 3, SIZE, SIZE) and raw.dtype == torch.uint8
    K32, RT32 = _dev(cull[0].astype(np.float32)), _dev(cull[1].astype(np.float32))
    want = []
    for f, (frame, can_bounds) in enumerate(made):
        assert set(frame) == FRAME_KEYS | {"msks", "Ks", "RT"} and np.array_equal(can_bounds, probe[f][1])
        assert {k: (tuple(frame[k].shape), frame[k].dtype) for k in ("msks", "Ks", "RT")} == {
            "msks": ((1, 3, SIZE, SIZE), torch.uint8), "Ks": ((1, 3, 3, 3), torch.float32), "RT": ((1, 3, 3, 4), torch.float32)}
        assert torch.equal(frame["Ks"][0], K32) and torch.equal(frame["RT"][0], RT32)
        border = _border(can_bounds, cull[0], cull[1], MARGIN)
        want.append(ops.mask_dilate(raw[f], border))
        share = float(raw[f].float().mean()), float(want[f].float().mean())
        print("frame %d: border %d, raw masks cover %.3f, dilated %.3f of the image" % (f, border, share[0], share[1]))
        assert 5 <= border <= 9 and 0.01 < share[0] < share[1] < 0.6
        assert torch.equal(frame["msks"][0], want[f]), f
        for k in FRAME_KEYS:
            assert torch.equal(frame[k], probe[f][0][k]), k
    # through the renderer: render_views over the driver's views against a batch assembled by hand from the same tensors
    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, True, "f32")
    cfg = RenderConfig(N_samples=64, perturb=0.0, H=SIZE, W=SIZE)
    culled, base = RendererMmsk(net, cfg), Renderer(net, cfg)
    nv = NovelViewRenderer(culled, SIZE, SIZE, DEV)
    cams = [_camera(cb, yaw=0.35 + 0.3 * f) for f, (_, cb) in enumerate(made)]
    views = list(drv.views(cams, *stacked, latent_index=[2, 3, 4], new_params=True, cull_cameras=cull, cull_margin=MARGIN))
    outs = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()} for o in nv.render_views(iter(views))]
    assert len(outs) == 3
    for f, out in enumerate(outs):
        by_hand = {k: made[f][0][k] for k in FRAME_KEYS}
        by_hand.update(msks=want[f][None], Ks=K32[None], RT=RT32[None])
        ref = nv.render_view(cams[f][0], cams[f][1], made[f][1], by_hand)
        assert out["n_rays"] == ref["n_rays"] > 0 and float(out["img"].max()) > 0.01
        assert H.same_bits(out["img"], ref["img"]) and H.same_bits(out["depth"], ref["depth"]), f
    batch = nv.view_batch(*views[1])
    with torch.no_grad():
        n_culled = int(torch.count_nonzero(culled.render(batch)["weights"]))
        n_base = int(torch.count_nonzero(base.render(batch)["weights"]))
    print("non-zero weights of frame 1: %d culled, %d unculled" % (n_culled, n_base))
    assert 0 < n_culled < n_base
    with pytest.raises(ValueError, match="cull_margin"):
        drv.frames(*stacked, latent_index=0, cull_cameras=cull, cull_margin=1.3)


def test_a_model_without_triangles_says_so():
    from neuralbody_amd import ops
    from neuralbody_amd.smpl_pose import PoseDriver, SmplModel

    arrays = {k: v for k, v in sr.case_model("tree321_new").items() if k != "f"}
    drv = PoseDriver(SmplModel.from_arrays(arrays, DEV))
    P = sr.case_params("tree321_new")
    (frame, can_bounds), = drv.frames(*P, latent_index=0)  # works exactly as today
    assert set(frame) == FRAME_KEYS
    cull = _cull_cameras(can_bounds)
    with pytest.raises(ops.NbError, match="triangle list"):
        drv.frames(*P, latent_index=0, cull_cameras=cull)
    with pytest.raises(ops.NbError, match="triangle list"):
        drv.silhouettes(drv.vertices(*P), cull)


# ---------------------------------------------------------------------------------------------------------- 6. defaults, plugin
def test_defaults_are_todays_items_and_cull_views_add_the_three_keys():
    from torch.utils.data.dataloader import default_collate

    from neuralbody_amd import _lib
    from neuralbody_amd.renderer import RenderConfig, RendererMmsk
    from neuralbody_amd.smpl_pose import MemoryPoseSource

    assert _lib.lib().nb_abi_version() == 20 and "nb_smpl_silhouette" in _lib.header_functions()
    drv, stacked = _small_body()
    items = [dict(poses=stacked[0][i], shapes=stacked[1][i], Rh=stacked[2][i], Th=stacked[3][i]) for i in range(2)]
    _, can_bounds = drv.frames(*stacked, latent_index=0)[0]
    K, RT = _camera(can_bounds)
    cull = _cull_cameras(can_bounds)
    cfg = types.SimpleNamespace(begin_ith_frame=5, frame_interval=2, num_train_frame=2, num_render_frame=-1, voxel_size=[0.005] * 3,
                                big_box=False, test_view=[0], H=SIZE, W=SIZE, ratio=1.0, params="new_params",
                                train=types.SimpleNamespace(num_workers=0), test=types.SimpleNamespace(batch_size=1))
    mod = H.load_plugin("light_stage_pose_dataset.py", cfg)
    ds = mod.Dataset("nowhere", "synthetic", "none.npy", "test", model=drv.model, device=DEV,
                     source=MemoryPoseSource(items, K, RT[:, :3], RT[:, 3], SIZE, SIZE, cull_cameras=cull))
    today = {"ray_o", "ray_d", "near", "far", "mask_at_box", "coord", "out_sh", "bounds", "R", "Th", "latent_index", "frame_index"}
    plain = ds[1]
    assert set(plain) == today
    cfg.cull_views, cfg.cull_margin = [2, 0], MARGIN
    item = ds[1]
    assert set(item) == today | {"msks", "Ks", "RT"}
    assert {k: (tuple(item[k].shape), item[k].dtype) for k in ("msks", "Ks", "RT")} == {
        "msks": ((2, SIZE, SIZE), torch.uint8), "Ks": ((2, 3, 3), torch.float32), "RT": ((2, 3, 4), torch.float32)}
    assert all(torch.equal(item[k], plain[k]) for k in today - {"frame_index"})
    frame = drv.frames(*[s[1:2] for s in stacked], latent_index=1, new_params=True,
                       cull_cameras=(cull[0][[2, 0]], cull[1][[2, 0]], SIZE, SIZE), cull_margin=MARGIN)[0][0]
    assert torch.equal(item["msks"], frame["msks"][0]) and torch.equal(item["RT"], _dev(cull[1][[2, 0]].astype(np.float32)))
    net = H.make_network(syn.make_weights(3, num_train_frame=7), DEV, True, "f32")
    with torch.no_grad():
        out = RendererMmsk(net, RenderConfig(N_samples=64, perturb=0.0, H=SIZE, W=SIZE)).render(default_collate([item]))
    n = item["ray_o"].shape[0]
    assert tuple(out["rgb_map"].shape) == (1, n, 3) and bool(torch.isfinite(out["rgb_map"]).all()) and float(out["rgb_map"].max()) > 0.01
