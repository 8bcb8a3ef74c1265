"""nb_train_rays, TrainRaySampler and the dataset on the device: the fixture the reference's own samplers produced
(tests/golden/train_rays.npz) with its draws replayed as uniforms, random uniforms against the numpy restatement
(tests/train_rays_ref.py), short batches, repeatability, and one DataLoader -> NetworkWrapper training step."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import train_rays_ref as trr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_G = trr.fixture()
FLOATS = ("rgb", "ray_o", "ray_d", "near", "far")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sampler(c, n_rays, **kw):
    from neuralbody_amd.train_rays import TrainRaySampler

    Hh, Ww = c["msk"].shape
    return TrainRaySampler(Hh, Ww, n_rays, mode=c["mode"], device=DEV, **kw)


def _sample(s, c, u):
    out = s.sample(_dev(c["img"]), _dev(c["msk"]), c["K"], c["R"], c["T"], c["bounds"], u=_dev(u), hull=c["hull"])
    return out, {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    assert got["status"].tolist() == want["status"].tolist(), what
    assert np.array_equal(got["pixel"], want["pixel"]), what
    assert got["mask_at_box"].dtype == bool and np.array_equal(got["mask_at_box"], want["mask_at_box"]), what
    for k in FLOATS:
        a, b = got[k], np.ascontiguousarray(want[k], np.float32)
        assert a.dtype == np.float32 and a.shape == b.shape, (what, k)
        diff = int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max(initial=0))
        print("%s %s: max difference %d ulp" % (what, k, diff))
        assert diff == 0, (what, k, diff)


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_fixture_case_with_replayed_draws(name):
    c = trr.case_inputs(_G, name)
    N = int(_G[name + "/N"])
    s = _sampler(c, N)
    _, got = _sample(s, c, trr.replayed_uniforms(_G, name))
    highs = _G[name + "/draws_high"]
    want = {k: _G[name + "/" + k] for k in FLOATS}
    want.update(pixel=_G[name + "/coord"].astype(np.int32), mask_at_box=_G[name + "/mask_at_box"],
                status=np.array([N, len(_G[name + "/draws_k"]), highs[0, 0], highs[0, 1]]))
    _assert_same(got, want, "case " + name)
    assert s.check() == (N, len(_G[name + "/draws_k"]), int(highs[0, 0]), int(highs[0, 1])) and s.n_short == 0
    assert s.check() is None  # nothing pending any more


def _case_a_source(n_frames=1, n_views=1):
    from neuralbody_amd.train_rays import MemoryFrameSource

    item = [_G["A/" + k] for k in ("img", "msk", "K", "R", "T")]
    return MemoryFrameSource([tuple(item + [f, v, _G["A/xyz"], _G["A/Rh"], _G["A/Th"]]) for f in range(n_frames) for v in range(n_views)])


def test_case_d_test_split_through_the_dataset():
    """The test branch is the existing nb_raygen (float32 near/far on the cast rays): mask and rgb exactly, the rays to the
    bounds tests/test_gpu_parity.py::test_raygen_matches_reference_golden holds nb_raygen to (the last float32 bit).
    Measured on an MI355X against the fixture: ray_o and ray_d 0 ulp, near and far at most 1 ulp (the float32 divisions and
    square root of the full-image path, which this change does not touch)."""
    from neuralbody_amd.train_rays import TrainDataConfig, TrainRayDataset

    ds = TrainRayDataset(_case_a_source(), TrainDataConfig(N_rand=96), split="test", device=DEV)
    item = ds[0]
    mask = item["mask_at_box"].cpu().numpy()
    assert mask.dtype == bool and mask.shape == (48 * 40,) and np.array_equal(mask, _G["D/mask_at_box"])
    assert np.array_equal(item["rgb"].cpu().numpy(), _G["D/rgb"])
    for k in ("ray_o", "ray_d", "near", "far"):
        a, b = item[k].cpu().numpy(), _G["D/" + k]
        print("case D %s: max difference %d ulp" % (k, np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()))
    np.testing.assert_allclose(item["ray_o"].cpu().numpy(), _G["D/ray_o"], rtol=3e-7, atol=1e-7)
    np.testing.assert_allclose(item["ray_d"].cpu().numpy(), _G["D/ray_d"], rtol=3e-7, atol=1e-7)
    np.testing.assert_allclose(item["near"].cpu().numpy(), _G["D/near"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(item["far"].cpu().numpy(), _G["D/far"], rtol=1e-6, atol=1e-7)
    for k in ("coord", "out_sh", "bounds", "R", "Th"):
        assert np.array_equal(item[k].cpu().numpy(), _G["A/frame_" + k]), k
    assert (int(item["latent_index"]), item["frame_index"], item["cam_ind"]) == (0, 0, 0)


def _random_case():
    """64 x 64, N = 1500 (three strides of the sampling workgroup, the last wave partial), a box whose silhouette leaves the
    image on one side, h36m labels."""
    from tests import synthetic as syn
    from neuralbody_amd.train_rays import bound_hull

    body = syn.make_body(seed=9, box=(0.7, 1.1, 0.3), rh=(0.1, 0.5, 0.0), n_verts=64)
    K, R, T = syn.make_camera(body, 64, 64, focal_factor=1.4, distance=1.8, yaw=0.4, pitch=0.15)
    K[0, 2] -= 14.0  # push the silhouette over the left border
    rs = np.random.RandomState(21)
    yy, xx = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
    r = ((yy - 30) / 22) ** 2 + ((xx - 16) / 13) ** 2
    msk = np.zeros((64, 64), np.uint8)
    msk[r <= 1.0] = 100
    msk[r <= 0.75] = 1
    hull = bound_hull(body["can_bounds"], K, np.concatenate([R, T], axis=1))
    assert hull[:, 0].min() < 0 < hull[:, 0].max()
    return dict(img=rs.uniform(0, 1, (64, 64, 3)).astype(np.float32), msk=msk, K=K, R=R, T=T, bounds=body["can_bounds"],
                hull=hull, mode="h36m"), rs.uniform(0, 1, (4, 1500)).astype(np.float32)


def test_random_uniforms_match_the_restatement_and_repeat_bit_for_bit():
    c, u = _random_case()
    want = trr.sample(u=u, body_ratio=0.5, **c)
    assert want["status"][0] == 1500 and want["status"][1] >= 2  # a deficit round happened
    s = _sampler(c, 1500)
    out1, got = _sample(s, c, u)
    _assert_same(got, want, "random 1500")
    torch.empty(1 << 22, device=DEV).normal_()  # other work in between: the second call's scratch is not the first's
    out2, _ = _sample(s, c, u)
    for k in out1:
        assert torch.equal(out1[k].view(torch.uint8).reshape(-1), out2[k].view(torch.uint8).reshape(-1)), k
    c["mode"] = "plain"
    _assert_same(_sample(_sampler(c, 1500), c, u)[1], trr.sample(u=u, body_ratio=0.5, **c), "random 1500 plain")
    _assert_same(_sample(_sampler(c, 1500, body_sample_ratio=0.3), c, u)[1], trr.sample(u=u, body_ratio=0.3, **c), "ratio 0.3")


def test_short_batch_is_padded_and_counted():
    """Every pixel is a candidate but the box covers about a quarter of the image: four rounds cannot fill the batch."""
    c = trr.case_inputs(_G, "A")
    c["msk"] = np.ones_like(c["msk"])
    c["hull"] = np.array([[0, 0], [39, 0], [39, 47], [0, 47]])
    u = np.random.RandomState(5).uniform(0, 1, (4, 96)).astype(np.float32)
    want = trr.sample(u=u, body_ratio=0.5, **c)
    n = int(want["status"][0])
    assert 0 < n < 96 and want["status"][1] == 4
    s = _sampler(c, 96)
    _, got = _sample(s, c, u)
    _assert_same(got, want, "short batch")
    assert got["mask_at_box"][:n].all() and not got["mask_at_box"][n:].any()
    assert (got["pixel"][n:] == -1).all() and (got["rgb"][n:] == 0).all() and (got["near"][n:] == 0).all() and (got["far"][n:] == 0).all()
    assert np.isfinite(got["ray_d"]).all() and np.array_equal(got["ray_d"][n:], np.tile(got["ray_d"][n], (96 - n, 1)))
    assert s.check()[0] == n and s.n_short == 1


def test_a_class_without_candidates_raises_at_check():
    c = trr.case_inputs(_G, "A")
    c["msk"] = np.zeros_like(c["msk"])  # h36m: no body pixel
    u = np.random.RandomState(6).uniform(0, 1, (4, 96)).astype(np.float32)
    s = _sampler(c, 96)
    _, got = _sample(s, c, u)
    _assert_same(got, trr.sample(u=u, body_ratio=0.5, **c), "no body")
    assert got["status"][2] == 0 and got["status"][0] < 96
    with pytest.raises(RuntimeError, match="no body pixel"):
        s.check()
    s2 = _sampler(c, 96, body_sample_ratio=0.0)  # no body draws: an empty body class is nobody's problem
    _sample(s2, c, u)
    assert s2.check()[0] == 96


def test_sample_issues_no_synchronising_call():
    """torch.cuda.set_sync_debug_mode('error') makes every synchronising torch call raise; that this build honours it is checked
    first with a call that must synchronise (.item()).  If it does not, one sample() is captured into a single-stream
    torch.cuda.graph instead (capture refuses synchronisation) and the replay must give the eager call's bits."""
    c = trr.case_inputs(_G, "A")
    s = _sampler(c, 96, seed=3)
    img, msk = _dev(c["img"]), _dev(c["msk"])
    u = s.uniforms()
    eager = s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"], u=u)  # warm-up: library load, allocator, generator
    s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"])
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    saved = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            out = s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"])  # draws its own uniforms too
    finally:
        torch.cuda.set_sync_debug_mode(saved)
    if honoured:
        print("no-sync check: torch.cuda.set_sync_debug_mode('error')")
    else:
        print("no-sync check: sync debug mode is not honoured by this build; capturing sample() in a torch.cuda.graph")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = s.sample(img, msk, c["K"], c["R"], c["T"], c["bounds"], u=u)
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(out[k].view(torch.uint8).reshape(-1), eager[k].view(torch.uint8).reshape(-1)), k
    assert s.check()[0] == 96 and bool(out["mask_at_box"].all())
    a = _sampler(c, 96, seed=3).sample(img, msk, c["K"], c["R"], c["T"], c["bounds"])  # the sampler's own generator:
    b = _sampler(c, 96, seed=3).sample(img, msk, c["K"], c["R"], c["T"], c["bounds"])  # same seed, same draws
    assert torch.equal(a["pixel"], b["pixel"]) and torch.equal(a["pixel"], eager["pixel"])


def test_bad_arguments_are_refused_and_launch_nothing():
    from neuralbody_amd import _lib, ops

    c = trr.case_inputs(_G, "A")
    img, msk, u = _dev(c["img"]), _dev(c["msk"]), _dev(np.zeros((4, 96), np.float32))
    args = (c["K"], c["R"], c["T"], c["bounds"])
    with pytest.raises(ValueError):
        ops.train_rays(img, msk[:-1], *args, c["hull"], "h36m", 0.5, u)
    with pytest.raises(_lib.NbError, match="n_hull"):
        ops.train_rays(img, msk, *args, c["hull"][:2], "h36m", 0.5, u)
    with pytest.raises(_lib.NbError, match="body_ratio"):
        ops.train_rays(img, msk, *args, c["hull"], "h36m", 1.5, u)
    with pytest.raises(_lib.NbError):
        ops.train_rays(img.cpu(), msk, *args, c["hull"], "h36m", 0.5, u)


def test_one_training_step_from_the_dataloader():
    """Dataset over an in-memory source of 2 views x 2 frames -> DataLoader(num_workers=0, default_collate) ->
    plugins/if_nerf_clight.NetworkWrapper: a finite loss, gradients everywhere, and the batch's rgb is img[pixel]."""
    from tests import synthetic as syn
    from neuralbody_amd.train_rays import MemoryFrameSource, TrainDataConfig, TrainRayDataset

    size, items, imgs = 64, [], []
    yy, xx = np.meshgrid(np.arange(float(size)), np.arange(float(size)), indexing="ij")
    r = ((yy - 32) / 20) ** 2 + ((xx - 32) / 12) ** 2
    msk = np.zeros((size, size), np.uint8)
    msk[r <= 1.0] = 100
    msk[r <= 0.8] = 1
    for f in range(2):
        th = (0.02 * f, 0.0, 0.01 * f)
        body = syn.make_body(seed=0, box=(0.3, 0.5, 0.2), th=th)
        for v in range(2):
            K, R, T = syn.make_camera(body, size, size, focal_factor=2.5, distance=1.5, yaw=0.35 + 0.5 * v)
            img = np.random.RandomState(10 * f + v).uniform(0, 1, (size, size, 3)).astype(np.float32)
            imgs.append(img)
            items.append((img, msk, K, R, T, f, v, body["world_verts"], np.zeros(3), np.asarray(th, np.float32).reshape(1, 3)))
    ds = TrainRayDataset(MemoryFrameSource(items), TrainDataConfig(N_rand=1024, num_train_frame=2), device=DEV)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    sd = syn.make_weights(0, num_train_frame=5)
    net = H.make_network(sd, DEV, True, "f32")
    wrapper = H.load_plugin("if_nerf_clight.py").NetworkWrapper(net)
    seen = []
    for i, batch in enumerate(loader):
        assert batch["rgb"].shape == (1, 1024, 3) and batch["rgb"].is_cuda and batch["mask_at_box"].dtype == torch.bool
        assert batch["latent_index"].tolist() == [i // 2] and batch["frame_index"].tolist() == [i // 2] and batch["cam_ind"].tolist() == [i % 2]
        pix = ds.last_sample["pixel"].cpu().numpy()
        n = int(ds.last_sample["status"][0])
        assert n == 1024
        assert np.array_equal(batch["rgb"][0].cpu().numpy(), imgs[i][pix[:, 0], pix[:, 1]])
        seen.append(pix)
        if i == 0:
            ret, loss, stats, _ = wrapper(batch)
            assert ret["rgb_map"].shape == (1, 1024, 3) and torch.isfinite(loss)
            loss.backward()
            for name, p in net.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert len(seen) == 4 and ds.sampler.n_checked == 3 and ds.sampler.n_short == 0
    assert not np.array_equal(seen[0], seen[1])  # the generator moves on from item to item
