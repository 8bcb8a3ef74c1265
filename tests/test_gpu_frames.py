"""Multi-frame sequences (run.py:94-100 / Trainer.train: every iteration frees the previous batch and `.cuda()`s a new one).

Round 1 cached the host copies of R / Th / bounds — and the reusable feature volumes and the tile order — under
(data_ptr, _version, shape).  The caching allocator hands a freed batch's addresses to the next batch, so frame k+1
could be marched with frame k's pose (VERDICT r01 "What's weak" #1, ADVICE high).  The pose block is now read by the
kernels from device memory and the remaining caches hold the tensors they were built from; this file renders frames
in a loop through FRESHLY allocated batches on ONE Network and checks every frame against the oracle.
`NB_FRAMES_EXPECT_STALE=1` inverts the assertion (used once, on the round-1 tree, to show that the test sees the bug:
profiles/r02_stale_pose_repro.md)."""
import os

import numpy as np
import pytest
import torch

from tests import synthetic as syn
from tests import helpers as H
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FRAMES = 8


def _frame(f):
    """Frame f: its own pose (R, Th), bounds and voxel coordinates; tensor SHAPES are identical for every f."""
    body = syn.make_body(seed=20 + f, box=(0.3, 0.5, 0.2), rh=(0.1 + 0.25 * f, 0.2 - 0.15 * f, -0.1 + 0.2 * f),
                         th=(0.05 - 0.1 * f, -0.1 + 0.07 * f, 0.2 + 0.11 * f))
    K, R, T = syn.make_camera(body, 16, 16, focal_factor=2.5, distance=1.5, yaw=0.35 + 0.3 * f)
    ray_o, ray_d, near, far, mask = syn.host_image_rays(16, 16, K, R, T, body["can_bounds"])
    return body, syn.make_batch(body, ray_o, ray_d, near, far, mask, latent_index=f % 7), (K, R, T)


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
def test_fresh_batch_per_frame_never_sees_the_previous_pose(precision):
    from neuralbody_amd.renderer import RenderConfig, Renderer
    from oracle import neuralbody_oracle as orc

    sd = syn.make_weights(3, num_train_frame=7)
    sdt = orc.tensor_state_dict(sd)
    net = H.make_network(sd, DEV, True, precision)
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
    errs, worst_prev = [], 0.0
    prev_ref = None
    for f in range(N_FRAMES):
        body, batch, _ = _frame(f)
        bd = H.device_batch(batch, DEV)  # fresh .cuda() tensors, like run.py:95-97
        with torch.no_grad():
            out = rend.render(bd)
        rgb = out["rgb_map"].cpu().numpy()
        del bd, out  # the allocator is now free to hand these addresses to frame f + 1
        with torch.no_grad():
            ref = orc.render(sdt, batch, n_samples=64, training=True)["rgb_map"].numpy()
        errs.append(float(np.abs(rgb - ref).max()) if rgb.shape == ref.shape else float("inf"))
        assert float(ref.max()) > 0.05, "degenerate frame %d" % f
        if prev_ref is not None and prev_ref.shape == ref.shape:
            worst_prev = max(worst_prev, float(np.abs(ref - prev_ref).max()))
        prev_ref = ref
    print("%s: per-frame rgb L-inf vs oracle: %s" % (precision, " ".join("%.1e" % e for e in errs)))
    if os.environ.get("NB_FRAMES_EXPECT_STALE"):
        assert max(errs) > 1e-3, "expected the round-1 tree to render some frame with a stale pose"
        return
    assert max(errs) <= H.RGB_TOL, errs


def test_a_pose_rewritten_under_a_new_frame_token_is_marched():
    """a caller that rewrites R / Th / bounds in place without moving their version counters (a raw-pointer writer) and
    says so with a new `frame_token` is marched with the new pose, not with the pose block kept for the old token."""
    from neuralbody_amd.renderer import RenderConfig, Renderer

    sd = syn.make_weights(3, num_train_frame=7)
    net = H.make_network(sd, DEV, True, H.DEFAULT_PRECISION)
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
    bd = H.device_batch(_frame(0)[1], DEV)
    moved = bd["Th"] + 0.05
    with torch.no_grad():
        old = rend.render(dict(bd, frame_token=0))["rgb_map"].clone()
        version = bd["Th"]._version
        bd["Th"].data.copy_(moved)  # through `.data`: the tensor's version counter does not move
        assert bd["Th"]._version == version
        got = rend.render(dict(bd, frame_token=1))["rgb_map"].clone()
        ref = rend.render(dict(bd, Th=moved.clone()))["rgb_map"]  # the new pose in a tensor of its own
    assert float((old - ref).abs().max()) > 1e-2  # the pose change is visible
    assert H.same_result(got, ref, "f16f6", tol=2e-5)


def test_reuse_volumes_follows_the_frame():
    """NovelViewRenderer(reuse_volumes=True): two views of frame A share one encode; frame B (fresh tensors, same shapes)
    must be re-encoded even if its `coord` lands on frame A's old address."""
    from neuralbody_amd.novel_view import NovelViewRenderer
    from neuralbody_amd.renderer import RenderConfig, Renderer

    sd = syn.make_weights(3, num_train_frame=7)
    net = H.make_network(sd, DEV, True, "f32")
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=24, W=24))
    fast = NovelViewRenderer(rend, 24, 24, DEV, reuse_volumes=True)
    slow = NovelViewRenderer(rend, 24, 24, DEV, reuse_volumes=False)
    calls = {"n": 0}
    enc = net.encode_sparse_voxels

    def counting(sp, save=None):
        calls["n"] += 1
        return enc(sp, save)

    net.encode_sparse_voxels = counting
    try:
        for f in range(4):
            body, batch, (K, R, T) = _frame(f)
            RT = np.concatenate([R, T.reshape(3, 1)], 1)
            keys = ("coord", "out_sh", "bounds", "R", "Th", "latent_index")
            frame = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).to(DEV) for k in keys}
            before = calls["n"]
            a = fast.render_view(K, RT, body["can_bounds"], frame)["img"].clone()
            a2 = fast.render_view(K, RT, body["can_bounds"], frame)["img"].clone()
            assert calls["n"] == before + 1, "the second view of a frame must reuse its volumes"
            b = slow.render_view(K, RT, body["can_bounds"], frame)["img"]
            assert torch.equal(a, b) and torch.equal(a2, b), "frame %d rendered from another frame's volumes" % f
            del frame, a, a2, b
    finally:
        net.encode_sparse_voxels = enc


@pytest.mark.parametrize("precision", ["f32", H.DEFAULT_PRECISION])
def test_prefetched_encoder_renders_the_same_frames(precision):
    """Renderer.prefetch: frame f + 1 encoded on a second stream beside frame f's march gives the frames of the serial loop
    (fresh batches per frame, dropped right after their render); the ticket of another frame is ignored; a frame tensor
    modified in place after the prefetch is encoded again."""
    from neuralbody_amd.renderer import RenderConfig, Renderer

    sd = syn.make_weights(3, num_train_frame=7)
    net = H.make_network(sd, DEV, True, precision)
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
    frames = [_frame(f)[1] for f in range(5)]
    with torch.no_grad():
        serial = [rend.render(H.device_batch(b, DEV))["rgb_map"].clone() for b in frames]
        calls = {"n": 0}
        enc = net.encode_sparse_voxels

        def counting(sp, save=None):
            calls["n"] += 1
            return enc(sp, save)

        net.encode_sparse_voxels = counting
        try:
            nxt = H.device_batch(frames[0], DEV)
            piped = []
            ticket = None
            for f in range(5):
                cur, nxt = nxt, (H.device_batch(frames[f + 1], DEV) if f + 1 < 5 else None)
                cur_ticket, ticket = ticket, (rend.prefetch(nxt) if nxt is not None else None)
                piped.append(rend.render(cur, prefetched=cur_ticket)["rgb_map"].clone())
                del cur, cur_ticket
            assert calls["n"] == 5, calls  # frame 0 inside its render(), 1..4 ahead
            # the other calling order: a fence in front of render(), the prefetch behind it (the march reaches the device first),
            # every ticket dropped as early as a caller can
            nxt, ticket, fenced = H.device_batch(frames[0], DEV), None, []
            for f in range(5):
                cur, nxt = nxt, (H.device_batch(frames[f + 1], DEV) if f + 1 < 5 else None)
                fence = rend.fence()
                fenced.append(rend.render(cur, prefetched=ticket)["rgb_map"].clone())
                del cur, ticket
                ticket = rend.prefetch(nxt, after=fence) if nxt is not None else None
            assert calls["n"] == 10, calls
            # a ticket of another frame: ignored, the rendered frame is encoded in place
            a, b = H.device_batch(frames[1], DEV), H.device_batch(frames[2], DEV)
            ta = rend.prefetch(a)
            other = rend.render(b, prefetched=ta)["rgb_map"].clone()
            assert calls["n"] == 12
            late = rend.render(a, prefetched=ta)["rgb_map"].clone()  # its own frame, two renders later
            assert calls["n"] == 12
            # in-place change of a frame tensor after the prefetch: the volumes are stale, render() encodes again
            c = H.device_batch(frames[3], DEV)
            tc = rend.prefetch(c)
            c["coord"].copy_(H.device_batch(frames[4], DEV)["coord"])
            for k in ("out_sh", "bounds", "R", "Th"):
                c[k].copy_(H.device_batch(frames[4], DEV)[k])
            c["latent_index"].copy_(H.device_batch(frames[4], DEV)["latent_index"])
            for k in ("ray_o", "ray_d", "near", "far", "mask_at_box"):
                c[k] = H.device_batch(frames[4], DEV)[k]
            changed = rend.render(c, prefetched=tc)["rgb_map"].clone()
            assert calls["n"] == 14
        finally:
            net.encode_sparse_voxels = enc
    torch.cuda.synchronize()
    def same(x, y):  # the encoder's batch statistics are sums of atomics: equal to rounding, run to run
        return x.shape == y.shape and float((x - y).abs().max()) <= 2e-6

    for f in range(5):
        assert same(piped[f], serial[f]) and same(fenced[f], serial[f]), f
        assert f == 0 or not same(serial[f], serial[f - 1]), "frames must differ for the test to see a mix-up"
    assert same(other, serial[2]) and same(late, serial[1]) and same(changed, serial[4])
    with pytest.raises(RuntimeError):
        rend.prefetch(H.device_batch(frames[0], DEV))  # autograd on: the training step encodes inside its graph


def test_prefetch_queues_behind_an_inline_encoder_pass():
    """a render() that encodes inline on the main stream (no ticket: the first view of a loop) followed by a fenced
    prefetch — the prefetched pass must queue behind the inline one, since in train() mode both update the BatchNorm running
    statistics in place.  The statistics and counters after the loop equal those of the serial loop."""
    import copy

    from neuralbody_amd.renderer import RenderConfig, Renderer

    sd = syn.make_weights(3, num_train_frame=7)
    net_a = H.make_network(sd, DEV, True, H.DEFAULT_PRECISION)
    net_b = copy.deepcopy(net_a)
    frames = [_frame(f)[1] for f in range(4)]
    with torch.no_grad():
        ra = Renderer(net_a, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
        for b in frames:
            ra.render(H.device_batch(b, DEV))
        rb = Renderer(net_b, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
        nxt, ticket = H.device_batch(frames[0], DEV), None
        for f in range(4):
            cur, nxt = nxt, (H.device_batch(frames[f + 1], DEV) if f + 1 < 4 else None)
            fence = rb.fence()
            rb.render(cur, prefetched=ticket)  # f == 0: encodes inline, then every later pass comes from a ticket
            assert getattr(rb, "_inline_enc", None) is not None  # recorded by the inline pass of f == 0
            ticket = rb.prefetch(nxt, after=fence) if nxt is not None else None
    torch.cuda.synchronize()
    sa, sb = net_a.state_dict(), net_b.state_dict()
    for k in sa:
        if k.endswith("num_batches_tracked"):
            assert int(sa[k]) == int(sb[k]) == 4, k
        elif "running_" in k:
            assert float((sa[k] - sb[k]).abs().max()) <= 1e-6 * max(1.0, float(sa[k].abs().max())), k


def test_rays_without_a_slot_read_zero():
    """a mask that names fewer pixels than the batch holds rays — the slot list then covers only the first rays; the
    others must come back as zeros, not as uninitialised memory."""
    from neuralbody_amd.renderer import RenderConfig, Renderer

    sd = syn.make_weights(3, num_train_frame=7)
    net = H.make_network(sd, DEV, True, H.DEFAULT_PRECISION)  # (batch statistics, as the other tests of this scene: a visible body)
    body, b, _ = _frame(0)
    bd = H.device_batch(b, DEV)
    n = bd["ray_o"].shape[1]
    rend = Renderer(net, RenderConfig(N_samples=64, perturb=0.0, H=16, W=16))
    short = bd["mask_at_box"].clone().reshape(-1)
    assert n >= 128
    keep = n - min(70, n // 3)
    idx = torch.nonzero(short).reshape(-1)[keep:]
    short[idx] = False  # the last rays have no pixel any more
    bad = dict(bd)
    bad["mask_at_box"] = short.reshape(bd["mask_at_box"].shape)
    with torch.no_grad():
        torch.empty((n, 64), device=DEV).fill_(float("nan"))  # poison the allocator's free blocks
        out = rend.render(bad)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["rgb_map"]).all()) and float(out["weights"][0, keep:].abs().max()) == 0.0
    assert float(out["rgb_map"][0, :keep].abs().max()) > 0.0


@pytest.mark.parametrize("precision", ["f16f6", "f32"])
def test_a_batch_of_two_frames_matches_the_reference_frame_by_frame(precision):
    """B = 2 through Renderer.render, prepare_sp_input / encode_sparse_voxels / calculate_density_color: two
    frames with their own vertices, pose, bounds, latent index and rays, one common out_sh (the batch maximum).  Fixture: the
    reference run frame by frame (tests/golden/scene_batch2.npz; the reference itself raises on the B = 2 batch)."""
    import os

    from neuralbody_amd.network import BatchedFeatureVolumes

    g = np.load(os.path.join(H.GOLDEN, "scene_batch2.npz"))
    r, sd, batch, frames = scenes.build_batch2()
    net = H.make_network(sd, DEV, True, precision)
    rend = H.make_renderer(net, dict(n_samples=r["n_samples"], perturb=False, white_bkgd=False))
    bd = H.device_batch(batch, DEV)
    with torch.no_grad():
        out = rend.render(bd)
        sp = rend.prepare_sp_input(bd)
        vols = net.encode_sparse_voxels(sp)
        again = rend.render(bd, feature_volume=vols)  # the batch's volumes handed back in: frame b marches frames[b]
    torch.cuda.synchronize()
    assert out["rgb_map"].shape == (2, r["n_rays"], 3) and out["weights"].shape == (2, r["n_rays"], r["n_samples"])
    err = H.assert_close(out["rgb_map"].cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    H.assert_close(out["acc_map"].cpu().numpy(), g["acc_map"], 2e-4, "acc_map")
    H.assert_close(out["weights"].cpu().numpy(), g["weights"], 2e-4, "weights")
    H.assert_close(out["depth_map"].cpu().numpy(), g["depth_map"], 2e-4, "depth_map")
    # (train-mode BatchNorm sums its statistics with atomics: a second encode of the same frame agrees to rounding)
    H.assert_close(again["rgb_map"].cpu().numpy(), out["rgb_map"].cpu().numpy(), 2e-5, "re-render from the batch's volumes")
    # the reference API on the batch: four [B,C,D,H,W] volumes at the common out_sh, and the point decoder frame by frame
    assert isinstance(vols, BatchedFeatureVolumes) and sp["batch_size"] == 2
    with torch.no_grad(), pytest.raises(NotImplementedError, match="ONE frame"):
        rend.prefetch(bd)
    D, Hh, W = sp["out_sh"]
    assert [tuple(v.shape) for v in vols] == [(2, c, D >> (l + 1), Hh >> (l + 1), W >> (l + 1)) for l, c in enumerate((32, 64, 128, 128))]
    wpts, z = rend.get_sampling_points(bd["ray_o"][:, ::16], bd["ray_d"][:, ::16], bd["near"][:, ::16], bd["far"][:, ::16])
    viewdir = bd["ray_d"][:, ::16] / torch.norm(bd["ray_d"][:, ::16], dim=2, keepdim=True)
    with torch.no_grad():
        raw = rend.get_density_color(wpts, viewdir, lambda x, v: net.calculate_density_color(x, v, vols, sp))
        dens = net.calculate_density(wpts.reshape(2, -1, 3), vols, sp)
    assert raw.shape == (2, wpts.shape[1] * r["n_samples"], 4) and dens.shape == (2, wpts.shape[1] * r["n_samples"], 1)
    assert float((raw[..., 3:] - dens).abs().max()) <= (2e-3 if precision == "f16f6" else 1e-5)
    pv = rend.get_pixel_value(bd["ray_o"][:, ::16], bd["ray_d"][:, ::16], bd["near"][:, ::16], bd["far"][:, ::16], vols, sp, bd)
    H.assert_close(pv["rgb_map"].cpu().numpy(), g["rgb_map"][:, ::16], 6e-5, "unfused path on the batch")
    print("batch of two frames, %s: rgb L-inf vs the reference run frame by frame %.2e" % (precision, err))


def test_a_batch_of_two_frames_trains():
    """The differentiable path on B = 2: the loss over both frames, gradients = the sum of the two single-frame passes."""
    r, sd, batch, frames = scenes.build_batch2()
    tgt = torch.rand((2, r["n_rays"], 3), generator=torch.Generator().manual_seed(5)).to(DEV)

    def grads(b_np, target):
        net = H.make_network(sd, DEV, True, "f32")
        rend = H.make_renderer(net, dict(n_samples=r["n_samples"], perturb=False, white_bkgd=False))
        out = rend.render(H.device_batch(b_np, DEV))
        loss = ((out["rgb_map"] - target) ** 2).sum()
        loss.backward()
        return float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    l2, g2 = grads(batch, tgt)
    l0, g0 = grads(frames[0], tgt[0:1])
    l1, g1 = grads(frames[1], tgt[1:2])
    torch.cuda.synchronize()
    assert abs(l2 - (l0 + l1)) <= 1e-5 * abs(l2)
    assert set(g2) == set(g0) == set(g1) and len(g2) >= 60
    for k in g2:
        scale = float(g2[k].abs().max()) + 1e-30
        assert float((g2[k] - (g0[k] + g1[k])).abs().max()) <= 2e-4 * scale, k


def test_prefetch_as_a_hip_graph_renders_the_same_views():
    """Renderer.use_encoder_graph: the prefetched encoder pass captured into two alternating HIP graphs (one launch per pass).  A loop
    over 7 views of one frame — pass 1 eager, passes 2 and 3 the captures, the rest replays — must give the images of the eager loop
    (train-mode BatchNorm as run.py renders: its statistics are summed with atomics, so two passes over one frame agree to rounding,
    not bit for bit), and a change of the weights must drop the captured graphs (they replay addresses AND packed weights)."""
    import bench

    dev = torch.device(DEV)
    sd, body, net, rend, bd, n = bench.build_scene(dev, 64, 64, 16, None)
    poses = bench.build_poses(dev, body, bd, 64, 64, n_poses=4)

    def loop(use_graph, n_views=7):
        rend.use_encoder_graph = use_graph
        rend._enc_graphs = None
        out, ticket = [], None
        with torch.no_grad():
            for i in range(n_views):
                fence = rend.fence()
                out.append(rend.render(poses[i % 4], prefetched=ticket)["rgb_map"].clone())
                ticket = rend.prefetch(poses[(i + 1) % 4], after=fence)
        torch.cuda.synchronize()
        return out

    eager = loop(False)
    graph = loop(True)
    st = rend._enc_graphs
    assert st is not None and len(st["slots"]) == 2 and st["seen"] == 7
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert H.same_result(a, b, "f16f6", tol=2e-5), "view %d differs between the eager and the graph-replayed encoder pass" % i
    assert float((eager[0] - eager[1]).abs().max()) > 1e-2  # the poses are different views
    # new weights: the key changes, the graphs are dropped and captured again
    with torch.no_grad():
        net.xyzc_net.conv4[6].weight.mul_(-1.0)  # (a scale would be undone by the BatchNorm behind the convolution)
    g2 = loop(True)
    assert rend._enc_graphs is not st and len(rend._enc_graphs["slots"]) == 2
    e2 = loop(False)
    for a, b in zip(e2, g2):
        assert H.same_result(a, b, "f16f6", tol=2e-5)
    assert float((e2[2] - eager[2]).abs().max()) > 1e-3  # ... and the new weights render something else
    rend.use_encoder_graph = False
