"""GPU tests of the backward pass (training step, §8 row a15) against PyTorch autograd run through the CPU oracle
(the reference's own backward IS autograd through the same operations).  Gradients are compared relative to the
largest reference entry of each tensor: fp32 GEMMs with different summation orders over N = rays x samples rows."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.golden import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# gradient agreement with a MASK-CONSISTENT float64 reference (same ReLU pattern on both sides), relative to each tensor's
# largest entry: what remains is fp32 rounding through 17 batch-statistics BatchNorm layers
ENC_TOL = 1e-4  # measured 8e-6 (encoder alone) / 1.2e-5 (whole training step, all 69 tensors)


def _rel(a, b, tol, name):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    assert err <= tol, "%s: max |diff| / max |ref| = %.3e > %.1e (ref max %.3e)" % (name, err, tol, scale)
    return err


def _encoder_masks(ctx):
    """ReLU masks of the HIP encoder forward (records of SparseConvNet.forward(save=...)) in the oracle's row order
    (linear voxel order of the layer's active set)."""
    masks = []
    for rec in ctx[1:]:
        n = int(rec["n_out"])
        order = torch.argsort(rec["out_lin"][:n].long())
        masks.append((rec["y"][:n][order] > 0).cpu())
    return masks


def _mlp_masks(tap):
    from neuralbody_amd.ops import TAP

    return {k: (tap[:, TAP[k][0]:TAP[k][1]] > 0).cpu() for k in ("h1", "h2", "h3", "V")}


def test_composite_bwd_matches_autograd():
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    rs = np.random.RandomState(11)
    for n, S, white in ((37, 64, False), (9, 128, True), (5, 20, False)):
        raw = torch.from_numpy((rs.standard_normal((n, S, 4)) * 2).astype(np.float32)).requires_grad_(True)
        z = torch.from_numpy(np.sort(rs.uniform(1, 3, (n, S)).astype(np.float32), axis=1))
        d = torch.from_numpy(rs.standard_normal((n, 3)).astype(np.float32))
        g_rgb = torch.from_numpy(rs.standard_normal((n, 3)).astype(np.float32))
        g_acc = torch.from_numpy(rs.standard_normal(n).astype(np.float32))
        g_dep = torch.from_numpy(rs.standard_normal(n).astype(np.float32))
        rgb, disp, acc, w, depth = orc.raw2outputs(raw, z, d, white)
        ((rgb * g_rgb).sum() + (acc * g_acc).sum() + (depth * g_dep).sum()).backward()
        got = ops.composite_bwd(raw.detach().to(DEV), z.to(DEV), d.to(DEV), g_rgb.to(DEV), white, g_acc.to(DEV), g_dep.to(DEV))
        _rel(got.cpu().numpy(), raw.grad.numpy(), 2e-5, "d raw n=%d S=%d" % (n, S))
        # rgb-only cotangent (the reference loss, if_nerf_clight.py:25)
        raw.grad = None
        rgb, disp, acc, w, depth = orc.raw2outputs(raw, z, d, white)
        (rgb * g_rgb).sum().backward()
        got = ops.composite_bwd(raw.detach().to(DEV), z.to(DEV), d.to(DEV), g_rgb.to(DEV), white)
        _rel(got.cpu().numpy(), raw.grad.numpy(), 2e-5, "d raw (rgb only)")


def test_sgemm_relu_colsum():
    from neuralbody_amd import ops

    rs = np.random.RandomState(3)
    a = torch.from_numpy(rs.standard_normal((257, 40)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rs.standard_normal((40, 33)).astype(np.float32)).to(DEV)
    wide = torch.from_numpy(rs.standard_normal((257, 100)).astype(np.float32)).to(DEV)
    np.testing.assert_allclose(ops.sgemm(a, b).cpu().numpy(), (a @ b).cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ops.sgemm(a, a, trans_a=True).cpu().numpy(), (a.T @ a).cpu().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(ops.sgemm(b, b, trans_b=True).cpu().numpy(), (b @ b.T).cpu().numpy(), rtol=1e-4, atol=1e-3)
    # column slices as operands and as the (accumulating) destination
    out = torch.ones((257, 50), device=DEV)
    ref = out.clone()
    ref[:, 10:43] += 2.0 * (wide[:, 5:45] @ b)
    ops.sgemm(wide[:, 5:45], b, out=out[:, 10:43], alpha=2.0, beta=1.0)
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ops.colsum(wide[:, 7:90]).cpu().numpy(), wide[:, 7:90].sum(0).cpu().numpy(), rtol=1e-4, atol=1e-3)
    # long-K transposed products take the split-K MFMA path (weight-gradient shape), incl. slices and accumulation
    big_a = torch.from_numpy(rs.standard_normal((9000, 70)).astype(np.float32)).to(DEV)
    big_b = torch.from_numpy(rs.standard_normal((9000, 45)).astype(np.float32)).to(DEV)
    ref = (big_a[:, 3:68].double().T @ big_b[:, 2:43].double()).float()
    np.testing.assert_allclose(ops.sgemm(big_a[:, 3:68], big_b[:, 2:43], trans_a=True).cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-3)
    acc = torch.full((65, 50), 0.5, device=DEV)
    ops.sgemm(big_a[:, 3:68], big_b[:, 2:43], trans_a=True, out=acc[:, 4:45], alpha=2.0, beta=1.0)
    np.testing.assert_allclose(acc[:, 4:45].cpu().numpy(), (0.5 + 2.0 * ref).cpu().numpy(), rtol=2e-4, atol=4e-3)
    assert float(acc[:, :4].min()) == 0.5 and float(acc[:, 45:].max()) == 0.5
    # fused epilogues of the backward chain: ReLU mask of the layer below + its bias gradient (column sums), accumulate form,
    # ragged sizes (rows not a multiple of 32, K odd, N not a multiple of 32) and strided operands
    for (m, k, n) in ((257, 3, 128), (1000, 129, 45), (64, 256, 352)):
        A = torch.from_numpy(rs.standard_normal((m, k + 5)).astype(np.float32)).to(DEV)
        Bm = torch.from_numpy(rs.standard_normal((k, n + 3)).astype(np.float32)).to(DEV)
        Y = torch.from_numpy(rs.standard_normal((m, n + 7)).astype(np.float32)).to(DEV)
        C0 = torch.from_numpy(rs.standard_normal((m, n + 2)).astype(np.float32)).to(DEV)
        ref = (C0[:, 1:n + 1].double() + A[:, 2:k + 2].double() @ Bm[:, 1:n + 1].double()) * (Y[:, 4:n + 4] > 0)
        out = C0.clone()
        cs = torch.full((n,), 0.25, device=DEV)
        ops.sgemm(A[:, 2:k + 2], Bm[:, 1:n + 1], out=out[:, 1:n + 1], beta=1.0, relu_mask=Y[:, 4:n + 4], colsum=cs)
        np.testing.assert_allclose(out[:, 1:n + 1].cpu().numpy(), ref.float().cpu().numpy(), rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(cs.cpu().numpy(), 0.25 + ref.sum(0).float().cpu().numpy(), rtol=1e-4, atol=2e-3)
        assert torch.equal(out[:, 0], C0[:, 0]) and torch.equal(out[:, n + 1], C0[:, n + 1])
    # weight-gradient shapes with 16-byte aligned rows take the 16-bit matrix pipe (bf16 head + remainder pairs, fragments by
    # ds_read_b64_tr_b16): ragged M = 346 (view_fc's input width) and N, a row count that is not a multiple of the 32-row chunk,
    # accumulation into a slice
    wa = torch.from_numpy(rs.standard_normal((5003, 400)).astype(np.float32)).to(DEV)
    wb = torch.from_numpy(rs.standard_normal((5003, 260)).astype(np.float32)).to(DEV)
    for (c0, c1, d0, d1) in ((8, 354, 4, 260), (0, 256, 0, 128), (16, 48, 100, 133)):
        ref = (wa[:, c0:c1].double().T @ wb[:, d0:d1].double()).float()
        got = ops.sgemm(wa[:, c0:c1], wb[:, d0:d1], trans_a=True)
        np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=4e-3)
        assert float((got - ref).abs().max()) <= 3e-5 * float(ref.abs().max()) + 1e-3  # ~2^-16 relative of the column norms
    acc2 = torch.full((346, 300), 0.25, device=DEV)
    ref = (wa[:, 8:354].double().T @ wb[:, 4:260].double()).float()
    ops.sgemm(wa[:, 8:354], wb[:, 4:260], trans_a=True, out=acc2[:, 20:276], alpha=0.5, beta=1.0)
    np.testing.assert_allclose(acc2[:, 20:276].cpu().numpy(), (0.25 + 0.5 * ref).cpu().numpy(), rtol=1e-4, atol=4e-3)
    assert float(acc2[:, :20].min()) == 0.25 and float(acc2[:, 276:].max()) == 0.25
    # dX shapes (thousands of rows, K a multiple of 32, aligned operands) take the 16-bit matrix pipe as well: bf16 pairs, the
    # fused ReLU-mask / bias-gradient epilogue, accumulation, ragged N and a row count that is not a multiple of 128
    for (m, k, n) in ((2050, 256, 352), (1100, 128, 260), (4096, 384, 128)):
        A = torch.from_numpy(rs.standard_normal((m, k + 8)).astype(np.float32)).to(DEV)
        Bm = torch.from_numpy(rs.standard_normal((k, n + 4)).astype(np.float32)).to(DEV)
        Y = torch.from_numpy(rs.standard_normal((m, n + 7)).astype(np.float32)).to(DEV)
        C0 = torch.from_numpy(rs.standard_normal((m, n + 8)).astype(np.float32)).to(DEV)
        full = C0[:, 4:n + 4].double() + A[:, 4:k + 4].double() @ Bm[:, :n].double()
        ref = full * (Y[:, 4:n + 4] > 0)
        out = C0.clone()
        cs = torch.full((n,), 0.25, device=DEV)
        ops.sgemm(A[:, 4:k + 4], Bm[:, :n], out=out[:, 4:n + 4], beta=1.0, relu_mask=Y[:, 4:n + 4], colsum=cs)
        scale = float(full.abs().max())
        assert float((out[:, 4:n + 4].double() - ref).abs().max()) <= 3e-5 * scale, (m, k, n)
        np.testing.assert_allclose(cs.cpu().numpy(), 0.25 + ref.sum(0).float().cpu().numpy(), rtol=1e-4, atol=3e-2)
        assert torch.equal(out[:, :4], C0[:, :4]) and torch.equal(out[:, n + 4:], C0[:, n + 4:])
        plain = ops.sgemm(A[:, 4:k + 4], Bm[:, :n])
        assert float((plain.double() - A[:, 4:k + 4].double() @ Bm[:, :n].double()).abs().max()) <= 3e-5 * scale
    # k = 0: an empty product — C = beta C (+ the epilogue), in both forms (the fast kernel pre-loaded operand
    # panels before looking at k)
    c0 = torch.from_numpy(rs.standard_normal((128, 256)).astype(np.float32)).to(DEV)
    c = c0.clone()
    ops.sgemm(torch.zeros((128, 0), device=DEV), torch.zeros((0, 256), device=DEV), out=c, beta=0.5)
    np.testing.assert_allclose(c.cpu().numpy(), 0.5 * c0.cpu().numpy(), rtol=1e-6)
    c = c0.clone()
    ops.sgemm(torch.zeros((0, 128), device=DEV), torch.zeros((0, 256), device=DEV), trans_a=True, out=c, beta=0.5)
    np.testing.assert_allclose(c.cpu().numpy(), 0.5 * c0.cpu().numpy(), rtol=1e-6)
    y = torch.from_numpy(rs.standard_normal((1001,)).astype(np.float32)).to(DEV)
    dy = torch.from_numpy(rs.standard_normal((1001,)).astype(np.float32)).to(DEV)
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert torch.equal(ops.relu_bwd_(dy.clone(), y), ref)


def test_decoder_backward_matches_autograd():
    """nb_decode_points(tap) -> nb_composite -> [nb_composite_bwd -> MLP backward -> nb_trilinear_bwd] against autograd
    through the oracle: gradients of every MLP parameter, of the frame's latent code and of the feature volumes."""
    from neuralbody_amd import ops, training
    from oracle import neuralbody_oracle as orc

    name = "small_dense"
    r, sd, body, batch, cam, _ = scenes.build(name)
    sdt, vols, out_sh = H.oracle_volumes(sd, batch, True)
    # the reference gradients are taken in float64 (same fp32 inputs): fp32 autograd on the CPU is itself only good to
    # ~3e-4 of the largest entry for the bias sums over thousands of samples
    sdt = {k: (v.double() if v.is_floating_point() else v) for k, v in sdt.items()}
    vols64 = [x.double() for x in vols]
    net = H.make_network(sd, DEV, True, "f32")
    bd = H.device_batch(batch, DEV)
    sp = H.sp_input_of(bd, out_sh)
    S = 64
    sel = slice(0, 300, 2)  # 150 rays
    ro, rd = torch.from_numpy(batch["ray_o"][:, sel]), torch.from_numpy(batch["ray_d"][:, sel])
    ne, fa = torch.from_numpy(batch["near"][:, sel]), torch.from_numpy(batch["far"][:, sel])
    wpts, z = orc.get_sampling_points(ro, rd, ne, fa, S)  # fp32 sample points, shared by both sides
    vd = rd / torch.norm(rd, dim=2, keepdim=True)
    w = wpts.reshape(1, -1, 3)
    v = vd[:, :, None].repeat(1, 1, S, 1).reshape(1, -1, 3)
    n_rays = ro.shape[1]
    g_rgb = torch.from_numpy(np.random.RandomState(5).standard_normal((n_rays, 3)).astype(np.float32))

    # ---- reference gradients: autograd through the oracle
    mlp_keys = [k for k in sdt if k.split(".")[0] in ("fc_0", "fc_1", "fc_2", "alpha_fc", "feature_fc", "latent_fc", "view_fc", "rgb_fc")]
    sdg = dict(sdt)
    for k in mlp_keys + ["latent.weight"]:
        sdg[k] = sdt[k].clone().requires_grad_(True)
    vols_g = [x.clone().requires_grad_(True) for x in vols64]
    sp_cpu = {"R": torch.from_numpy(batch["R"]).double(), "Th": torch.from_numpy(batch["Th"]).double(),
              "bounds": torch.from_numpy(batch["bounds"]).double(),
              "latent_index": torch.from_numpy(batch["latent_index"]), "out_sh": out_sh}
    raw_ref = orc.calculate_density_color(sdg, w.double(), v.double(), vols_g, sp_cpu)
    rgb_ref = orc.raw2outputs(raw_ref.reshape(-1, S, 4), z.view(-1, S).double(), rd.reshape(-1, 3).double(), True)[0]
    (rgb_ref * g_rgb.double()).sum().backward()

    # ---- HIP path
    scene = net.make_scene([x.to(DEV) for x in vols], sp)
    lb = net.latent_bias(bd["latent_index"])
    wd, vdd = w[0].to(DEV).contiguous(), v[0].to(DEV).contiguous()
    raw, tap = ops.decode_points(scene, net.packed_weights(), lb, wd, vdd, debug=True, precision="f32")
    zd, rdd = z.view(-1, S).to(DEV).contiguous(), rd.reshape(-1, 3).to(DEV).contiguous()
    rgb = ops.composite(raw.view(-1, S, 4), zd, rdd, True)[0]
    _rel(rgb.cpu().numpy(), rgb_ref.detach().numpy(), 1e-4, "forward rgb")
    d_raw = ops.composite_bwd(raw.view(-1, S, 4), zd, rdd, g_rgb.to(DEV), True)
    grads, dF = training.decoder_backward(net, tap, d_raw.view(-1, 4), bd["latent_index"])
    for k in mlp_keys:
        ref = sdg[k].grad.numpy()
        got = grads[k].cpu().numpy().reshape(ref.shape)
        e = _rel(got, ref, 1e-4, "grad " + k)
    li = int(batch["latent_index"][0])
    _rel(grads["latent.row"].cpu().numpy(), sdg["latent.weight"].grad[li].numpy(), 1e-4, "grad latent row")
    assert float(sdg["latent.weight"].grad.abs().sum() - sdg["latent.weight"].grad[li].abs().sum()) == 0.0
    # ---- trilinear backward: index grids from the volumes' active sets, gradients of the active rows
    grids, drows, acts = [], [], []
    for x in vols:
        act = (x[0].abs().sum(0) > 0)  # [D,H,W]
        idx = torch.cumsum(act.reshape(-1).long(), 0) - 1
        grid = torch.where(act.reshape(-1), idx, torch.full_like(idx, -1)).to(torch.int32).view(act.shape)
        grids.append(grid.to(DEV).contiguous())
        drows.append(torch.zeros((int(act.sum()), x.shape[1]), dtype=torch.float32, device=DEV))
        acts.append(act)
    ops.trilinear_bwd(scene, grids, drows, wd, dF)
    torch.cuda.synchronize()
    for l, (x, act) in enumerate(zip(vols_g, acts)):
        ref = x.grad[0].permute(1, 2, 3, 0)[act].numpy()  # [n_active, C], linear voxel order == row order
        _rel(drows[l].cpu().numpy(), ref, 1e-4, "grad of active voxels, level %d" % l)
        assert np.abs(ref).max() > 0
    # the same sum with the contributions of consecutive points pre-summed per voxel (the training step passes N_samples;
    # any run length, ragged tail included, must give the same gradients)
    for run in (S, 7):
        drows2 = [torch.zeros_like(d) for d in drows]
        ops.trilinear_bwd(scene, grids, drows2, wd, dF, run_length=run)
        for l in range(4):
            _rel(drows2[l].cpu().numpy(), drows[l].cpu().numpy(), 2e-5, "run_length %d, level %d" % (run, l))


def test_encoder_backward_matches_autograd():
    """encoder_backward (BN+ReLU / sparse-conv input & weight gradients / code scatter) alone: random cotangents on the
    active voxels of the four dense volumes, against float64 autograd through the oracle's encoder."""
    from neuralbody_amd import training
    from neuralbody_amd.renderer import Renderer
    from oracle import neuralbody_oracle as orc

    r, sd, body, batch, cam, _ = scenes.build("small")
    net = H.make_network(sd, DEV, True, "f32")
    bd = H.device_batch(batch, DEV)
    sp = Renderer(net).prepare_sp_input(bd)
    ctx = []
    with torch.no_grad():
        vols = net.encode_sparse_voxels(sp, save=ctx)
    # the float64 reference differentiates through the SAME ReLU masks as the fp32 kernels took (activations within
    # rounding of zero otherwise fall on different sides and bound the agreement at ~1e-2)
    sdg = {}
    for k, v in orc.tensor_state_dict(sd).items():
        sdg[k] = v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v
    out_sh = batch["out_sh"].max(0).tolist()
    vols_ref = orc.encode_sparse_voxels(sdg, torch.from_numpy(batch["coord"]), out_sh, training=True, relu_masks=_encoder_masks(ctx))
    rs = np.random.RandomState(21)
    cots = [torch.from_numpy(rs.standard_normal(tuple(v.shape)).astype(np.float32)) for v in vols_ref]
    sum((v * c.double()).sum() for v, c in zip(vols_ref, cots)).backward()
    dense = [rec for rec in ctx[1:] if rec["level"] is not None]
    drows = []
    for rec, c in zip(dense, cots):
        n = int(rec["n_out"])
        lin = rec["out_lin"][:n].long().cpu()
        flat = c[0].permute(1, 2, 3, 0).reshape(-1, c.shape[1])  # [DHW, C]
        d = torch.zeros((rec["n_out_max"], c.shape[1]), dtype=torch.float32)
        d[:n] = flat[lin]
        drows.append(d.to(DEV))
    g, dcodes = training.encoder_backward(net.xyzc_net, ctx, drows)
    torch.cuda.synchronize()
    worst = 0.0
    for name, gr in g.items():
        ref = sdg[name].grad.numpy()
        worst = max(worst, _rel(gr.cpu().numpy().reshape(ref.shape), ref, ENC_TOL, "grad " + name))
    worst = max(worst, _rel(dcodes.cpu().numpy(), sdg["c.weight"].grad.numpy(), ENC_TOL, "grad c.weight"))
    assert len(g) == 17 * 3
    print("encoder backward: worst max|diff|/max|ref| = %.2e over 52 tensors" % worst)


def test_neighbour_table_and_backward_input_follow_the_index_rule():
    """The one device function that states the spconv index rule, from both of its call directions, on a (5, 6, 7) grid with 40
    active voxels (all eight corners among them), stride 1 and 2: the neighbour table that enc_conv_bwd_weight leaves in
    `rulebook` (forward gather) against a loop over (row, offset) of in = stride * out - 1 + k, and enc_conv_bwd_input
    (transposed gather under the mirrored offset) against a float64 scatter over that same table."""
    from neuralbody_amd import ops

    dhw, cin, cout = (5, 6, 7), 16, 32
    rs = np.random.RandomState(3)
    corners = [(z, y, x) for z in (0, dhw[0] - 1) for y in (0, dhw[1] - 1) for x in (0, dhw[2] - 1)]
    rest = [c for c in np.ndindex(*dhw) if c not in corners]
    coord = np.array(corners + [rest[i] for i in rs.choice(len(rest), 32, replace=False)], np.int32)
    n_in = len(coord)
    in_grid, _, in_lin, n_rows = ops.enc_voxelize(torch.from_numpy(coord).to(DEV), dhw)
    assert int(n_rows) == n_in
    weight = torch.from_numpy(rs.standard_normal((3, 3, 3, cin, cout)).astype(np.float32)).to(DEV)
    in_rows = torch.from_numpy(rs.standard_normal((n_in, cin)).astype(np.float32)).to(DEV)
    grid_np = in_grid.cpu().numpy()
    for stride in (1, 2):
        if stride == 1:
            out_grid, out_lin, n_out, n_out_max, out_dhw = in_grid, in_lin, n_rows, n_in, list(dhw)
        else:
            out_grid, out_lin, n_out, n_out_max, out_dhw = ops.enc_downsample_index(in_lin, n_rows, n_in, dhw)
        no = int(n_out)
        dx = torch.from_numpy(rs.standard_normal((n_out_max, cout)).astype(np.float32)).to(DEV)
        rulebook = []
        ops.enc_conv_bwd_weight(in_rows, in_grid, dhw, out_lin, n_out, n_out_max, out_dhw, stride, dx, cin, cout, rulebook=rulebook)
        got = rulebook[0].cpu().numpy().reshape(-1, 27)[:no]
        want = np.full((no, 27), -1, np.int32)
        for r, (z, y, x) in enumerate(zip(*np.unravel_index(out_lin[:no].cpu().numpy(), out_dhw))):
            for o, (kd, kh, kw) in enumerate(np.ndindex(3, 3, 3)):
                i = (stride * z - 1 + kd, stride * y - 1 + kh, stride * x - 1 + kw)
                if all(0 <= v < s for v, s in zip(i, dhw)):
                    want[r, o] = grid_np[i]
        assert (want >= 0).sum() > no, "stride %d: the table has neighbours beyond the centres" % stride
        np.testing.assert_array_equal(got, want, err_msg="neighbour table, stride %d" % stride)
        din = ops.enc_conv_bwd_input(dx, out_grid, out_dhw, in_lin, n_rows, n_in, dhw, stride, weight)
        ref = np.zeros((n_in, cin))
        w64, dx64 = weight.cpu().numpy().astype(np.float64).reshape(27, cin, cout), dx.cpu().numpy().astype(np.float64)
        for r, o in zip(*np.nonzero(want >= 0)):
            ref[want[r, o]] += w64[o] @ dx64[r]
        _rel(din.cpu().numpy(), ref, ENC_TOL, "din, stride %d" % stride)


def test_full_training_step_gradients_match_autograd():
    """Renderer.render under autograd (encoder + decode + composite, forward and backward all HIP) against float64
    autograd through the whole oracle: the gradient of EVERY parameter (MLP, latent codes, 17 sparse conv weights,
    17 BatchNorm affine pairs, the 6890 vertex codes)."""
    training_step_gradients_match_autograd()


def training_step_gradients_match_autograd(voxel_size=None):
    """The check of the test above; `voxel_size` (dhw, None: the fixtures' 5 mm cube) for tests/test_gpu_aniso_voxels.py."""
    from oracle import neuralbody_oracle as orc

    r, sd, body, batch, cam, _ = scenes.build("small_dense", voxel_size)
    vs = (0.005, 0.005, 0.005) if voxel_size is None else tuple(voxel_size)
    n_use = 96
    b_np = dict(batch)
    for k in ("ray_o", "ray_d", "near", "far"):
        b_np[k] = batch[k][:, :n_use]
    g_rgb = torch.from_numpy(np.random.RandomState(9).standard_normal((1, n_use, 3)).astype(np.float32))

    # ---- HIP (first: its ReLU masks are handed to the reference)
    from neuralbody_amd import training

    net = H.make_network(sd, DEV, True, "f32", voxel_size)
    rend = H.make_renderer(net, dict(r, white_bkgd=True))
    bd = H.device_batch(b_np, DEV)
    training.DEBUG_CAPTURE = {}
    try:
        out = rend.render(bd)
        cap = training.DEBUG_CAPTURE
    finally:
        training.DEBUG_CAPTURE = None
    assert out["rgb_map"].requires_grad
    masks = {"encoder": _encoder_masks(cap["enc_ctx"]), "mlp": _mlp_masks(cap["tap"])}

    # ---- reference: float64 autograd through the oracle (same fp32 inputs, same ReLU masks)
    sdg = {}
    for k, v in orc.tensor_state_dict(sd).items():
        sdg[k] = v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v
    out_ref = orc.render(sdg, {k: (torch.from_numpy(v).double() if v.dtype == np.float32 else v) for k, v in b_np.items()},
                         n_samples=64, voxel_size=vs, training=True, white_bkgd=True, relu_masks=masks)
    (out_ref["rgb_map"] * g_rgb.double()).sum().backward()
    _rel(out["rgb_map"].detach().cpu().numpy(), out_ref["rgb_map"].detach().numpy(), 1e-4, "forward rgb")
    (out["rgb_map"] * g_rgb.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    worst = {}
    for name, p in net.named_parameters():
        ref = sdg[name].grad
        assert ref is not None, name
        assert p.grad is not None, "no gradient for " + name
        group = name.split(".")[0] if not name.startswith("xyzc_net") else ".".join(name.split(".")[:2])
        # the encoder gradients pass through 17 fp32 layers of batch-statistics BatchNorm (g - mean(g) - xhat mean(g xhat)
        # cancels heavily): fp32 vs the float64 reference agrees to ~3e-3 of the largest entry, the decoder to ~1e-4
        # (the decoder gradients, checked to 1e-4 on exact volumes in the test above, here inherit the fp32 encoder's
        # ~1e-4 feature noise relative to the float64 reference volumes)
        # End to end the comparison is only as good as the forward agreement: the fixture's x12 density gain turns the
        # fp32 encoder's ~1e-4 feature noise into flipped ReLUs / shifted alphas for a few samples, so this test checks
        # the plumbing of the whole chain at 2e-2; the component tests carry the tight bounds.
        tol = ENC_TOL
        e = _rel(p.grad.cpu().numpy(), ref.numpy().reshape(p.shape), tol, "grad " + name)
        worst[group] = max(worst.get(group, 0.0), e)
    print("worst relative gradient error per group:", {k: "%.1e" % v for k, v in worst.items()})


def test_network_wrapper_training_steps_reduce_loss():
    """The trainer-facing contract (lib/train/trainers/if_nerf_clight.py:18-36 + lib/train/trainers/trainer.py:46-53):
    NetworkWrapper(batch) -> (ret, loss, scalar_stats, image_stats); loss.backward(); clip_grad_value_(40); Adam step.
    A few steps on one synthetic batch must reduce the loss, every parameter must receive a finite gradient, and BN
    running statistics must advance once per forward."""
    import importlib.util
    import os
    import sys
    import types

    from tests import synthetic as syn

    # the plugin imports the reference's `lib.config.cfg`; stand in for it (the GPU box has no reference tree)
    cfgmod = types.ModuleType("lib.config")
    cfgmod.cfg = types.SimpleNamespace(N_samples=64, perturb=1.0, raw_noise_std=0.0, white_bkgd=False, H=512, W=512, ratio=1.0)
    saved = {k: sys.modules.get(k) for k in ("lib", "lib.config")}
    sys.modules["lib"] = types.ModuleType("lib")
    sys.modules["lib.config"] = cfgmod
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("nb_plugin_trainer", os.path.join(root, "neuralbody_amd", "plugins", "if_nerf_clight.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

    sd = syn.make_weights(0, num_train_frame=5)
    body = syn.make_body(seed=0, box=(0.3, 0.5, 0.2))
    K, R, T = syn.make_camera(body, 64, 64, focal_factor=2.5, distance=1.5)
    ro, rd, near, far, mask = syn.host_image_rays(64, 64, K, R, T, body["can_bounds"])
    rs = np.random.RandomState(0)
    pick = rs.choice(ro.shape[0], 1024, replace=False)  # N_rand = 1024 random rays (latent_xyzc_313.yaml:66)
    batch = syn.make_batch(body, ro[pick], rd[pick], near[pick], far[pick], np.ones(1024, bool), latent_index=2)
    batch["rgb"] = rs.uniform(0, 1, (1, 1024, 3)).astype(np.float32)
    bd = H.device_batch(batch, DEV)
    net = H.make_network(sd, DEV, True, "f32")
    wrapper = mod.NetworkWrapper(net)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    losses = []
    for it in range(6):
        ret, loss, stats, image_stats = wrapper(bd)
        assert set(stats) == {"img_loss", "loss"} and ret["rgb_map"].shape == (1, 1024, 3)
        opt.zero_grad()
        loss.mean().backward()
        for name, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        torch.nn.utils.clip_grad_value_(net.parameters(), 40)
        opt.step()
        losses.append(float(loss))
    print("training losses:", ["%.5f" % l for l in losses])
    assert losses[-1] < losses[0], losses
    assert int(net.xyzc_net.conv0[1].num_batches_tracked) == 6


# the fixture's gradients come from the unmodified reference in fp32 on the CPU, whose ReLU masks are its own: a handful of
# activations within rounding of zero fall on the other side here (the mask-consistent float64 tests above agree to 1e-5)
FIXTURE_TOL = 2e-3


def test_training_step_matches_reference_fixture():
    """One training step (forward with the fixture's jitter, MSE loss, backward) against the gradients of the UNMODIFIED
    reference (tests/golden/train_step.npz): loss to 1e-5, per-parameter gradient norms and probe entries to FIXTURE_TOL
    of the tensor's largest gradient entry."""
    g = np.load(H.GOLDEN + "/train_step.npz")
    r, sd, batch, t_rand = scenes.build_train()
    net = H.make_network(sd, DEV, True, "f32")
    rend = H.make_renderer(net, dict(n_samples=r["n_samples"], perturb=True, white_bkgd=False))
    bd = H.device_batch(batch, DEV)
    out = rend.render(bd, t_rand=torch.from_numpy(t_rand).to(DEV))
    mask = bd["mask_at_box"]
    loss = torch.mean((out["rgb_map"][mask] - bd["rgb"][mask]) ** 2)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5, (float(loss.detach()), float(g["loss"]))
    H.assert_close(out["rgb_map"].detach().cpu().numpy(), g["rgb_map"], H.RGB_TOL, "rgb_map", rel=False)
    worst = 0.0
    for name, p in net.named_parameters():
        gr = p.grad.cpu().numpy().astype(np.float64)
        scale = max(float(g["max/" + name]), 1e-30)
        e1 = abs(np.sqrt((gr ** 2).sum()) - float(g["norm/" + name])) / max(float(g["norm/" + name]), 1e-30)
        idx = scenes.grad_probe_indices(gr.shape)
        e2 = np.abs(gr.reshape(-1)[idx] - g["probe/" + name]).max() / scale
        worst = max(worst, e1, e2)
        assert e1 <= FIXTURE_TOL and e2 <= FIXTURE_TOL, (name, e1, e2)
    print("training step vs reference fixture: worst relative deviation %.2e over %d tensors" % (worst, len(list(net.parameters()))))


def test_training_step_with_raw_noise():
    """cfg.raw_noise_std != 0 on the differentiable path (nerf_net_utils.py:31-35: sigma + randn * std in front of the relu; no
    shipped config trains with it): the forward equals the inference path's render with the same noise realisation (itself held
    to the reference's formula by test_raw_noise_std_matches_the_reference_formula), the gradients flow through the NOISY
    densities (checked on alpha_fc.bias, which shifts every density alike, against a central difference of the loss)."""
    r, sd, body, batch, cam, _ = scenes.build("small_dense")
    n_use, S = 128, r["n_samples"]
    b_np = dict(batch)
    for k in ("ray_o", "ray_d", "near", "far"):
        b_np[k] = batch[k][:, :n_use]
    bd = H.device_batch(b_np, DEV)
    gen = torch.Generator().manual_seed(11)
    noise = torch.randn(1, n_use, S, generator=gen).to(DEV)
    target = torch.rand(1, n_use, 3, generator=gen).to(DEV)

    def loss_of(net, grad):
        rend = H.make_renderer(net, dict(r, white_bkgd=False))
        rend.cfg.raw_noise_std = 0.7
        if grad:
            out = rend.render(bd, raw_noise=noise)
        else:
            with torch.no_grad():
                out = rend.render(bd, raw_noise=noise)
        return out, ((out["rgb_map"] - target) ** 2).sum()

    net = H.make_network(sd, DEV, True, "f32")
    out, loss = loss_of(net, True)
    assert out["rgb_map"].requires_grad
    loss.backward()
    g_noisy = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    assert len(g_noisy) >= 60 and all(bool(torch.isfinite(v).all()) for v in g_noisy.values())
    with torch.no_grad():
        inf_out, _ = loss_of(H.make_network(sd, DEV, True, "f32"), False)
    H.assert_close(out["rgb_map"].detach().cpu().numpy(), inf_out["rgb_map"].cpu().numpy(), 2e-5, "noisy forward, training vs inference path")
    # without noise the gradients are others
    net0 = H.make_network(sd, DEV, True, "f32")
    rend0 = H.make_renderer(net0, dict(r, white_bkgd=False))
    ((rend0.render(bd)["rgb_map"] - target) ** 2).sum().backward()
    assert float((net0.alpha_fc.bias.grad - g_noisy["alpha_fc.bias"]).abs().max()) > 1e-3 * float(g_noisy["alpha_fc.bias"].abs().max())
    # central difference on alpha_fc.bias
    h = 2e-2
    vals = []
    for sgn in (+1, -1):
        m = H.make_network(sd, DEV, True, "f32")
        with torch.no_grad():
            m.alpha_fc.bias += sgn * h
            vals.append(float(loss_of(m, False)[1]))
    fd = (vals[0] - vals[1]) / (2 * h)
    an = float(g_noisy["alpha_fc.bias"][0])
    print("d loss / d alpha_fc.bias with raw noise: analytic %.5f, central difference %.5f" % (an, fd))
    assert abs(an - fd) <= 0.05 * max(abs(fd), 1e-3)
