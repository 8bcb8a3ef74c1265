"""Float64 models of the training-loss kernels (include/nb_hip.h: nb_ray_distortion, nb_composite_bwd_maps).

distortion_ref      L and G by the direct O(S^2) double sums of the header's formulas
composite_maps_ref  float64 autograd through oracle.neuralbody_oracle.raw2outputs of sum g . out over the given cotangents, with the
                    header's rule for the disparity: rays whose q = depth / acc is not greater than 1e-10 drop their d_disp term
"""
import numpy as np
import torch


def intervals(z):
    """(m, delta) [n,S] float64 of depths z [n,S]; (None, None) rows are not special-cased here: span <= 0 rows come back as zeros
    with ok == False."""
    z = np.asarray(z, np.float64)
    n, S = z.shape
    span = z[:, -1] - z[:, 0]
    ok = span > 0
    safe = np.where(ok, span, 1.0)
    s = (z - z[:, :1]) / safe[:, None]
    m = s.copy()
    delta = np.zeros_like(s)
    if S > 1:
        m[:, :-1] = (s[:, :-1] + s[:, 1:]) / 2
        delta[:, :-1] = s[:, 1:] - s[:, :-1]
    m[~ok] = 0.0
    delta[~ok] = 0.0
    return m, delta, ok


def distortion_ref_many(ws, z, chunk=32):
    """distortion_ref of several weight arrays on the SAME depths: the [S,S] table |m_k - m_j| of a chunk of rays is formed once
    and every weight array summed against it (a direct double sum all the same) -> [(L, G), ...]."""
    ws = [np.asarray(w, np.float64) for w in ws]
    m, delta, ok = intervals(z)
    n, S = m.shape
    As = [np.empty((n, S)) for _ in ws]
    for b in range(0, n, chunk):
        D = np.abs(m[b:b + chunk, :, None] - m[b:b + chunk, None, :])  # [c,S,S]
        for w, A in zip(ws, As):
            A[b:b + chunk] = np.einsum("nkj,nj->nk", D, w[b:b + chunk])  # A_k = sum_j w_j |m_k - m_j|
    out = []
    for w, A in zip(ws, As):
        L = (w * A).sum(-1) + (w * w * delta).sum(-1) / 3
        G = 2 * A + 2 * w * delta / 3
        L[~ok] = 0.0
        G[~ok] = 0.0
        out.append((L, G))
    return out


def distortion_ref(w, z):
    """-> (L [n], G [n,S]) float64: L = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i, G = dL/dw; zeros where span <= 0."""
    return distortion_ref_many([w], z)[0]


def distortion_loss_torch(w, z):
    """The same L as a float64 torch expression of w (for autograd checks of G); z constant."""
    m, delta, ok = intervals(z)
    m, delta = torch.from_numpy(m), torch.from_numpy(delta)
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((-1, -2))
    L = pair + (w * w * delta).sum(-1) / 3
    return L * torch.from_numpy(ok.astype(np.float64))


def composite_maps_ref(raw, z, ray_d, white_bkgd, g_rgb=None, g_acc=None, g_depth=None, g_disp=None, g_weights=None):
    """d raw [n,S,4] float64 (numpy) of sum g . out through the oracle's raw2outputs in float64, every input converted exactly.
    Also returns the float64 acc [n] (the tests draw their disparity cases by it)."""
    from oracle import neuralbody_oracle as orc

    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    raw_t = t(raw).clone().requires_grad_(True)
    raw_in, z_in = raw_t, t(z)
    if raw_in.shape[1] == 1:
        # one sample: raw2outputs, like the reference's own, shapes its 1e10 column after an empty slice and every map becomes an empty
        # sum; the kernels give a lone sample the dist 1e10 |d| of any ray's last sample.  As tests/test_gpu_backward_kernels.py does,
        # the reference is the same function on two samples, the second one without density at z + 1e10
        nothing = torch.tensor([0.0, 0.0, 0.0, -1.0], dtype=torch.float64).expand(raw_in.shape[0], 1, 4)
        raw_in, z_in = torch.cat([raw_t, nothing], 1), torch.cat([z_in, z_in + 1e10], 1)
        if g_weights is not None:
            g_weights = np.concatenate([np.asarray(g_weights, np.float64), np.zeros((raw_in.shape[0], 1))], 1)
    rgb, disp, acc, w, depth = orc.raw2outputs(raw_in, z_in, t(ray_d), white_bkgd)
    total = raw_t.sum() * 0.0
    for out, g in ((rgb, g_rgb), (acc, g_acc), (depth, g_depth), (w, g_weights)):
        if g is not None:
            total = total + (out * t(g)).sum()
    if g_disp is not None:
        with torch.no_grad():
            q = depth / acc
            keep = q > 1e-10  # False for a smaller value, a tie and NaN
        if bool(keep.any()):
            # the dropped rays are taken out BEFORE the forward: indexing disp instead would send 0 / 0 = NaN down their depth / acc
            disp_kept = orc.raw2outputs(raw_in[keep], z_in[keep], t(ray_d)[keep], white_bkgd)[1]
            total = total + (disp_kept * t(g_disp)[keep]).sum()
    total.backward()
    return raw_t.grad.numpy(), acc.detach().numpy()
