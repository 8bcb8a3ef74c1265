"""float64 restatement of the vanilla-NeRF baseline's TRAINING step on top of tests/nerf_ref.py (numpy only, nothing of the
package): the forward with every activation kept (the columns of nb_nerf_decode_tap's tap), the backward written out layer by
layer (the columns of nb_nerf_bwd_chain's d-tap and the 24 parameter gradients of a module in the reference's shapes), the
stratified jitter of volume_renderer.py:56-70 in fp32, and the whole step of lib/train/trainers/nerf.py:18-37 (both passes, the two
image losses, the gradients of all 48 parameters) at GIVEN fp32 depths.

Like _linear in nerf_ref.py, every product that the exact tests rely on is audited: `audit` receives, per product, the bits an
exact evaluation needs, i.e. log2 of the largest possible partial sum in units of the operands' common quantum.  Below 24 means
fp32 gives the float64 numbers in any summation order."""
import numpy as np

from tests import nerf_ref as ref

TAP_COLS, DTAP_COLS = 2528, 2432
# (first column, width) of each slice: include/nb_hip.h, nb_nerf_decode_tap / nb_nerf_bwd_chain
TAP_H, TAP_FEATURE, TAP_V, TAP_PTS, TAP_VIEW = 0, 2048, 2304, 2432, 2496
PARAM_NAMES = ["%s.%s" % (name, kind) for name, _, _ in ref.LAYERS for kind in ("weight", "bias")]  # named_parameters() order
GRAD_TOL = 1e-4  # max |diff| / max |ref| per tensor: the project's gradient budget (ENC_TOL in tests/test_gpu_backward.py)
EMBED_TOL = 4e-7  # include/nb_hip.h, nb_nerf_decode: the device's sine against sin / cos of the fp32 argument, absolute


def _params(sd, module):
    return {k[len(module) + 1:]: np.asarray(v, np.float64) for k, v in sd.items() if k.startswith(module + ".")}


def _bits(pairs, audit):
    """pairs: [(a [n,K], w [K,m]), ...] whose products are summed into one [n,m] result.  Any partial sum, in any order, is a multiple
    of the common quantum 2^-f bounded by sum |a| |w|; exact in fp32 when bound * 2^f < 2^24."""
    if audit is None:
        return
    f = max(ref._frac_bits(a) + ref._frac_bits(w) for a, w in pairs)
    bound = sum(np.abs(a) @ np.abs(w) for a, w in pairs).max()
    audit.append(float(np.log2(bound + 1e-300)) + f)


def forward_tap(sd, module, pts, viewdirs):
    """Nerf.forward in float64 with everything kept: pts [n,S,3], viewdirs [n,3] (fp32 values) -> dict
    raw [n*S,4], tap [n*S,2528] (the device's columns), z: the ten pre-activations (z0 .. z7, feature, the view layer's)."""
    p = _params(sd, module)
    n, S = pts.shape[:2]
    e_p = ref.embed(pts.reshape(-1, 3), ref.XYZ_RES)
    e_v = ref.embed(np.broadcast_to(np.asarray(viewdirs)[:, None, :], (n, S, 3)).reshape(-1, 3), ref.VIEW_RES)
    lin = lambda name, x: x @ p[name + ".weight"].T + p[name + ".bias"]  # noqa: E731
    tap = np.zeros((n * S, TAP_COLS))
    zs, h = [], e_p
    for i in range(8):
        zs.append(lin("pts_linears.%d" % i, h))
        h = np.maximum(zs[-1], 0.0)
        tap[:, 256 * i:256 * i + 256] = h
        if i == 4:
            h = np.concatenate([e_p, h], -1)  # nerf.py:53: the input first
    alpha = lin("alpha_linear", h)
    feature = lin("feature_linear", h)
    zs.append(feature)
    zs.append(lin("views_linears.0", np.concatenate([feature, e_v], -1)))  # nerf.py:58
    V = np.maximum(zs[-1], 0.0)
    rgb = lin("rgb_linear", V)
    tap[:, TAP_FEATURE:TAP_FEATURE + 256], tap[:, TAP_V:TAP_V + 128] = feature, V
    tap[:, TAP_PTS:TAP_PTS + 63], tap[:, TAP_VIEW:TAP_VIEW + 27] = e_p, e_v
    return {"raw": np.concatenate([rgb, alpha], -1), "tap": tap, "z": zs}


def backward(sd, module, tap, d_raw, audit=None, audit_w=None):
    """The backward of Nerf.forward in float64 from the forward's tap and d_raw [n_pts,4] -> dict
    dtap [n_pts,2432] (dz0 .. dz7 | dfeat | dV: the gradient of every pre-activation, the device's columns),
    pre: the same gradients BEFORE their relu masks (dz7 .. dz0 order is dtap's: pre[i] belongs to z_i; pre[9] to the view layer),
    grads: {PARAM_NAMES entry: gradient in the reference's shape}.
    The relu mask is the stored activation > 0: a pre-activation that is exactly 0 passes nothing (torch.relu's backward).
    audit: bits of the chain's products (see _bits); audit_w: bits of the weight-gradient sums over the samples, dyadic
    columns only (a sine or cosine column of an embedding is no dyadic number and takes no part)."""
    p = _params(sd, module)
    tap, d_raw = np.asarray(tap, np.float64), np.asarray(d_raw, np.float64).reshape(-1, 4)
    h = [tap[:, 256 * i:256 * i + 256] for i in range(8)]
    feature, V = tap[:, TAP_FEATURE:TAP_FEATURE + 256], tap[:, TAP_V:TAP_V + 128]
    e_p, e_v = tap[:, TAP_PTS:TAP_PTS + 63], tap[:, TAP_VIEW:TAP_VIEW + 27]
    d_rgb, d_sig = d_raw[:, :3], d_raw[:, 3:4]
    W = lambda name: p[name + ".weight"]  # noqa: E731
    pre, dz = [None] * 10, [None] * 10
    _bits([(d_rgb, W("rgb_linear"))], audit)
    pre[9] = d_rgb @ W("rgb_linear")
    dz[9] = pre[9] * (V > 0)
    _bits([(dz[9], W("views_linears.0")[:, :256])], audit)
    pre[8] = dz[8] = dz[9] @ W("views_linears.0")[:, :256]  # feature_linear has no activation
    _bits([(dz[8], W("feature_linear")), (d_sig, W("alpha_linear"))], audit)
    pre[7] = dz[8] @ W("feature_linear") + d_sig @ W("alpha_linear")
    dz[7] = pre[7] * (h[7] > 0)
    for L in range(7, 0, -1):
        w = W("pts_linears.%d" % L)
        w = w[:, 63:] if L == 5 else w  # the skip's 63 input columns have no gradient to pass on
        _bits([(dz[L], w)], audit)
        pre[L - 1] = dz[L] @ w
        dz[L - 1] = pre[L - 1] * (h[L - 1] > 0)
    dtap = np.concatenate(dz[:8] + [dz[8], dz[9]], -1)
    assert dtap.shape[1] == DTAP_COLS
    inputs = {"pts_linears.0": e_p, "pts_linears.5": np.concatenate([e_p, h[4]], -1), "views_linears.0": np.concatenate([feature, e_v], -1),
              "feature_linear": h[7], "alpha_linear": h[7], "rgb_linear": V}
    inputs.update({"pts_linears.%d" % i: h[i - 1] for i in (1, 2, 3, 4, 6, 7)})
    outs = {"views_linears.0": dz[9], "feature_linear": dz[8], "alpha_linear": d_sig, "rgb_linear": d_rgb}
    outs.update({"pts_linears.%d" % i: dz[i] for i in range(8)})
    grads = {}
    for name, _, _ in ref.LAYERS:
        x, d = inputs[name], outs[name]
        if audit_w is not None:
            cols = dyadic_columns(name)
            _bits([(d.T, x[:, cols])], audit_w)
            _bits([(d.T, np.ones((d.shape[0], 1)))], audit_w)
        grads[name + ".weight"] = d.T @ x
        grads[name + ".bias"] = d.sum(0)
    return {"dtap": dtap, "pre": pre, "grads": grads}


def dyadic_columns(name):
    """Columns of layer `name`'s input that hold dyadic numbers on the lattice: all but the sines and cosines of an embedding."""
    if name == "pts_linears.0":
        return np.arange(3)
    if name == "pts_linears.5":
        return np.concatenate([np.arange(3), np.arange(63, 319)])
    if name == "views_linears.0":
        return np.arange(259)
    return np.arange(dict((n, i) for n, _, i in ref.LAYERS)[name])


def lattice_d_raw(n_pts, seed=4):
    """d raw for the exact tests: multiples of 1/2 in [-1, 1], zeros among them."""
    return (np.random.RandomState(seed).randint(-2, 3, (n_pts, 4)) * 0.5).astype(np.float32)


def zero_preactivations_under_gradient(fwd, bwd):
    """Number of (sample, unit) pairs whose pre-activation is exactly 0 while a non-zero gradient arrives: the cases that tell
    `> 0` from `>= 0` in the relu's backward."""
    count = 0
    for i in list(range(8)) + [9]:
        count += int(np.sum((fwd["z"][i] == 0.0) & (bwd["pre"][i] != 0.0)))
    return count


# ------------------------------------------------------------------------------------------------ the jitter
def jitter_f32(z_vals, t_rand):
    """volume_renderer.py:56-70, one fp32 rounding per operation: mids = .5 * (z[1:] + z[:-1]); upper = [mids, z[-1]];
    lower = [z[0], mids]; z = lower + (upper - lower) * t_rand. -> [n,S] float32"""
    z, t = np.asarray(z_vals, np.float32), np.asarray(t_rand, np.float32)
    mids = (np.float32(0.5) * (z[:, 1:] + z[:, :-1]).astype(np.float32)).astype(np.float32)
    upper = np.concatenate([mids, z[:, -1:]], -1)
    lower = np.concatenate([z[:, :1], mids], -1)
    return (lower + ((upper - lower).astype(np.float32) * t).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the whole step
def composite_bwd(raw, z, ray_d, g_rgb=None, g_acc=None, g_depth=None, g_disp=None, g_weights=None, white_bkgd=False):
    """d raw [n,S,4] float64 of sum g . out through raw2outputs in float64 (tests/ray_loss_ref.py)."""
    from tests import ray_loss_ref

    return ray_loss_ref.composite_maps_ref(raw, z, ray_d, white_bkgd, g_rgb=g_rgb, g_acc=g_acc, g_depth=g_depth, g_disp=g_disp,
                                           g_weights=g_weights)[0]


def train_step(sd, ray_o, ray_d, z_coarse, z_fine, rgb, mask, viewdirs=None):
    """lib/train/trainers/nerf.py:18-37 in float64 at given fp32 depths (z_coarse [n,S] after the jitter, z_fine [n,S+N] the merged
    depths of the fine pass; both constants of the step, volume_renderer.py:91): img_loss = mean((rgb_map - rgb)[mask]^2) over
    mask_at_box, img_loss0 = mean((rgb0 - rgb)^2) over all rays, loss their sum. -> dict loss, img_loss, img_loss0, rgb_map, rgb0,
    grads {state-dict name: gradient}."""
    rgb, mask = np.asarray(rgb, np.float64), np.asarray(mask).astype(bool)
    v = ref.viewdirs_device(ray_d) if viewdirs is None else viewdirs
    out = {"grads": {}}
    for module, z, key in (("model", z_coarse, "rgb0"), ("model_fine", z_fine, "rgb_map")):
        n, S = z.shape
        fwd = forward_tap(sd, module, ref.points_f32(ray_o, ray_d, z), v)
        raw = fwd["raw"].reshape(n, S, 4)
        rgb_map = ref.raw2outputs(raw, z, ray_d)[0]
        if key == "rgb0":
            diff = rgb_map - rgb
            g = 2.0 * diff / diff.size
        else:
            diff = (rgb_map - rgb)[mask]
            g = np.zeros_like(rgb_map)
            g[mask] = 2.0 * diff / diff.size
        out[key] = rgb_map
        out["img_loss0" if key == "rgb0" else "img_loss"] = float(np.mean(diff ** 2))
        d_raw = composite_bwd(raw, z, ray_d, g_rgb=g)
        for name, grad in backward(sd, module, fwd["tap"], d_raw)["grads"].items():
            out["grads"]["%s.%s" % (module, name)] = grad
    out["loss"] = out["img_loss"] + out["img_loss0"]
    return out


def rel_err(got, want):
    """max |got - want| / max |want| (the gradient budget's measure; 0 / 0 = 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if want.size else 0.0
    e = float(np.abs(got - want).max()) if want.size else 0.0
    return 0.0 if e == 0.0 else e / scale if scale > 0 else np.inf
