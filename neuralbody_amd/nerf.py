"""The vanilla-NeRF baseline of the paper's comparison (configs/nerf/nerf_313.yaml): the reference's
lib/networks/nerf.py as `NerfNetwork` and lib/networks/renderer/volume_renderer.py as `VolumeRenderer`.  The 8 x 256 MLP runs as
one HIP kernel from the positional encoding to raw (nb_nerf_decode), the per-ray work between the two passes is the hierarchical
sampling that exists (nb_composite, nb_importance_sample) plus a depth-only merge (nb_importance_merge_z).  There is no PyTorch
fallback: without the library every call raises.

Inference only unless the network is built with trainable=True.  Then, under gradients, the forward is nb_nerf_decode_tap (f32,
with an activation tap), the backward the existing GEMMs: eleven with relu-mask and column-sum epilogues for the gradients of all
pre-activations and the bias gradients, fourteen for the weight gradients, and the composite's backward nb_composite_bwd_maps.
nb_nerf_bwd_chain, the same chain fused into one exact-fp32 kernel, measured slower and serves tools and tests."""
import torch
import torch.nn as nn

from . import mesh_extract, ops
from ._memo import Memo, tkey

# the one configuration the reference ships (configs/nerf/nerf_313.yaml:59-72) and the kernel is built for
SUPPORTED = {"netdepth": 8, "netwidth": 256, "netdepth_fine": 8, "netwidth_fine": 256, "use_viewdirs": True, "xyz_res": 10,
             "view_res": 4}
PRECISIONS = ("auto", "f32", "f16x3")
# what 'auto' runs.  Decided by measurement, not per call: 'f16x3' (fp16 head + remainder, three products) holds every map of the
# fixture render to the project's budget on the MI355X (DESIGN.md §4.20 has the numbers; tests/test_gpu_nerf.py re-measures it and
# fails if this constant and the measurement disagree), so it is the default; 'f32' is the parity mode.
AUTO_ARITHMETIC = "f16x3"


class Nerf(nn.Module):
    """The parameters of lib/networks/nerf.py:8-43 for D = 8, W = 256, skips = [4], use_viewdirs — names, shapes and creation order
    (so also the default initialisation under a seed) are the reference's."""

    def __init__(self):
        super().__init__()
        self.pts_linears = nn.ModuleList([nn.Linear(63, 256)] + [nn.Linear(319 if i == 4 else 256, 256) for i in range(7)])
        self.views_linears = nn.ModuleList([nn.Linear(283, 128)])
        self.feature_linear = nn.Linear(256, 256)
        self.alpha_linear = nn.Linear(256, 1)
        self.rgb_linear = nn.Linear(128, 3)


# the 24 parameters of one Nerf module in named_parameters() order
PARAM_NAMES = ["%s.%s" % (layer, kind) for layer in ["pts_linears.%d" % i for i in range(8)] +
               ["views_linears.0", "feature_linear", "alpha_linear", "rgb_linear"] for kind in ("weight", "bias")]


def _cut(buf, where):
    return buf[:, where[0]:where[0] + where[1]]


def input_gradients(tap, d_raw, weights):
    """The input-gradient chain of one Nerf module as ops.sgemm launches whose epilogues apply the relu mask of the layer below
    (the forward's own stored activation: > 0 passes) and sum the bias gradient: tap [n_pts, 2528], d_raw [n_pts, 4], weights
    (`NerfNetwork.train_weights`) -> (d-tap [n_pts, 2432] = dz0 .. dz7 | dfeat | dV, nb_nerf_bwd_chain's layout, and its column
    sums [2432]).  Eleven launches.  Exact fp32 below 1024 samples, bf16 head + remainder pairs from there on (include/nb_hip.h,
    nb_sgemm).  This is the product path: at 196 608 samples it takes 2.56 ms with the bias sums against 2.80 ms of
    nb_nerf_bwd_chain without them, which therefore stays an entry point for tools and tests only."""
    T, D = ops.NERF_TAP, ops.NERF_DTAP
    n_pts = tap.shape[0]
    dtap = torch.empty((n_pts, ops.NERF_DTAP_COLS), dtype=torch.float32, device=tap.device)
    sums = torch.zeros(ops.NERF_DTAP_COLS, dtype=torch.float32, device=tap.device)
    col = lambda where: sums[where[0]:where[0] + where[1]]  # noqa: E731
    dV, dfeat = _cut(dtap, D["V"]), _cut(dtap, D["feature"])
    ops.sgemm(d_raw[:, 0:3], weights["rgb"], out=dV, relu_mask=_cut(tap, T["V"]), colsum=col(D["V"]))
    ops.sgemm(dV, weights["views_feature"], out=dfeat, colsum=col(D["feature"]))
    dz = _cut(dtap, D["z"](7))
    ops.sgemm(dfeat, weights["feature"], out=dz)
    ops.sgemm(d_raw[:, 3:4], weights["alpha"], out=dz, beta=1.0, relu_mask=_cut(tap, T["h"](7)), colsum=col(D["z"](7)))
    for L in range(7, 0, -1):
        nxt = _cut(dtap, D["z"](L - 1))
        ops.sgemm(dz, weights["pts"][L], out=nxt, relu_mask=_cut(tap, T["h"](L - 1)), colsum=col(D["z"](L - 1)))
        dz = nxt
    return dtap, sums


def density_input_gradients(tap, weights, dtap=None):
    """input_gradients' sibling for d_raw = (0, 0, 0, 1), the gradient of the density alone: the view branch passes nothing on, so
    its three launches (rgb_linear, views_linears[0], feature_linear) are not made and dz7 is alpha_linear's weight under h7's relu
    mask.  tap [n, 2528], weights (`NerfNetwork.grad_weights`) -> (d-tap [n, 2432] whose dz0 .. dz7 slices are written, dE [n, 64]:
    the gradient by the 63 point-embedding columns and a zero, held in the first 64 columns of the d-tap's otherwise unused
    feature slice).  Ten launches, no bias sums; the kernels and their arithmetic are input_gradients' (exact fp32 below 1024 points,
    bf16 head + remainder pairs from there on), which this function does not touch."""
    T, D = ops.NERF_TAP, ops.NERF_DTAP
    n = tap.shape[0]
    if dtap is None:
        dtap = torch.empty((n, ops.NERF_DTAP_COLS), dtype=torch.float32, device=tap.device)
    dz = _cut(dtap, D["z"](7))
    d_alpha = torch.ones((n, 1), dtype=torch.float32, device=tap.device)
    ops.sgemm(d_alpha, weights["alpha"], out=dz, relu_mask=_cut(tap, T["h"](7)))
    for L in range(7, 0, -1):
        nxt = _cut(dtap, D["z"](L - 1))
        ops.sgemm(dz, weights["pts"][L], out=nxt, relu_mask=_cut(tap, T["h"](L - 1)))
        dz = nxt
    d_emb = dtap[:, D["feature"][0]:D["feature"][0] + 64]
    ops.sgemm(_cut(dtap, D["z"](0)), weights["emb0"], out=d_emb)
    ops.sgemm(_cut(dtap, D["z"](5)), weights["emb5"], out=d_emb, beta=1.0)
    return dtap, d_emb


def param_grads(tap, dtap, d_raw, sums=None):
    """The 24 parameter gradients of one Nerf module, in PARAM_NAMES order and the REFERENCE's shapes, from the forward's tap
    [n_pts, 2528], the d-tap [n_pts, 2432] and d_raw [n_pts, 4]: dW = dz^T x (ops.sgemm, trans_a) over column slices of the
    buffers, db = the d-tap's column sums (`sums` [2432] from input_gradients' epilogues; None: one ops.colsum over the whole
    d-tap) and one ops.colsum of d_raw for the two heads.  The skip layer's columns are [input_pts | h] and the view layer's
    [feature | input_views] (nerf.py:53,58); the taps' zero-pad columns are not part of any slice."""
    def wgrad(dz, *xs):
        if len(xs) == 1:
            return ops.sgemm(dz, xs[0], trans_a=True)
        out, c = torch.empty((dz.shape[1], sum(x.shape[1] for x in xs)), dtype=torch.float32, device=dz.device), 0
        for x in xs:
            ops.sgemm(dz, x, trans_a=True, out=out[:, c:c + x.shape[1]])
            c += x.shape[1]
        return out

    T, D = ops.NERF_TAP, ops.NERF_DTAP
    if sums is None:
        sums = ops.colsum(dtap)
    bias = lambda where: sums[where[0]:where[0] + where[1]]  # noqa: E731
    head = ops.colsum(d_raw)  # [4]: rgb_linear's three, alpha_linear's one
    h = [_cut(tap, T["h"](i)) for i in range(8)]
    pts, view, feature, V = _cut(tap, T["pts"]), _cut(tap, T["view"]), _cut(tap, T["feature"]), _cut(tap, T["V"])
    grads = []
    for i in range(8):
        dz = _cut(dtap, D["z"](i))
        grads += [wgrad(dz, *((pts,) if i == 0 else ((pts, h[4]) if i == 5 else (h[i - 1],)))), bias(D["z"](i))]
    dV, dfeat = _cut(dtap, D["V"]), _cut(dtap, D["feature"])
    grads += [wgrad(dV, feature, view), bias(D["V"]), wgrad(dfeat, h[7]), bias(D["feature"])]
    grads += [wgrad(d_raw[:, 3:4], h[7]), head[3:4], wgrad(d_raw[:, 0:3], V), head[0:3]]
    return grads


class _DecodeTrain(torch.autograd.Function):
    """raw = Nerf module(rays, depths) with a backward: forward nb_nerf_decode_tap, backward input_gradients + param_grads.  The
    rays and the depths get no gradient (z_samples are detached in the reference, rays are data)."""

    @staticmethod
    def forward(ctx, net, model, ray_o, ray_d, z_vals, *params):
        fwd, weights = net.packed_train(model)  # the blob and the backward's weights at the parameter version of this forward
        raw, tap = ops.nerf_decode_tap(fwd, ray_o, ray_d, z_vals)
        ctx.weights = weights
        ctx.save_for_backward(tap)
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        tap, = ctx.saved_tensors
        d_raw = d_raw.contiguous().view(-1, 4)
        if tap.shape[0] == 0:
            return (None,) * 5 + tuple(torch.zeros_like(p) for p in ctx.weights["params"])
        dtap, sums = input_gradients(tap, d_raw, ctx.weights)
        return (None, None, None, None, None) + tuple(param_grads(tap, dtap, d_raw, sums))


class _Composite(torch.autograd.Function):
    """raw2outputs with a backward for all five outputs (nb_composite / nb_composite_bwd_maps); depths and rays are constants."""

    @staticmethod
    def forward(ctx, raw, z_vals, ray_d, white_bkgd):
        ctx.save_for_backward(raw, z_vals, ray_d)
        ctx.white_bkgd = white_bkgd
        return ops.composite(raw, z_vals, ray_d, white_bkgd)

    @staticmethod
    def backward(ctx, d_rgb, d_disp, d_acc, d_weights, d_depth):
        raw, z_vals, ray_d = ctx.saved_tensors
        c = lambda t: None if t is None else t.contiguous()  # noqa: E731
        return ops.composite_bwd_maps(raw, z_vals, ray_d, ctx.white_bkgd, d_rgb_map=c(d_rgb), d_acc_map=c(d_acc),
                                      d_depth_map=c(d_depth), d_disp_map=c(d_disp), d_weights=c(d_weights)), None, None, None


class NerfNetwork(nn.Module):
    """lib/networks/nerf.py:111-158.  state_dict(): the reference's 48 entries (model.* and model_fine.*), so its checkpoints load
    with load_state_dict.  precision: 'f32' (exact fp32 fma chains on the fp32 MFMA, the parity mode), 'f16x3' (fp16 MFMA, operands
    split into head and remainder, fp32 accumulation; activations must stay inside fp16's range, 65504) or 'auto' =
    AUTO_ARITHMETIC.  trainable: False keeps the network inference only (training mode and gradients are refused); True lets
    train() / eval() switch modes and, under torch.enable_grad(), runs decode / forward through an autograd function whose forward
    is always 'f32' (precision governs inference only) and whose backward returns the 24 gradients of the module called."""

    def __init__(self, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10, view_res=4,
                 precision="auto", trainable=False):
        super().__init__()
        given = {"netdepth": int(netdepth), "netwidth": int(netwidth), "netdepth_fine": int(netdepth_fine),
                 "netwidth_fine": int(netwidth_fine), "use_viewdirs": bool(use_viewdirs), "xyz_res": int(xyz_res),
                 "view_res": int(view_res)}
        for key, want in SUPPORTED.items():
            if given[key] != want:
                raise NotImplementedError("%s = %r: the fused NeRF kernel is built for %s = %r only, the configuration the reference "
                                          "ships (configs/nerf/nerf_313.yaml)" % (key, given[key], key, want))
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
        self.precision = precision
        self.trainable = bool(trainable)
        self.model = Nerf()
        self.model_fine = Nerf()
        # slot 'packed' / 'packed_fine': the MFMA-ordered blob of a module, rebuilt when a parameter changes; 'train' / 'train_fine':
        # the f32 blob and the backward's weights of the training step, likewise (an optimizer step bumps every version counter)
        self._memo = Memo()

    def nerf_precision(self):
        """The arithmetic nb_nerf_decode runs: 'auto' is AUTO_ARITHMETIC."""
        return AUTO_ARITHMETIC if self.precision == "auto" else self.precision

    def _module(self, model):
        return self.model_fine if model == "fine" else self.model

    def _inference_only(self, what):
        if self.trainable:
            return
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("%s is inference only: the fused MLP has no backward.  Call .eval() (run.py:57,89 put the "
                                      "network into train() mode; plugins/nerf.py keeps its Network in eval mode for that reason) "
                                      "and wrap the call in torch.no_grad(), as run.py:66,98 does" % what)

    def packed(self, model=""):
        """The packed blob of `model` ('' coarse, 'fine'), cached per module and parameter version."""
        mod, prec = self._module(model), self.nerf_precision()
        params = {k: v.detach() for k, v in mod.named_parameters()}
        key = (prec, tkey(*mod.parameters()))
        return self._memo.get("packed_fine" if model == "fine" else "packed", key, lambda: ops.nerf_pack(params, prec))

    def packed_train(self, model=""):
        """(f32 blob, train_weights) of `model` for the training step, cached per module and parameter version."""
        mod = self._module(model)
        params = {k: v.detach() for k, v in mod.named_parameters()}
        return self._memo.get("train_fine" if model == "fine" else "train", (tkey(*mod.parameters()),),
                              lambda: (ops.nerf_pack(params, "f32"), self.train_weights(model)))

    def train_weights(self, model=""):
        """What input_gradients multiplies by: COPIES of the module's weights (the backward runs the forward's version even after an
        in-place update), the two that are column slices of a wider matrix as contiguous matrices: rows of the [256, 319] and
        [128, 283] weights are not 16-byte aligned, which the fast GEMM kernels need (training.py:decoder_backward copies likewise)."""
        mod = self._module(model)
        w = lambda lin: lin.weight.detach().clone()  # noqa: E731
        pts = [w(lin) for lin in mod.pts_linears]
        pts[5] = pts[5][:, 63:].contiguous()  # the skip's 63 input columns have no gradient to pass on
        return {"pts": pts, "views_feature": mod.views_linears[0].weight.detach()[:, :256].contiguous(), "feature": w(mod.feature_linear),
                "alpha": w(mod.alpha_linear), "rgb": w(mod.rgb_linear), "params": [p.detach() for p in mod.parameters()]}

    def grad_weights(self, model=""):
        """What density_input_gradients multiplies by, cached per module and parameter version: pts_linears[1..7] (of the skip layer
        its 256 h columns), alpha_linear, and the two matrices that carry a gradient to the embedding, pts_linears[0] [256,63] and
        the skip's first 63 columns, each as a contiguous zero-padded [256,64] matrix (rows of 63 floats are not 16-byte aligned)."""
        mod = self._module(model)

        def build():
            w = [lin.weight.detach() for lin in mod.pts_linears]
            pad = lambda m: torch.nn.functional.pad(m, (0, 1)).contiguous()  # noqa: E731
            pts = [None] + [w[i] if i != 5 else w[5][:, 63:].contiguous() for i in range(1, 8)]
            return {"pts": pts, "alpha": mod.alpha_linear.weight.detach(), "emb0": pad(w[0]), "emb5": pad(w[5][:, :63])}

        return self._memo.get("grad_fine" if model == "fine" else "grad", (tkey(*mod.parameters()),), build)

    def density(self, pts, model=""):
        """lib/networks/nerf_mesh.py:45-54,125-138: alpha [n] at the points pts [n,3], the raw output of alpha_linear (no relu), by
        nb_nerf_density: the trunk alone, the bits of forward(...)[..., 3] at the same points.  Inference only, like `decode`."""
        self._inference_only("NerfNetwork.density")
        if pts.dim() != 2 or pts.shape[-1] != 3:
            raise ValueError("pts must be [n,3], got %s" % (tuple(pts.shape),))
        return ops.nerf_density(self.packed(model), pts.float().contiguous(), self.nerf_precision())

    # density_gradient: tap plus d-tap of one chunk stay below this many bytes (a bound on memory, not a tuning knob)
    GRADIENT_CHUNK_BYTES = 1 << 30

    def density_gradient(self, pts, model=""):
        """(alpha [n], d alpha / d p [n,3]) at the points pts [n,3], without autograd and on an inference-only network: the forward
        is nb_nerf_decode_tap (always f32, the points as rays of depth 0 like `forward`), the chain density_input_gradients, the last
        step nb_nerf_embed_grad on the tap's own embedding columns.  alpha has the bits of density() in 'f32'.  In chunks of
        GRADIENT_CHUNK_BYTES // (tap + d-tap bytes per point) = 54 120 points."""
        self._inference_only("NerfNetwork.density_gradient")
        if pts.dim() != 2 or pts.shape[-1] != 3:
            raise ValueError("pts must be [n,3], got %s" % (tuple(pts.shape),))
        pts = pts.float().contiguous()
        n, dev = pts.shape[0], pts.device
        alpha = torch.empty((n,), dtype=torch.float32, device=dev)
        grad = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n == 0:
            return alpha, grad
        mod = self._module(model)
        params = {k: v.detach() for k, v in mod.named_parameters()}
        packed = self.packed(model) if self.nerf_precision() == "f32" else \
            self._memo.get("grad_packed_fine" if model == "fine" else "grad_packed", (tkey(*mod.parameters()),),
                           lambda: ops.nerf_pack(params, "f32"))
        weights = self.grad_weights(model)
        chunk = max(1, self.GRADIENT_CHUNK_BYTES // (4 * (ops.NERF_TAP_COLS + ops.NERF_DTAP_COLS)))
        m = min(n, chunk)
        tap = torch.empty((m, ops.NERF_TAP_COLS), dtype=torch.float32, device=dev)
        dtap = torch.empty((m, ops.NERF_DTAP_COLS), dtype=torch.float32, device=dev)
        raw = torch.empty((m, 1, 4), dtype=torch.float32, device=dev)
        zero = torch.zeros((m, 1), dtype=torch.float32, device=dev)
        first = ops.NERF_TAP["pts"][0]
        for i in range(0, n, chunk):
            k = min(chunk, n - i)
            o = pts[i:i + k]
            # the direction is not read by the trunk; any non-zero one keeps d / |d| finite
            d = torch.zeros_like(o)
            d[:, 2] = 1.0
            ops.nerf_decode_tap(packed, o, d, zero[:k], out=raw[:k], tap=tap[:k])
            alpha[i:i + k] = raw[:k, 0, 3]
            _, d_emb = density_input_gradients(tap[:k], weights, dtap[:k])
            ops.nerf_embed_grad(tap[:k, first:first + 64], d_emb, out=grad[i:i + k])
        return alpha, grad

    def _wants_grad(self, model):
        return self.trainable and torch.is_grad_enabled() and any(p.requires_grad for p in self._module(model).parameters())

    def _decode(self, ray_o, ray_d, z_vals, model):
        if self._wants_grad(model):
            return _DecodeTrain.apply(self, model, ray_o.detach(), ray_d.detach(), z_vals.detach(), *self._module(model).parameters())
        return ops.nerf_decode(self.packed(model), ray_o, ray_d, z_vals, self.nerf_precision())

    def decode(self, ray_o, ray_d, z_vals, model=""):
        """raw [n,S,4] at the depths z_vals [n,S] of the rays ray_o / ray_d [n,3]: the point is o + d z, the direction d / |d|."""
        self._inference_only("NerfNetwork.decode")
        return self._decode(ray_o, ray_d, z_vals, model)

    def forward(self, pts, viewdirs, model=""):
        """nerf.py:140-158: pts [n,S,3], viewdirs [n,3] -> raw [n,S,4] on the device.  The points go to the kernel as rays of depth 0
        (o + d * 0 = o exactly); it renormalises the direction, which moves a unit vector by at most an ulp."""
        self._inference_only("NerfNetwork.forward")
        if pts.dim() != 3 or pts.shape[-1] != 3 or tuple(viewdirs.shape) != (pts.shape[0], 3):
            raise ValueError("pts must be [n,S,3] and viewdirs [n,3], got %s and %s" % (tuple(pts.shape), tuple(viewdirs.shape)))
        n, S = pts.shape[:2]
        o = pts.reshape(-1, 3).float().contiguous()
        d = viewdirs[:, None].expand(n, S, 3).reshape(-1, 3).float().contiguous()
        z = torch.zeros((n * S, 1), dtype=torch.float32, device=pts.device)
        return self._decode(o, d, z, model).view(n, S, 4)


class VolumeRendererConfig:
    """What VolumeRenderer reads of a config: the keys of configs/nerf/nerf_313.yaml with its values."""

    def __init__(self, N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=0.0, white_bkgd=False, lindisp=False,
                 chunk=32768):
        self.N_samples, self.N_importance, self.perturb = int(N_samples), int(N_importance), float(perturb)
        self.raw_noise_std, self.white_bkgd, self.lindisp, self.chunk = float(raw_noise_std), bool(white_bkgd), bool(lindisp), int(chunk)


class VolumeRenderer:
    """lib/networks/renderer/volume_renderer.py:6-156 over a NerfNetwork, in chunks of cfg.chunk rays.  Per chunk: the coarse depths
    (Renderer.get_sampling_points' arithmetic: near * (1 - t) + far * t), nb_nerf_decode with the coarse module, nb_composite,
    nb_importance_sample on its weights, nb_importance_merge_z, nb_nerf_decode of ALL merged depths with the fine module
    (volume_renderer.py:93-101), nb_composite.

    Training (a NerfNetwork(trainable=True) under torch.enable_grad()): rgb_map, rgb0, acc_map, acc0, depth_map, disp_map, disp0
    and (render_rays) weights carry gradients to the parameters, the composite's backward being nb_composite_bwd_maps; the depths
    are constants (z_samples are detached, volume_renderer.py:91), so the coarse module learns from the coarse maps alone.  The
    stratified jitter of volume_renderer.py:56-70 runs when perturb > 0 and the network is in training mode.  Memory: every
    sample of a pass keeps TAP_BYTES of tap until the backward, which adds DTAP_BYTES of d-tap, so under gradients a chunk holds
    at most GRAD_CHUNK_BYTES // ((N_samples + N_importance) * (TAP_BYTES + DTAP_BYTES)) rays (at least 1), whatever cfg.chunk
    says: tap and d-tap of one pass stay below 8 GiB.  1024 rays of 64 + 128 samples are 3.9 GB and one chunk (the limit is 2255
    rays); the default chunk of 32768 rays would be 126 GB.  The cap bounds one pass of one chunk only, NOT the step: autograd
    keeps the tap of every chunk, coarse and fine, until loss.backward() has run, so a render under gradients holds
    total rays x (2 N_samples + N_importance) x TAP_BYTES whatever the chunking (2.65 GB at 1024 rays of 64 + 128).  A large
    N_rand needs that much memory, or a backward per chunk by the caller."""

    TAP_BYTES, DTAP_BYTES, GRAD_CHUNK_BYTES = 4 * ops.NERF_TAP_COLS, 4 * ops.NERF_DTAP_COLS, 8 << 30

    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg if cfg is not None else VolumeRendererConfig()
        self._memo = Memo(t_vals=4, u_det=4)

    def _t_vals(self, S, dev):
        return self._memo.get("t_vals", (S, str(dev)), lambda: torch.linspace(0.0, 1.0, steps=S).to(dev))

    def _composite(self, raw, z_vals, ray_d, raw_noise):
        """raw2outputs (nerf_net_utils.py:6-51): the noise of raw_noise_std goes onto a copy's densities, as Renderer._add_raw_noise."""
        std = float(self.cfg.raw_noise_std)
        if std != 0.0:
            noise = torch.randn(raw.shape[:2], device=raw.device) if raw_noise is None else raw_noise.reshape(raw.shape[:2]).to(raw)
            raw = raw.clone()
            raw[..., 3] += noise * std
        if raw.requires_grad:
            return _Composite.apply(raw, z_vals, ray_d, bool(self.cfg.white_bkgd))
        return ops.composite(raw, z_vals, ray_d, bool(self.cfg.white_bkgd))

    def _jitters(self):
        """volume_renderer.py:56: the stratified jitter belongs to a network in training mode (only a trainable one gets there)."""
        return float(self.cfg.perturb) > 0.0 and bool(getattr(self.net, "trainable", False)) and self.net.training

    def grad_chunk(self):
        """Rays per chunk under gradients (the class docstring's rule)."""
        T = int(self.cfg.N_samples) + max(0, int(self.cfg.N_importance))
        return max(1, self.GRAD_CHUNK_BYTES // (T * (self.TAP_BYTES + self.DTAP_BYTES)))

    def render_rays(self, ray_o, ray_d, near, far, u=None, raw_noise=None, t_rand=None):
        """One chunk: ray_o / ray_d [n,3], near / far [n] -> the reference's dict with flat shapes (rgb_map [n,3], disp_map, acc_map,
        depth_map [n], raw [n,S+N,4]; with N_importance > 0 also rgb0, disp0, acc0, z_std [n]) plus z_vals [n,S+N].
        u: [N] or [n,N] numbers in [0,1) used instead of linspace (perturb == 0) or torch.rand (otherwise).
        raw_noise: (coarse [n,S], fine [n,S+N]) standard-normal tensors used instead of torch.randn when raw_noise_std != 0.
        t_rand: [n,S] numbers in [0,1) used instead of torch.rand by the stratified jitter, when that runs (_jitters).  Under
        gradients the dict also has weights [n,S+N] (the last pass's), differentiable like the maps."""
        cfg = self.cfg
        if bool(cfg.lindisp):
            raise NotImplementedError("lindisp = True: the coarse depths are formed linearly in depth only (volume_renderer.py:50); "
                                      "configs/nerf/nerf_313.yaml has lindisp: False")
        S, N = int(cfg.N_samples), int(cfg.N_importance)
        if N < 0:
            raise ValueError("N_importance must be >= 0, got %d" % N)
        dev = ray_o.device
        ray_o, ray_d = ray_o.float().contiguous(), ray_d.float().contiguous()
        near, far = near.float().contiguous(), far.float().contiguous()
        t_vals = self._t_vals(S, dev)
        # volume_renderer.py:48-54
        z_coarse = (near[:, None] * (1.0 - t_vals) + far[:, None] * t_vals).contiguous()
        jitter = self._jitters()
        if jitter:  # volume_renderer.py:56-70, the same fp32 operations in the same order
            mids = 0.5 * (z_coarse[..., 1:] + z_coarse[..., :-1])
            upper = torch.cat([mids, z_coarse[..., -1:]], -1)
            lower = torch.cat([z_coarse[..., :1], mids], -1)
            t_rand = torch.rand(z_coarse.shape, device=dev) if t_rand is None else t_rand.reshape(z_coarse.shape).to(upper)
            t_rand = t_rand.contiguous()
            z_coarse = (lower + (upper - lower) * t_rand).contiguous()
        raw = self.net.decode(ray_o, ray_d, z_coarse)
        rgb, disp, acc, weights, depth = self._composite(raw, z_coarse, ray_d, None if raw_noise is None else raw_noise[0])
        ret = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "depth_map": depth, "raw": raw, "z_vals": z_coarse}
        grad = weights.requires_grad
        if N == 0:
            if grad:
                ret["weights"] = weights
            return ret
        weights = weights.detach()  # volume_renderer.py:91: z_samples carry no gradient
        if u is None:
            if float(cfg.perturb) == 0.0:  # the reference's det (volume_renderer.py:90)
                u = self._memo.get("u_det", (N, str(dev)), lambda: torch.linspace(0.0, 1.0, steps=N).to(dev))
            else:
                u = torch.rand((ray_o.shape[0], N), device=dev)
        # nb_importance_sample forms the coarse depths itself, by the same statements (nb_march_common.h: z_sample): the jitter's
        # t_rand goes along so that its bins are the midpoints of the depths the coarse pass decoded
        smp = ops.importance_sample(ray_o, ray_d, near, far, t_vals, t_rand if jitter else None, weights, u.float().contiguous(),
                                    want_z_coarse=False)
        z_vals = ops.importance_merge_z(z_coarse, smp["z_fine"])
        raw = self.net.decode(ray_o, ray_d, z_vals, model="fine")
        rgb, disp, acc, weights, depth = self._composite(raw, z_vals, ray_d, None if raw_noise is None else raw_noise[1])
        out = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "depth_map": depth, "raw": raw, "rgb0": ret["rgb_map"],
               "disp0": ret["disp_map"], "acc0": ret["acc_map"], "z_std": smp["z_std"], "z_vals": z_vals}
        if grad:
            out["weights"] = weights
        return out

    def render(self, batch, t_rand=None, feature_volume=None, u=None, raw_noise=None):
        """volume_renderer.py:141-156: batch ray_o / ray_d [B,n,3], near / far [B,n] -> rgb_map [B,n,3], disp_map / acc_map [B,n,1],
        depth_map [B,n], raw [B,n,(S+N)*4] and, with N_importance > 0, rgb0 [B,n,3], disp0 / acc0 / z_std [B,n,1]; z_vals [B,n,S+N] is
        an addition.  u [B,n,N] (or [N]) and raw_noise ([B,n,S], [B,n,S+N]) replace the random numbers, for tests.  t_rand and
        feature_volume are what NovelViewRenderer hands every renderer: there is no jitter in inference and no encoder here.  With a
        trainable network t_rand [B,n,S] replaces torch.rand in the stratified jitter (when that runs: perturb > 0 and training
        mode); under gradients weights [B,n,S+N] is added and the chunk is capped (the class docstring's rule)."""
        trainable = bool(getattr(self.net, "trainable", False))
        if t_rand is not None and not trainable:
            raise NotImplementedError("t_rand: the stratified jitter belongs to training (volume_renderer.py:56), which needs a "
                                      "NerfNetwork(trainable=True)")
        ray_o, ray_d = batch["ray_o"], batch["ray_d"]
        B, n = ray_o.shape[:2]
        o, d = ray_o.reshape(-1, 3), ray_d.reshape(-1, 3)
        near, far = batch["near"].reshape(-1), batch["far"].reshape(-1)
        total, chunk = B * n, max(1, int(self.cfg.chunk))
        if trainable and torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters()):
            chunk = min(chunk, self.grad_chunk())
        if t_rand is not None:
            t_rand = t_rand.reshape(total, -1)
        if u is not None and u.dim() > 1:
            u = u.reshape(total, -1)
        if raw_noise is not None:
            raw_noise = tuple(r.reshape(total, -1) for r in raw_noise)
        parts = {}
        for i in (range(0, total, chunk) if total else (0,)):
            sl = slice(i, i + chunk)
            out = self.render_rays(o[sl], d[sl], near[sl], far[sl], u=u if u is None or u.dim() == 1 else u[sl],
                                   raw_noise=None if raw_noise is None else tuple(r[sl] for r in raw_noise),
                                   t_rand=None if t_rand is None else t_rand[sl])
            for k, v in out.items():
                parts.setdefault(k, []).append(v)
        ret = {}
        for k, v in parts.items():
            v = v[0] if len(v) == 1 else torch.cat(v, 0)
            ret[k] = v.reshape(B, n) if k == "depth_map" else v.reshape(B, n, v[0].numel() if total else _width(k, self.cfg))
        return ret


def _width(key, cfg):
    """Last dimension of an output of VolumeRenderer.render (needed only for an empty batch, where no row shows it)."""
    T = int(cfg.N_samples) + int(cfg.N_importance)
    return {"rgb_map": 3, "rgb0": 3, "raw": 4 * T, "z_vals": T, "weights": T}.get(key, 1)


class NerfMeshConfig:
    """What NerfMeshRenderer reads of a config: mesh_th and N_importance of configs/nerf/nerf_313.yaml, and the keys RendererMesh
    has for its options (not reference keys, off unless set)."""

    def __init__(self, mesh_th=5.0, N_importance=128, mesh_backend="auto", mesh_components="all", mesh_color=False,
                 mesh_normals="faces"):
        self.mesh_th, self.N_importance, self.mesh_backend = float(mesh_th), int(N_importance), str(mesh_backend)
        self.mesh_components, self.mesh_color, self.mesh_normals = mesh_components, bool(mesh_color), str(mesh_normals)


class NerfMeshRenderer:
    """lib/networks/renderer/volume_mesh_renderer.py:84-107 over a NerfNetwork: the density of the baseline on the lattice of the
    mesh dataset and the mesh of its iso-surface cube == cfg.mesh_th.  The cube holds the raw output of alpha_linear (the reference
    does not relu it) at the lattice points flagged `inside` and 0 elsewhere, padded by 10.  The module asked is the fine one when
    cfg.N_importance > 0 and the coarse one otherwise (volume_mesh_renderer.py:50-55).  The density is ONE nb_nerf_density launch,
    the trunk of the MLP alone (the reference chunks cfg.chunk points per call); the lattice forms and everything behind the cube
    are RendererMesh's (mesh_extract), so cfg.mesh_components, cfg.mesh_color, cfg.mesh_normals: field and the visualizer's
    mesh_render work as they do there.  Colours: one NerfNetwork.forward at the vertices looking along -normal; field normals:
    NerfNetwork.density_gradient."""

    PAD = mesh_extract.PAD

    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg if cfg is not None else NerfMeshConfig()

    def model(self):
        """'fine' with cfg.N_importance > 0, '' otherwise."""
        return "fine" if int(self.cfg.N_importance) > 0 else ""

    def _field(self):
        model = self.model()

        def raw(wpts, viewdir):  # [1,V,3] each: every vertex its own direction, so V "rays" of one sample
            return self.net.forward(wpts[0][:, None].contiguous(), viewdir[0].contiguous(), model=model)

        return mesh_extract.FieldQueries(density=lambda wpts: self.net.density(wpts, model=model), raw=raw,
                                         gradient=lambda wpts: self.net.density_gradient(wpts, model=model)[1])

    def density_cube(self, batch, pad=PAD):
        """-> DEVICE float32 [X+2*pad, Y+2*pad, Z+2*pad] (mesh_extract.lattice_cube: the reference dataset's `pts` + `inside`, or
        `axis_x / axis_y / axis_z` + the device-carved `inside` of plugins/light_stage_mesh_dataset.py)."""
        return mesh_extract.lattice_cube(batch, pad, self._field().density)

    def extract_mesh(self, batch, world=False, cube=None, components="all", colors=False, normals="faces"):
        """RendererMesh.extract_mesh's semantics (mesh_extract.mesh_from_cube): DEVICE (vertices, triangles), or a ColoredMesh."""
        if cube is None:
            cube = self.density_cube(batch)
        return mesh_extract.mesh_from_cube(batch, cube, self.cfg.mesh_th, self._field(), world=world, components=components,
                                           colors=colors, normals=normals, pad=self.PAD)

    def render(self, batch):
        """volume_mesh_renderer.py:84-107 -> {"cube", "mesh"}, as RendererMesh.render (mesh_extract.render_mesh)."""
        return mesh_extract.render_mesh(self.cfg, batch, lambda: (self.density_cube(batch), self._field()))
