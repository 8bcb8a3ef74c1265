"""The vanilla-NeRF baseline of the paper's comparison (configs/nerf/nerf_313.yaml), inference only: the reference's
lib/networks/nerf.py as `NerfNetwork` and lib/networks/renderer/volume_renderer.py as `VolumeRenderer`.  The 8 x 256 MLP runs as
one HIP kernel from the positional encoding to raw (nb_nerf_decode), the per-ray work between the two passes is the hierarchical
sampling that exists (nb_composite, nb_importance_sample) plus a depth-only merge (nb_importance_merge_z).  There is no PyTorch
fallback: without the library every call raises."""
import torch
import torch.nn as nn

from . import ops
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


class NerfNetwork(nn.Module):
    """lib/networks/nerf.py:111-158.  state_dict(): the reference's 48 entries (model.* and model_fine.*), so its checkpoints load
    with load_state_dict.  precision: 'f32' (exact fp32 fma chains on the fp32 MFMA, the parity mode), 'f16x3' (fp16 MFMA, operands
    split into head and remainder, fp32 accumulation; activations must stay inside fp16's range, 65504) or 'auto' =
    AUTO_ARITHMETIC."""

    def __init__(self, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, xyz_res=10, view_res=4,
                 precision="auto"):
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
        self.model = Nerf()
        self.model_fine = Nerf()
        self._memo = Memo()  # slot 'packed' / 'packed_fine': the MFMA-ordered blob of a module, rebuilt when a parameter changes

    def nerf_precision(self):
        """The arithmetic nb_nerf_decode runs: 'auto' is AUTO_ARITHMETIC."""
        return AUTO_ARITHMETIC if self.precision == "auto" else self.precision

    def _module(self, model):
        return self.model_fine if model == "fine" else self.model

    def _inference_only(self, what):
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

    def decode(self, ray_o, ray_d, z_vals, model=""):
        """raw [n,S,4] at the depths z_vals [n,S] of the rays ray_o / ray_d [n,3]: the point is o + d z, the direction d / |d|."""
        self._inference_only("NerfNetwork.decode")
        return ops.nerf_decode(self.packed(model), ray_o, ray_d, z_vals, self.nerf_precision())

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
        return ops.nerf_decode(self.packed(model), o, d, z, self.nerf_precision()).view(n, S, 4)


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
    (volume_renderer.py:93-101), nb_composite."""

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
        return ops.composite(raw, z_vals, ray_d, bool(self.cfg.white_bkgd))

    def render_rays(self, ray_o, ray_d, near, far, u=None, raw_noise=None):
        """One chunk: ray_o / ray_d [n,3], near / far [n] -> the reference's dict with flat shapes (rgb_map [n,3], disp_map, acc_map,
        depth_map [n], raw [n,S+N,4]; with N_importance > 0 also rgb0, disp0, acc0, z_std [n]) plus z_vals [n,S+N].
        u: [N] or [n,N] numbers in [0,1) used instead of linspace (perturb == 0) or torch.rand (otherwise).
        raw_noise: (coarse [n,S], fine [n,S+N]) standard-normal tensors used instead of torch.randn when raw_noise_std != 0."""
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
        # volume_renderer.py:48-54; the stratified jitter (:56-70) needs net.training, which the network refuses
        z_coarse = (near[:, None] * (1.0 - t_vals) + far[:, None] * t_vals).contiguous()
        raw = self.net.decode(ray_o, ray_d, z_coarse)
        rgb, disp, acc, weights, depth = self._composite(raw, z_coarse, ray_d, None if raw_noise is None else raw_noise[0])
        ret = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "depth_map": depth, "raw": raw, "z_vals": z_coarse}
        if N == 0:
            return ret
        if u is None:
            if float(cfg.perturb) == 0.0:  # the reference's det (volume_renderer.py:90)
                u = self._memo.get("u_det", (N, str(dev)), lambda: torch.linspace(0.0, 1.0, steps=N).to(dev))
            else:
                u = torch.rand((ray_o.shape[0], N), device=dev)
        smp = ops.importance_sample(ray_o, ray_d, near, far, t_vals, None, weights, u.float().contiguous(), want_z_coarse=False)
        z_vals = ops.importance_merge_z(z_coarse, smp["z_fine"])
        raw = self.net.decode(ray_o, ray_d, z_vals, model="fine")
        rgb, disp, acc, weights, depth = self._composite(raw, z_vals, ray_d, None if raw_noise is None else raw_noise[1])
        return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "depth_map": depth, "raw": raw, "rgb0": ret["rgb_map"],
                "disp0": ret["disp_map"], "acc0": ret["acc_map"], "z_std": smp["z_std"], "z_vals": z_vals}

    def render(self, batch, t_rand=None, feature_volume=None, u=None, raw_noise=None):
        """volume_renderer.py:141-156: batch ray_o / ray_d [B,n,3], near / far [B,n] -> rgb_map [B,n,3], disp_map / acc_map [B,n,1],
        depth_map [B,n], raw [B,n,(S+N)*4] and, with N_importance > 0, rgb0 [B,n,3], disp0 / acc0 / z_std [B,n,1]; z_vals [B,n,S+N] is
        an addition.  u [B,n,N] (or [N]) and raw_noise ([B,n,S], [B,n,S+N]) replace the random numbers, for tests.  t_rand and
        feature_volume are what NovelViewRenderer hands every renderer: there is no jitter in inference and no encoder here."""
        if t_rand is not None:
            raise NotImplementedError("t_rand: the stratified jitter belongs to training (volume_renderer.py:56), which is out of scope")
        ray_o, ray_d = batch["ray_o"], batch["ray_d"]
        B, n = ray_o.shape[:2]
        o, d = ray_o.reshape(-1, 3), ray_d.reshape(-1, 3)
        near, far = batch["near"].reshape(-1), batch["far"].reshape(-1)
        total, chunk = B * n, max(1, int(self.cfg.chunk))
        if u is not None and u.dim() > 1:
            u = u.reshape(total, -1)
        if raw_noise is not None:
            raw_noise = tuple(r.reshape(total, -1) for r in raw_noise)
        parts = {}
        for i in (range(0, total, chunk) if total else (0,)):
            sl = slice(i, i + chunk)
            out = self.render_rays(o[sl], d[sl], near[sl], far[sl], u=u if u is None or u.dim() == 1 else u[sl],
                                   raw_noise=None if raw_noise is None else tuple(r[sl] for r in raw_noise))
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
    return {"rgb_map": 3, "rgb0": 3, "raw": 4 * T, "z_vals": T}.get(key, 1)
