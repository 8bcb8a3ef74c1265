"""Tensor-level wrappers over the C ABI (include/nb_hip.h).  Every function validates device,
dtype, contiguity and shape, then hands raw device pointers + the current HIP stream to
libnb_hip.so.  Nothing here computes: there is no PyTorch / CPU fallback for any operator."""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import NbCull, NbError, NbFold, NbMlpParams, NbScene, NbSmplModel, check, ptr

LEVEL_CHANNELS = (32, 64, 128, 128)
DBG_WIDTH = 1600
# activation tap layout of nb_decode_points(debug=True): F | h1 | h2 | h3 | G | V | PE (csrc/nb_march_common.h TAP_*)
TAP = {"F": (0, 352), "h1": (352, 608), "h2": (608, 864), "h3": (864, 1120), "G": (1120, 1376), "V": (1376, 1504),
       "PE": (1504, 1594)}
# bench.py sets this to a list to collect (start, end) HIP events bracketing every nb_march launch on
# the stream it is enqueued on
MARCH_EVENTS = None
FIXUP_CAP = 32768  # rays the march's last-sample fix-up list holds by default (2 MB of scratch; the bench view lists ~50)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise NbError("%s must live on a HIP device (got %s); the HIP path has no CPU fallback" % (name, t.device))
    return t


def _req(t, dtype, shape=None, name="tensor"):
    _on_device(t, name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None:
        if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    return t


def volume_as_channels_last(v):
    """[1,C,D,H,W] (any strides) -> contiguous [D,H,W,C] view or copy."""
    if v.dim() != 5 or v.shape[0] != 1:
        raise ValueError("feature volume must be [1,C,D,H,W] (batch 1), got %s" % (tuple(v.shape),))
    return v[0].permute(1, 2, 3, 0).contiguous()  # no copy when the storage is already channels-last


def make_pose(R, Th, bounds, device=None):
    """The per-frame pose block the kernels read from DEVICE memory: R[9] row-major | Th[3] | bounds_min[3] (15 fp32).
    R (any shape with 9 elements), Th (>= 3 elements), bounds ([..,2,3] or 3 elements: the minimum corner is taken) may
    be device tensors — sp_input['R'|'Th'|'bounds'] as they are, no host round trip, no sync — or host sequences."""
    def dev_flat(x, n):
        if not isinstance(x, torch.Tensor):
            import numpy as np

            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        x = x.detach().reshape(-1)[:n].to(device=device if device is not None else x.device, dtype=torch.float32)
        if x.numel() != n:
            raise ValueError("pose component has %d elements, expected >= %d" % (x.numel(), n))
        return x

    if device is None:
        device = next((x.device for x in (R, Th, bounds) if isinstance(x, torch.Tensor)), None)
    pose = torch.cat([dev_flat(R, 9), dev_flat(Th, 3), dev_flat(bounds, 3)])
    return _req(pose, torch.float32, (15,), "pose")


def sparsify(volume_cl):
    """nb_sparsify: active set of a dense channels-last volume [D,H,W,C] that came without one -> (grid [D,H,W] int32,
    rows_lin [cap] int32, n_rows [1] int32, cap).  Capacity = every voxel (no device -> host read)."""
    _req(volume_cl, torch.float32, (None, None, None, None), "volume")
    dhw = [int(v) for v in volume_cl.shape[:3]]
    nvox = dhw[0] * dhw[1] * dhw[2]
    dev = volume_cl.device
    grid = torch.empty(dhw, dtype=torch.int32, device=dev)
    buf = torch.zeros(nvox + 1, dtype=torch.int32, device=dev)
    rows_lin, n_rows = buf[:nvox], buf[nvox:]
    scratch = scan_scratch(nvox, dev)
    check(_lib.lib().nb_sparsify(ptr(volume_cl), _i3(dhw), int(volume_cl.shape[3]), ptr(grid), ptr(rows_lin), ptr(n_rows),
                                 nvox, ptr(scratch), _stream()), "nb_sparsify")
    return grid, rows_lin, n_rows, nvox


def fold_build(volumes_cl, sparse, fc0_w, rows=None, n_sat=None):
    """nb_fold_build: the fc_0-folded planes of one frame (precision 'f16f6').  volumes_cl: the four channels-last volumes
    (or, with `rows`, just their [D,H,W] shapes); sparse: per level (grid, rows_lin, n_rows[1], n_rows_max) — the encoder's index
    structures, or `sparsify`'s; rows: per level the ACTIVE rows themselves, compact [>= n_rows_max, C] fp32 (the encoder's
    output before `.dense()`): the dense volumes are then not read and need not exist; fc0_w [256,352(,1)].
    Returns (NbFold, keepalive); keepalive[0] = the planes, keepalive[1] = n_saturated [1] int32 (see include/nb_hip.h)."""
    if fc0_w.dim() == 3:
        fc0_w = fc0_w[:, :, 0]
    fc0_w = fc0_w.detach()
    if not fc0_w.is_contiguous():
        fc0_w = fc0_w.contiguous()
    _req(fc0_w, torch.float32, (256, 352), "fc0_w")
    v4, l4, n4, caps = (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_int32 * 4)()
    f = NbFold()
    base = 0
    keep_src = []
    for l, (v, (grid, rows_lin, n_rows, cap)) in enumerate(zip(volumes_cl, sparse)):
        dhw = tuple(int(x) for x in (v.shape[:3] if isinstance(v, torch.Tensor) else v))
        _req(grid, torch.int32, dhw, "grid[%d]" % l)
        _req(n_rows, torch.int32, (1,), "n_rows[%d]" % l)
        cap = max(int(cap), 1)
        if rows is not None:
            r = _req(rows[l], torch.float32, (None, LEVEL_CHANNELS[l]), "rows[%d]" % l)
            if r.shape[0] < cap:
                raise ValueError("rows[%d] shorter than its capacity" % l)
            v4[l], l4[l] = r.data_ptr(), None
            keep_src.append(r)
        else:
            _req(v, torch.float32, (None, None, None, LEVEL_CHANNELS[l]), "volume[%d]" % l)
            _req(rows_lin, torch.int32, (None,), "rows_lin[%d]" % l)
            if rows_lin.shape[0] < cap:
                raise ValueError("rows_lin[%d] shorter than its capacity" % l)
            v4[l], l4[l] = v.data_ptr(), rows_lin.data_ptr()
            keep_src.append(v)
        n4[l], caps[l] = n_rows.data_ptr(), cap
        f.grid[l] = grid.data_ptr()
        f.row_base[l] = base
        base += cap
    if base >= (1 << 21):
        raise ValueError("fold_build: %d rows exceed the 2 GiB plane the march addresses with 32-bit offsets" % base)
    dev = fc0_w.device
    urows = torch.empty((base + 1, 512), dtype=torch.int16, device=dev)
    if n_sat is None:
        n_sat = torch.zeros(1, dtype=torch.int32, device=dev)
    _req(n_sat, torch.int32, (1,), "n_sat")
    f.urows = urows.data_ptr()
    f.zero_row = base
    check(_lib.lib().nb_fold_build(v4, l4, n4, caps, ptr(fc0_w), ptr(urows), ptr(n_sat), _stream()), "nb_fold_build")
    return f, [urows, n_sat, fc0_w] + keep_src + [t for sp in sparse for t in sp[:3]]


def make_scene(volumes_cl, pose, voxel_size, out_sh, fold=None):
    """volumes_cl: four contiguous [D,H,W,C] fp32 device tensors — or, with `fold` (precision 'f16f6' reads the folded planes,
    never the volumes), just their (D, H, W) shapes; pose: the 15-float DEVICE block of make_pose; voxel_size (3, dhw) and
    out_sh (3) are HOST sequences; fold: `fold_build`'s result.  Returns (NbScene, keepalive)."""
    sc = NbScene()
    if len(volumes_cl) != 4:
        raise ValueError("expected 4 feature volumes")
    keep = [pose]
    for l, v in enumerate(volumes_cl):
        if isinstance(v, torch.Tensor):
            _req(v, torch.float32, (None, None, None, LEVEL_CHANNELS[l]), "volume[%d]" % l)
            sc.vol[l] = v.data_ptr()
            keep.append(v)
            dhw = v.shape[:3]
        else:
            if fold is None:
                raise ValueError("volume[%d] given as a shape: only a scene with folded planes can do without the volume" % l)
            sc.vol[l] = None
            dhw = v
        for k in range(3):
            sc.vol_dhw[l][k] = int(dhw[k])
    _req(pose, torch.float32, (15,), "pose")
    sc.pose = pose.data_ptr()
    for k in range(3):
        sc.voxel_size[k] = float(voxel_size[k])
        sc.out_sh[k] = int(out_sh[k])
    if fold is not None:
        sc.fold = C.pointer(fold[0])
        keep += [fold[0]] + list(fold[1])
    return sc, keep


def mlp_pack_size():
    return int(_lib.lib().nb_mlp_pack_size())


def _mlp_params(params):
    """params: dict name -> fp32 device tensor ([out,in] or [out,in,1] weights, [out] biases)."""
    shapes = {"fc0": (256, 352), "fc1": (256, 256), "fc2": (256, 256), "alpha": (1, 256), "feature": (256, 256),
              "latent": (256, 384), "view": (128, 346), "rgb": (3, 128)}
    p = NbMlpParams()
    keep = []
    for name, (o, i) in shapes.items():
        w = params[name + "_w"]
        b = params[name + "_b"]
        if w.dim() == 3 and w.shape[2] == 1:
            w = w[:, :, 0]
        w = w.detach()
        b = b.detach()
        if not w.is_contiguous():
            w = w.contiguous()
        _req(w, torch.float32, (o, i), name + "_w")
        _req(b, torch.float32, (o,), name + "_b")
        setattr(p, name + "_w", w.data_ptr())
        setattr(p, name + "_b", b.data_ptr())
        keep += [w, b]
    return p, keep


def mlp_pack(params, out=None, precisions=None):
    """nb_mlp_pack(_sections): re-order the decoder weights into MFMA fragment order -> 1-D fp32 blob.  `precisions`:
    iterable of arithmetic names whose sections are needed (None: all)."""
    p, keep = _mlp_params(params)
    dev = keep[0].device
    if out is None:
        out = torch.zeros(mlp_pack_size(), dtype=torch.float32, device=dev)  # sections not asked for stay zero, never stale
    _req(out, torch.float32, (mlp_pack_size(),), "packed")
    bits = 3 if precisions is None else (1 | sum(_lib.PACK_SECTIONS[q] for q in set(precisions)))
    check(_lib.lib().nb_mlp_pack_sections(C.byref(p), ptr(out), int(bits), _stream()), "nb_mlp_pack_sections")
    return out


def six_bit_small_fraction(packed):
    """Per layer the 'f16f6' kernel runs with six-bit cross terms (fc_1, fc_2, the folded feature_fc / latent_fc / view_fc
    layer): the share of non-zero weights below 1/8 of their (row, 32 K) block's maximum, counted while that section was
    packed (nb_mlp_six_bit_stats_offset).  Device tensor [3]."""
    off = int(_lib.lib().nb_mlp_six_bit_stats_offset())
    c = packed[off:off + 6].view(torch.int32).reshape(3, 2).to(torch.float32)
    return c[:, 0] / c[:, 1].clamp_min(1.0)


def mlp_latent_bias(params, latent_row, out=None):
    p, keep = _mlp_params(params)
    latent_row = latent_row.detach()
    _req(latent_row, torch.float32, (128,), "latent_row")
    n = int(_lib.lib().nb_mlp_latent_bias_size())
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=latent_row.device)
    _req(out, torch.float32, (n,), "latent_bias")
    check(_lib.lib().nb_mlp_latent_bias(C.byref(p), ptr(latent_row), ptr(out), _stream()), "nb_mlp_latent_bias")
    return out


def decode_points(scene, packed, latent_bias, wpts, viewdir=None, density_only=False, debug=False, precision="f32"):
    """nb_decode_points: wpts [n,3] (+ viewdir [n,3]) -> raw [n,4] (or sigma [n,1])."""
    sc, _keep = scene
    _req(packed, torch.float32, (mlp_pack_size(),), "packed")
    _req(wpts, torch.float32, (None, 3), "wpts")
    n = wpts.shape[0]
    if not density_only:
        _req(viewdir, torch.float32, (n, 3), "viewdir")
        _req(latent_bias, torch.float32, (int(_lib.lib().nb_mlp_latent_bias_size()),), "latent_bias")
    out = torch.empty((n, 1 if density_only else 4), dtype=torch.float32, device=wpts.device)
    dbg = None
    if debug and density_only:
        raise ValueError("decode_points: the activation tap (debug) is written by the colour decode only; density_only has none")
    if debug:  # the kernel writes columns [0, 1594) of every point's tap; the six pad columns are cleared (a strided 1.5 MB fill,
        dbg = torch.empty((n, DBG_WIDTH), dtype=torch.float32, device=wpts.device)  # not the 419 MB of a training batch)
        dbg[:, TAP["PE"][1]:].zero_()
    check(_lib.lib().nb_decode_points(C.byref(sc), ptr(packed), ptr(latent_bias), ptr(wpts), ptr(viewdir), n,
                                      1 if density_only else 0, ptr(out), ptr(dbg), _lib.PRECISIONS[precision],
                                      _stream()), "nb_decode_points")
    return (out, dbg) if debug else out


def march(scene, packed, latent_bias, ray_o, ray_d, near, far, t_vals, t_rand=None, white_bkgd=False,
          want_raw=False, precision="f32", ray_order=None, cull=None, order_covers_all=False, fixup=True):
    """nb_march: all rays of one batch element -> dict of per-ray outputs.  With a `ray_order` the kernel stores only the rays
    its slots name: unless the caller vouches that every ray has a slot (`order_covers_all`, e.g. the slot list of a fully
    covered image) the outputs start out as zeros, so a ray without a slot reads 0 and never uninitialised memory.
    `fixup` (precision 'f16f6'): hand the call the scratch of its last-sample fix-up (include/nb_hip.h, `ill_scratch`) — True:
    room for min(n, FIXUP_CAP) rays, an int: for that many; the result then carries it as 'ill_scratch' (int32 view: [rays
    listed, rays whose 1e10-interval step changed side, ...])."""
    sc, _keep = scene
    _req(packed, torch.float32, (mlp_pack_size(),), "packed")
    _req(latent_bias, torch.float32, (int(_lib.lib().nb_mlp_latent_bias_size()),), "latent_bias")
    _req(ray_o, torch.float32, (None, 3), "ray_o")
    n = ray_o.shape[0]
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    _req(near, torch.float32, (n,), "near")
    _req(far, torch.float32, (n,), "far")
    _req(t_vals, torch.float32, (None,), "t_vals")
    S = t_vals.shape[0]
    if t_rand is not None:
        _req(t_rand, torch.float32, (n, S), "t_rand")
    n_slots = 0
    if ray_order is not None:
        _req(ray_order, torch.int32, (None,), "ray_order")
        n_slots = int(ray_order.shape[0])
        if n_slots == 0 or n_slots % 64:
            raise ValueError("ray_order holds %d slots: a positive multiple of 64 (ops.tile_slots)" % n_slots)
    dev = ray_o.device
    alloc = torch.zeros if (ray_order is not None and not order_covers_all) else torch.empty
    rgb = alloc((n, 3), dtype=torch.float32, device=dev)
    disp = alloc((n,), dtype=torch.float32, device=dev)
    acc = alloc((n,), dtype=torch.float32, device=dev)
    weights = alloc((n, S), dtype=torch.float32, device=dev)
    depth = alloc((n,), dtype=torch.float32, device=dev)
    raw = alloc((n, S, 4), dtype=torch.float32, device=dev) if want_raw else None
    ill, ill_bytes = None, 0
    if fixup and precision == "f16f6" and n > 0:
        ill_bytes = _lib.ill_scratch_bytes(min(n, FIXUP_CAP) if fixup is True else max(int(fixup), 1))
        ill = torch.empty(ill_bytes // 4, dtype=torch.int32, device=dev)
    ev = None
    if MARCH_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    check(_lib.lib().nb_march(C.byref(sc), ptr(packed), ptr(latent_bias), ptr(ray_o), ptr(ray_d), ptr(near), ptr(far),
                              n, S, ptr(t_vals), ptr(t_rand), ptr(ray_order), n_slots,
                              C.byref(cull[0]) if cull is not None else None, 1 if white_bkgd else 0, ptr(rgb), ptr(disp),
                              ptr(acc),
                              ptr(weights), ptr(depth), ptr(raw), ptr(ill), ill_bytes, _lib.PRECISIONS[precision], _stream()), "nb_march")
    if ev is not None:
        ev[1].record()
        MARCH_EVENTS.append(ev)
    ret = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "weights": weights, "depth_map": depth}
    if want_raw:
        ret["raw"] = raw
    if ill is not None:
        ret["ill_scratch"] = ill
    return ret


def composite(raw, z_vals, ray_d, white_bkgd=False):
    """nb_composite: raw2outputs on device. raw [n,S,4], z_vals [n,S], ray_d [n,3]."""
    _req(raw, torch.float32, (None, None, 4), "raw")
    n, S = raw.shape[:2]
    _req(z_vals, torch.float32, (n, S), "z_vals")
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    dev = raw.device
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((n,), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    weights = torch.empty((n, S), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    check(_lib.lib().nb_composite(ptr(raw), ptr(z_vals), ptr(ray_d), n, S, 1 if white_bkgd else 0, ptr(rgb), ptr(disp),
                                  ptr(acc), ptr(weights), ptr(depth), _stream()), "nb_composite")
    return rgb, disp, acc, weights, depth


# --------------------------------------------------------------------------------- encoder
def scan_scratch(n, device):
    return torch.empty(int(_lib.lib().nb_scan_scratch_size(int(n))), dtype=torch.uint8, device=device)


def _i3(v):
    return (C.c_int32 * 3)(int(v[0]), int(v[1]), int(v[2]))


def enc_voxelize(coord, dhw, buf=None, grid=None):
    """nb_enc_voxelize: coord [n,3] int32 (d,h,w) -> (grid [D,H,W] i32, rows_vert, rows_lin, n_rows[1]).
    buf: a ZEROED int32 [2 * max(n, 1) + 1] buffer of the caller's for the three outputs (the encoder clears the index buffers of
    all its levels with one fill); grid: an int32 [D,H,W] buffer ALREADY FILLED WITH -1 (likewise one fill for all levels)."""
    _req(coord, torch.int32, (None, 3), "coord")
    n = coord.shape[0]
    dev = coord.device
    prefilled = grid is not None
    if grid is None:
        grid = torch.empty([int(s) for s in dhw], dtype=torch.int32, device=dev)
    _req(grid, torch.int32, tuple(int(s) for s in dhw), "grid")
    m = max(n, 1)
    if buf is None:
        buf = torch.zeros(2 * m + 1, dtype=torch.int32, device=dev)  # one fill
    else:
        _req(buf, torch.int32, (2 * m + 1,), "buf")
    rows_vert, rows_lin, n_rows = buf[:m], buf[m:2 * m], buf[2 * m:]
    scratch = scan_scratch(n, dev)
    check(_lib.lib().nb_enc_voxelize(ptr(coord), n, _i3(dhw), ptr(grid), ptr(rows_vert), ptr(rows_lin), ptr(n_rows),
                                     ptr(scratch), 1 if prefilled else 0, _stream()), "nb_enc_voxelize")
    return grid, rows_vert, rows_lin, n_rows


def down_dhw(dhw):
    return [(int(s) - 1) // 2 + 1 for s in dhw]


def down_capacity(n_in_max, in_dhw):
    """Row capacity of the strided convolution's output index set: every input row has at most 8 parents."""
    out_dhw = down_dhw(in_dhw)
    return max(min(8 * int(n_in_max), out_dhw[0] * out_dhw[1] * out_dhw[2]), 1)


def enc_downsample_index(in_lin, n_in, n_in_max, in_dhw, scratch=None, buf=None, grid=None):
    """nb_enc_downsample_index -> (out_grid, out_lin, n_out[1], n_out_max, out_dhw).
    buf: a ZEROED int32 [down_capacity(n_in_max, in_dhw) + 1] buffer of the caller's for out_lin and n_out."""
    _req(in_lin, torch.int32, (None,), "in_lin")
    _req(n_in, torch.int32, (1,), "n_in")
    dev = in_lin.device
    out_dhw = down_dhw(in_dhw)
    nvox = out_dhw[0] * out_dhw[1] * out_dhw[2]
    n_out_max = down_capacity(n_in_max, in_dhw)
    prefilled = grid is not None  # an int32 [Do,Ho,Wo] buffer already filled with -1
    out_grid = grid if prefilled else torch.empty(out_dhw, dtype=torch.int32, device=dev)
    _req(out_grid, torch.int32, tuple(out_dhw), "out_grid")
    if buf is None:
        buf = torch.zeros(n_out_max + 1, dtype=torch.int32, device=dev)  # one fill
    else:
        _req(buf, torch.int32, (n_out_max + 1,), "buf")
    out_lin, n_out = buf[:n_out_max], buf[n_out_max:]
    if scratch is None:
        scratch = scan_scratch(nvox, dev)
    check(_lib.lib().nb_enc_downsample_index(ptr(in_lin), ptr(n_in), int(n_in_max), _i3(in_dhw), _i3(out_dhw),
                                             ptr(out_grid), ptr(out_lin), ptr(n_out), n_out_max, ptr(scratch),
                                             1 if prefilled else 0, _stream()), "nb_enc_downsample_index")
    return out_grid, out_lin, n_out, n_out_max, out_dhw


def enc_downsample_index_all(in_lin, n_in, n_in_max, in_dhw, bufs, grids, scratch=None):
    """nb_enc_downsample_index_all: the index sets of len(bufs) successive strided levels in three launches -> a list of
    (out_grid, out_lin, n_out[1], n_out_max, out_dhw), one per level, equal to chained enc_downsample_index calls.
    bufs[l]: a ZEROED int32 [capacity_l + 1] buffer for out_lin and n_out (capacity_l = down_capacity of the level above);
    grids[l]: an int32 [D_l, H_l, W_l] buffer ALREADY FILLED WITH -1."""
    _req(in_lin, torch.int32, (None,), "in_lin")
    _req(n_in, torch.int32, (1,), "n_in")
    n_levels = len(bufs)
    if n_levels != len(grids) or not 1 <= n_levels <= 4:
        raise ValueError("1..4 levels, one buffer and one grid each")
    dev = in_lin.device
    out, cap, d = [], int(n_in_max), [int(x) for x in in_dhw]
    for l in range(n_levels):
        cap, d = down_capacity(cap, d), down_dhw(d)
        _req(grids[l], torch.int32, tuple(d), "grids[%d]" % l)
        _req(bufs[l], torch.int32, (cap + 1,), "bufs[%d]" % l)
        out.append((grids[l], bufs[l][:cap], bufs[l][cap:], cap, list(d)))
    if scratch is None:
        scratch = scan_scratch(max(math.prod(out[0][4]), 64), dev)
    pg = (C.c_void_p * n_levels)(*[o[0].data_ptr() for o in out])
    pl = (C.c_void_p * n_levels)(*[o[1].data_ptr() for o in out])
    pn = (C.c_void_p * n_levels)(*[o[2].data_ptr() for o in out])
    caps = (C.c_int32 * n_levels)(*[o[3] for o in out])
    check(_lib.lib().nb_enc_downsample_index_all(ptr(in_lin), ptr(n_in), int(n_in_max), _i3(in_dhw), n_levels, pg, pl, pn, caps,
                                                 ptr(scratch), 1, _stream()), "nb_enc_downsample_index_all")
    return out


def _enc_conv(entry, in_rows, cin, cout, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, weight, stats, flags, pre=()):
    """enc_conv / enc_conv16: the index-set and statistics checks, the outputs and the call (`pre`: what the entry point takes
    between the rows and the grid).  flags: bit 0 (NB_CONV_STATS_ZEROED) is set here."""
    _req(in_grid, torch.int32, tuple(int(s) for s in in_dhw), "in_grid")
    _req(out_lin, torch.int32, (None,), "out_lin")
    _req(n_out, torch.int32, (1,), "n_out")
    if out_lin.shape[0] < n_out_max:
        raise ValueError("out_lin shorter than n_out_max")
    dev = in_rows.device
    out_rows = torch.empty((max(int(n_out_max), 1), cout), dtype=torch.float32, device=dev)
    if stats is None:
        stats = torch.empty(2 * cout, dtype=torch.float64, device=dev)
    else:
        _req(stats, torch.float64, (2 * cout,), "stats")
        flags |= 1
    check(getattr(_lib.lib(), entry)(ptr(in_rows), *pre, ptr(in_grid), _i3(in_dhw), ptr(out_lin), ptr(n_out), int(n_out_max),
                                     _i3(out_dhw), int(stride), ptr(weight), cin, cout, ptr(out_rows), ptr(stats), flags,
                                     _stream()), entry)
    return out_rows, stats


def enc_conv(in_rows, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, weight, stats=None):
    """nb_enc_conv -> (out_rows [n_out_max, Cout], stats [2*Cout] fp64).  `stats`: a ZEROED fp64 [2*Cout] buffer of the
    caller's (the encoder clears the statistics of all its layers with one fill) — else the call allocates and clears one."""
    _req(weight, torch.float32, (3, 3, 3, None, None), "conv weight")
    cin, cout = int(weight.shape[3]), int(weight.shape[4])
    _req(in_rows, torch.float32, (None, cin), "in_rows")
    return _enc_conv("nb_enc_conv", in_rows, cin, cout, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, weight, stats, 0)


def _enc_bn_relu(entry, rows, n_rows, n_rows_max, stats, gamma, beta, running_mean, running_var, training, eps, rows_lin, dense,
                 momentum, rows_out, split=None):
    """enc_bn_relu / enc_bn_relu_split: the checks, batch_stats and the call (split: the second one's extra output)."""
    c = int(rows.shape[1])
    _req(rows, torch.float32, (None, c), "rows")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _req(t, torch.float32, (c,), nm)
    if stats is not None:
        _req(stats, torch.float64, (2 * c,), "stats")
    if dense is not None:
        _req(dense, torch.float32, (None, None, None, c), "dense")
        _req(rows_lin, torch.int32, (None,), "rows_lin")
    if rows_out is not None:
        _req(rows_out, torch.float32, tuple(rows.shape), "rows_out")
    batch_stats = torch.empty(2 * c + 1, dtype=torch.float32, device=rows.device)
    check(getattr(_lib.lib(), entry)(ptr(rows), ptr(n_rows), int(n_rows_max), c, ptr(stats), ptr(gamma), ptr(beta),
                                     ptr(running_mean), ptr(running_var), 1 if training else 0, float(eps), float(momentum),
                                     ptr(batch_stats), ptr(rows_lin), ptr(dense), *(() if split is None else (ptr(split),)),
                                     ptr(rows_out), _stream()), entry)
    return batch_stats


def enc_bn_relu(rows, n_rows, n_rows_max, stats, gamma, beta, running_mean, running_var, training, eps,
                rows_lin=None, dense=None, momentum=-1.0, rows_out=None):
    """nb_enc_bn_relu (in place on rows) -> batch_stats [2C+1] = mean | biased var | n_rows.
    momentum >= 0 (training only): running_mean / running_var are updated in place by the kernel."""
    return _enc_bn_relu("nb_enc_bn_relu", rows, n_rows, n_rows_max, stats, gamma, beta, running_mean, running_var, training, eps,
                        rows_lin, dense, momentum, rows_out)


def enc_conv_pack16(weight, backward_input=False):
    """nb_enc_conv_pack16: spconv-layout fp32 weight -> head / remainder B fragments (int16 tensor): fp16 pairs of the forward
    convolution, or (backward_input) bf16 pairs of the stride-1 layer's backward-input convolution (mirrored offsets,
    transposed slabs: a convolution with Cout input and Cin output channels)."""
    _req(weight, torch.float32, (3, 3, 3, None, None), "conv weight")
    cin, cout = int(weight.shape[3]), int(weight.shape[4])
    packed = torch.empty(27 * cin * cout * 2, dtype=torch.int16, device=weight.device)
    ci, co, mode = (cout, cin, 1) if backward_input else (cin, cout, 0)
    check(_lib.lib().nb_enc_conv_pack16(ptr(weight), ci, co, ptr(packed), mode, _stream()), "nb_enc_conv_pack16")
    return packed


def enc_conv_pack16_batch(jobs):
    """nb_enc_conv_pack16_batch: jobs = [(weight [3,3,3,Cin,Cout], backward_input)] -> list of packed int16 tensors, one launch
    (per 32 jobs)."""
    outs = []
    for i0 in range(0, len(jobs), 32):
        chunk = jobs[i0:i0 + 32]
        n = len(chunk)
        w_p, out_p = (C.c_void_p * n)(), (C.c_void_p * n)()
        cin_a, cout_a, mode_a = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
        for i, (weight, bwd) in enumerate(chunk):
            _req(weight, torch.float32, (3, 3, 3, None, None), "conv weight")
            ci, co = int(weight.shape[3]), int(weight.shape[4])
            packed = torch.empty(27 * ci * co * 2, dtype=torch.int16, device=weight.device)
            outs.append(packed)
            w_p[i], out_p[i] = weight.data_ptr(), packed.data_ptr()
            cin_a[i], cout_a[i], mode_a[i] = (co, ci, 1) if bwd else (ci, co, 0)
        check(_lib.lib().nb_enc_conv_pack16_batch(n, w_p, cin_a, cout_a, out_p, mode_a, _stream()), "nb_enc_conv_pack16_batch")
    return outs


def enc_conv16(in_split, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, wpacked, cin, cout, stats=None,
               bf16=False):
    """nb_enc_conv16 on split rows (int16 [2, cap, Cin]: fp16 heads | remainders) -> (out_rows fp32, stats fp64); `stats` as
    in enc_conv.  bf16: the planes and the packed weight are bf16 pairs (the backward-input convolution)."""
    _req(in_split, torch.int16, (2, None, cin), "in_split")
    _req(wpacked, torch.int16, (27 * cin * cout * 2,), "wpacked")
    return _enc_conv("nb_enc_conv16", in_split, cin, cout, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, wpacked, stats,
                     2 if bf16 else 0, pre=(int(in_split.shape[1]),))  # NB_CONV_BF16


CONV16_VARIANTS = ("KS", "LDS_ALL_TILES", "LDS_TWO_TILES", "WAVE_ALL_TILES", "WAVE_ONE_TILE")


def enc_conv16_variant(cin, cout, n_out_max):
    """nb_enc_conv16_variant: the forward kernel enc_conv16 runs for this pair and row capacity, as a name of CONV16_VARIANTS (the
    enum's order), or None for a pair it does not take.  Nothing is launched."""
    v = int(_lib.lib().nb_enc_conv16_variant(int(cin), int(cout), int(n_out_max)))
    return None if v < 0 else CONV16_VARIANTS[v]


def enc_bn_relu_split(rows, n_rows, n_rows_max, stats, gamma, beta, running_mean, running_var, training, eps,
                      rows_lin=None, dense=None, momentum=-1.0, rows_out=None):
    """nb_enc_bn_relu_split -> (rows_split int16 [2, n_rows_max, C], batch_stats); rows_out (fp32, same shape as rows):
    receives the activated rows in fp32 as well (training forward)."""
    n_rows_max = max(int(n_rows_max), 1)
    if rows.shape[0] < n_rows_max:
        raise ValueError("rows shorter than n_rows_max")
    split = torch.empty((2, n_rows_max, int(rows.shape[1])), dtype=torch.int16, device=rows.device)
    batch_stats = _enc_bn_relu("nb_enc_bn_relu_split", rows, n_rows, n_rows_max, stats, gamma, beta, running_mean, running_var,
                               training, eps, rows_lin, dense, momentum, rows_out, split)
    return split, batch_stats


def enc_gather_codes(codes, rows_vert, n_rows, n_rows_max):
    _req(codes, torch.float32, (None, None), "codes")
    _req(rows_vert, torch.int32, (None,), "rows_vert")
    c = int(codes.shape[1])
    rows = torch.empty((max(int(n_rows_max), 1), c), dtype=torch.float32, device=codes.device)
    check(_lib.lib().nb_enc_gather_codes(ptr(codes), ptr(rows_vert), ptr(n_rows), int(n_rows_max), c, ptr(rows),
                                         _stream()), "nb_enc_gather_codes")
    return rows


# --------------------------------------------------------------------------------- ray generation
def _host_cam(K, R, T, bounds):
    """The host camera block of the ray entries: K, R [3,3], T [3] as C doubles and bounds [2,3] as C floats."""
    import numpy as np

    K = np.asarray(K, np.float64).reshape(9)
    R = np.asarray(R, np.float64).reshape(9)
    T = np.asarray(T, np.float64).reshape(3)
    b = np.asarray(bounds, np.float32).reshape(6)
    return (C.c_double * 9)(*K), (C.c_double * 9)(*R), (C.c_double * 3)(*T), (C.c_float * 6)(*b)


def _raygen_buffers(n, device):
    """raygen's 6-tuple for n pixels (ray_o, ray_d, near, far, mask_at_box, n_rays[1]) and the scan scratch."""
    ray_o = torch.empty((n, 3), dtype=torch.float32, device=device)
    ray_d = torch.empty((n, 3), dtype=torch.float32, device=device)
    near = torch.empty(n, dtype=torch.float32, device=device)
    far = torch.empty(n, dtype=torch.float32, device=device)
    mask = torch.empty(n, dtype=torch.uint8, device=device)
    n_rays = torch.zeros(1, dtype=torch.int32, device=device)
    return (ray_o, ray_d, near, far, mask, n_rays), scan_scratch(n, device)


def raygen(H, W, K, R, T, bounds, device):
    """nb_raygen: K, R [3,3], T [3] host float64 arrays; bounds [2,3] host float32 (world AABB).
    Returns device tensors (ray_o, ray_d, near, far, mask_at_box, n_rays[1]) with H*W capacity; the
    first n_rays rows are valid."""
    cam = _host_cam(K, R, T, bounds)
    out, scratch = _raygen_buffers(int(H) * int(W), device)
    with torch.cuda.device(device):
        check(_lib.lib().nb_raygen(int(H), int(W), *cam, *(ptr(t) for t in out), ptr(scratch), _stream()), "nb_raygen")
    return out


def train_rays_scratch(H, W, device):
    """Scratch of nb_train_rays for an H x W image; ValueError for sizes the call refuses."""
    n_bytes = int(_lib.lib().nb_train_rays_scratch_size(int(H), int(W)))
    if n_bytes <= 0:
        raise ValueError("train_rays: unsupported image size %d x %d (both >= 1, H*W <= 2^30)" % (H, W))
    return torch.empty(n_bytes, dtype=torch.uint8, device=device)


def train_rays(img, msk, K, R, T, bounds, hull, mode, body_ratio, u, scratch=None):
    """nb_train_rays: img [H,W,3] fp32 and msk [H,W] uint8 device tensors; K, R [3,3], T [3] host float64; bounds [2,3] host
    float32 (can_bounds); hull [n,2] host int (x, y), CCW (train_rays.bound_hull); mode 'h36m' | 'plain'; u [n_rounds, n_rays]
    fp32 device uniforms.  Returns a dict of device tensors rgb, ray_o, ray_d [n_rays,3], near, far [n_rays], pixel [n_rays,2]
    int32 (y, x), mask_at_box [n_rays] uint8 and status [4] int32 {n_filled, rounds_used, count_body, count_bound}.
    Nothing is read back."""
    import numpy as np

    if mode not in _lib.SAMPLE_MODES:
        raise ValueError("train_rays: mode must be one of %s, got %r" % (sorted(_lib.SAMPLE_MODES), mode))
    _req(img, torch.float32, (None, None, 3), "img")
    H, W = int(img.shape[0]), int(img.shape[1])
    _req(msk, torch.uint8, (H, W), "msk")
    _req(u, torch.float32, (None, None), "u")
    dev = img.device
    if msk.device != dev or u.device != dev:
        raise ValueError("img, msk and u must share one device")
    n_rounds, n = int(u.shape[0]), int(u.shape[1])
    cam = _host_cam(K, R, T, bounds)
    hull = np.ascontiguousarray(np.asarray(hull, np.int64).reshape(-1, 2))
    if np.abs(hull).max(initial=0) >= 1 << 30:
        raise ValueError("train_rays: hull coordinate with magnitude >= 2^30")
    hull_c = (C.c_int32 * hull.size)(*[int(v) for v in hull.reshape(-1)])
    if scratch is None:
        scratch = train_rays_scratch(H, W, dev)
    out = {"rgb": torch.empty((n, 3), dtype=torch.float32, device=dev), "ray_o": torch.empty((n, 3), dtype=torch.float32, device=dev),
           "ray_d": torch.empty((n, 3), dtype=torch.float32, device=dev), "near": torch.empty(n, dtype=torch.float32, device=dev),
           "far": torch.empty(n, dtype=torch.float32, device=dev), "pixel": torch.empty((n, 2), dtype=torch.int32, device=dev),
           "mask_at_box": torch.empty(n, dtype=torch.uint8, device=dev), "status": torch.empty(4, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        check(_lib.lib().nb_train_rays(H, W, *cam, C.cast(hull_c, C.c_void_p), hull.shape[0], ptr(msk), ptr(img), _lib.SAMPLE_MODES[mode],
                                       float(body_ratio), ptr(u), n_rounds, n, ptr(out["rgb"]), ptr(out["ray_o"]),
                                       ptr(out["ray_d"]), ptr(out["near"]), ptr(out["far"]), ptr(out["pixel"]),
                                       ptr(out["mask_at_box"]), ptr(out["status"]), ptr(scratch), _stream()), "nb_train_rays")
    return out


def image_assemble(mask_at_box, rgb_map, depth_map=None, white_bkgd=False, bgr=False, scale=1.0):
    """nb_image_assemble: mask_at_box [H*W] uint8/bool (any shape, flattened), rgb_map [n,3] and optional depth_map [n]
    in compacted pixel order -> (img [H*W,3], depth [H*W] or None) on device."""
    mask = mask_at_box.reshape(-1)
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    _req(mask, torch.uint8, (None,), "mask_at_box")
    _req(rgb_map, torch.float32, (None, 3), "rgb_map")
    n_pix, n = mask.shape[0], rgb_map.shape[0]
    if depth_map is not None:
        _req(depth_map, torch.float32, (n,), "depth_map")
    img = torch.empty((n_pix, 3), dtype=torch.float32, device=mask.device)
    depth = torch.empty(n_pix, dtype=torch.float32, device=mask.device) if depth_map is not None else None
    scratch = scan_scratch(n_pix, mask.device)
    with torch.cuda.device(mask.device):
        check(_lib.lib().nb_image_assemble(ptr(mask), n_pix, ptr(rgb_map), ptr(depth_map), n, 1 if white_bkgd else 0,
                                           1 if bgr else 0, float(scale), ptr(img), ptr(depth), ptr(scratch), _stream()),
              "nb_image_assemble")
    return img, depth


def eval_metrics(mask_at_box, H, W, rgb_pred, rgb_gt, white_bkgd=False, whole_img=False, out=None):
    """nb_eval_metrics: mask_at_box [H*W] uint8/bool (any shape, flattened), rgb_pred and rgb_gt [n,3] in compacted pixel
    order -> out, a [8] float64 device tensor {mse, psnr, ssim, x, y, w, h, n_windows} (if_nerf.py:47-74 for one view).
    Nothing is read back: ssim is NaN where compare_ssim would raise (crop under 7 pixels on a side)."""
    H, W = int(H), int(W)
    mask = mask_at_box.reshape(-1)
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    _req(mask, torch.uint8, (H * W,), "mask_at_box")
    _req(rgb_pred, torch.float32, (None, 3), "rgb_pred")
    _req(rgb_gt, torch.float32, (rgb_pred.shape[0], 3), "rgb_gt")
    if out is None:
        out = torch.empty(8, dtype=torch.float64, device=mask.device)
    _req(out, torch.float64, (8,), "out")
    if rgb_pred.device != mask.device or rgb_gt.device != mask.device or out.device != mask.device:
        raise ValueError("mask_at_box, rgb_pred, rgb_gt and out must share one device")
    n_bytes = int(_lib.lib().nb_eval_metrics_scratch_size(H, W))
    if n_bytes <= 0:
        raise ValueError("eval_metrics: unsupported image size %d x %d" % (H, W))
    scratch = torch.empty(n_bytes, dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        check(_lib.lib().nb_eval_metrics(ptr(mask), H, W, ptr(rgb_pred), ptr(rgb_gt), rgb_pred.shape[0],
                                         1 if white_bkgd else 0, 1 if whole_img else 0, ptr(out), ptr(scratch), _stream()),
              "nb_eval_metrics")
    return out


def marching_cubes_scratch(shape, device):
    """Scratch of nb_marching_cubes_count / _emit for an [X,Y,Z] cube; ValueError for shapes the calls refuse."""
    n_bytes = int(_lib.lib().nb_marching_cubes_scratch_size(_i3(shape))) if len(shape) == 3 else 0
    if n_bytes <= 0:
        raise ValueError("marching_cubes: unsupported cube shape %s (every side >= 2, 3*X*Y*Z <= 2^31 - 1)" % (tuple(shape),))
    return torch.empty(n_bytes, dtype=torch.uint8, device=device)


def marching_cubes_count(cube, iso, scratch, counts=None):
    """nb_marching_cubes_count: -> counts, a [2] int32 device tensor {n_vertices, n_triangles}; nothing is read back."""
    _req(cube, torch.float32, (None, None, None), "cube")
    if counts is None:
        counts = torch.empty(2, dtype=torch.int32, device=cube.device)
    _req(counts, torch.int32, (2,), "counts")
    with torch.cuda.device(cube.device):
        check(_lib.lib().nb_marching_cubes_count(ptr(cube), _i3(cube.shape), float(iso), ptr(counts), ptr(scratch), _stream()),
              "nb_marching_cubes_count")
    return counts


def marching_cubes_emit(cube, iso, scratch, vertices, triangles):
    """nb_marching_cubes_emit into caller-owned buffers (vertices [Vcap,3] float32, triangles [Tcap,3] int32) after
    marching_cubes_count on the same cube, iso and scratch.  Raises NbError, with the buffers untouched, when they are too small."""
    _req(cube, torch.float32, (None, None, None), "cube")
    _req(vertices, torch.float32, (None, 3), "vertices")
    _req(triangles, torch.int32, (None, 3), "triangles")
    with torch.cuda.device(cube.device):
        check(_lib.lib().nb_marching_cubes_emit(ptr(cube), _i3(cube.shape), float(iso), ptr(vertices), ptr(triangles),
                                                vertices.shape[0], triangles.shape[0], ptr(scratch), _stream()),
              "nb_marching_cubes_emit")
    return vertices, triangles


def marching_cubes(cube, iso):
    """Marching cubes of a device fp32 cube [X,Y,Z] (if_mesh_renderer.py:46-52 without the host): -> (vertices [V,3] float32 in
    lattice index units, triangles [T,3] int32), device tensors of the exact size, in the order include/nb_hip.h states.
    Count, ONE host read of the two counts, allocate, emit."""
    _req(cube, torch.float32, (None, None, None), "cube")
    scratch = marching_cubes_scratch(cube.shape, cube.device)
    n_vert, n_tri = (int(v) for v in marching_cubes_count(cube, iso, scratch).tolist())
    vertices = torch.empty((n_vert, 3), dtype=torch.float32, device=cube.device)
    triangles = torch.empty((n_tri, 3), dtype=torch.int32, device=cube.device)
    return marching_cubes_emit(cube, iso, scratch, vertices, triangles)


TILE = 8  # rays are marched in 8 x 8 pixel tiles (64 slots = one workgroup of the fused march), made of four 4 x 4 blocks


def tile_pixels(H, W, device):
    """Static part of the slot list of an H x W image: slot -> pixel id (row-major), -1 where the tile sticks out of the image.
    Slot s = 64 * tile + 16 * block + 4 * (y % 4) + (x % 4), tiles row-major, blocks row-major inside a tile: 64 consecutive
    slots = one compact 8 x 8 tile (the voxels its samples touch at a depth step are a few small boxes), every 16 = one 4 x 4
    block (one wave's samples), every 32 = an 8 x 4 half tile."""
    ht, wt = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    s = torch.arange(ht * wt * 64, device=device)
    tile, inner = torch.div(s, 64, rounding_mode="floor"), s % 64
    blk, r = torch.div(inner, 16, rounding_mode="floor"), inner % 16
    py = torch.div(tile, wt, rounding_mode="floor") * TILE + torch.div(blk, 2, rounding_mode="floor") * 4 + torch.div(r, 4, rounding_mode="floor")
    px = (tile % wt) * TILE + (blk % 2) * 4 + r % 4
    pix = py * W + px
    return torch.where((py < H) & (px < W), pix, torch.full_like(pix, -1))


def tile_slots(mask, slot_pixels, begin=0, end=None):
    """The `ray_order` of nb_march (include/nb_hip.h) for the rays of an image: `mask` [H*W] bool/uint8 = which pixels have a
    ray (the rays are the mask's non-zeros in pixel order, batch['mask_at_box']), `slot_pixels` = tile_pixels(H, W), [begin, end)
    = the range of rays to march (a rank's share).  Every tile keeps its own 64 slots: missing pixels become padding slots
    (they march the tile's first ray and store nothing), tiles without a ray are dead.  No host synchronisation: cumulative
    sum + gathers on the device.  int32 [tiles * 64]; entries index the rays of the range (ray - begin)."""
    m = mask.reshape(-1) != 0
    idx = torch.cumsum(m.to(torch.int32), 0, dtype=torch.int32) - 1  # ray index of every pixel that has one
    ok = m & (idx >= begin)
    if end is not None:
        ok = ok & (idx < end)
    p = slot_pixels.clamp_min(0)
    ok_s = ok[p] & (slot_pixels >= 0)
    ray = idx[p] - begin
    big = 1 << 30
    first = torch.where(ok_s, ray, torch.full_like(ray, big)).view(-1, 64).amin(1, keepdim=True)
    fill = torch.where(first < big, -(first + 1), torch.full_like(first, _lib.SLOT_DEAD))
    return torch.where(ok_s.view(-1, 64), ray.view(-1, 64), fill).reshape(-1).to(torch.int32).contiguous()


# --------------------------------------------------------------------------------- backward pass
def composite_bwd(raw, z_vals, ray_d, d_rgb_map, white_bkgd=False, d_acc_map=None, d_depth_map=None):
    """nb_composite_bwd: d raw [n,S,4] from d rgb_map [n,3] (+ optional d acc_map / d depth_map [n])."""
    _req(raw, torch.float32, (None, None, 4), "raw")
    n, S = raw.shape[:2]
    _req(z_vals, torch.float32, (n, S), "z_vals")
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    _req(d_rgb_map, torch.float32, (n, 3), "d_rgb_map")
    for t, nm in ((d_acc_map, "d_acc_map"), (d_depth_map, "d_depth_map")):
        if t is not None:
            _req(t, torch.float32, (n,), nm)
    d_raw = torch.empty_like(raw)
    check(_lib.lib().nb_composite_bwd(ptr(raw), ptr(z_vals), ptr(ray_d), n, S, 1 if white_bkgd else 0, ptr(d_rgb_map),
                                      ptr(d_acc_map), ptr(d_depth_map), ptr(d_raw), _stream()), "nb_composite_bwd")
    return d_raw


def composite_bwd_maps(raw, z_vals, ray_d, white_bkgd=False, d_rgb_map=None, d_acc_map=None, d_depth_map=None, d_disp_map=None,
                       d_weights=None):
    """nb_composite_bwd_maps: d raw [n,S,4] from the cotangents of any of raw2outputs' five outputs (d rgb_map [n,3], d acc_map /
    d depth_map / d disp_map [n], d weights [n,S]; None = 0, at least one must be given).  A ray whose depth / acc is not greater
    than 1e-10 (acc == 0 included) takes nothing from d_disp_map."""
    _req(raw, torch.float32, (None, None, 4), "raw")
    n, S = raw.shape[:2]
    _req(z_vals, torch.float32, (n, S), "z_vals")
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    for t, shape, nm in ((d_rgb_map, (n, 3), "d_rgb_map"), (d_acc_map, (n,), "d_acc_map"), (d_depth_map, (n,), "d_depth_map"),
                         (d_disp_map, (n,), "d_disp_map"), (d_weights, (n, S), "d_weights")):
        if t is not None:
            _req(t, torch.float32, shape, nm)
    d_raw = torch.empty_like(raw)
    check(_lib.lib().nb_composite_bwd_maps(ptr(raw), ptr(z_vals), ptr(ray_d), n, S, 1 if white_bkgd else 0, ptr(d_rgb_map),
                                           ptr(d_acc_map), ptr(d_depth_map), ptr(d_disp_map), ptr(d_weights), ptr(d_raw), _stream()),
          "nb_composite_bwd_maps")
    return d_raw


def ray_distortion_raw(weights, z_vals, want_grad=True):
    """nb_ray_distortion: (loss [n], G [n,S] = d loss / d weights, or None when not wanted) of weights, z_vals [n,S]."""
    _req(weights, torch.float32, (None, None), "weights")
    n, S = weights.shape
    _req(z_vals, torch.float32, (n, S), "z_vals")
    loss = torch.empty((n,), dtype=torch.float32, device=weights.device)
    G = torch.empty_like(weights) if want_grad else None
    check(_lib.lib().nb_ray_distortion(ptr(weights), ptr(z_vals), n, S, ptr(loss), ptr(G), _stream()), "nb_ray_distortion")
    return loss, G


class _RayDistortion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, z_vals):
        want = ctx.needs_input_grad[0]  # under no_grad (or for constant weights) G is not computed
        loss, G = ray_distortion_raw(weights.detach(), z_vals.detach(), want_grad=want)
        ctx.G = G
        return loss

    @staticmethod
    def backward(ctx, g):
        if ctx.G is None:
            return None, None
        return g[:, None] * ctx.G, None  # z_vals: sample depths are constants of the step, as in the reference


def ray_distortion(weights, z_vals):
    """Distortion loss per ray [n] of weights, z_vals [n,S] (include/nb_hip.h: nb_ray_distortion), differentiable in `weights`:
    the forward's one kernel call also writes G = d loss / d weights, the backward returns g[:, None] * G."""
    if not torch.is_grad_enabled():
        return ray_distortion_raw(weights, z_vals, want_grad=False)[0]
    return _RayDistortion.apply(weights, z_vals)


def _mat(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or \
            (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        raise ValueError("%s must be a 2-D fp32 HIP tensor with unit column stride" % name)
    return t


def sgemm(a, b, trans_a=False, trans_b=False, out=None, alpha=1.0, beta=0.0, relu_mask=None, colsum=None):
    """nb_gemm_fused (fp32 MFMA kernels of libnb_hip.so): out[m,n] = alpha * op(a) @ op(b) + beta * out, row-major; a / b /
    out may be column slices of wider matrices (row stride = leading dimension).  Epilogues of the backward chain (not with
    trans_a): relu_mask [m, n] (slice allowed): out is zeroed where relu_mask <= 0; colsum [n]: += column sums of out."""
    _mat(a, "a")
    _mat(b, "b")
    m, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    k2, n = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if k != k2:
        raise ValueError("sgemm: inner dimensions %d vs %d" % (k, k2))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
        beta = 0.0
    _mat(out, "out")
    if tuple(out.shape) != (m, n):
        raise ValueError("sgemm: out is %s, expected %s" % (tuple(out.shape), (m, n)))
    ldy = 0
    if relu_mask is not None:
        _mat(relu_mask, "relu_mask")
        if tuple(relu_mask.shape) != (m, n):
            raise ValueError("sgemm: relu_mask is %s, expected %s" % (tuple(relu_mask.shape), (m, n)))
        ldy = relu_mask.stride(0)
    if colsum is not None:
        _req(colsum, torch.float32, (n,), "colsum")
    if (relu_mask is not None or colsum is not None) and trans_a:
        raise ValueError("sgemm: epilogues are not available for the weight-gradient form (trans_a)")
    check(_lib.lib().nb_gemm_fused(1 if trans_a else 0, 1 if trans_b else 0, m, n, k, float(alpha), ptr(a), a.stride(0), ptr(b),
                                   b.stride(0), float(beta), ptr(out), out.stride(0), ptr(relu_mask), ldy, ptr(colsum),
                                   _stream()), "nb_gemm_fused")
    return out


GEMM_VARIANTS = ("SCALE_ONLY", "TN", "TN16", "ROWS", "ROWS_FAST", "ROWS_FAST_T", "ROWS16")


def gemm_variant(a, b, trans_a=False, trans_b=False):
    """nb_gemm_variant: the kernel `sgemm(a, b, trans_a, trans_b)` launches, as a name of GEMM_VARIANTS (the enum's order);
    "SCALE_ONLY" = trans_a with k == 0.  Nothing is launched and nothing is read: only the shapes, the row strides and the
    alignment of the data pointers count, so host tensors do as well as device ones."""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("%s must be a 2-D fp32 tensor with unit column stride" % name)
    m, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    k2, n = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if k != k2:
        raise ValueError("gemm_variant: inner dimensions %d vs %d" % (k, k2))
    return GEMM_VARIANTS[int(_lib.lib().nb_gemm_variant(1 if trans_a else 0, 1 if trans_b else 0, m, n, k, ptr(a), a.stride(0),
                                                        ptr(b), b.stride(0)))]


def relu_bwd_(dy, y):
    """nb_relu_bwd in place: dy *= (y > 0); y is the post-activation value."""
    _req(dy, torch.float32, None, "dy")
    _req(y, torch.float32, tuple(dy.shape), "y")
    check(_lib.lib().nb_relu_bwd(ptr(dy), ptr(y), dy.numel(), _stream()), "nb_relu_bwd")
    return dy


def colsum(x, out=None):
    """nb_colsum: out[c] += sum_r x[r, c] (x may be a column slice)."""
    _mat(x, "x")
    if out is None:
        out = torch.zeros(x.shape[1], dtype=torch.float32, device=x.device)
    _req(out, torch.float32, (x.shape[1],), "out")
    check(_lib.lib().nb_colsum(ptr(x), x.shape[0], x.shape[1], x.stride(0), ptr(out), _stream()), "nb_colsum")
    return out


def trilinear_bwd(scene, grids, drows, wpts, d_feat, run_length=1):
    """nb_trilinear_bwd: d_feat [n,352] -> drows[l] += gradient of the active rows of level l.  run_length: the points come as
    runs of that many consecutive samples of one ray (contributions to one voxel are pre-summed along a run)."""
    sc, _keep = scene
    _req(wpts, torch.float32, (None, 3), "wpts")
    n = wpts.shape[0]
    _req(d_feat, torch.float32, (n, 352), "d_feat")
    g4 = (C.c_void_p * 4)()
    d4 = (C.c_void_p * 4)()
    for l in range(4):
        _req(grids[l], torch.int32, tuple(int(v) for v in sc.vol_dhw[l]), "grid[%d]" % l)
        _req(drows[l], torch.float32, (None, LEVEL_CHANNELS[l]), "drows[%d]" % l)
        g4[l] = grids[l].data_ptr()
        d4[l] = drows[l].data_ptr()
    check(_lib.lib().nb_trilinear_bwd(C.byref(sc), g4, d4, ptr(wpts), ptr(d_feat), n, int(run_length), _stream()),
          "nb_trilinear_bwd")
    return drows


def trilinear_grad(scene, grids, rows, wpts, d_feat, out=None):
    """nb_trilinear_grad: d_feat [n,352] -> grad [n,3] = d/dp sum_c d_feat[p,c] F_c(p) in world axes; rows[l]: the ACTIVE rows of
    level l, compact [>= every id grids[l] holds, C_l] (the scene's dense volumes are not read)."""
    sc, _keep = scene
    _req(wpts, torch.float32, (None, 3), "wpts")
    n = wpts.shape[0]
    _req(d_feat, torch.float32, (n, 352), "d_feat")
    dev = wpts.device
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _req(out, torch.float32, (n, 3), "grad")
    g4 = (C.c_void_p * 4)()
    r4 = (C.c_void_p * 4)()
    for l in range(4):
        _req(grids[l], torch.int32, tuple(int(v) for v in sc.vol_dhw[l]), "grid[%d]" % l)
        _req(rows[l], torch.float32, (None, LEVEL_CHANNELS[l]), "rows[%d]" % l)
        g4[l] = grids[l].data_ptr()
        r4[l] = rows[l].data_ptr()
    for t, name in [(d_feat, "d_feat"), (out, "grad")] + [(x, "grids / rows") for x in list(grids) + list(rows)]:
        if t.device != dev:
            raise ValueError("trilinear_grad: %s lives on %s, wpts on %s" % (name, t.device, dev))
    with torch.cuda.device(dev):
        check(_lib.lib().nb_trilinear_grad(C.byref(sc), g4, r4, ptr(wpts), ptr(d_feat), n, ptr(out), _stream()), "nb_trilinear_grad")
    return out


def _march_rays(ray_o, ray_d, near, far, t_vals, t_rand, weights):
    _req(ray_o, torch.float32, (None, 3), "ray_o")
    n = ray_o.shape[0]
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    _req(near, torch.float32, (n,), "near")
    _req(far, torch.float32, (n,), "far")
    _req(t_vals, torch.float32, (None,), "t_vals")
    S = t_vals.shape[0]
    if t_rand is not None:
        _req(t_rand, torch.float32, (n, S), "t_rand")
    _req(weights, torch.float32, (n, S), "weights")
    if n * S >= 2 ** 31 - 256:
        raise ValueError("%d rays x %d samples: the sample list holds fewer than 2^31 - 256" % (n, S))
    return n, S


def normal_select(ray_o, ray_d, near, far, t_vals, t_rand, weights, w_min, idx=None, wpts=None, scratch=None, n_out=None):
    """nb_normal_select: the samples of a marched view with weights >= w_min, in (ray, sample) order, into idx [cap] int32
    (= ray * S + s) and wpts [cap,3] fp32 (their positions by the march's own steps); both None: count only -> n_out, a [2] int32
    device tensor {min(total, cap), total}; nothing is read back."""
    n, S = _march_rays(ray_o, ray_d, near, far, t_vals, t_rand, weights)
    dev = ray_o.device
    if (wpts is None) != (idx is None):
        raise ValueError("wpts and idx come together")
    cap = 0
    if wpts is not None:
        _req(wpts, torch.float32, (None, 3), "wpts")
        cap = min(int(wpts.shape[0]), 2 ** 31 - 1)
        _req(idx, torch.int32, (int(wpts.shape[0]),), "idx")
    if n_out is None:
        n_out = torch.zeros(2, dtype=torch.int32, device=dev)  # (a view without samples launches nothing: the count is 0)
    _req(n_out, torch.int32, (2,), "n_out")
    if scratch is None:
        scratch = scan_scratch(max(n * S, 1), dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_normal_select(ptr(ray_o), ptr(ray_d), ptr(near), ptr(far), n, S, ptr(t_vals), ptr(t_rand), ptr(weights),
                                          float(w_min), cap, ptr(idx), ptr(wpts), ptr(n_out), ptr(scratch), _stream()),
              "nb_normal_select")
    return n_out


def normal_composite(idx, grad, weights, normal_map=None, normal_acc=None):
    """nb_normal_composite: idx [m] int32 (normal_select's, ascending), grad [m,3] = d sigma / dp of those samples, weights [n,S]
    -> (normal_map [n,3]: unit or zero, normal_acc [n]: the selected samples' weight); every ray is written."""
    _req(weights, torch.float32, (None, None), "weights")
    n, S = weights.shape
    _req(idx, torch.int32, (None,), "idx")
    m = idx.shape[0]
    _req(grad, torch.float32, (m, 3), "grad")
    dev = weights.device
    if normal_map is None:
        normal_map = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if normal_acc is None:
        normal_acc = torch.empty((n,), dtype=torch.float32, device=dev)
    _req(normal_map, torch.float32, (n, 3), "normal_map")
    _req(normal_acc, torch.float32, (n,), "normal_acc")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_normal_composite(ptr(idx), ptr(grad), m, ptr(weights), n, S, ptr(normal_map), ptr(normal_acc), _stream()),
              "nb_normal_composite")
    return normal_map, normal_acc


# ------------------------------------------------------------------------------------------- hierarchical sampling
IMPORTANCE_MAX, MERGED_MAX = 128, 512  # nb_importance_sample / nb_importance_merge: n_importance, n_samples + n_importance


def importance_sample(ray_o, ray_d, near, far, t_vals, t_rand, weights, u, cull=None, pose=None, want_z_coarse=True):
    """nb_importance_sample: the importance depths of every ray from the coarse pass's weights [n,S] (sample_pdf, nerf_net_utils.py:55-90,
    on the midpoints of the march's own depths).  u [N] (shared by all rays: linspace(0, 1, N)) or [n,N] (per ray).  cull: the
    (NbCull, keepalive) of make_cull — the result then carries keep [n,N] uint8; pose: the 15-float block of make_pose (needed by a
    pre_affine cull only).  -> dict z_fine [n,N], wpts / viewdir [n,N,3], z_std [n], z_coarse [n,S] (unless want_z_coarse is False),
    keep or None."""
    n, S = _march_rays(ray_o, ray_d, near, far, t_vals, t_rand, weights)
    if u.dim() not in (1, 2):
        raise ValueError("u is [N] or [n, N], got %s" % (tuple(u.shape),))
    N = int(u.shape[-1])
    _req(u, torch.float32, (N,) if u.dim() == 1 else (n, N), "u")
    dev = ray_o.device
    out = {"z_fine": torch.empty((n, N), dtype=torch.float32, device=dev),
           "wpts": torch.empty((n, N, 3), dtype=torch.float32, device=dev),
           "viewdir": torch.empty((n, N, 3), dtype=torch.float32, device=dev),
           "z_std": torch.empty((n,), dtype=torch.float32, device=dev),
           "z_coarse": torch.empty((n, S), dtype=torch.float32, device=dev) if want_z_coarse else None,
           "keep": torch.empty((n, N), dtype=torch.uint8, device=dev) if cull is not None else None}
    if pose is not None:
        _req(pose, torch.float32, (15,), "pose")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_importance_sample(ptr(ray_o), ptr(ray_d), ptr(near), ptr(far), n, S, ptr(t_vals), ptr(t_rand), ptr(weights),
                                              N, ptr(u), 1 if u.dim() == 2 else 0, C.byref(cull[0]) if cull is not None else None,
                                              ptr(pose), ptr(out["z_coarse"]), ptr(out["z_fine"]), ptr(out["wpts"]), ptr(out["viewdir"]),
                                              ptr(out["keep"]), ptr(out["z_std"]), _stream()), "nb_importance_sample")
    return out


def importance_merge(z_coarse, raw_coarse, z_fine, raw_fine, keep=None):
    """nb_importance_merge: z_coarse [n,S] + raw_coarse [n,S,4] and z_fine [n,N] + raw_fine [n,N,4] -> (z_vals [n,S+N], raw [n,S+N,4])
    sorted by depth, stable (coarse before fine at equal depth); raw = 0 for fine samples with keep [n,N] uint8 == 0."""
    _req(z_coarse, torch.float32, (None, None), "z_coarse")
    n, S = z_coarse.shape
    _req(raw_coarse, torch.float32, (n, S, 4), "raw_coarse")
    _req(z_fine, torch.float32, (n, None), "z_fine")
    N = int(z_fine.shape[1])
    _req(raw_fine, torch.float32, (n, N, 4), "raw_fine")
    if keep is not None:
        _req(keep, torch.uint8, (n, N), "keep")
    dev = z_coarse.device
    z_vals = torch.empty((n, S + N), dtype=torch.float32, device=dev)
    raw = torch.empty((n, S + N, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_importance_merge(ptr(z_coarse), ptr(raw_coarse), ptr(z_fine), ptr(raw_fine), ptr(keep), n, S, N, ptr(z_vals),
                                             ptr(raw), _stream()), "nb_importance_merge")
    return z_vals, raw


class ZeroArena:
    """One zero fill for everything a pass accumulates into (atomics, column sums, scatter targets): `take(shape, dtype)` hands
    out views of a single torch.zeros buffer sized by a planning pass over the same requests (`ZeroArena.plan()` counts)."""

    def __init__(self, n_bytes, device):
        self.buf = torch.zeros((int(n_bytes) + 7) // 8, dtype=torch.float64, device=device).view(torch.uint8)
        self.slack = self.buf.numel() - int(n_bytes)  # rounding of the buffer to whole doubles
        self.off = 0

    @staticmethod
    def size_of(requests):
        return sum((math.prod(shape) * torch.empty((), dtype=dt).element_size() + 15) // 16 * 16 for shape, dt in requests)

    def take(self, shape, dtype=torch.float32):
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        if self.off + n > self.buf.numel():
            raise RuntimeError("ZeroArena exhausted: planned %d bytes, asked for %d more at %d" % (self.buf.numel(), n, self.off))
        t = self.buf[self.off:self.off + n].view(dtype).view(shape)
        self.off += (n + 15) // 16 * 16
        return t


def enc_bn_relu_bwd(dy, y, x, n_rows, n_rows_max, batch_stats, eps, gamma, want_split=False, sums=None):
    """nb_enc_bn_relu_bwd -> (dx, dgamma, dbeta) or, with want_split, (dx, dgamma, dbeta, dx_split int16 [2, rows, C]: dx as bf16
    head / remainder planes for the backward-input convolution on the matrix pipe)."""
    c = int(x.shape[1])
    for t, nm in ((dy, "dy"), (y, "y"), (x, "x")):
        _req(t, torch.float32, (None, c), nm)
    _req(batch_stats, torch.float32, (2 * c + 1,), "batch_stats")
    _req(gamma, torch.float32, (c,), "gamma")
    dev = x.device
    zeroed = sums is not None  # a ZeroArena view: the call's own memset is skipped
    if sums is None:
        sums = torch.empty(2 * c, dtype=torch.float64, device=dev)
    _req(sums, torch.float64, (2 * c,), "sums")
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    split = torch.empty((2, max(int(n_rows_max), 1), c), dtype=torch.int16, device=dev) if want_split else None
    check(_lib.lib().nb_enc_bn_relu_bwd(ptr(dy), ptr(y), ptr(x), ptr(n_rows), int(n_rows_max), c, ptr(batch_stats),
                                        float(eps), ptr(gamma), ptr(sums), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(split),
                                        1 if zeroed else 0, _stream()), "nb_enc_bn_relu_bwd")
    return (dx, dgamma, dbeta, split) if want_split else (dx, dgamma, dbeta)


def enc_conv_bwd_input(dx, out_grid, out_dhw, in_lin, n_in, n_in_max, in_dhw, stride, weight, out=None):
    """nb_enc_conv_bwd_input -> din [n_in_max, Cin]; out: a ZEROED buffer of that shape (ZeroArena), default torch.zeros."""
    cin, cout = int(weight.shape[3]), int(weight.shape[4])
    _req(dx, torch.float32, (None, cout), "dx")
    _req(out_grid, torch.int32, tuple(int(s) for s in out_dhw), "out_grid")
    _req(in_lin, torch.int32, (None,), "in_lin")
    din = out if out is not None else torch.zeros((max(int(n_in_max), 1), cin), dtype=torch.float32, device=dx.device)
    _req(din, torch.float32, (max(int(n_in_max), 1), cin), "din")
    check(_lib.lib().nb_enc_conv_bwd_input(ptr(dx), ptr(out_grid), _i3(out_dhw), ptr(in_lin), ptr(n_in), int(n_in_max),
                                           _i3(in_dhw), int(stride), ptr(weight), cin, cout, ptr(din), _stream()),
          "nb_enc_conv_bwd_input")
    return din


def enc_conv_bwd_weight(in_rows, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, dx, cin, cout, dx_split=None, out=None,
                        rulebook=None):
    """nb_enc_conv_bwd_weight -> dW [3,3,3,Cin,Cout].  dx_split (int16 [2, n_out_max, Cout], enc_bn_relu_bwd(want_split=True)):
    the product runs on the 16-bit matrix pipe with bf16 pairs (Cin >= 32)."""
    _req(in_rows, torch.float32, (None, cin), "in_rows")
    _req(dx, torch.float32, (None, cout), "dx")
    if dx_split is not None:
        _req(dx_split, torch.int16, (2, max(int(n_out_max), 1), cout), "dx_split")
    zeroed = out is not None  # a ZeroArena view: the call's own memset is skipped
    dw = out if zeroed else torch.empty((3, 3, 3, cin, cout), dtype=torch.float32, device=dx.device)
    _req(dw, torch.float32, (3, 3, 3, cin, cout), "dweight")
    # rulebook: a one-element list cache shared by the layers of one (input grid, output rows, stride): the first call fills it,
    # the others reuse the neighbour table (the three submanifold layers of a level have the same one)
    ready = rulebook is not None and len(rulebook) == 1
    rb = rulebook[0] if ready else torch.empty(max(int(n_out_max), 1) * 27, dtype=torch.int32, device=dx.device)
    _req(rb, torch.int32, (max(int(n_out_max), 1) * 27,), "rulebook")
    check(_lib.lib().nb_enc_conv_bwd_weight(ptr(in_rows), ptr(in_grid), _i3(in_dhw), ptr(out_lin), ptr(n_out),
                                            int(n_out_max), _i3(out_dhw), int(stride), ptr(dx), ptr(dx_split), cin, cout,
                                            ptr(dw), ptr(rb), (1 if zeroed else 0) | (2 if ready else 0), _stream()),
          "nb_enc_conv_bwd_weight")
    if rulebook is not None and not ready:
        rulebook.append(rb)
    return dw


def enc_scatter_codes_bwd(drows, rows_vert, n_rows, n_rows_max, n_codes, out=None):
    c = int(drows.shape[1])
    dcodes = out if out is not None else torch.zeros((n_codes, c), dtype=torch.float32, device=drows.device)
    _req(dcodes, torch.float32, (n_codes, c), "dcodes")
    check(_lib.lib().nb_enc_scatter_codes_bwd(ptr(drows), ptr(rows_vert), ptr(n_rows), int(n_rows_max), c, ptr(dcodes),
                                              _stream()), "nb_enc_scatter_codes_bwd")
    return dcodes


def _cull_cams(RT, K, nv):
    """The [nv,21] fp32 camera block of nb_cull and nb_smpl_silhouette: per view RT's 12 floats | K's 9."""
    if not 1 <= nv <= 64:
        raise ValueError("1..64 mask views supported, got %d" % nv)
    cam = torch.cat([RT.detach().reshape(nv, 12).float(), K.detach().reshape(nv, 9).float()], 1).contiguous()
    return _req(cam, torch.float32, (nv, 21), "cam")


def make_cull(masks, RT, K, R0=None, Th0=None):
    """nb_cull from DEVICE tensors: masks [n_views,H,W] uint8 (non-zero = inside), RT [n_views,3,4], K [n_views,3,3]
    (batch['msks'][0], batch['RT'][0], batch['Ks'][0]); R0 [3,3] / Th0 [3] select the _msk variant (snapshot-frame
    placement).  Nothing visits the host.  Returns (NbCull, keepalive)."""
    masks = masks if masks.dtype == torch.uint8 else masks.to(torch.uint8)
    masks = masks.contiguous()
    _req(masks, torch.uint8, (None, None, None), "masks")
    nv, H, W = (int(v) for v in masks.shape)
    cam = _cull_cams(RT, K, nv)
    c = NbCull()
    c.n_views, c.H, c.W = nv, H, W
    c.pre_affine = 0 if R0 is None else 1
    c.msk = masks.data_ptr()
    c.cam = cam.data_ptr()
    keep = [masks, cam]
    if R0 is not None:
        snap = torch.cat([R0.detach().reshape(9).float(), Th0.detach().reshape(-1)[:3].float()]).contiguous()
        _req(snap, torch.float32, (12,), "snap")
        c.snap = snap.data_ptr()
        keep.append(snap)
    return c, keep


# ------------------------------------------------------------------------------------------- the mesh pass's query lattice
def _lattice(axes):
    """(ax, ay, az) device fp32 vectors -> (dims, number of points); ValueError for lattices the calls refuse."""
    if len(axes) != 3:
        raise ValueError("a lattice is three axis vectors, got %d" % len(axes))
    for name, a in zip(("axis_x", "axis_y", "axis_z"), axes):
        _req(a, torch.float32, (None,), name)
    dims = [int(a.shape[0]) for a in axes]
    n = dims[0] * dims[1] * dims[2]
    if min(dims) < 1 or n > 2 ** 31 - 1:
        raise ValueError("lattice %s: every side >= 1 and at most 2^31 - 1 points" % (dims,))
    if len(set(a.device for a in axes)) != 1:
        raise ValueError("the three axes live on different devices")
    return dims, n


def lattice_scratch(dims, device):
    """Scratch of lattice_carve / lattice_gather for an [X,Y,Z] lattice."""
    return scan_scratch(int(dims[0]) * int(dims[1]) * int(dims[2]), device)


def _window(entry, stack, name, border, out, in_place=None):
    """nb_mask_dilate / nb_mask_band of a device uint8 [V,H,W] stack called `name` -> a new [V,H,W]; in_place: the ValueError text
    for out = the stack (None: left to the library)."""
    _req(stack, torch.uint8, (None, None, None), name)
    border = int(border)
    if border < 1 or border % 2 == 0 or border > 255:
        raise ValueError("border must be odd, 1..255, got %d" % border)
    if stack.numel() == 0:
        raise ValueError("%s is empty: %s" % (name, tuple(stack.shape)))
    if out is None:
        out = torch.empty_like(stack)
    _req(out, torch.uint8, tuple(stack.shape), "out")
    if in_place and out.data_ptr() == stack.data_ptr():
        raise ValueError(in_place)
    with torch.cuda.device(stack.device):
        check(getattr(_lib.lib(), entry)(ptr(stack), *stack.shape, border, ptr(out), _stream()), entry)
    return out


def mask_dilate(masks, border=5, out=None):
    """nb_mask_dilate: cv2.dilate(m, ones((border, border))) of every mask of a device uint8 [V,H,W] stack -> a new [V,H,W]."""
    return _window("nb_mask_dilate", masks, "masks", border, out)


def lattice_carve(axes, cull, scratch=None, inside=None, n_inside=None):
    """nb_lattice_carve: axes = (ax [X], ay [Y], az [Z]) device fp32, cull = the NbCull of make_cull (whose keepalive the caller
    holds) -> (inside [X,Y,Z] uint8, n_inside [1] int32), device tensors; nothing is read back."""
    dims, n = _lattice(axes)
    dev = axes[0].device
    if not isinstance(cull, NbCull):
        raise TypeError("cull must be the NbCull of ops.make_cull")
    if inside is None:
        inside = torch.empty(dims, dtype=torch.uint8, device=dev)
    if n_inside is None:
        n_inside = torch.empty(1, dtype=torch.int32, device=dev)
    _req(inside, torch.uint8, tuple(dims), "inside")
    _req(n_inside, torch.int32, (1,), "n_inside")
    if scratch is None:
        scratch = lattice_scratch(dims, dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_lattice_carve(ptr(axes[0]), ptr(axes[1]), ptr(axes[2]), _i3(dims), C.byref(cull), ptr(inside),
                                          ptr(n_inside), ptr(scratch), _stream()), "nb_lattice_carve")
    return inside, n_inside


def lattice_gather(axes, inside, wpts=None, lin=None, scratch=None, n_out=None):
    """nb_lattice_gather: the flagged points of a device uint8 bitmap [X,Y,Z] in linear order into wpts [cap,3] fp32 and
    lin [cap] int32 (both None: count only) -> n_out, a [2] int32 device tensor {min(total, cap), total}; nothing is read back."""
    dims, n = _lattice(axes)
    dev = axes[0].device
    _req(inside, torch.uint8, tuple(dims), "inside")
    if (wpts is None) != (lin is None):
        raise ValueError("wpts and lin come together")
    cap = 0
    if wpts is not None:
        _req(wpts, torch.float32, (None, 3), "wpts")
        cap = min(int(wpts.shape[0]), 2 ** 31 - 1)
        _req(lin, torch.int32, (int(wpts.shape[0]),), "lin")
    if n_out is None:
        n_out = torch.empty(2, dtype=torch.int32, device=dev)
    _req(n_out, torch.int32, (2,), "n_out")
    if scratch is None:
        scratch = lattice_scratch(dims, dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_lattice_gather(ptr(axes[0]), ptr(axes[1]), ptr(axes[2]), _i3(dims), ptr(inside), cap, ptr(wpts),
                                           ptr(lin), ptr(n_out), ptr(scratch), _stream()), "nb_lattice_gather")
    return n_out


def lattice_scatter(alpha, lin, dims, pad, cube=None):
    """nb_lattice_scatter: alpha (device fp32 with n elements along ONE dimension, any stride: the [1,n,1] of calculate_density,
    or a column of a wider tensor) at the lattice points lin [n] int32 -> cube [X+2*pad, Y+2*pad, Z+2*pad] fp32, 0 elsewhere
    (a `cube` of the caller's must be zeroed)."""
    if _on_device(alpha, "alpha").dtype != torch.float32:
        raise ValueError("alpha must be torch.float32, got %s" % (alpha.dtype,))
    _req(lin, torch.int32, (None,), "lin")
    n = int(lin.shape[0])
    long_dims = [d for d in range(alpha.dim()) if alpha.shape[d] != 1]
    if alpha.numel() != n or len(long_dims) > 1:
        raise ValueError("alpha has shape %s, expected %d elements along one dimension" % (tuple(alpha.shape), n))
    stride = int(alpha.stride(long_dims[0])) if long_dims else 1
    if stride < 1:
        raise ValueError("alpha has stride %d" % stride)
    dims, pad = [int(d) for d in dims], int(pad)
    shape = tuple(d + 2 * pad for d in dims)
    if cube is None:
        cube = torch.zeros(shape, dtype=torch.float32, device=alpha.device)
    _req(cube, torch.float32, shape, "cube")
    with torch.cuda.device(alpha.device):
        check(_lib.lib().nb_lattice_scatter(ptr(alpha), stride, ptr(lin), n, _i3(dims), pad, ptr(cube), _stream()),
              "nb_lattice_scatter")
    return cube


# ------------------------------------------------------------------------------------------- a frame's geometry from SMPL parameters
SMPL_MODEL_SHAPES = {"v_template": (None, 3), "shapedirs": (_lib.SMPL_BETAS, None), "posedirs": (_lib.SMPL_POSE_BASIS, None),
                     "weights": (_lib.SMPL_JOINTS, None), "j_template": (_lib.SMPL_JOINTS, 3),
                     "j_shapedirs": (_lib.SMPL_JOINTS, 3, _lib.SMPL_BETAS)}


def make_smpl_model(arrays, parents):
    """The nb_smpl_model of device fp32 arrays laid out as include/nb_hip.h says: v_template [V,3], shapedirs [10,3V], posedirs
    [207,3V] (or None: a model for new_params = False only), weights [24,V], j_template [24,3], j_shapedirs [24,3,10], and the
    host list `parents` [24] -> (NbSmplModel, keepalive list)."""
    V = int(_req(arrays["v_template"], torch.float32, (None, 3), "v_template").shape[0])
    if V < 1:
        raise ValueError("the model has no vertices")
    m, keep = NbSmplModel(), []
    for name, shape in SMPL_MODEL_SHAPES.items():
        t = arrays.get(name)
        if t is None and name == "posedirs":
            continue
        shape = tuple(3 * V if s is None and name in ("shapedirs", "posedirs") else V if s is None else s for s in shape)
        _req(t, torch.float32, shape, name)
        if t.device != arrays["v_template"].device:
            raise ValueError("%s lives on %s, v_template on %s" % (name, t.device, arrays["v_template"].device))
        setattr(m, name, t.data_ptr())
        keep.append(t)
    parents = [int(v) for v in parents]
    if len(parents) != _lib.SMPL_JOINTS or parents[0] != -1 or any(not 0 <= pa < j for j, pa in enumerate(parents) if j > 0):
        raise ValueError("parents must be %d entries with parents[0] = -1 and 0 <= parents[j] < j, got %s" % (_lib.SMPL_JOINTS, parents))
    m.n_verts = V
    m.parents[:] = parents
    return m, keep


def smpl_pose(model, params, new_params=False, verts=None, joints=None, ws=None):
    """nb_smpl_pose: model = the NbSmplModel of make_smpl_model (whose keepalive the caller holds), params device fp32 [F,88]
    (poses 72 | shapes 10 | Rh 3 | Th 3 per frame) -> (verts [F,V,3], joints [F,24,3]) device fp32; nothing is read back."""
    if not isinstance(model, NbSmplModel):
        raise TypeError("model must be the NbSmplModel of ops.make_smpl_model")
    _req(params, torch.float32, (None, _lib.SMPL_PARAMS), "params")
    F, V, dev = int(params.shape[0]), int(model.n_verts), params.device
    if not 1 <= F <= 65535:
        raise ValueError("params holds %d frames (1 .. 65535 per call)" % F)
    if new_params and not model.posedirs:
        raise ValueError("new_params needs a model with posedirs")
    if verts is None:
        verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    if joints is None:
        joints = torch.empty((F, _lib.SMPL_JOINTS, 3), dtype=torch.float32, device=dev)
    if ws is None:
        ws = torch.empty((F, _lib.SMPL_WS_FLOATS), dtype=torch.float32, device=dev)
    _req(verts, torch.float32, (F, V, 3), "verts")
    _req(joints, torch.float32, (F, _lib.SMPL_JOINTS, 3), "joints")
    _req(ws, torch.float32, (F, _lib.SMPL_WS_FLOATS), "ws")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_smpl_pose(C.byref(model), ptr(params), F, 1 if new_params else 0, ptr(ws), ptr(verts), ptr(joints),
                                      _stream()), "nb_smpl_pose")
    return verts, joints


def _rows3(t, F, name):
    """A device fp32 [F,3] whose rows are contiguous (a column block of a wider row-major tensor included) -> its row stride."""
    _on_device(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != (F, 3) or t.stride(1) != 1 or (F > 1 and t.stride(0) < 3):
        raise ValueError("%s must be float32 [%d,3] with contiguous rows, got %s %s strides %s" % (name, F, t.dtype, tuple(t.shape),
                                                                                                t.stride()))
    return int(t.stride(0)) if F > 1 else 3


def smpl_voxelize(verts, Rh, Th, voxel_size, pad="zju"):
    """nb_smpl_voxelize: verts device fp32 [F,V,3] (world), Rh, Th device fp32 [F,3] (contiguous rows, one common row stride),
    voxel_size three Python floats (dhw), pad 'zju' | 'big_box' | 'snapshot' -> dict of device tensors coord [F,V,3] i32,
    out_sh [F,3] i32, bounds [F,2,3], R [F,3,3] and summary [F,9] i32 (can_bounds' six floats bit-cast | out_sh)."""
    _req(verts, torch.float32, (None, None, 3), "verts")
    F, V, dev = int(verts.shape[0]), int(verts.shape[1]), verts.device
    if F < 1 or V < 1:
        raise ValueError("verts is empty: %s" % (tuple(verts.shape),))
    s_rh, s_th = _rows3(Rh, F, "Rh"), _rows3(Th, F, "Th")
    if s_rh != s_th:
        raise ValueError("Rh and Th have different row strides (%d, %d)" % (s_rh, s_th))
    if Rh.device != dev or Th.device != dev:
        raise ValueError("verts, Rh and Th live on different devices")
    if pad not in _lib.PAD_MODES:
        raise ValueError("pad must be one of %s, got %r" % (sorted(_lib.PAD_MODES), pad))
    vs = [float(v) for v in voxel_size]
    if len(vs) != 3 or not all(0.0 < v < math.inf for v in vs):
        raise ValueError("voxel_size must be three positive floats, got %r" % (voxel_size,))
    out = {"coord": torch.empty((F, V, 3), dtype=torch.int32, device=dev), "out_sh": torch.empty((F, 3), dtype=torch.int32, device=dev),
           "bounds": torch.empty((F, 2, 3), dtype=torch.float32, device=dev), "R": torch.empty((F, 3, 3), dtype=torch.float32, device=dev),
           "summary": torch.empty((F, 9), dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        check(_lib.lib().nb_smpl_voxelize(ptr(verts), V, F, ptr(Rh), ptr(Th), s_rh, (C.c_double * 3)(*vs), _lib.PAD_MODES[pad],
                                          ptr(out["coord"]), ptr(out["out_sh"]), ptr(out["bounds"]), ptr(out["R"]),
                                          ptr(out["summary"]), _stream()), "nb_smpl_voxelize")
    return out


# ------------------------------------------------------------------------------------------- cull masks of a posed body
def _raster_scratch(entry, dims, device, refusal):
    n = int(getattr(_lib.lib(), entry)(*(int(d) for d in dims)))
    if n <= 0:  # dimensions the library refuses
        raise ValueError(refusal % dims)
    return torch.empty(n, dtype=torch.uint8, device=device)


def smpl_silhouette_scratch(F, V, Nf, nv, device):
    """Scratch of smpl_silhouette for F frames of V vertices and Nf triangles in nv views."""
    return _raster_scratch("nb_smpl_silhouette_scratch_size", (F, V, Nf, nv), device, "no silhouettes for F = %d, V = %d, Nf = %d, "
                           "nv = %d (F 1..65535, nv 1..64, F nv V and F nv Nf < 2^31)")


def _body_raster(entry, scratch_fn, out_dtype, out_tail, verts, faces, RT, K, H, W, out, scratch):
    """smpl_silhouette and body_depth_range: the posed body's triangles through the cull cameras into `out`, [F,nv,H,W] + out_tail."""
    _req(verts, torch.float32, (None, None, 3), "verts")
    _req(faces, torch.int32, (None, 3), "faces")
    F, V, Nf, dev = int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0]), verts.device
    H, W = int(H), int(W)
    if F < 1 or V < 1 or Nf < 1:
        raise ValueError("verts %s or faces %s is empty" % (tuple(verts.shape), tuple(faces.shape)))
    if not 1 <= H <= 32768 or not 1 <= W <= 32768:
        raise ValueError("H = %d, W = %d (1..32768)" % (H, W))
    _on_device(RT, "RT")
    nv = int(_on_device(K, "K").shape[0])
    if tuple(RT.shape) != (nv, 3, 4) or tuple(K.shape) != (nv, 3, 3):
        raise ValueError("RT %s, K %s: expected [%d,3,4] and [%d,3,3]" % (tuple(RT.shape), tuple(K.shape), nv, nv))
    if faces.device != dev or RT.device != dev or K.device != dev:
        raise ValueError("verts, faces, RT and K live on different devices")
    cam = _cull_cams(RT, K, nv)
    if scratch is None:
        scratch = scratch_fn(F, V, Nf, nv, dev)
    _req(scratch, torch.uint8, (None,), "scratch")
    if out is None:
        out = torch.empty((F, nv, H, W) + out_tail, dtype=out_dtype, device=dev)
    _req(out, out_dtype, (F, nv, H, W) + out_tail, "out")
    with torch.cuda.device(dev):
        check(getattr(_lib.lib(), entry)(ptr(verts), ptr(faces), ptr(cam), F, V, Nf, nv, H, W, ptr(scratch), int(scratch.numel()),
                                         ptr(out), _stream()), entry)
    return out


def smpl_silhouette(verts, faces, RT, K, H, W, out=None, scratch=None):
    """nb_smpl_silhouette: verts device fp32 [F,V,3] (world), faces device int32 [Nf,3] (indices 0..V-1, validated where the list
    is made: SmplModel), RT [nv,3,4], K [nv,3,3] device tensors (the cull cameras, as make_cull takes them), H, W the mask size
    -> device uint8 [F,nv,H,W], 1 where the body's triangles meet the pixel; nothing is read back."""
    return _body_raster("nb_smpl_silhouette", smpl_silhouette_scratch, torch.uint8, (), verts, faces, RT, K, H, W, out, scratch)


# ------------------------------------------------------------------------------------------- ray bounds from the posed body
def body_depth_range_scratch(F, V, Nf, nv, device):
    """Scratch of body_depth_range for F frames of V vertices and Nf triangles in nv views."""
    return _raster_scratch("nb_body_depth_range_scratch_size", (F, V, Nf, nv), device, "no depth ranges for F = %d, V = %d, Nf = %d, "
                           "nv = %d (F 1..65535, nv 1..64, F nv V and F nv Nf < 2^31)")


def body_depth_range(verts, faces, RT, K, H, W, out=None, scratch=None):
    """nb_body_depth_range: the arguments of smpl_silhouette -> device fp32 [F,nv,H,W,2], per pixel the smallest and the largest
    camera depth of the vertices of the triangles that meet it: (+inf, -inf) where none does, (-inf, +inf) all over a view that does
    not bound (a vertex nearer than 0.01 m or projecting beyond 32768 px); nothing is read back."""
    return _body_raster("nb_body_depth_range", body_depth_range_scratch, torch.float32, (2,), verts, faces, RT, K, H, W, out, scratch)


def depth_range_widen(ranges, border=1, tile=1, out=None):
    """nb_depth_range_widen: device fp32 [...,H,W,2] depth ranges (no NaN) -> a new tensor of the same shape: every pixel takes the
    min of the lower and the max of the upper ends over its border x border window (odd, 1..255; outside the image ignored), then
    every aligned tile x tile block (1, 2, 4, 8 or 16; origin pixel (0, 0)) the min / max over its pixels."""
    _req(ranges, torch.float32, name="ranges")
    if ranges.dim() < 3 or ranges.shape[-1] != 2 or ranges.numel() == 0:
        raise ValueError("ranges must be a non-empty [...,H,W,2], got %s" % (tuple(ranges.shape),))
    border, tile = int(border), int(tile)
    if border < 1 or border % 2 == 0 or border > 255:
        raise ValueError("border must be odd, 1..255, got %d" % border)
    if tile not in (1, 2, 4, 8, 16):
        raise ValueError("tile must be 1, 2, 4, 8 or 16, got %d" % tile)
    H, W = int(ranges.shape[-3]), int(ranges.shape[-2])
    if out is None:
        out = torch.empty_like(ranges)
    _req(out, torch.float32, tuple(ranges.shape), "out")
    if out.data_ptr() == ranges.data_ptr():
        raise ValueError("out must be another tensor than ranges")
    with torch.cuda.device(ranges.device):
        check(_lib.lib().nb_depth_range_widen(ptr(ranges), ranges.numel() // (2 * H * W), H, W, border, tile, ptr(out), _stream()),
              "nb_depth_range_widen")
    return out


def raygen_body(H, W, K, R, T, bounds, depth_range, margin=0.0):
    """nb_raygen_body: raygen's host arguments, depth_range device fp32 [H,W,2] (body_depth_range of the SAME camera, widened) and
    margin in metres: near = max(near, range0 - margin), far = min(far, range1 + margin), a pixel kept iff raygen keeps it and
    near < far.  K's last row must be (0, 0, 1).  Returns raygen's 6-tuple on depth_range's device."""
    H, W = int(H), int(W)
    _req(depth_range, torch.float32, (H, W, 2), "depth_range")
    device = depth_range.device
    cam = _host_cam(K, R, T, bounds)
    out, scratch = _raygen_buffers(H * W, device)
    with torch.cuda.device(device):
        check(_lib.lib().nb_raygen_body(H, W, *cam, ptr(depth_range), float(margin), *(ptr(t) for t in out), ptr(scratch), _stream()),
              "nb_raygen_body")
    return out


# ------------------------------------------------------------------------------------------- pictures of an extracted mesh
MESH_CAM_FLOATS = 24  # NB_MESH_CAM_FLOATS: affine 3 x 4 | normal rotation 3 x 3 | 3 of padding


def mesh_vertex_normals(vertices, triangles, out=None, scratch=None):
    """nb_mesh_vertex_normals: vertices device fp32 [V,3], triangles device int32 [T,3] (a face with an index outside 0..V-1 is
    skipped) -> device fp32 [V,3], compute_normal of tools/render_mesh.py:32-51 with order-independent sums; a vertex no face
    uses gets (0,0,0).  scratch: the [V,3] int32 accumulator (allocated when None; a dirty one is fine).  Nothing is read back."""
    _req(vertices, torch.float32, (None, 3), "vertices")
    _req(triangles, torch.int32, (None, 3), "triangles")
    V, T, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    if triangles.device != dev:
        raise ValueError("vertices and triangles live on different devices")
    if scratch is None:
        scratch = torch.empty((V, 3), dtype=torch.int32, device=dev)
    _req(scratch, torch.int32, (V, 3), "scratch")
    if out is None:
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    _req(out, torch.float32, (V, 3), "out")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_vertex_normals(ptr(vertices), ptr(triangles), V, T, ptr(scratch), ptr(out), _stream()),
              "nb_mesh_vertex_normals")
    return out


def mesh_render_scratch(n_views, H, W, T, device):
    """Scratch of mesh_render for n_views pictures of H x W pixels of T triangles."""
    return _raster_scratch("nb_mesh_render_scratch_size", (n_views, H, W, T), device, "no pictures for n_views = %d, H = %d, W = %d, "
                           "T = %d (n_views >= 1, H, W 1..32768, n_views H W and n_views T < 2^31 - 256)")


def mesh_render(vertices, normals, triangles, cams, H, W, out=None, want_face_id=False, want_depth=False, scratch=None,
                face_id=None, depth=None, _entry="nb_mesh_render"):
    """nb_mesh_render: vertices, normals device fp32 [V,3], triangles device int32 [T,3], cams device fp32 [n,24] (per view the
    3 x 4 affine to (x_px, y_px, depth) | the 3 x 3 rotation of the normals | 3 of padding: mesh_render.turntable_cams) ->
    rgb device fp32 [n,H,W,3], white where nothing is drawn; with want_face_id and / or want_depth a tuple (rgb[, face_id int32
    [n,H,W], -1 = background][, depth fp32 [n,H,W], +inf = background]); `face_id` / `depth` are buffers to fill for them (wanted
    when given).  Nothing is read back."""
    _req(vertices, torch.float32, (None, 3), "vertices")
    V, dev = int(vertices.shape[0]), vertices.device
    _req(normals, torch.float32, (V, 3), "normals")
    _req(triangles, torch.int32, (None, 3), "triangles")
    _req(cams, torch.float32, (None, MESH_CAM_FLOATS), "cams")
    T, n, H, W = int(triangles.shape[0]), int(cams.shape[0]), int(H), int(W)
    if normals.device != dev or triangles.device != dev or cams.device != dev:
        raise ValueError("vertices, normals, triangles and cams live on different devices")
    if n < 1:
        raise ValueError("cams holds no view")
    if V < 1:
        T = 0  # nothing a face could index: every face would be skipped
    if scratch is None:
        scratch = mesh_render_scratch(n, H, W, T, dev)
    _req(scratch, torch.uint8, (None,), "scratch")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
    _req(out, torch.float32, (n, H, W, 3), "out")
    if face_id is None and want_face_id:
        face_id = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    if depth is None and want_depth:
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    if face_id is not None:
        _req(face_id, torch.int32, (n, H, W), "face_id")
    if depth is not None:
        _req(depth, torch.float32, (n, H, W), "depth")
    with torch.cuda.device(dev):
        check(getattr(_lib.lib(), _entry)(ptr(vertices), ptr(normals), ptr(triangles), V, T, ptr(cams), n, H, W, ptr(out), ptr(face_id),
                                          ptr(depth), ptr(scratch), int(scratch.numel()), _stream()), _entry)
    extra = tuple(t for t in (face_id, depth) if t is not None)
    return (out,) + extra if extra else out


def mesh_render_attr(vertices, attr, triangles, cams, H, W, out=None, want_face_id=False, want_depth=False, scratch=None,
                     face_id=None, depth=None):
    """nb_mesh_render_attr: mesh_render with the vertex colours read from `attr`, device fp32 [V,3] (mesh_vertex_colors' rgb_f),
    instead of computed from normals; arguments, outputs and scratch as mesh_render.  Nothing is read back."""
    return mesh_render(vertices, attr, triangles, cams, H, W, out=out, want_face_id=want_face_id, want_depth=want_depth,
                       scratch=scratch, face_id=face_id, depth=depth, _entry="nb_mesh_render_attr")


# ------------------------------------------------------------------------------------------- an animatable mesh
def mesh_closest_scratch(V, Nf, device):
    """Scratch of mesh_closest against a surface of V vertices and Nf triangles."""
    return _raster_scratch("nb_mesh_closest_scratch_size", (V, Nf), device, "no closest-point query for V = %d, Nf = %d (each >= 1, "
                           "3 V and 3 Nf < 2^31 - 256)")


def mesh_closest(points, vertices, triangles, scratch=None, face=None, bary=None, dist2=None, exhaustive=False, count_tiles=False):
    """nb_mesh_closest: points device fp32 [P,3], vertices device fp32 [V,3], triangles device int32 [Nf,3] -> (face int32 [P],
    bary fp32 [P,3], dist2 fp32 [P]): the closest triangle over all of them (the lower index on a tie), the barycentric
    coordinates of the closest point and the squared distance; face = -1, bary = 0, dist2 = +inf for a non-finite point or a
    surface without a valid face.  `exhaustive`, `count_tiles`: for benchmarks (no tile skipped; mesh_closest_tile_counts reads
    the scratch afterwards).  Nothing is read back."""
    _req(points, torch.float32, (None, 3), "points")
    _req(vertices, torch.float32, (None, 3), "vertices")
    _req(triangles, torch.int32, (None, 3), "triangles")
    P, V, Nf, dev = int(points.shape[0]), int(vertices.shape[0]), int(triangles.shape[0]), points.device
    if vertices.device != dev or triangles.device != dev:
        raise ValueError("points, vertices and triangles live on different devices")
    if P < 1 or V < 1 or Nf < 1:
        raise ValueError("points %s, vertices %s or triangles %s is empty" % (tuple(points.shape), tuple(vertices.shape),
                                                                              tuple(triangles.shape)))
    if scratch is None:
        scratch = mesh_closest_scratch(V, Nf, dev)
    _req(scratch, torch.uint8, (None,), "scratch")
    face = torch.empty((P,), dtype=torch.int32, device=dev) if face is None else face
    bary = torch.empty((P, 3), dtype=torch.float32, device=dev) if bary is None else bary
    dist2 = torch.empty((P,), dtype=torch.float32, device=dev) if dist2 is None else dist2
    _req(face, torch.int32, (P,), "face")
    _req(bary, torch.float32, (P, 3), "bary")
    _req(dist2, torch.float32, (P,), "dist2")
    flags = (_lib.CLOSEST_EXHAUSTIVE if exhaustive else 0) | (_lib.CLOSEST_COUNT_TILES if count_tiles else 0)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_closest(ptr(points), ptr(vertices), ptr(triangles), P, V, Nf, flags, ptr(scratch), int(scratch.numel()),
                                         ptr(face), ptr(bary), ptr(dist2), _stream()), "nb_mesh_closest")
    return face, bary, dist2


def mesh_closest_tile_counts(scratch):
    """(tiles skipped, tiles met) of the last mesh_closest(count_tiles=True) on this scratch, summed over its waves (a read-back)."""
    c = scratch[32:48].view(torch.int64).cpu()
    return int(c[0]), int(c[1])


def mesh_rig_bind(model, params, ws, triangles, points, face, bary):
    """nb_mesh_rig_bind: model = the BODY's NbSmplModel, params device fp32 [88] and ws device fp32 [512]: the bind frame's rows of
    one smpl_pose call, triangles device int32 [Nf,3] the body's, points device fp32 [P,3] with face [P], bary [P,3] of
    mesh_closest against the posed body -> (weights [24,P], shapedirs [10,3P], v_template [P,3], status int32 [4] = unbound,
    degenerate, 0, 0), the rig's arrays in the layout of make_smpl_model.  Nothing is read back."""
    if not isinstance(model, NbSmplModel):
        raise TypeError("model must be the NbSmplModel of ops.make_smpl_model")
    _req(params, torch.float32, (_lib.SMPL_PARAMS,), "params")
    _req(ws, torch.float32, (_lib.SMPL_WS_FLOATS,), "ws")
    _req(triangles, torch.int32, (None, 3), "triangles")
    _req(points, torch.float32, (None, 3), "points")
    P, Nf, dev = int(points.shape[0]), int(triangles.shape[0]), points.device
    _req(face, torch.int32, (P,), "face")
    _req(bary, torch.float32, (P, 3), "bary")
    if P < 1 or Nf < 1:
        raise ValueError("points %s or triangles %s is empty" % (tuple(points.shape), tuple(triangles.shape)))
    if any(t.device != dev for t in (params, ws, triangles, face, bary)):
        raise ValueError("params, ws, triangles, points, face and bary live on different devices")
    weights = torch.empty((_lib.SMPL_JOINTS, P), dtype=torch.float32, device=dev)
    shapedirs = torch.empty((_lib.SMPL_BETAS, 3 * P), dtype=torch.float32, device=dev)
    v_template = torch.empty((P, 3), dtype=torch.float32, device=dev)
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_rig_bind(C.byref(model), ptr(params), ptr(ws), ptr(triangles), Nf, ptr(points), ptr(face), ptr(bary), P,
                                          ptr(weights), ptr(shapedirs), ptr(v_template), ptr(status), _stream()), "nb_mesh_rig_bind")
    return weights, shapedirs, v_template, status


# ------------------------------------------------------------------------------------------- the extracted mesh cleaned and coloured
MESH_HOOK_ROUNDS = 4  # NB_MESH_HOOK_ROUNDS


def _mesh(vertices, triangles, V=None):
    """(V, T, device) of a face list and, when given, the vertices it indexes."""
    _req(triangles, torch.int32, (None, 3), "triangles")
    if vertices is not None:
        _req(vertices, torch.float32, (None, 3), "vertices")
        if vertices.device != triangles.device:
            raise ValueError("vertices and triangles live on different devices")
        V = vertices.shape[0]
    return int(V), int(triangles.shape[0]), triangles.device


def mesh_clean_scratch(V, T, device):
    """The one scratch of mesh_components, mesh_component_select and mesh_compact for a mesh of V vertices and T triangles."""
    return _raster_scratch("nb_mesh_clean_scratch_size", (V, T), device, "no mesh clean-up for V = %d, T = %d (0..2^31 - 257)")


def _clean_scratch(scratch, V, T, dev):
    if scratch is None:
        scratch = mesh_clean_scratch(V, T, dev)
        scratch[:4].zero_()  # the give-up word, for a caller that starts behind mesh_components
    return _req(scratch, torch.uint8, (None,), "scratch")


def mesh_give_up(scratch):
    """The give-up word of a clean-up scratch as a device int32 [1] view: 0, or 1 when mesh_components could not finish."""
    return _req(scratch, torch.uint8, (None,), "scratch")[:4].view(torch.int32)


def mesh_components(triangles, n_vertices, out=None, scratch=None):
    """nb_mesh_components: triangles device int32 [T,3] over n_vertices vertices (a face with an index outside 0..V-1 is skipped)
    -> label device int32 [V]: the smallest vertex index of each vertex's connected component; a vertex no face uses is its own.
    scratch: mesh_clean_scratch(V, T, device) (allocated when None); pass the same one on to mesh_component_select and
    mesh_compact, which read its give-up word.  Nothing is read back."""
    V, T, dev = _mesh(None, triangles, n_vertices)
    scratch = _clean_scratch(scratch, V, T, dev)
    if out is None:
        out = torch.empty(V, dtype=torch.int32, device=dev)
    _req(out, torch.int32, (V,), "out")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_components(ptr(triangles), V, T, ptr(out), ptr(scratch), _stream()), "nb_mesh_components")
    return out


def mesh_component_select(label, triangles, components="largest", keep=None, stats=None, scratch=None):
    """nb_mesh_component_select: label device int32 [V] (mesh_components), triangles device int32 [T,3]; components "largest"
    (the component of most faces, a tie going to the smaller label) or a float f in (0, 1] (every component of at least
    ceil(f * largest) faces; 1.0 is "largest") -> (keep_vertex device uint8 [V], stats device int32 [4] = {components that
    have a face, components kept, faces of the largest, faces kept}).  A component without a face is never kept.  Nothing is
    read back."""
    _req(label, torch.int32, (None,), "label")
    V, T, dev = _mesh(None, triangles, label.shape[0])
    if label.device != dev:
        raise ValueError("label and triangles live on different devices")
    fraction = mesh_components_fraction(components)
    if fraction is None:
        raise ValueError("components = 'all' selects nothing: skip the call")
    scratch = _clean_scratch(scratch, V, T, dev)
    if keep is None:
        keep = torch.empty(V, dtype=torch.uint8, device=dev)
    if stats is None:
        stats = torch.empty(4, dtype=torch.int32, device=dev)
    _req(keep, torch.uint8, (V,), "keep")
    _req(stats, torch.int32, (4,), "stats")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_component_select(ptr(label), ptr(triangles), V, T, fraction, ptr(keep), ptr(stats), ptr(scratch),
                                                  _stream()), "nb_mesh_component_select")
    return keep, stats


def mesh_components_fraction(components):
    """The `components` argument of the mesh pass as nb_mesh_component_select's min_fraction: "all" / None / False -> None (no
    clean-up), "largest" -> 1.0, a number in (0, 1] -> itself; anything else is a ValueError."""
    if components is None or components is False or components == "all":
        return None
    if components == "largest":
        return 1.0
    if isinstance(components, (int, float)) and not isinstance(components, bool) and 0.0 < float(components) <= 1.0:
        return float(components)
    raise ValueError("components must be 'all', 'largest' or a number in (0, 1], got %r" % (components,))


def mesh_compact_count(triangles, keep, scratch, counts=None):
    """nb_mesh_compact_count: the two scans of mesh_compact -> counts, a [2] int32 device tensor {kept vertices, kept triangles};
    nothing is read back."""
    _req(keep, torch.uint8, (None,), "keep")
    V, T, dev = _mesh(None, triangles, keep.shape[0])
    if keep.device != dev:
        raise ValueError("keep and triangles live on different devices")
    _req(scratch, torch.uint8, (None,), "scratch")
    if counts is None:
        counts = torch.empty(2, dtype=torch.int32, device=dev)
    _req(counts, torch.int32, (2,), "counts")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_compact_count(ptr(triangles), ptr(keep), V, T, ptr(counts), ptr(scratch), _stream()),
              "nb_mesh_compact_count")
    return counts


def _kept_counts(counts):
    """The ONE 8-byte read of a compaction: (kept vertices, kept triangles) on the host; NbError for NB_EINTERNAL."""
    n_vert, n_tri = (int(v) for v in counts.tolist())
    if n_vert == _lib.EINTERNAL or n_tri == _lib.EINTERNAL:
        raise NbError("nb_mesh_components failed (%d, NB_EINTERNAL): a hook or a walk to the root was still unfinished after %d "
                      "rounds; no label was written" % (_lib.EINTERNAL, MESH_HOOK_ROUNDS))
    return n_vert, n_tri


def mesh_compact_emit(vertices, triangles, scratch, counts, vertices_out, triangles_out, attr=None, attr_out=None):
    """nb_mesh_compact into caller-owned buffers (vertices_out [Vcap,3] float32, triangles_out [Tcap,3] int32, attr_out [Vcap,3]
    float32 iff attr is given) after mesh_compact_count on the same triangles, flags and scratch.  counts: that call's result,
    as the device tensor (read here, the one 8-byte read) or as the pair of ints already read.  Raises NbError, with the buffers
    untouched, when they are too small."""
    V, T, dev = _mesh(vertices, triangles)
    _req(scratch, torch.uint8, (None,), "scratch")
    _req(vertices_out, torch.float32, (None, 3), "vertices_out")
    _req(triangles_out, torch.int32, (None, 3), "triangles_out")
    if (attr is None) != (attr_out is None):
        raise ValueError("attr and attr_out go together")
    if attr is not None:
        _req(attr, torch.float32, (V, 3), "attr")
        _req(attr_out, torch.float32, (vertices_out.shape[0], 3), "attr_out")
    n_vert, n_tri = _kept_counts(counts) if isinstance(counts, torch.Tensor) else (int(counts[0]), int(counts[1]))
    if n_vert > vertices_out.shape[0] or n_tri > triangles_out.shape[0]:
        raise NbError("nb_mesh_compact failed (-1): the kept mesh has %d vertices and %d triangles, the buffers hold %d and %d" % (
            n_vert, n_tri, vertices_out.shape[0], triangles_out.shape[0]))
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_compact(ptr(vertices), ptr(triangles), ptr(attr), V, T, ptr(vertices_out), ptr(triangles_out),
                                         ptr(attr_out), vertices_out.shape[0], triangles_out.shape[0], ptr(scratch), _stream()),
              "nb_mesh_compact")
    return (vertices_out, triangles_out) if attr is None else (vertices_out, triangles_out, attr_out)


def mesh_compact(vertices, triangles, keep, attr=None, scratch=None):
    """The kept part of a mesh as a mesh of its own: vertices device fp32 [V,3], triangles device int32 [T,3], keep device uint8
    [V] (mesh_component_select) -> (vertices [V',3], triangles [T',3][, attr [V',3]]), device tensors of the exact size; kept
    vertices and triangles keep their relative order, the indices are renumbered, an optional per-vertex fp32 [V,3] attribute
    (normals, colours) travels with its vertex.  A triangle is kept iff its indices are in range and its first vertex is kept.
    Count, ONE host read of the two counts, allocate, emit."""
    V, T, dev = _mesh(vertices, triangles)
    _req(keep, torch.uint8, (V,), "keep")
    scratch = _clean_scratch(scratch, V, T, dev)
    n_vert, n_tri = _kept_counts(mesh_compact_count(triangles, keep, scratch))
    vertices_out = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    triangles_out = torch.empty((n_tri, 3), dtype=torch.int32, device=dev)
    attr_out = None if attr is None else torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    return mesh_compact_emit(vertices, triangles, scratch, (n_vert, n_tri), vertices_out, triangles_out, attr, attr_out)


def mesh_color_query(vertices_idx, normals, step, origin, pad):
    """nb_mesh_color_query: vertices_idx device fp32 [V,3] (index units of the padded cube), normals device fp32 [V,3], step and
    origin device fp32 [3], pad a number -> (wpts [V,3] = (v - pad) * step + origin, three fp32 operations per axis; viewdir [V,3]
    = -normal, (0, 0, -1) for a zero normal).  Nothing is read back."""
    _req(vertices_idx, torch.float32, (None, 3), "vertices_idx")
    V, dev = int(vertices_idx.shape[0]), vertices_idx.device
    _req(normals, torch.float32, (V, 3), "normals")
    _req(step, torch.float32, (3,), "step")
    _req(origin, torch.float32, (3,), "origin")
    if normals.device != dev or step.device != dev or origin.device != dev:
        raise ValueError("vertices_idx, normals, step and origin live on different devices")
    wpts, viewdir = torch.empty_like(vertices_idx), torch.empty_like(vertices_idx)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_color_query(ptr(vertices_idx), ptr(normals), ptr(step), ptr(origin), float(pad), V, ptr(wpts),
                                             ptr(viewdir), _stream()), "nb_mesh_color_query")
    return wpts, viewdir


def mesh_color_finish(raw):
    """nb_mesh_color_finish: raw device fp32 [V,4] (calculate_density_color) -> (rgb_f fp32 [V,3] = sigmoid of the three logits,
    rgb_u8 uint8 [V,3] = rint(255 rgb_f), half to even).  Nothing is read back."""
    _req(raw, torch.float32, (None, 4), "raw")
    V, dev = int(raw.shape[0]), raw.device
    rgb_f = torch.empty((V, 3), dtype=torch.float32, device=dev)
    rgb_u8 = torch.empty((V, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().nb_mesh_color_finish(ptr(raw), V, ptr(rgb_f), ptr(rgb_u8), _stream()), "nb_mesh_color_finish")
    return rgb_f, rgb_u8


def mesh_vertex_colors(vertices_idx, normals, step, origin, pad, decode):
    """The colour of every vertex from the colour head: mesh_color_query, ONE call of `decode(wpts [1,V,3], viewdir [1,V,3]) ->
    raw [1,V,4]` (Network.calculate_density_color bound to the frame's feature volumes), mesh_color_finish -> (rgb_f fp32 [V,3],
    rgb_u8 uint8 [V,3], wpts, viewdir).  A mesh without vertices asks nothing."""
    wpts, viewdir = mesh_color_query(vertices_idx, normals, step, origin, pad)
    if vertices_idx.shape[0] == 0:
        raw = torch.empty((0, 4), dtype=torch.float32, device=vertices_idx.device)
    else:
        raw = decode(wpts[None], viewdir[None]).reshape(-1, 4).float().contiguous()
    return mesh_color_finish(raw) + (wpts, viewdir)


# ------------------------------------------------------------------------------------------- a photographed frame
def mask_band(labels, border=5, out=None):
    """nb_mask_band: get_mask of multi_view_dataset.py:58-64 for every label image of a device uint8 [V,H,W] stack -> a new
    [V,H,W]: (label != 0), and 100 where the border x border erosion and dilation of it differ.  border = 1: (label != 0)."""
    return _window("nb_mask_band", labels, "labels", border, out, in_place="out is labels: the band is not computed in place")


def image_undistort(rgb, msk, cam, n=1, fill=None):
    """nb_image_undistort: cv2.undistort(src, K, D), the reduction by the integer factor n (INTER_AREA for the image,
    INTER_NEAREST for the mask) and the background fill of multi_view_dataset.py:129-142, from the files' bytes.
    rgb: device uint8 [H,W,3] or [V,H,W,3], or None; msk: device uint8 [H,W] or [V,H,W], or None; cam: host float64 [12] or
    [V,12], fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 per view (image_prep.camera_constants); fill: None, 'black' or 'white' (the
    image where the reduced mask is 0).  -> (img fp32 [(V,)H/n,W/n,3] or None, msk uint8 [(V,)H/n,W/n] or None)."""
    import numpy as np

    if rgb is None and msk is None:
        raise ValueError("image_undistort: neither an image nor a mask")
    if fill not in _lib.FILL_MODES:
        raise ValueError("fill must be None, 'black' or 'white', got %r" % (fill,))
    if fill is not None and (msk is None or rgb is None):
        raise ValueError("fill = %r needs both an image and a mask" % (fill,))
    cam = np.ascontiguousarray(np.asarray(cam, dtype=np.float64))
    batched = cam.ndim == 2
    if cam.ndim not in (1, 2) or cam.shape[-1] != _lib.CAM_DOUBLES:
        raise ValueError("cam has shape %s, expected [12] or [V,12]" % (cam.shape,))
    cam = cam.reshape(-1, _lib.CAM_DOUBLES)
    V = int(cam.shape[0])
    if V < 1 or not np.all(np.isfinite(cam)) or np.any(cam[:, :2] == 0.0):
        raise ValueError("cam: at least one view, every constant finite, fx and fy non-zero")
    lead = (V,) if batched else ()
    first = rgb if rgb is not None else msk
    if first.dim() < 2 + len(lead):
        raise ValueError("%s has shape %s for cam %s" % ("rgb" if rgb is not None else "msk", tuple(first.shape), cam.shape))
    H, W = (int(v) for v in first.shape[len(lead):len(lead) + 2])
    if rgb is not None:
        _req(rgb, torch.uint8, lead + (H, W, 3), "rgb")
    if msk is not None:
        _req(msk, torch.uint8, lead + (H, W), "msk")
        if rgb is not None and msk.device != rgb.device:
            raise ValueError("rgb and msk live on different devices")
    n = int(n)
    if H < 1 or W < 1 or H > 32768 or W > 32768 or 3 * V * H * W > 2 ** 31 - 1:
        raise ValueError("no frame of V = %d, H = %d, W = %d (H, W 1..32768, 3 V H W at most 2^31 - 1)" % (V, H, W))
    if n < 1 or H % n or W % n:
        raise ValueError("n = %d must be >= 1 and divide H = %d and W = %d" % (n, H, W))
    dev = first.device
    img_out = torch.empty(lead + (H // n, W // n, 3), dtype=torch.float32, device=dev) if rgb is not None else None
    msk_out = torch.empty(lead + (H // n, W // n), dtype=torch.uint8, device=dev) if msk is not None else None
    with torch.cuda.device(dev):
        check(_lib.lib().nb_image_undistort(ptr(rgb), ptr(msk), cam.ctypes.data_as(C.POINTER(C.c_double)), V, H, W, n,
                                            _lib.FILL_MODES[fill], ptr(img_out), ptr(msk_out), _stream()), "nb_image_undistort")
    return img_out, msk_out


# ------------------------------------------------------------------------------------------- vanilla-NeRF baseline
NERF_PRECISIONS = {"f32": 0, "f16x3": 2}  # nb_nerf_pack / nb_nerf_decode: NB_PREC_F32, NB_PREC_F16X3
# one Nerf module's parameters in nb_nerf_params order, as (attribute path, shape)
NERF_PARAM_SHAPES = [("pts_linears.%d" % i, (256, 63 if i == 0 else (319 if i == 5 else 256))) for i in range(8)] + \
                    [("views_linears.0", (128, 283)), ("feature_linear", (256, 256)), ("alpha_linear", (1, 256)), ("rgb_linear", (3, 128))]


def _nerf_precision(precision):
    if precision not in NERF_PRECISIONS:
        raise ValueError("nerf precision must be one of %s, got %r" % (sorted(NERF_PRECISIONS), precision))
    return NERF_PRECISIONS[precision]


def nerf_pack_size(precision="f32"):
    return int(_lib.lib().nb_nerf_pack_size(_nerf_precision(precision)))


def nerf_pack(params, precision="f32", out=None):
    """nb_nerf_pack: params maps '<layer>.weight' / '<layer>.bias' (the names of one reference Nerf module's state_dict) to fp32
    device tensors in the reference's shapes -> the packed blob [nerf_pack_size()]."""
    prec = _nerf_precision(precision)
    p = _lib.NbNerfParams()
    dev = None
    for name, shape in NERF_PARAM_SHAPES:
        w = _req(params[name + ".weight"], torch.float32, shape, name + ".weight")
        b = _req(params[name + ".bias"], torch.float32, (shape[0],), name + ".bias")
        dev = w.device if dev is None else dev
        if w.device != dev or b.device != dev:
            raise ValueError("nerf_pack: %s lives on %s, the first parameter on %s" % (name, w.device, dev))
        if name.startswith("pts_linears."):
            i = int(name.split(".")[1])
            p.pts_w[i], p.pts_b[i] = w.data_ptr(), b.data_ptr()
        else:
            field = name.split("_")[0]  # views_linears.0 -> views, feature_linear -> feature, ...
            setattr(p, field + "_w", w.data_ptr())
            setattr(p, field + "_b", b.data_ptr())
    if out is None:
        out = torch.empty(nerf_pack_size(precision), dtype=torch.float32, device=dev)
    _req(out, torch.float32, (nerf_pack_size(precision),), "out")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_nerf_pack(C.byref(p), ptr(out), prec, _stream()), "nb_nerf_pack")
    return out


def nerf_decode(packed, ray_o, ray_d, z_vals, precision="f32", out=None):
    """nb_nerf_decode: raw [n,S,4] of the packed Nerf module at the depths z_vals [n,S] of the rays ray_o / ray_d [n,3]
    (points fl32(o + fl32(d z)), direction d / |d|)."""
    prec = _nerf_precision(precision)
    _req(z_vals, torch.float32, (None, None), "z_vals")
    n, S = z_vals.shape
    _req(ray_o, torch.float32, (n, 3), "ray_o")
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    _req(packed, torch.float32, (nerf_pack_size(precision),), "packed")
    if out is None:
        out = torch.empty((n, S, 4), dtype=torch.float32, device=z_vals.device)
    _req(out, torch.float32, (n, S, 4), "out")
    with torch.cuda.device(z_vals.device):
        check(_lib.lib().nb_nerf_decode(ptr(packed), ptr(ray_o), ptr(ray_d), ptr(z_vals), n, S, ptr(out), prec, _stream()),
              "nb_nerf_decode")
    return out


def nerf_density(packed, pts, precision="f32", out=None):
    """nb_nerf_density: alpha [n] of the packed Nerf module's trunk at the points pts [n,3] (alpha_linear's raw output, no relu):
    the bits of nerf_decode(...)[..., 3] at the same points."""
    prec = _nerf_precision(precision)
    _req(pts, torch.float32, (None, 3), "pts")
    n = pts.shape[0]
    _req(packed, torch.float32, (nerf_pack_size(precision),), "packed")
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=pts.device)
    _req(out, torch.float32, (n,), "out")
    with torch.cuda.device(pts.device):
        check(_lib.lib().nb_nerf_density(ptr(packed), ptr(pts), n, ptr(out), prec, _stream()), "nb_nerf_density")
    return out


def nerf_embed_grad(emb, d_emb, out=None):
    """nb_nerf_embed_grad: emb [n,>=63] the forward's point-embedding columns and d_emb [n,>=63] the gradient by them (both may be
    column slices of wider matrices) -> grad [n,3], the gradient by the point."""
    _mat(emb, "emb")
    _mat(d_emb, "d_emb")
    n = emb.shape[0]
    if emb.shape[1] < 63 or d_emb.shape[1] < 63 or d_emb.shape[0] != n or d_emb.device != emb.device:
        raise ValueError("emb and d_emb must be [n, >= 63] on one device, got %s and %s" % (tuple(emb.shape), tuple(d_emb.shape)))
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=emb.device)
    _req(out, torch.float32, (n, 3), "out")
    with torch.cuda.device(emb.device):
        check(_lib.lib().nb_nerf_embed_grad(ptr(emb), max(emb.stride(0), 63), ptr(d_emb), max(d_emb.stride(0), 63), n, ptr(out),
                                            _stream()), "nb_nerf_embed_grad")
    return out


NERF_TAP_COLS, NERF_DTAP_COLS = 2528, 2432  # NB_NERF_TAP_COLS, NB_NERF_DTAP_COLS
# column slices of the tap (include/nb_hip.h: nb_nerf_decode_tap) and of the d-tap (nb_nerf_bwd_chain), as (first, width)
NERF_TAP = {"h": lambda i: (256 * i, 256), "feature": (2048, 256), "V": (2304, 128), "pts": (2432, 63), "view": (2496, 27)}
NERF_DTAP = {"z": lambda i: (256 * i, 256), "feature": (2048, 256), "V": (2304, 128)}


def nerf_decode_tap(packed, ray_o, ray_d, z_vals, out=None, tap=None):
    """nb_nerf_decode_tap: (raw [n,S,4], tap [n*S, NERF_TAP_COLS]) of the f32-packed Nerf module: nerf_decode(..., 'f32')'s raw bit
    for bit plus every activation the backward needs (the training forward)."""
    _req(z_vals, torch.float32, (None, None), "z_vals")
    n, S = z_vals.shape
    _req(ray_o, torch.float32, (n, 3), "ray_o")
    _req(ray_d, torch.float32, (n, 3), "ray_d")
    _req(packed, torch.float32, (nerf_pack_size("f32"),), "packed")
    if out is None:
        out = torch.empty((n, S, 4), dtype=torch.float32, device=z_vals.device)
    _req(out, torch.float32, (n, S, 4), "out")
    if tap is None:
        tap = torch.empty((n * S, NERF_TAP_COLS), dtype=torch.float32, device=z_vals.device)
    _req(tap, torch.float32, (n * S, NERF_TAP_COLS), "tap")
    with torch.cuda.device(z_vals.device):
        check(_lib.lib().nb_nerf_decode_tap(ptr(packed), ptr(ray_o), ptr(ray_d), ptr(z_vals), n, S, ptr(out), ptr(tap), _stream()),
              "nb_nerf_decode_tap")
    return out, tap


def nerf_pack_bwd_size():
    return int(_lib.lib().nb_nerf_pack_bwd_size())


def nerf_pack_bwd(params, out=None):
    """nb_nerf_pack_bwd: params as for nerf_pack (the biases are not read) -> the transposed blob [nerf_pack_bwd_size()] of the
    input-gradient chain."""
    p = _lib.NbNerfParams()
    dev = None
    for name, shape in NERF_PARAM_SHAPES:
        w = _req(params[name + ".weight"], torch.float32, shape, name + ".weight")
        dev = w.device if dev is None else dev
        if w.device != dev:
            raise ValueError("nerf_pack_bwd: %s lives on %s, the first parameter on %s" % (name, w.device, dev))
        if name.startswith("pts_linears."):
            p.pts_w[int(name.split(".")[1])] = w.data_ptr()
        else:
            setattr(p, name.split("_")[0] + "_w", w.data_ptr())
    if out is None:
        out = torch.empty(nerf_pack_bwd_size(), dtype=torch.float32, device=dev)
    _req(out, torch.float32, (nerf_pack_bwd_size(),), "out")
    with torch.cuda.device(dev):
        check(_lib.lib().nb_nerf_pack_bwd(C.byref(p), ptr(out), _stream()), "nb_nerf_pack_bwd")
    return out


def nerf_bwd_chain(packed_bwd, tap, d_raw, dtap=None):
    """nb_nerf_bwd_chain: d_raw [n_pts,4] (or [n,S,4]) and the forward's tap [n_pts, NERF_TAP_COLS] -> the d-tap
    [n_pts, NERF_DTAP_COLS], the gradient of every pre-activation.  A given dtap may have more rows: only the first n_pts are
    written."""
    _req(tap, torch.float32, (None, NERF_TAP_COLS), "tap")
    n_pts = tap.shape[0]
    _req(d_raw, torch.float32, None, "d_raw")
    if d_raw.numel() != n_pts * 4 or d_raw.shape[-1] != 4:
        raise ValueError("d_raw must hold [%d, 4] values, got %s" % (n_pts, tuple(d_raw.shape)))
    _req(packed_bwd, torch.float32, (nerf_pack_bwd_size(),), "packed_bwd")
    if dtap is None:
        dtap = torch.empty((n_pts, NERF_DTAP_COLS), dtype=torch.float32, device=tap.device)
    _req(dtap, torch.float32, (None, NERF_DTAP_COLS), "dtap")
    if dtap.shape[0] < n_pts:
        raise ValueError("dtap has %d rows, the tap %d" % (dtap.shape[0], n_pts))
    with torch.cuda.device(tap.device):
        check(_lib.lib().nb_nerf_bwd_chain(ptr(packed_bwd), ptr(tap), ptr(d_raw), n_pts, ptr(dtap), _stream()), "nb_nerf_bwd_chain")
    return dtap


def importance_merge_z(z_coarse, z_fine):
    """nb_importance_merge_z: z_coarse [n,S] and z_fine [n,N] -> z_vals [n,S+N] sorted by depth (importance_merge's stable rule,
    depths alone)."""
    _req(z_coarse, torch.float32, (None, None), "z_coarse")
    n, S = z_coarse.shape
    _req(z_fine, torch.float32, (n, None), "z_fine")
    N = int(z_fine.shape[1])
    z_vals = torch.empty((n, S + N), dtype=torch.float32, device=z_coarse.device)
    with torch.cuda.device(z_coarse.device):
        check(_lib.lib().nb_importance_merge_z(ptr(z_coarse), ptr(z_fine), n, S, N, ptr(z_vals), _stream()), "nb_importance_merge_z")
    return z_vals
