"""The multi-step ray loop of nb_march_kernel (fp32) and nb_march_fold_kernel<0, CULL> + nb_march_fixup_kernel (f16f6) against exact
models, through the product ABI alone (tests/march_ray_cases.py says how the inputs are made and where the bounds come from):

A. the integrator — sample depths, intervals, RayAccum::add / composite_step, the vectorised weight stores, slot lists, culled
   samples — against a float64 composite of the decoder output the kernel itself composited (want_raw), within (8 + S / 2) 2^-24;
B. the sample positions — the raw output of a multi-sample march against nb_decode_points on p = o + d z[s] built in numpy float32:
   bit for bit in fp32, within the f16f6 point tolerance of test_gpu_fold.py for f16f6;
C. the f16f6 kernel's pipelined preparation of step s + 1 inside step s (and the sequential one at step 0 and behind a skipped
   step) on lattice rays, bit for bit against the operand-exact model of tests/f16f6_model.py.

What these tests catch (each made once in a scratch copy of the kernels, the narrowest tests selected):
   the interval of step s taken as z[s] - z[s-1]                 A [S16-jit] (error / bound 7.7e4) and, without jitter, A [S16-f32] (1.09)
   the jitter's upper end at s == S - 1 from the general formula  A [S16-t1]
   the vector weight stores writing slot i to i ^ 1               A [S16-f32], [S16-f16f6], [S24-f32]
   the next step's grid coordinates published to sample j ^ 1     C [whole], [narrow], [half]
   a culled sample keeping its decoded density                    A [S16-cull], C [cull]
"""
import time

import numpy as np
import pytest
import torch

from tests import f16f6_phase_cases as C
from tests import helpers as H
from tests import march_ray_cases as R
from tests.test_gpu_f16f6_phases import Rig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# precision, fixup: the fix-up rewrites the last density in raw, so raw is what was composited either way
ARITHMETICS = (("f32", True), ("f16f6", True), ("f16f6", False))
ARITH_IDS = ("f32", "f16f6", "f16f6-nofixup")
POINT_TOL_F16F6 = 2.5e-3  # f16f6 point decodes against fp32, relative to max(1, |ref|): test_gpu_fold.py


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_SCENE = {}


def _scene():
    """The 'small_dense' scene on the device, once: one network, its encoder's volumes, and the scene / weights / latent bias of both
    arithmetics."""
    if not _SCENE:
        from neuralbody_amd.renderer import Renderer
        from tests.golden import scenes

        r, sd, body, batch, cam, _ = scenes.build("small_dense")
        net = H.make_network(sd, DEV, True, precision="f32")
        bd = H.device_batch(batch, DEV)
        with torch.no_grad():
            sp = Renderer(net).prepare_sp_input(bd)
            vols = net.encode_sparse_voxels(sp)
            _SCENE.update(net=net, sp=sp, vols=vols, lb=net.latent_bias(sp["latent_index"]),
                          scene=dict((p, net.make_scene(vols, sp, p)) for p in ("f32", "f16f6")),
                          packed=dict((p, net.packed_weights(p)) for p in ("f32", "f16f6")))
        torch.cuda.synchronize()
    return _SCENE


_INPUTS = {}


def _inputs(case):
    """a_inputs(case) and its device tensors, once per case."""
    if case[0] not in _INPUTS:
        from neuralbody_amd import ops

        d = R.a_inputs(case)
        t = dict((k, _dev(d[k])) for k in ("ray_o", "ray_d", "near", "far", "t_vals"))
        t["t_rand"] = None if d["t_rand"] is None else _dev(d["t_rand"])
        t["slots"] = None if d["slots"] is None else _dev(d["slots"])
        t["cull"] = None
        if d["inside"] is not None:
            t["cull"] = ops.make_cull(_dev(d["cull_mask"][None]), _dev(d["cull_RT"][None]), _dev(d["cull_K"][None]))
        _INPUTS[case[0]] = (d, t)
    return _INPUTS[case[0]]


def _march(case, precision, fixup=True):
    from neuralbody_amd import ops

    sc = _scene()
    d, t = _inputs(case)
    with torch.no_grad():
        out = ops.march(sc["scene"][precision], sc["packed"][precision], sc["lb"], t["ray_o"], t["ray_d"], t["near"], t["far"], t["t_vals"],
                        t["t_rand"], white_bkgd=d["white"], want_raw=True, precision=precision, ray_order=t["slots"], cull=t["cull"],
                        fixup=fixup)
    torch.cuda.synchronize()
    return d, dict((k, v.cpu().numpy()) for k, v in out.items() if k != "ill_scratch")


# --------------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("arith", ARITHMETICS, ids=ARITH_IDS)
@pytest.mark.parametrize("case", R.A_CASES, ids=lambda c: c[0])
def test_integrator_against_float64_composite_of_its_own_raw(case, arith):
    """Weights, rgb and acc within tol(S) = (8 + S / 2) 2^-24 of the float64 composite of the kernel's own raw output at the depths
    of z_vals_f32, depth within tol(S) max z, acc = sum(weights) to the same bound, disp = 1 / max(1e-10, depth / acc) of the stored
    depth and acc within 4 x 2^-24 relative with NaN exactly where acc == 0; culled samples have raw == 0 and rays without a slot
    read 0 everywhere.  The fixture: at least a quarter of the rays end between 0.05 and 0.95 opacity, at least one hits nothing,
    and neighbouring weights differ.

    'Neighbouring weights differ' as it can hold here: more than half of the samples of this scene have a non-positive density and
    therefore a weight of exactly 0, so that among ALL neighbouring pairs of the rays with acc > 0.05 only 0.30 .. 0.65 differ (1.0 at
    S = 2); 'above 0.9' is asserted over the pairs in which either weight is not zero (measured 1.0), and 'above 0.25' over all."""
    precision, fixup = arith
    t0 = time.time()
    d, got = _march(case, precision, fixup)
    S, has = d["S"], d["has_slot"]
    raw = got["raw"]
    assert raw.shape == (R.N_RAYS, S, 4)
    for k, v in got.items():  # rays without a slot read 0
        assert not v[~has].any(), k
    if d["inside"] is not None:
        culled = ~d["inside"][has]
        assert not raw[has][culled].any(), "a culled sample has raw != 0"
        assert (raw[has][~culled] != 0).any(-1).mean() > 0.99  # ... and the others were decoded
    else:
        assert (raw[has] != 0).any(-1).all()
    sel = dict((k, v[has]) for k, v in got.items())
    ratios = R.integrator_ratios(sel, raw[has], d["z"][has], d["ray_d"][has], d["white"])
    fig = R.fixture_figures(got["weights"], got["acc_map"], has)
    print("%s %s: %.2f s; |error| / tol: %s; fixture: %s" % (d["name"], ARITH_IDS[ARITHMETICS.index(arith)], time.time() - t0,
                                                            ", ".join("%s %.3f" % kv for kv in sorted(ratios.items())),
                                                            ", ".join("%s %.3g" % kv for kv in sorted(fig.items()))))
    assert fig["mid"] >= 0.25 and fig["zero"] >= 1, fig
    assert fig["distinct_live"] > 0.9 and fig["distinct_all"] > 0.25, fig
    assert np.isnan(got["disp_map"][has][got["acc_map"][has] == 0]).all()
    for name, r in sorted(ratios.items()):
        assert r <= 1.0, "%s: %s misses its bound: |error| / tol = %.3f" % (d["name"], name, r)


# --------------------------------------------------------------------------------------------------------------------------- B
_POINTS = {}


def _point_reference(case):
    """fp32 nb_decode_points of the case's sample points p = o + d z[s] (numpy float32) with view direction d / |d|, [n, S, 4]; once."""
    if case[0] not in _POINTS:
        from neuralbody_amd import ops

        sc = _scene()
        d, _ = _inputs(case)
        p = d["p"].reshape(-1, 3)
        v = np.repeat(d["v"], d["S"], 0)
        with torch.no_grad():
            ref = ops.decode_points(sc["scene"]["f32"], sc["packed"]["f32"], sc["lb"], _dev(p), _dev(v), precision="f32")
        torch.cuda.synchronize()
        _POINTS[case[0]] = ref.reshape(R.N_RAYS, d["S"], 4)
    return _POINTS[case[0]]


@pytest.mark.parametrize("precision", ["f32", "f16f6"])
@pytest.mark.parametrize("case", R.B_CASES, ids=lambda c: c[0])
def test_raw_of_a_march_is_the_point_decode_of_its_sample_positions(case, precision):
    """fp32: raw[r, s] of the march is nb_decode_points of p = fadd(o, fmul(d, z[s])) and v = d / |d| BIT FOR BIT on every sample
    the cull keeps (both kernels call the same decode; the arithmetic does not depend on the grouping).  f16f6 (grouping-dependent):
    within 2.5e-3 of the fp32 point decode, ten times less than what moving every sample by one depth step changes.

    This test found the march's depths and positions contracted into FMAs (the `_rn` intrinsics are plain operators to hipcc): 12209
    of 12800 fp32 raw values differed from the point decode.  z_lin, z_jitter, ray_point and ray_norm (nb_march_common.h) now round
    every operation on its own; 0 values differ.  Measured f16f6 distance: 1.2e-3; one depth step moves the reference by 0.5."""
    d, got = _march(case, precision)
    ref_t = _point_reference(case)
    keep = np.ones((R.N_RAYS, d["S"]), bool) if d["inside"] is None else d["inside"]
    raw_t = torch.from_numpy(got["raw"])
    ref = ref_t.cpu().numpy()
    scale = np.maximum(1.0, np.abs(ref.astype(np.float64)))
    if precision == "f32":
        a, b = raw_t[torch.from_numpy(keep)], ref_t.cpu()[torch.from_numpy(keep)]
        differ = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())
        print("%s f32: %d of %d values differ from the point decode" % (d["name"], differ, a.numel()))
        assert H.same_bits(a, b), "%d of %d raw values differ from nb_decode_points of the same points" % (differ, a.numel())
    else:
        err = (np.abs(got["raw"].astype(np.float64) - ref) / scale)[keep]
        print("%s f16f6: largest |raw - fp32 point decode| / max(1, |ref|) = %.3e" % (d["name"], float(err.max())))
        assert float(err.max()) <= POINT_TOL_F16F6
    # the fixture: one depth step further is another value
    shift = (np.abs(ref[:, 1:].astype(np.float64) - ref[:, :-1]) / scale[:, 1:]).max(-1)
    print("%s: one depth step moves the fp32 reference by %.3e (median sample)" % (d["name"], float(np.median(shift))))
    assert float(np.median(shift)) > 10 * POINT_TOL_F16F6


# --------------------------------------------------------------------------------------------------------------------------- C
class RayRig(Rig):
    """A lattice ray case on the device: Rig's scene and read-outs, the march over the case's rays instead of one-sample rays."""

    def __init__(self, case):
        super(RayRig, self).__init__(case)
        self.rays = [_dev(getattr(case, k)) for k in ("ray_o", "ray_d", "near", "far", "t_vals")]
        self.cull = None
        if case.cull is not None:
            mask, RT, Kc = case.cull
            self.cull = self.ops.make_cull(_dev(mask), _dev(RT[None]), _dev(Kc[None]))
        self.culled = torch.from_numpy(~case.inside.reshape(-1)).to(DEV)

    def raw(self, mode):
        """[64 S, 4] in (ray, step) order of the current parameters; a culled sample must read 0 in every read-out."""
        ops = self.ops
        packed = ops.mlp_pack(self.params, precisions=("f16f6",))
        out = ops.march(self.scene, packed, self.lb, *self.rays, want_raw=True, precision="f16f6", fixup=False, cull=self.cull)
        raw = out["raw"].reshape(-1, 4)
        assert not bool(raw[self.culled].any()), "a culled sample has raw != 0"
        return raw


_RIGS, _EXPECTED = {}, {}


def _assert_rays_exact(key):
    case = R.get(key)
    if key not in _RIGS:
        _RIGS[key] = RayRig(case)
        exp = R.ray_expected(case)[0]
        exp.setflags(write=False)
        _EXPECTED[key] = exp
    t0 = time.time()
    got = _RIGS[key].read("march").reshape(len(case.rows), 64, case.S)
    torch.cuda.synchronize()
    want = _EXPECTED[key]
    bad = got != want
    print("%s: %d x 64 x %d read-outs in %.2f s, %d differ, largest |difference| %.3e of %.3e" % (
        case.name, got.shape[0], case.S, time.time() - t0, int(bad.sum()), float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert (want[:, case.inside] != 0).mean() > 0.3
    if bad.any():
        i, r, s = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d read-outs differ from the model; first: row %d ray %d step %d got %r, model %r" % (
            case.name, int(bad.sum()), bad.size, case.rows[i], r, s, got[i, r, s], want[i, r, s]))


@pytest.mark.parametrize("key", R.RAY_KEYS, ids=lambda k: k[0] + ("-colour" if k[1] else ""))
def test_lattice_rays_bit_for_bit(key):
    """64 lattice rays through nb_march_fold_kernel<0, CULL>: the first layer's output of every (ray, step) read through identity
    layers and one-hot alpha_fc rows (the colour head's through rgb_fc on 'whole'), bit for bit the model's value of that step's
    point; 0 on culled samples, the model's value on the steps right behind a skipped one."""
    _assert_rays_exact(key)
