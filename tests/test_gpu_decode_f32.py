"""The exact fp32 point decoder (nb_points_kernel<DENSITY_ONLY, DBG>, whose decode<> body nb_march_kernel shares) and nb_composite
against float64, stage by stage, through ops.make_pose / make_scene / mlp_pack / mlp_latent_bias / decode_points(debug=True) with
ops.TAP, and ops.composite (the row-count test calls nb_decode_points through the C ABI on sentinel-filled buffers it owns).  Inputs,
references, path predicates and the derivation of every bound: tests/decode_f32_cases.py; what the CPU can say about them (lattice
preconditions, the path of every wave and level, the visibility of a list of mistakes): tests/test_decode_f32_host.py.

A. the trilinear gather: bit for bit on the lattice scene under two poses, on every path; within (6 + 8) 2^-24 sum |w| |v| on a
   realistic scene under a real rotation;
B. every layer from the tap: bit for bit on integer weights; the 84 sines and cosines tied to the PE tap, rgb_fc to the V tap; the
   three instantiations against each other; within (K + 2) 2^-24 (|b| + sum |w| |x|) of the float64 product of the kernel's own
   tapped input on realistic weights;
C. the positional encodings within 4e-7 of float64 sin / cos;
D. nb_composite within (8 + S/2) 2^-24 of march_ray_cases.composite_f64.

What these tests catch (each made once in a scratch copy of the kernels, none of them reading or writing out of range; every other
test of this file kept passing):
   cy of grid_coords formed with R[3] for R[1]                      A [*-permuted] (identity cannot see it), realistic gather, B exact
   tile 3 of every layer biased by tile 4's fragment                B exact, realistic layers, rgb tie
   the last NB_PF weight fragments of a layer = its first           B exact, realistic layers, rgb tie
   the x0 + 1 corner clamped, not zeroed, at the last plane (tile)  A [edges-clustered-*] alone: the per-lane path is another code
   encoding slots 5 and 6 exchanged in the packer's q >= 128 map    the PE tie, realistic layers
   T of nb_composite not multiplied into the trip's product         D [129-*], [200-*] (the third trip on)
   the first voxel of the LDS tile filled from its x neighbour      every A case with a tile path, row counts, odd points, realistic gather, rgb tie
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decode_f32_cases as dc
from tests import march_operand_cases as K
from tests import march_ray_cases as R
from tests import spconv_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
_CACHE = {}


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)  # (the cases' arrays are read-only)


def _scene(vols, pose, voxel=dc.VOXEL, out_sh=dc.OUT_SH):
    from neuralbody_amd import ops

    return ops.make_scene([_dev(v) for v in vols], ops.make_pose(pose["R"], pose["Th"], pose["bmin"], device=DEV), voxel, out_sh)


def _weights(p, code):
    """(packed blob, latent bias) of host parameters on the device"""
    from neuralbody_amd import ops

    pd = dict((k, _dev(v)) for k, v in p.items())
    packed = ops.mlp_pack(pd, precisions=["f32"])
    lb = ops.mlp_latent_bias(pd, _dev(code))
    torch.cuda.synchronize()
    return packed, lb


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _realistic_weights():
    return _cached("realistic-weights", lambda: _weights(*dc.realistic_params()))


def _lattice_scene(pose_name, poison_for=None):
    return _scene(dc.distinct_volumes() if poison_for is None else poison_for, dc.POSES[pose_name])


def _decode(scene, weights, pts, vd):
    """-> (raw [n, 4], tap [n, 1600]) as numpy"""
    from neuralbody_amd import ops

    raw, dbg = ops.decode_points(scene, weights[0], weights[1], _dev(pts), _dev(vd), debug=True)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), dbg.cpu().numpy()


def _tap(dbg, name):
    from neuralbody_amd import ops

    lo, hi = ops.TAP[name]
    return dbg[:, lo:hi]


def _directions(n, seed=1):
    v = np.random.RandomState(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _same_numbers(got, ref64):
    """got (fp32) holds the float64 reference's numbers (0.0 == -0.0; a NaN is a difference); the reference is fp32-representable"""
    ref32 = ref64.astype(F32)
    assert np.array_equal(ref32.astype(np.float64), ref64), "the reference is no fp32 number: not a lattice case"
    return bool(np.array_equal(got, ref32))


def _first_difference(got, ref64):
    bad = np.argwhere(got != ref64.astype(F32))
    i = tuple(bad[0])
    return "%d elements differ, the first at %s: got %r, want %r" % (len(bad), i, got[i], ref64[i])


# ------------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("pose", list(dc.POSES))
@pytest.mark.parametrize("case", dc.a_cases(), ids=repr)
def test_gather_lattice_bit_for_bit(case, pose):
    """EXACT.  dbg[:, F] of every point equals gather_f64 on the distinct-integer volumes, whichever path its wave takes on each level
    (the host test says which).  A second run on volumes that hold POISON wherever no point reads a weighted value gives the same bits,
    features and raw alike: clamped out-of-bounds corners, and whatever else a tile holds, do not reach the result.  'workgroups': the
    two waves that come again in the second workgroup repeat their bits."""
    w, g = dc.case_grid(case.q, pose)
    ref, S, touched = dc.gather_f64(g.astype(np.float64), dc.distinct_volumes())
    dc.assert_gather_lattice(S)
    vd = _directions(len(w))
    raw, dbg = _decode(_lattice_scene(pose), _realistic_weights(), w, vd)
    F = _tap(dbg, "F")
    assert _same_numbers(F, ref), _first_difference(F, ref)
    raw2, dbg2 = _decode(_lattice_scene(pose, dc.poisoned(dc.distinct_volumes(), touched)), _realistic_weights(), w, vd)
    assert np.array_equal(_tap(dbg2, "F"), F), "a voxel that carries no weight reached the features"
    assert np.array_equal(raw2.view(np.uint32), raw.view(np.uint32))
    if case.name == "workgroups":
        assert np.array_equal(dbg[128:192, :1120].view(np.uint32), dbg[0:64, :1120].view(np.uint32))  # F, h1, h2, h3: no view direction
        assert np.array_equal(raw[128:192, 3].view(np.uint32), raw[0:64, 3].view(np.uint32))


def _decode_abi(scene, weights, pts_dev, vd_dev, n, variant, n_all):
    """nb_decode_points on the first n points into caller-owned buffers of n_all rows filled with SENTINEL.  variant: 'dbg'
    (<false, true>), 'colour' (<false, false>) or 'density' (<true, false>, without view directions and latent bias)
    -> (raw [n_all, 4 or 1], tap [n_all, 1600] or None)"""
    from neuralbody_amd import _lib, ops

    density = variant == "density"
    out = torch.full((n_all, 1 if density else 4), dc.SENTINEL, dtype=torch.float32, device=DEV)
    dbg = torch.full((n_all, ops.DBG_WIDTH), dc.SENTINEL, dtype=torch.float32, device=DEV) if variant == "dbg" else None
    _lib.check(_lib.lib().nb_decode_points(C.byref(scene[0]), _lib.ptr(weights[0]), None if density else _lib.ptr(weights[1]),
                                           _lib.ptr(pts_dev), None if density else _lib.ptr(vd_dev), n, 1 if density else 0,
                                           _lib.ptr(out), _lib.ptr(dbg), _lib.PRECISIONS["f32"],
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nb_decode_points")
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dbg is None else dbg.cpu().numpy()


def test_row_counts_three_instantiations_and_sentinels():
    """EXACT.  n = 1, 31, 32, 33, 127, 128, 129 and all of 192 points whose last wave is, at n = 1, 33 and 129, a single clustered
    point in front of padding lanes: the features of the rows below n are gather_f64's, the rows from n on of the raw and tap buffers
    keep their sentinel, and nb_points_kernel<true, false> (sigma alone, no view direction, no latent bias) and <false, false> give
    the bits of <false, true> at every n."""
    q = dc.rows_case()
    n_all = len(q)
    w, g = dc.case_grid(q, "identity")
    ref, S, _ = dc.gather_f64(g.astype(np.float64), dc.distinct_volumes())
    dc.assert_gather_lattice(S)
    scene, weights = _lattice_scene("identity"), _realistic_weights()
    pts, vd = _dev(w), _dev(_directions(n_all))
    full, _ = _decode_abi(scene, weights, pts, vd, n_all, "dbg", n_all)
    assert np.isfinite(full).all() and len(np.unique(full[:, 3])) > n_all // 2
    sent = F32(dc.SENTINEL)
    for n in sc.row_counts(n_all, dc.ROW_COUNTS):
        raw, dbg = _decode_abi(scene, weights, pts, vd, n, "dbg", n_all)
        assert _same_numbers(dbg[:n, :352], ref[:n]), "n = %d: %s" % (n, _first_difference(dbg[:n, :352], ref[:n]))
        assert np.all(dbg[n:] == sent) and np.all(raw[n:] == sent), "n = %d: a row from n on was written" % n
        assert np.all(dbg[:n, :1594] != sent) and np.all(dbg[:n, 1594:] == sent)
        assert np.array_equal(raw[:n].view(np.uint32), full[:n].view(np.uint32)), "n = %d: raw depends on the row count" % n
        colour, _ = _decode_abi(scene, weights, pts, vd, n, "colour", n_all)
        assert np.array_equal(colour.view(np.uint32), raw.view(np.uint32)), "n = %d: <false, false> against <false, true>" % n
        sigma, _ = _decode_abi(scene, weights, pts, vd, n, "density", n_all)
        assert np.array_equal(sigma[:, 0].view(np.uint32), raw[:, 3].view(np.uint32)), "n = %d: <true, false> against <false, true>" % n


def test_odd_points_do_not_disturb_their_wave():
    """A NaN point and a point whose x is +inf inside a clustered wave: fminf / fmaxf drop the NaN from the box, the +inf stretches
    it to the last plane, the lanes' own indices clamp to -2 / size + 1 (every corner out of bounds, every address clamped into the
    tile).  The other points' features and sigma keep the bits they have without the two, and the two points' features are finite."""
    odd, plain, where = dc.odd_case()
    scene, weights = _lattice_scene("identity"), _realistic_weights()
    vd = _directions(len(odd))
    got = _decode(scene, weights, dc.world_points(odd, dc.POSES["identity"]), vd)
    want = _decode(scene, weights, dc.world_points(plain, dc.POSES["identity"]), vd)
    others = np.setdiff1d(np.arange(len(odd)), where)
    assert np.array_equal(_tap(got[1], "F")[others].view(np.uint32), _tap(want[1], "F")[others].view(np.uint32))
    assert np.array_equal(got[0][others, 3].view(np.uint32), want[0][others, 3].view(np.uint32))
    assert np.isfinite(_tap(got[1], "F")[list(where)]).all()
    ref, _, _ = dc.gather_f64(dc.case_grid(plain, "identity")[1].astype(np.float64), dc.distinct_volumes())
    assert _same_numbers(_tap(want[1], "F"), ref)


def _realistic_run():
    """the realistic scene decoded once with the realistic weights: dict of the scene, the view directions, raw and tap"""
    def make():
        s = dc.realistic_scene()
        vd = _directions(len(s["pts"]), 3)
        raw, dbg = _decode(_scene(s["vols"], s["pose"], s["voxel"], s["out_sh"]), _realistic_weights(), s["pts"], vd)
        return dict(scene=s, vd=vd, raw=raw, dbg=dbg)
    return _cached("realistic-run", make)


def test_gather_realistic_within_the_derived_bound():
    """BOUNDED.  |got - ref| <= (6 + 8) 2^-24 sum |w| |v| per element: index coordinates in fp32 by the kernel's own operations
    (grid_coords32, bwd_cases.unnormalize), weights and sums in float64; both gather paths occur on every level."""
    run = _realistic_run()
    s = run["scene"]
    ref, S, _ = dc.gather_f64(s["g"], s["vols"], index_dtype=F32)
    ratios = dc.gather_ratios(_tap(run["dbg"], "F"), ref, S)
    paths, _ = dc.wave_paths(s["g"], shapes=s["shapes"])
    print("realistic gather, %d points: worst |error| / bound per level: %s; waves on the tile per level: %s of %d" % (
        len(s["pts"]), ", ".join("%.3f" % r for r in ratios), [sum(p[l] == "T" for p in paths) for l in range(4)], len(paths)))
    assert max(ratios) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------------------------------- B
def _stages(raw, dbg):
    out = dict((name, _tap(dbg, name)) for name in ("h1", "h2", "h3", "G", "V"))
    out["sigma"], out["rgb"] = raw[:, 3:4], raw[:, :3]
    return out


def test_layers_exact_chain_bit_for_bit():
    """EXACT.  Voxel-centre points, integer volumes and sparse integer weights: F, h1, h2, h3, sigma, G (the merged layer the packer
    forms, with the bias of nb_mlp_latent_bias), V and rgb equal one float64 chain, each layer computed from the reference of the
    layer below."""
    p, code = dc.exact_params()
    q, v, vols = dc.exact_points()
    w, g = dc.case_grid(q, dc.B_POSE)
    F, S, _ = dc.gather_f64(g.astype(np.float64), vols)
    chain = dc.layer_chain(p, code, F, dc.raw_encodings(w, v))
    for stage in dc.STAGES:
        sc.assert_lattice(chain[stage][1] / dc.EXACT_UNIT[stage], 1.0)
    raw, dbg = _decode(_scene(vols, dc.POSES[dc.B_POSE]), _weights(p, code), w, v)
    assert _same_numbers(_tap(dbg, "F"), F)
    pe = _tap(dbg, "PE")
    assert np.array_equal(pe[:, 0:3].view(np.uint32), v.view(np.uint32)) and np.array_equal(pe[:, 27:30].view(np.uint32), w.view(np.uint32))
    got = _stages(raw, dbg)
    wrong = [s for s in dc.STAGES if not _same_numbers(got[s], chain[s][0])]
    assert not wrong, "%s: %s" % (wrong, _first_difference(got[wrong[0]], chain[wrong[0]][0]))


def test_encoding_columns_meet_their_weights():
    """EXACT.  view_fc = one +1 (then one -1) per row on encoding column r, r < 90, all else zero: V[:, r] = relu(+-PE[:, r]) in bits,
    rows 90 .. 127 stay zero.  Column c of the weights meets entry c of the encodings, for all 90."""
    pts, dirs = dc.pe_points()
    scene = _lattice_scene("identity")
    zero = np.zeros(128, F32)
    for sign in (1.0, -1.0):
        raw, dbg = _decode(scene, _weights(dc.pe_tie_params(sign), zero), pts, dirs)
        pe, V = _tap(dbg, "PE"), _tap(dbg, "V")
        assert np.isfinite(pe).all() and len(np.unique(pe, axis=1).T) == 90
        want = np.maximum(F32(sign) * pe, F32(0.0))
        assert np.array_equal(V[:, :90], want), "sign %+d: columns %s" % (sign, np.nonzero((V[:, :90] != want).any(0))[0])
        assert not V[:, 90:].any() and not raw.any()
        assert (want > 0).any(0).all(), "every column passes the ReLU somewhere"


def test_rgb_reads_every_view_column():
    """EXACT.  The realistic weights with rgb_fc = one +-1 per channel, walked over all 128 columns of V in 43 packs: the logits are
    +-V's bits, through the VALU tail and add_halves; every column of V is alive on these points."""
    s = dc.realistic_scene()
    p, code = dc.realistic_params()
    n = 256
    pts, vd = s["pts"][:n], _directions(n, 3)
    scene = _scene(s["vols"], s["pose"], s["voxel"], s["out_sh"])
    seen = set()
    for t in range(43):
        pt, cols, signs = dc.rgb_tie(p, t)
        raw, dbg = _decode(scene, _weights(pt, code), pts, vd)
        V = _tap(dbg, "V")
        assert np.array_equal(raw[:, :3], V[:, cols] * signs[None, :]), (t, cols)
        seen |= set(int(c) for c in cols if (V[:, c] > 0).any())
    assert len(seen) == 128, "V is alive in every column: %d" % len(seen)


def _pack_layout():
    """where the merged layer and its bias sit, found with probes: (lo, hi, natural flat index at each position of the merged
    section), natural index at each position of the latent bias"""
    def make():
        p = K.zero_params()
        p["feature_w"] = K.distinct_integers((256, 256), 46)
        p["latent_w"][:, :256] = np.eye(256, dtype=F32)
        sec = _weights(p, np.zeros(128, F32))[0].cpu().numpy()
        nz = np.nonzero(sec)[0]
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        assert hi - lo == 65536 and nz.size == 65536
        flat = np.argsort(p["feature_w"].reshape(-1))
        sigma = flat[sec[lo:hi].astype(np.int64) - 1]
        assert sorted(sigma.tolist()) == list(range(65536))
        b = K.zero_params()
        b["latent_b"] = np.arange(1, 257, dtype=F32)
        order = _weights(b, np.zeros(128, F32))[1].cpu().numpy()[:256].astype(np.int64) - 1
        assert sorted(order.tolist()) == list(range(256))
        return lo, hi, sigma, order
    return _cached("pack-layout", make)


def test_layers_realistic_within_the_derived_bound():
    """BOUNDED.  Every stage against the float64 product of the kernel's own tapped input (behind its ReLU), within
    (K + 2) 2^-24 (|b| + sum |w| |x|), K = 352, 256, 256, 256 (sigma), 256 (G), 346, 128 (rgb).  G takes the fp32 merged matrix and
    bias read back from the pack and nb_mlp_latent_bias (their rounding is the packer's, held by test_gpu_march_operands.py)."""
    run = _realistic_run()
    p, code = dc.realistic_params()
    packed, lb = _realistic_weights()
    lo, hi, sigma, order = _pack_layout()
    merged = np.empty(65536)
    merged[sigma] = packed.cpu().numpy()[lo:hi].astype(np.float64)
    lb_nat = np.empty(256)
    lb_nat[order] = lb.cpu().numpy()[:256].astype(np.float64)
    got = _stages(run["raw"], run["dbg"])
    inputs = {"h1": _tap(run["dbg"], "F"), "h2": got["h1"], "h3": got["h2"], "sigma": got["h3"], "G": got["h3"], "V": got["G"],
              "rgb": got["V"]}
    ref = dc.layer_chain(p, code, inputs["h1"], _tap(run["dbg"], "PE"), merged=merged.reshape(256, 256), lb=lb_nat, inputs=inputs)
    ratios = {}
    for stage in dc.STAGES:
        val, S = ref[stage]
        ratios[stage] = sc.worst_ratio(got[stage], val, dc.layer_bound(stage, S))
        if stage in ("h1", "h2", "h3", "V"):
            zeros = float((got[stage] == 0).mean())
            assert 0.2 <= zeros <= 0.8, (stage, zeros)
    print("realistic layers, %d points: worst |error| / bound per stage: %s" % (
        len(run["raw"]), ", ".join("%s %.3f" % (s, ratios[s]) for s in dc.STAGES)))
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------------------------------- C
def test_positional_encoding_against_float64():
    """BOUNDED.  |PE - sin / cos in float64 of the fp32 argument x 2^k| <= 4e-7 (the figure stated above sin_rev) over the arguments
    of decode_f32_cases.pe_points; the six raw columns are the inputs' bits."""
    pts, dirs = dc.pe_points()
    raw, dbg = _decode(_lattice_scene("identity"), _realistic_weights(), pts, dirs)
    pe = _tap(dbg, "PE")
    ref = dc.encodings_f64(pts, dirs)
    assert np.array_equal(pe[:, 0:3].view(np.uint32), dirs.view(np.uint32)), "the view direction's raw columns"
    assert np.array_equal(pe[:, 27:30].view(np.uint32), pts.view(np.uint32)), "the point's raw columns"
    err = np.abs(pe.astype(np.float64) - ref)
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    print("positional encoding, %d points: max |error| = %.3e (column %d, bound %.1e); per block: view %.3e, point %.3e" % (
        len(pts), err.max(), worst[1], dc.PE_TOL, err[:, :27].max(), err[:, 27:].max()))
    assert err.max() <= dc.PE_TOL, (err.max(), worst)
    assert np.all(np.abs(pe[:, 3:27]) <= 1.0) and np.all(np.abs(pe[:, 30:]) <= 1.0)


# ------------------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("S", dc.COMPOSITE_S)
def test_composite_against_float64(S, white):
    """BOUNDED.  weights, rgb, acc within tol(S) = (8 + S/2) 2^-24 of composite_f64, depth within tol(S) max z, acc = sum(weights) to
    the same bound, disp against disp_f64 of the kernel's own depth and acc with NaN exactly where acc == 0; n = 1, 3, 4, 5, 9 rays
    (four a workgroup) of the kinds of decode_f32_cases.RAY_KINDS.  Weights stay >= 0 and finite behind a saturated sample."""
    from neuralbody_amd import ops

    worst = {}
    for n in dc.COMPOSITE_N:
        raw, z, d, kinds = dc.composite_inputs(S, n)
        rgb, disp, acc, weights, depth = (t.cpu().numpy() for t in ops.composite(_dev(raw), _dev(z), _dev(d), white_bkgd=white))
        got = dict(weights=weights, rgb_map=rgb, acc_map=acc, depth_map=depth, disp_map=disp)
        assert np.isfinite(weights).all() and np.all(weights >= 0), (n, kinds)
        ratios = R.integrator_ratios(got, raw, z, d, white)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for r, kind in enumerate(kinds):
            if kind in ("no_density", "sigma_zero", "zero_direction"):
                assert acc[r] == 0 and not weights[r].any() and np.isnan(disp[r]), (n, kind)
    print("composite S = %d, %s background: worst |error| / bound: %s" % (
        S, "white" if white else "black", ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, worst
