"""Every kernel of the decoder's backward (csrc/nb_backward.hip) against a float64 reference of the same operation, at the sizes its
tiles make interesting (32 x 32 for the fp32 split-K kernel, 128 x 128 for the others, 1024-row blocks), through ops.sgemm,
ops.colsum, ops.relu_bwd_, ops.trilinear_bwd and ops.composite_bwd only.  Inputs, references, lattices and bounds:
tests/bwd_cases.py (its preconditions are asserted on the CPU by tests/test_bwd_kernel_cases_host.py).  A lattice case is compared
element for element as numbers (the sign of a zero is not looked at); every GEMM case first asserts the kernel the dispatch picks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bwd_cases as bc
from tests import bwd_device as bd
from tests import spconv_cases as sc

pytestmark = pytest.mark.gpu
DEV = bd.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(res, what=""):
    assert res["guards"], "%s %s: the columns beside the destination slice changed" % (res, what)
    assert res["exact"], "%s %s: differs from the float64 reference" % (res, what)
    assert res.get("colsum_exact", True), "%s %s: column sums differ from the float64 reference" % (res, what)
    return res.get("colsum_ratio", 0.0)


def _with_epilogues(cases, lattices, seed, remainders="both", epilogues=bc.EPILOGUES):
    """every case x lattice x epilogue; -> the worst column-sum error / bound of the launches held to the bound"""
    rs = np.random.RandomState(seed)
    worst, n = 0.0, 0
    for case in cases:
        for lattice in lattices:
            prep = bd.prepare(case, lattice, rs, remainders)
            for name in epilogues:
                mask, colsum, alpha, beta = bc.epilogue_args(name)
                ratio = _check(bd.run(prep, rs, alpha, beta, mask, colsum, expect=case[0]), name)
                assert ratio <= 1.0, (case, lattice, name, ratio)
                worst, n = max(worst, ratio), n + 1
    print("%d launches of %s; column sums held to n_rows 2^-24 sum |C|: worst error / bound %.3f" % (n, cases[0][0], worst))
    return worst


# ------------------------------------------------------------------------------------------------------------------ (a) .. (e)
def test_general_kernel():
    """(a) gemm_rows_kernel: ragged everything, op(B) = B and B^T, strided operands and destination; the aligned-looking shape
    reaches it by a 4-byte offset of A and by an 8-byte offset of B"""
    _with_epilogues(bc.rows_cases(), ("int", "sparse"), 100)


@pytest.mark.parametrize("m", bc.FAST_M[False])
def test_aligned_fp32_kernel(m):
    """(b) gemm_rows_fast_kernel<false>: one, an odd number of and many K chunks; n around the 128-column tile"""
    _with_epilogues(bc.fast_cases(False, m), ("int", "sparse"), 200 + m)


@pytest.mark.parametrize("m", bc.FAST_M[True])
def test_aligned_fp32_kernel_transposed_b(m):
    """(b) gemm_rows_fast_kernel<true>, which takes any m"""
    _with_epilogues(bc.fast_cases(True, m), ("int", "sparse"), 300 + m)


@pytest.mark.parametrize("m", bc.ROWS16_M)
def test_bf16_pair_rows_kernel(m):
    """(c) gemm_rows16_kernel against three_products (dense and sparse two-part lattices; integers for exact column sums)"""
    _with_epilogues(bc.rows16_cases(m), ("int", "dense", "sparse"), 400 + m)
    # remainders on one operand only: a dropped a_l b_h and a dropped a_h b_l each fail alone
    one = [("ROWS16", False, False, m, k, n, (4, 4)) for k, n in ((96, 260), (384, 127))]
    for which in ("a", "b"):
        _with_epilogues(one, ("dense",), 450 + m, remainders=which, epilogues=("none", "mask+colsum+beta"))


@pytest.mark.parametrize("k", bc.TN_K)
def test_split_k_fp32_kernel(k):
    """(d) gemm_tn_kernel: alpha = 2 into a beta = 1 slice, and beta = 0 over NaN"""
    rs = np.random.RandomState(500 + k)
    for i, case in enumerate(bc.tn_cases(k)):
        for lattice in ("int", "sparse"):
            prep = bd.prepare(case, lattice, rs)
            _check(bd.run(prep, rs, alpha=2.0, beta=1.0, expect="TN"))
            if i % 4 == 0:
                _check(bd.run(prep, rs, alpha=1.0, beta=0.0, expect="TN"))


@pytest.mark.parametrize("k", bc.TN16_K)
def test_split_k_bf16_pair_kernel(k):
    """(e) gemm_tn16_kernel against three_products: alpha = 0.5 accumulated into a slice; one-sided remainders"""
    rs = np.random.RandomState(600 + k)
    for case in bc.tn16_cases(k):
        for lattice, rem in (("dense", "both"), ("dense", "a"), ("dense", "b"), ("sparse", "both"), ("int", "both")):
            prep = bd.prepare(case, lattice, rs, rem)
            _check(bd.run(prep, rs, alpha=0.5, beta=1.0, expect="TN16"), rem)
        _check(bd.run(prep, rs, alpha=1.0, beta=0.0, expect="TN16"))


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_empty_products_and_beta_zero_over_nan():
    """k = 0 in both forms (C = beta C and the epilogue); beta = 0 over a NaN-filled destination on every kernel (bd.run fills
    it so whenever beta is 0: no NaN survives, or `exact` fails); m == 0 and n == 0 touch nothing"""
    from neuralbody_amd import ops

    rs = np.random.RandomState(700)
    for beta in (0.0, 1.0):
        prep = bd.prepare(("ROWS", False, False, 130, 0, 70, (4, 4)), "int", rs)
        _check(bd.run(prep, rs, 1.0, beta, mask=True, colsum=True, expect="ROWS"))
        prep = bd.prepare(("ROWS", False, True, 130, 0, 70, (4, 4)), "int", rs)
        _check(bd.run(prep, rs, 2.0, beta, expect="ROWS"))
        prep = bd.prepare(("SCALE_ONLY", True, False, 70, 0, 130, (4, 4)), "int", rs)
        _check(bd.run(prep, rs, 2.0, beta, expect="SCALE_ONLY"))
    one_of_each = (("ROWS", False, False, 33, 3, 31, (2, 1)), ("ROWS_FAST", False, False, 129, 48, 130, (4, 4)),
                   ("ROWS_FAST_T", False, True, 129, 48, 130, (4, 4)), ("ROWS16", False, False, 1025, 96, 260, (4, 4)),
                   ("TN", True, False, 33, 257, 70, (4, 4)), ("TN16", True, False, 129, 1056, 33, (8, 4)))
    for case in one_of_each:
        res = bd.run(bd.prepare(case, "int", rs), rs, 1.0, 0.0, expect=case[0])
        _check(res)
    # m == 0, n == 0: nothing is launched, nothing changes
    guard = torch.full((8, 16), bc.GUARD, device=DEV)
    cs = torch.full((5,), 2.5, device=DEV)
    ones = torch.ones((16, 16), device=DEV)  # (an empty slice's data pointer is NULL: an empty result must not need its operands)
    ops.sgemm(ones[:0, :16], ones[:16, :5], out=guard[:0, 3:8], beta=0.0, relu_mask=guard[:0, 1:6], colsum=cs)
    ops.sgemm(ones[:8, :16], ones[:16, 3:3], out=guard[:, 3:3], beta=0.0)
    ops.sgemm(ones[:16, 3:3], ones[:16, :5], trans_a=True, out=guard[:0, 3:8], beta=0.0)
    assert bool((guard == bc.GUARD).all()) and bool((cs == 2.5).all())


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_split_switched_off_in_a_fresh_process():
    """NB_BWD_SPLIT=0 (read once per process): the large shapes of (c) and (e) run on the fp32 kernels and equal the FULL product
    on the sparse two-part lattice, where the pair kernels' answer differs on most elements"""
    env = dict(os.environ, NB_BWD_SPLIT="0")
    out = subprocess.run([sys.executable, "-m", "tests.bwd_device"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, "the child ended with status %s:\n%s" % (out.returncode, out.stderr[-3000:])
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 * len(bc.split_off_cases())
    for res, case in zip(lines, [c for c in bc.split_off_cases() for _ in range(2)]):
        assert res["case"] == list(case[:6]) and res["variant"] == case[0] and case[0] in ("ROWS_FAST", "TN"), res
        print(res)
        _check(res)
        assert res.get("colsum_ratio", 0.0) <= 1.0, res
    assert {r["lattice"] for r in lines} == {"sparse", "int"} and {r["variant"] for r in lines} == {"ROWS_FAST", "TN"}


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_colsum_on_both_sides_of_the_slab_switch():
    from neuralbody_amd import ops

    rs = np.random.RandomState(800)
    for n_rows in bc.COLSUM_ROWS:
        wide = sc.lattice32(rs, (n_rows, 90))
        xd = bd.dev(wide)
        for n_cols in bc.COLSUM_COLS:
            out0 = sc.lattice32(rs, (n_cols,)) + 0.5
            got = ops.colsum(xd[:, 5:5 + n_cols], out=bd.dev(out0)).cpu().numpy()
            ref = out0.astype(np.float64) + wide[:, 5:5 + n_cols].astype(np.float64).sum(0)
            assert bd.same_numbers(got, ref), (n_rows, n_cols)
    # realistic: fp64 partials per slab, so only the conversions of the partials and the atomic additions round
    n_rows, n_cols = 9000, 83
    x = rs.standard_normal((n_rows, 90)).astype(np.float32)
    got = ops.colsum(bd.dev(x)[:, 5:5 + n_cols]).cpu().numpy().astype(np.float64)
    x64 = x[:, 5:5 + n_cols].astype(np.float64)
    bound = (bc.colsum_slabs(n_rows) + 1) * 2.0 ** -24 * np.abs(x64).sum(0)
    ratio = float(np.max(np.abs(got - x64.sum(0)) / bound))
    print("colsum 9000 x 83 normals: worst error / ((slabs + 1) 2^-24 sum |x|) = %.3f" % ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("n", bc.RELU_N)
def test_relu_bwd_decides_zero_nan_and_subnormals_as_torch_does(n):
    """dy = y > 0 ? dy : 0 with y holding 0.0, -0.0, NaN, 2^-126, the subnormal 2^-140 and +-inf: bit for bit torch.where on the CPU
    (F.relu's backward passes the gradient where the output is > 0: a subnormal output counts as positive)"""
    from neuralbody_amd import ops

    rs = np.random.RandomState(900 + n)
    y, dy = bc.relu_values(rs, n), rs.standard_normal(n).astype(np.float32)
    want = torch.where(torch.from_numpy(y) > 0, torch.from_numpy(dy), torch.zeros(n))
    got = ops.relu_bwd_(bd.dev(dy), bd.dev(y)).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, got, want)
    # (the same values decide the relu_mask epilogue of every masked GEMM case above: bc.mask_values strews them in)


# ------------------------------------------------------------------------------------------------------------------ (j)
def _tri_scene(shapes, bounds_min, voxel_size, out_sh):
    from neuralbody_amd import ops

    vols = [torch.zeros(tuple(sh) + (c,), device=DEV) for sh, c in zip(shapes, bc.LEVEL_CHANNELS)]  # not read by the backward
    pose = ops.make_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.asarray(bounds_min, np.float32), device=DEV)
    return ops.make_scene(vols, pose, voxel_size, out_sh)


def _tri_run(scene, s, run):
    from neuralbody_amd import ops

    grids = [bd.dev(g) for g in s["grids"]]
    drows = [torch.zeros((r, c), device=DEV) for r, c in zip(s["n_rows"], bc.LEVEL_CHANNELS)]
    ops.trilinear_bwd(scene, grids, drows, bd.dev(s["pts"]), bd.dev(s["d_feat"]), run_length=run)
    return [d.cpu().numpy() for d in drows]


def test_trilinear_bwd_on_the_lattice_scene():
    """points inside, on every face, edge and corner, just outside each side, far outside (the clamp), a walk that keeps its base
    voxel on the coarse levels only, inactive corners, dF groups zero on some levels: every run length gives the reference's bits"""
    s = bc.tri_lattice_scene()
    ref, S, _ = bc.trilinear_scatter(bc.tri_lattice_grid(s), s["d_feat"], s["grids"])
    bc.assert_tri_lattice(S)
    scene = _tri_scene(bc.TRI_SHAPES, (0.0, 0.0, 0.0), bc.TRI_VOXEL, bc.TRI_OUT_SH)
    n = len(s["pts"])
    for run in bc.TRI_RUNS + (n, n + 5):
        got = _tri_run(scene, s, run)
        for l in range(4):
            assert bd.same_numbers(got[l], ref[l]), "run_length %d, level %d: %d elements differ" % (
                run, l, int((got[l] != ref[l].astype(np.float32)).sum()))


def test_trilinear_bwd_on_the_synthetic_scene():
    """sample points of the synthetic body's rays, normal dF, against the float64 scatter within c sum |w| |dF| (bc.c_trilinear)"""
    s = bc.tri_realistic_scene()
    g = bc.fp32_grid(s["pts"], s["bounds_min"], s["voxel_size"], s["out_sh"])
    ref, S, K = bc.trilinear_scatter(g, s["d_feat"], s["grids"], index_dtype=np.float32)
    scene = _tri_scene([gr.shape for gr in s["grids"]], s["bounds_min"], s["voxel_size"], s["out_sh"])
    for run in (1, s["run"]):
        got = _tri_run(scene, s, run)
        for l in range(4):
            c = bc.c_trilinear(K[l].max())
            ratio = sc.worst_ratio(got[l], ref[l], S[l]) / c
            print("trilinear backward, run_length %d, level %d: worst error / (c sum |w| |dF|) = %.3f (c = %.2e, K = %d)" % (
                run, l, ratio, c, K[l].max()))
            assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------ (k)
def _composite_case(raw, z, d, white, cots, name):
    from neuralbody_amd import ops
    from oracle import neuralbody_oracle as orc

    raw64 = torch.from_numpy(raw).double().requires_grad_(True)
    raw_in, z_in = raw64, torch.from_numpy(z).double()
    if raw.shape[1] == 1:
        # raw2outputs, like the reference's own, gives the 1e10 column the shape of a slice of `dists`, which is empty for one
        # sample: every map is then an empty sum.  The kernels (forward and backward alike) give a lone sample the dist 1e10 |d|
        # that the last sample of any ray has, so its reference is the same function on two samples, the second one without
        # density at z + 1e10: it weighs nothing and makes the first sample's dist 1e10 |d|.
        assert orc.raw2outputs(raw64, z_in, torch.from_numpy(d).double(), white)[3].numel() == 0
        nothing = torch.tensor([0.0, 0.0, 0.0, -1.0], dtype=torch.float64).expand(raw.shape[0], 1, 4)
        raw_in, z_in = torch.cat([raw64, nothing], 1), torch.cat([z_in, z_in + 1e10], 1)
    rgb, _, acc, _, depth = orc.raw2outputs(raw_in, z_in, torch.from_numpy(d).double(), white)
    g_rgb, g_acc, g_dep = cots
    loss = (rgb * torch.from_numpy(g_rgb).double()).sum()
    if g_acc is not None:
        loss = loss + (acc * torch.from_numpy(g_acc).double()).sum() + (depth * torch.from_numpy(g_dep).double()).sum()
    loss.backward()
    ref = raw64.grad.numpy()
    got = ops.composite_bwd(bd.dev(raw), bd.dev(z), bd.dev(d), bd.dev(g_rgb), white, None if g_acc is None else bd.dev(g_acc),
                            None if g_dep is None else bd.dev(g_dep)).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    # where the float64 reference itself is inf or NaN the device must give the same class; elsewhere the 2e-5 criterion of
    # test_gpu_backward._rel: max |diff| over the largest finite reference entry
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and \
        np.array_equal(np.isneginf(got), np.isneginf(ref)), name
    scale = max(float(np.abs(ref[finite]).max(initial=0.0)), 1e-30)
    err = float(np.abs(got[finite] - ref[finite]).max(initial=0.0)) / scale
    assert err <= 2e-5, "%s: max |diff| / max |ref| = %.3e (ref max %.3e)" % (name, err, scale)
    return err


@pytest.mark.parametrize("white", [False, True])
def test_composite_bwd_edges(white):
    """S = 1; 1, 64 and 65 rays (one thread each, 64 a workgroup); all sigma <= 0; alpha saturated before the last sample; a zero ray
    direction; all three cotangents and rgb alone"""
    rs = np.random.RandomState(1000 + white)
    worst = 0.0
    for n, S in ((1, 1), (64, 1), (65, 1), (1, 24), (64, 24), (65, 24)):
        raw = (rs.standard_normal((n, S, 4)) * 2).astype(np.float32)
        z = np.sort(rs.uniform(1, 3, (n, S)).astype(np.float32), axis=1)
        d = rs.standard_normal((n, 3)).astype(np.float32)
        if n > 1:                                   # (a lone ray keeps its random densities)
            raw[0, :, 3] = -np.abs(raw[0, :, 3])    # ray 0: no density anywhere
            raw[1, :, 3] = 0.0                      # ray 1: sigma == 0
            raw[2, S // 3, 3] = 3e4                 # ray 2: alpha saturates at a third of the way
            raw[3, :, 3] = 1e3                      # ray 3: saturated from the first sample on
            d[4] = 0.0                              # ray 4: a zero direction (every dist is 0)
        else:
            raw[0, 0, 3] = abs(raw[0, 0, 3]) + 0.1      # ... with density on its first sample
        cots = (rs.standard_normal((n, 3)).astype(np.float32), rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32))
        worst = max(worst, _composite_case(raw, z, d, white, cots, "n=%d S=%d, three cotangents" % (n, S)))
        worst = max(worst, _composite_case(raw, z, d, white, (cots[0], None, None), "n=%d S=%d, rgb only" % (n, S)))
    print("composite backward edges, white_bkgd=%s: worst max |diff| / max |ref| = %.2e" % (white, worst))
