"""Host-side checks of what tests/test_gpu_backward_kernels.py stands on (tests/bwd_cases.py): every lattice case meets its
precondition, the float64 references agree with torch on the CPU, and every case table reaches the kernel it names
(nb_gemm_variant swept over sizes, strides and alignments: all seven kernels, every threshold of the dispatch)."""
import os

import numpy as np
import pytest
import torch

from neuralbody_amd import build, ops
from tests import bwd_cases as bc
from tests import spconv_cases as sc

SPLIT = not os.environ.get("NB_BWD_SPLIT", "1").startswith("0")


def _expected_variant(ta, tb, m, n, k, a_ptr, lda, b_ptr, ldb, split=True):
    """include/nb_hip.h's rule (nb_sgemm, nb_gemm_fused, nb_gemm_variant), restated"""
    rows_aligned = lda % 4 == 0 and ldb % 4 == 0 and a_ptr % 16 == 0 and b_ptr % 16 == 0
    if ta:
        if k == 0:
            return "SCALE_ONLY"
        return "TN16" if split and m >= 32 and n >= 32 and k >= 1024 and rows_aligned else "TN"
    if k == 0 or k % 16 or not rows_aligned:
        return "ROWS"
    if split and not tb and k % 32 == 0 and m >= 1024:
        return "ROWS16"
    return "ROWS_FAST_T" if tb else "ROWS_FAST"


def _case_views(case):
    sa, sb = bc.stored_shapes(case)
    return bc.host_view(sa, case[6][0]), bc.host_view(sb, case[6][1])


def test_sparse_lattice_is_exact_on_both_arithmetics_with_different_answers():
    h, l = sc.split(np.array([bc.SPARSE, -bc.SPARSE, 0.0], np.float32), "bf16")
    assert h.tolist() == [1.0, -1.0, 0.0] and l.tolist() == [2.0 ** -9, -2.0 ** -9, 0.0]
    assert bc.SPARSE ** 2 == 1 + 2.0 ** -8 + 2.0 ** -18 and float(np.float32(bc.SPARSE ** 2)) == bc.SPARSE ** 2
    assert bc.KEEP * bc.SPARSE ** 2 < 64 and 64 / bc.UNIT["sparse"] == 2 ** 24
    for k in sorted(set(bc.FAST_K + bc.ROWS16_K + bc.TN_K + bc.TN16_K + (3, 129))):
        pos = bc.keep_positions(k)
        assert len(pos) <= bc.KEEP and len(np.unique(pos)) == len(pos) and pos.min() == 0 and pos.max() == k - 1
        if k > bc.KEEP:
            assert set((pos % 32).tolist()) == set(range(32)), "every slot of a 32-wide K chunk"
            assert set((pos // 1024).tolist()) == set(range((k + 1023) // 1024)), "every 1024-row block"
            if k <= 384:
                assert set((pos // 32).tolist()) == set(range((k + 31) // 32)), "every K chunk of the rows kernels"
            if k in bc.FAST_K:
                assert set((pos // 16).tolist()) == set(range(k // 16)), "every 16-wide K chunk of the aligned fp32 kernels"
            if k <= 2049:
                assert set((pos // 256).tolist()) == set(range((k + 255) // 256)), "every 256-row wave chunk of the fp32 split-K kernel"
    # the largest shape: both references are fp32 numbers and differ on most elements
    case = ("ROWS16", False, False, 2050, 384, 352, (4, 4))
    a, b = bc.operands(case, "sparse", np.random.RandomState(1))
    full, S = bc.product(case, a, b, "fp32")
    pairs, _ = bc.product(case, a, b, "pairs")
    sc.assert_lattice(S, bc.UNIT["sparse"])
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full) and np.array_equal(pairs.astype(np.float32).astype(np.float64), pairs)
    assert float((full != pairs).mean()) > 0.8
    assert np.array_equal(full - pairs, bc.product(case, a.l, b.l, "fp32")[0]), "the dropped term"
    for v in (a, b):  # an Operand's parts are spconv_cases.split's
        h, l = sc.split(v.x, "bf16")
        assert np.array_equal(h, v.h) and np.array_equal(l, v.l) and np.array_equal(v.h + v.l, v.x.astype(np.float64))
    ints = bc.operands(case, "int", np.random.RandomState(2))[0]
    h, l = sc.split(ints.x, "bf16")
    assert np.array_equal(h, ints.h) and not l.any() and not ints.l.any(), "integers -3 .. 3 are bf16 numbers"


def _check_preconditions(cases, lattices, seed):
    rs = np.random.RandomState(seed)
    worst = {}
    for case in cases:
        m, k, n = case[3:6]
        for lattice in lattices:
            a, b = bc.operands(case, lattice, rs)
            S = bc.product(case, a, b, "fp32")[1]
            c0 = np.full((m, n), 3.0)
            for alpha in (1.0, 2.0, 0.5):
                bc.assert_case_lattice(S, alpha * S + c0, lattice, alpha)
            worst[lattice] = max(worst.get(lattice, 0.0), float(S.max(initial=0.0)) / bc.UNIT[lattice])
    return worst


def test_lattice_preconditions_hold_for_every_gemm_case_the_gpu_file_runs():
    """with the worst C0 (|3| everywhere) and every alpha, whatever the epilogue a case takes"""
    fp32 = bc.rows_cases() + [c for tb in (False, True) for m in bc.FAST_M[tb] for c in bc.fast_cases(tb, m)] + \
        [c for k in bc.TN_K for c in bc.tn_cases(k)] + bc.split_off_cases()
    _check_preconditions(fp32, ("int", "sparse"), 1)
    pairs = [c for m in bc.ROWS16_M for c in bc.rows16_cases(m)] + [c for k in bc.TN16_K for c in bc.tn16_cases(k)]
    worst = _check_preconditions(pairs, ("int", "dense", "sparse"), 2)
    print("largest sum |a| |b| in units: %s of 2^24 = %d" % ({k: int(v) for k, v in worst.items()}, 2 ** 24))
    # integer column sums are exact for every case that compares them bit for bit (2050 rows x |C| <= 384 x 9 + 3)
    assert 2050 * (2 * 384 * 9 + 3) < 2 ** 24
    # colsum's own cases
    assert max(bc.COLSUM_ROWS) * 3 + 3 < 2 ** 24
    assert [bc.colsum_slabs(r) for r in bc.COLSUM_ROWS] == [1, 1, 4, 4, 8]


def test_one_sided_remainders_isolate_each_cross_term():
    case = ("TN16", True, False, 129, 1056, 33, (8, 4))
    rs = np.random.RandomState(3)
    for which in ("a", "b"):
        a, b = bc.operands(case, "dense", rs, remainders=which)
        (ah, al), (bh, bl) = sc.split(a.x, "bf16"), sc.split(b.x, "bf16")
        assert all(np.array_equal(p, q) for p, q in zip((ah, al, bh, bl), (a.h, a.l, b.h, b.l)))
        assert (al != 0).any() == (which == "a") and (bl != 0).any() == (which == "b")
        full, _ = bc.product(case, a, b, "fp32")
        pairs, _ = bc.product(case, a, b, "pairs")
        heads = ah.T @ bh
        assert np.array_equal(full, pairs) and float((pairs != heads).mean()) > 0.9, "the one cross term carries the whole remainder"


def test_gemm_reference_agrees_with_torch():
    rs = np.random.RandomState(4)
    for case in (("ROWS", False, True, 33, 19, 31, (2, 1)), ("ROWS_FAST", False, False, 129, 48, 130, (4, 4)), ("TN", True, False, 70, 257, 33, (4, 4))):
        m, k, n = case[3:6]
        sa, sb = bc.stored_shapes(case)
        a, b = rs.standard_normal(sa).astype(np.float32), rs.standard_normal(sb).astype(np.float32)
        c0, y = rs.standard_normal((m, n)).astype(np.float32), bc.mask_values(rs, (m, n))
        prod, S = bc.product(case, a, b, "fp32")
        ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        want = torch.matmul(ta.t() if case[1] else ta, tb.t() if case[2] else tb)
        np.testing.assert_allclose(prod, want.numpy(), rtol=0, atol=1e-12 * float(S.max()))
        C, cs, Sout = bc.epilogue(prod, S, 0.5, 1.0, c0, y)
        wt = torch.where(torch.from_numpy(y) > 0, 0.5 * want + torch.from_numpy(c0).double(), torch.zeros_like(want))
        np.testing.assert_allclose(C, wt.numpy(), rtol=0, atol=1e-12 * float(Sout.max()))
        np.testing.assert_allclose(cs, wt.sum(0).numpy(), rtol=0, atol=1e-12 * float(Sout.sum(0).max()))
        assert np.all(C[~(np.nan_to_num(y, nan=-1.0) > 0)] == 0) and (Sout >= np.abs(C) - 1e-12).all()
    # the mask decides every special value as torch's comparison does
    sp = torch.tensor(bc.SPECIALS, dtype=torch.float32)
    assert (sp > 0).tolist() == [False, False, False, True, True, True, False]
    y = bc.mask_values(rs, (64, 64))
    for v in bc.SPECIALS:
        assert (np.isnan(y).any() if v != v else ((y == np.float32(v)) & (np.signbit(y) == np.signbit(np.float32(v)))).any()), v
    for n in bc.RELU_N:
        y = bc.relu_values(rs, n)
        assert y.shape == (n,) and (n < 16 or (np.isnan(y).sum() == 2 and np.isinf(y).sum() == 2 and (y == np.float32(2.0 ** -140)).sum() == 2 and np.isnan(y[-1])))


def test_gemm_variant_over_sizes_strides_and_alignments():
    """every threshold of the dispatch from both sides, against the header's rule; all seven kernels are reached"""
    build.build(verbose=False)
    assert ops.GEMM_VARIANTS == bc.VARIANTS
    sizes = (1, 15, 16, 17, 31, 32, 33, 48, 64, 1023, 1024, 1025, 2047, 2048, 2049, 4200)
    buf = torch.empty(4200 * 4216 + 64, dtype=torch.float32)  # never touched: only addresses count
    assert buf.data_ptr() % 64 == 0

    def view(rows, cols, ld_mod, off):
        ld = cols + (-cols) % 4 + 4 + ld_mod
        return torch.as_strided(buf, (rows, cols), (ld, 1), off), ld

    seen, n_calls = set(), 0
    layouts = [(0, 0, 0, 0), (2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 0), (0, 0, 2, 0), (0, 0, 0, 1), (0, 0, 0, 2), (0, 0, 4, 4), (2, 2, 1, 1)]
    for ta, tb in ((False, False), (False, True), (True, False)):
        for m in sizes:
            for k in (0,) + sizes:
                for n in (1, 31, 32, 33):
                    for lda_mod, ldb_mod, a_off, b_off in layouts:
                        a, lda = view(*((k, m) if ta else (m, k)), lda_mod, a_off)
                        b, ldb = view(*((n, k) if tb else (k, n)), ldb_mod, b_off)
                        got = ops.gemm_variant(a, b, trans_a=ta, trans_b=tb)
                        want = _expected_variant(ta, tb, m, n, k, 4 * a_off, lda, 4 * b_off, ldb, SPLIT)
                        assert got == want, (ta, tb, m, n, k, lda, ldb, a_off, b_off, got, want)
                        seen.add(got)
                        n_calls += 1
    print("nb_gemm_variant: %d calls, kernels seen: %s" % (n_calls, sorted(seen)))
    assert seen == set(bc.VARIANTS) if SPLIT else seen == set(bc.VARIANTS) - {"TN16", "ROWS16"}
    # k % 16 and k % 32 on the aligned kernels
    for k in range(1, 130):
        a, _ = view(2050, k, 0, 0)
        b, _ = view(k, 64, 0, 0)
        want = "ROWS" if k % 16 else ("ROWS16" if k % 32 == 0 and SPLIT else "ROWS_FAST")
        assert ops.gemm_variant(a, b) == want, k
    with pytest.raises(ValueError):
        ops.gemm_variant(view(4, 5, 0, 0)[0], view(6, 7, 0, 0)[0])


def test_every_case_table_reaches_the_kernel_it_names():
    build.build(verbose=False)
    cases = bc.all_default_cases()
    assert {c[0] for c in cases} == set(bc.VARIANTS) - {"SCALE_ONLY"}
    for case in cases:
        a, b = _case_views(case)
        m, k, n = case[3:6]
        want = _expected_variant(case[1], case[2], m, n, k, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), True)
        assert want == case[0], case
        if SPLIT:
            assert ops.gemm_variant(a, b, trans_a=case[1], trans_b=case[2]) == case[0], case
    for case in bc.split_off_cases():
        a, b = _case_views(case)
        m, k, n = case[3:6]
        assert _expected_variant(case[1], case[2], m, n, k, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), False) == case[0], case
        assert _expected_variant(case[1], case[2], m, n, k, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), True) in ("ROWS16", "TN16"), case
    empty = bc.host_view((0, 128), 4), bc.host_view((0, 256), 4)
    assert ops.gemm_variant(*empty, trans_a=True) == "SCALE_ONLY"
    assert ops.gemm_variant(bc.host_view((128, 0), 4), bc.host_view((0, 256), 4)) == "ROWS"


def test_trilinear_lattice_scene_holds_what_the_kernel_can_get_wrong():
    s = bc.tri_lattice_scene()
    pts, dF, grids = s["pts"], s["d_feat"], s["grids"]
    n = len(pts)
    assert all(n % r for r in bc.TRI_RUNS if r > 1) and n > max(bc.TRI_RUNS)
    assert [tuple(g.shape) for g in grids] == list(bc.TRI_SHAPES)
    assert len({sh[a] for sh in bc.TRI_SHAPES for a in range(3)}) >= 5, "sizes differ per axis and level"
    for sh in bc.TRI_SHAPES:
        assert all((v - 1) & (v - 2) == 0 and v >= 3 for v in sh), "size - 1 a power of two"
    g = bc.tri_lattice_grid(s)
    g64 = np.stack([(pts[:, a].astype(np.float64) / bc.TRI_VOXEL[2 - a] / bc.TRI_OUT_SH[2 - a]) * 2 - 1 for a in range(3)], 1)
    assert np.array_equal(g.astype(np.float64), g64), "the normalised coordinates are fp32 numbers"
    kinds = {"inside": 0, "on_face": 0, "corner": 0, "near_low": 0, "near_high": 0, "far": 0}
    for l, sh in enumerate(bc.TRI_SHAPES):
        idx = [bc.unnormalize(g[:, a], sh[2 - a], np.float32) for a in range(3)]  # x, y, z
        idx64 = [bc.unnormalize(g64[:, a], sh[2 - a]) for a in range(3)]
        assert all(np.array_equal(i.astype(np.float64), j) for i, j in zip(idx, idx64)), "the index coordinates are fp32 numbers"
        den = [4 * bc.TRI_OUT_SH[2 - a] // (sh[2 - a] - 1) for a in range(3)]
        assert all(np.array_equal(i * d, np.round(i * d)) for i, d in zip(idx64, den)) and int(np.prod(den)) == bc.tri_weight_denominator(l)
        assert bc.tri_weight_denominator(l) <= 2 ** 15
        if l == 0:
            size = [sh[2], sh[1], sh[0]]
            ins = np.all([(i > 0) & (i < s_ - 1) for i, s_ in zip(idx64, size)], 0)
            face = np.any([(i == 0) | (i == s_ - 1) for i, s_ in zip(idx64, size)], 0)
            corner = np.all([(i == 0) | (i == s_ - 1) for i, s_ in zip(idx64, size)], 0)
            kinds["inside"], kinds["on_face"], kinds["corner"] = int(ins.sum()), int(face.sum()), int(corner.sum())
            kinds["near_low"] = int(np.any([(i > -1) & (i < 0) for i in idx64], 0).sum())
            kinds["near_high"] = int(np.any([(i > s_ - 1) & (i < s_) for i, s_ in zip(idx64, size)], 0).sum())
            kinds["far"] = int(np.any([(i < -2) | (i > s_ + 1) for i, s_ in zip(idx64, size)], 0).sum())
            base0 = np.stack([np.floor(i) for i in idx64], 1)[:20]
        if l == 3:
            base3 = np.stack([np.floor(i) for i in idx64], 1)[:20]
        assert (grids[l] < 0).any() and (grids[l] >= 0).sum() == s["n_rows"][l]
    assert kinds["corner"] == 8 and kinds["far"] >= 6 and kinds["near_low"] >= 6 and kinds["near_high"] >= 6 and kinds["inside"] >= 20, kinds
    assert kinds["on_face"] >= 26
    change0, change3 = (np.diff(base0, axis=0) != 0).any(1), (np.diff(base3, axis=0) != 0).any(1)
    assert change0.sum() > change3.sum() and (~change3).sum() >= 10, "the walk shares its base voxel on the coarse level, not on the fine one"
    groups = dF.reshape(n, 88, 4)
    zero = (groups == 0).all(2)
    assert zero.any() and any(zero[p].any() and not zero[p].all() for p in range(n)), "a point whose group is zero on some levels only"
    drows, S, K = bc.trilinear_scatter(g, dF, grids)
    bc.assert_tri_lattice(S)
    for l in range(4):
        assert np.array_equal(drows[l].astype(np.float32).astype(np.float64), drows[l]) and np.abs(drows[l]).max() > 0
    # fp32 and float64 index coordinates give the same reference here
    again = bc.trilinear_scatter(g, dF, grids, index_dtype=np.float32)[0]
    assert all(np.array_equal(p, q) for p, q in zip(drows, again))


def test_trilinear_reference_agrees_with_grid_sample_autograd():
    s = bc.tri_lattice_scene()
    g = bc.tri_lattice_grid(s).astype(np.float64)
    for name, (gg, dF, grids) in (("lattice", (g, s["d_feat"], s["grids"])), ("random", bc.random_tri_scene())):
        got, S, _ = bc.trilinear_scatter(gg, dF, grids)
        want = bc.autograd_scatter(gg, dF, grids)
        for l in range(4):
            assert got[l].shape == want[l].shape
            err = float(np.abs(got[l] - want[l]).max())
            assert err <= 1e-12 * max(float(S[l].max()), 1.0), (name, l, err)
            assert np.abs(want[l]).max() > 0


def test_trilinear_realistic_scene():
    s = bc.tri_realistic_scene()
    n = len(s["pts"])
    assert n % s["run"] == 0 and 2000 <= n <= 20000, n
    g = bc.fp32_grid(s["pts"], s["bounds_min"], s["voxel_size"], s["out_sh"])
    drows, S, K = bc.trilinear_scatter(g, s["d_feat"], s["grids"], index_dtype=np.float32)
    for l in range(4):
        assert K[l].max() > 4 and np.abs(drows[l]).max() > 0 and s["n_rows"][l] == drows[l].shape[0]
    inside = np.all(np.abs(g) <= 1, 1).mean()
    assert 0.3 < inside < 1.0, "points inside and outside the volume"
