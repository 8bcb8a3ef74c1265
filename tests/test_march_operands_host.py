"""The references and cases of the march-operand tests themselves (tests/march_operand_cases.py, tests/fold_stream_ref.py), on the CPU:
the reference quantisers at every grid point, midpoint and one fp32 ulp either side; that the lattice inputs are exact; that the case
tables reach every boundary of the fold kernel's workgroups; that the stream decoder accounts for every byte once."""
import math

import numpy as np
import pytest

from tests import fold_stream_ref as S
from tests import march_operand_cases as MC


def _ulp_neighbours(x):
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(-np.inf))), float(np.nextafter(x, np.float32(np.inf)))


@pytest.mark.parametrize("name", ["e2m1", "e2m3"])
def test_reference_quantisers_round_to_nearest_even_and_saturate(name):
    grid, code_of, top = {"e2m1": (S.E2M1_GRID, S.e2m1_code, 6.0), "e2m3": (S.E2M3_GRID, S.e2m3_code, 7.5)}[name]
    n = len(grid)
    assert list(grid) == sorted(grid) and grid[0] == 0.0 and grid[-1] == top and len(set(grid)) == n
    for sign, bit in ((1.0, 0), (-1.0, n)):
        for c, g in enumerate(grid):
            want = c + (bit if g != 0.0 else 0)  # -0.0 is not below zero
            assert int(code_of(sign * g)) == want, (sign, g)
        for c in range(n - 1):
            mid = 0.5 * (grid[c] + grid[c + 1])
            even = c if c % 2 == 0 else c + 1
            lo, hi = _ulp_neighbours(mid)
            assert int(code_of(sign * mid)) == even + bit, (sign, mid)
            assert int(code_of(sign * lo)) == c + bit and int(code_of(sign * hi)) == c + 1 + bit, (sign, mid)
        for big in (top, _ulp_neighbours(top)[1], 100.0, 3.2e38, np.inf):
            assert int(code_of(sign * big)) == n - 1 + bit
    assert int(code_of(-1e-9)) == n, "a negative value that rounds to zero keeps its sign bit"
    x = np.array([[0.26, -2.5], [7.0, 0.0]])
    assert code_of(x).shape == x.shape and code_of(x).dtype == np.uint8


def test_the_e2m1_midpoint_table_is_the_quantisers():
    assert [int(S.e2m1_code(m)) for m in MC.MIDPOINTS] == list(MC.MIDPOINT_CODES)
    assert np.array_equal(S.e2m1_code(MC.EDGE_ELEMENTS), MC.EDGE_CODES)
    assert np.array_equal(S.e2m1_value(MC.EDGE_CODES)[:2], [6.0, -6.0])


@pytest.mark.parametrize("top", [6.0, 7.5])
def test_reference_block_exponent(top):
    for e in range(-20, 21):
        exact = np.float32(top * 2.0 ** e)
        lo, hi = _ulp_neighbours(exact)
        assert S.block_exponent(exact, top) == e
        assert S.block_exponent(lo, top) == e
        assert S.block_exponent(hi, top) == e + 1
    assert S.block_exponent(0.0, top) == 0
    assert S.block_exponent(3.0e38, top) == 0 and S.block_exponent(np.inf, top) == 0 and S.block_exponent(3.2e38, top) == 0
    assert S.block_exponent(2.0 ** -140, top) == -120 and S.block_exponent(2.9e38, top) == 120
    # the definition itself, on a sweep: the smallest exponent that fits
    for a in np.random.RandomState(0).lognormal(0.0, 8.0, 200).astype(np.float32):
        ex = S.block_exponent(a, top)
        assert float(a) * 2.0 ** -ex <= top < float(a) * 2.0 ** -(ex - 1)


# ------------------------------------------------------------------------------------------------------------ nb_fold_build
def _chain32(v, w, order):
    """fp32 sum of the fp32 products v_k w_k, one rounding per operation, terms in `order`."""
    s = np.zeros((v.shape[0], w.shape[0]), np.float32)
    for k in order:
        s = (s + (v[:, k:k + 1] * w[None, :, k]).astype(np.float32)).astype(np.float32)
    return s


@pytest.mark.parametrize("scale_log2", MC.LATTICE_SCALES)
def test_lattice_products_are_exact_in_fp32(scale_log2):
    case = MC.VALUE_CASE
    fc0 = MC.lattice_fc0(1, scale_log2)
    rows = MC.lattice_rows(case, 2)
    unit = 2.0 ** (scale_log2 - 6)
    assert np.all(fc0 / unit == np.round(fc0 / unit)) and np.abs(fc0).max() == 2.0 ** scale_log2
    u64 = MC.fold_u64(rows, case, fc0)
    for l, k in enumerate(MC.live_rows(case)):
        v = rows[l][:k]
        assert np.all(v == np.round(v)) and np.abs(v).max() == 8 and 0.4 < (v == 0).mean() < 0.6
        w = fc0[:, MC.LEVEL_BASE[l]:MC.LEVEL_BASE[l] + MC.LEVEL_C[l]]
        c = MC.LEVEL_C[l]
        assert MC.fold_abs64(rows, case, fc0)[l].max() < 2.0 ** (11 + scale_log2)
        fwd, rev = _chain32(v, w, range(c)), _chain32(v, w, list(range(1, c, 2)) + list(range(c - 2, -1, -2)))
        assert np.array_equal(fwd.astype(np.float64), u64[l]) and np.array_equal(rev.astype(np.float64), u64[l])
        planes, off = MC.split_planes(u64[l])
        assert not off.any()
        if scale_log2 == 0:
            assert np.array_equal(MC.planes_value(planes), u64[l]), "head + remainder carry the 17 bits of an unscaled product"
            assert np.count_nonzero(planes[:, 256:]) > 20, "products of more than 11 bits: non-zero remainders"
        else:
            h = planes[:, :256].view(np.float16)
            assert np.all(np.abs(h[h != 0]) < 2.0 ** -3) and ((h != 0) & (np.abs(h) < 2.0 ** -14)).mean() > 0.001, "fp16 subnormal heads"
            r = u64[l].astype(np.float32) - h.astype(np.float32)
            if scale_log2 == -20:
                assert ((r != 0) & (np.abs(r) <= 2.0 ** -25)).mean() > 0.1, "remainders at and below half the fp16 subnormal quantum"
                assert (np.abs(r) == 2.0 ** -25).any(), "ties of the remainder's rounding"


def test_saturating_case_has_every_kind_of_offender():
    case = MC.VALUE_CASE
    fc0 = MC.lattice_fc0(1, 7)
    rows = MC.saturating_rows(case, 2, fc0)
    u64 = MC.fold_u64(rows, case, fc0)
    want, nan, n_off = MC.expected_planes(u64, case)
    bases, zero_row = MC.row_bases(case)
    assert np.isnan(u64[1][3]).all() and np.isnan(u64[1][2]).any() and np.isinf(u64[1][2]).any()
    assert all(np.isfinite(u64[l]).all() for l in (0, 2, 3))
    for l in range(4):
        u = u64[l][np.isfinite(u64[l])]
        assert np.all(u / 2 == np.round(u / 2)) and np.abs(u).max() < 2.0 ** 24 and (np.abs(u) > 65504).any()
        clamped = np.abs(u64[l]) > 65504
        got = want[bases[l]:bases[l] + u64[l].shape[0]]
        assert np.all(np.abs(got[:, :256].view(np.float16)[clamped]) == 65504) and np.all(got[:, 256:][clamped] == 0)
    assert n_off == sum(int((~(np.abs(u) <= 65504)).sum()) for u in u64) > 256 + 4
    assert nan.sum() == 2 * sum(int(np.isnan(u).sum()) for u in u64)


def test_single_offender_is_single():
    case = MC.VALUE_CASE
    fc0, rows = MC.single_offender(case, 11)
    u64 = MC.fold_u64(rows, case, fc0)
    l, r, f = MC.LONE_OFFENDER
    assert u64[l][r, f] == 2.0 ** 17 and r % 32 >= 4 and f % 64 != 0
    off = [np.argwhere(~(np.abs(u) <= 65504)).tolist() for u in u64]
    assert off == [[], [], [[r, f]], []]
    assert all(np.all(u / 2 == np.round(u / 2)) and np.abs(u).max() < 2.0 ** 24 for u in u64)
    assert MC.expected_planes(u64, case)[2] == 1


def test_fold_cases_reach_every_boundary_on_every_level():
    assert len(MC.FOLD_CASES) == 10
    for l in range(4):
        wg = MC.ROWS_WG[l]
        seen = [(min(case[l][0], case[l][1]),) + tuple(case[l]) for case in MC.FOLD_CASES]
        live = sorted(s[0] for s in seen)
        assert live == sorted([0, 1, 31, 32, 33, wg - 1, wg, wg + 1, wg + 2, 2 * wg + 1]), (l, live)
        # (level, live rows mod workgroup, whole workgroups): the classes a later edit must not drop
        assert {(k % wg, k // wg) for k in live} == {(0, 0), (1, 0), (31, 0), (32, 0), (33, 0), (wg - 1, 0), (0, 1), (1, 1), (2, 1), (1, 2)}
        assert (0, 0, 1) in seen, "no active row, capacity 1"
        assert sum(n == cap for _, n, cap in seen) >= 5, "capacity = count"
        assert any(n > cap for _, n, cap in seen), "a device count beyond the capacity"
        # workgroups whose first row is at or beyond the live rows
        assert any(-(-cap // wg) > max(-(-k // wg), 1) for k, _, cap in seen)
        assert any(0 < k and -(-cap // wg) >= -(-k // wg) + 2 for k, _, cap in seen)
    for case in MC.FOLD_CASES + (MC.VALUE_CASE,):
        caps = [cap for _, cap in case]
        assert len(set(caps)) == 4, "four different capacities in a call"
        assert len({(n, cap) for n, cap in case}) == 4
        assert sum(caps) + 1 + MC.SLACK_ROWS < 2000, "a few hundred rows"
    assert [min(n, cap) % 32 for n, cap in MC.VALUE_CASE] == [1, 1, 1, 0]


def test_scattered_rows_are_not_neighbours_and_the_rest_is_poison():
    case = MC.FOLD_CASES[2]
    rows = MC.lattice_rows(case, 3)
    for l, (vol, lin) in enumerate(MC.scatter_rows(rows, case, 4)):
        k = MC.live_rows(case)[l]
        assert lin.shape == (case[l][1],) and len(set(lin.tolist())) == lin.size and lin.max() < vol.shape[0]
        assert np.all(np.abs(np.diff(np.sort(lin))) >= 2)
        if k > 2:
            assert not np.all(np.diff(lin[:k]) > 0), "a permutation, not linear order"
        assert np.array_equal(vol[lin[:k]], rows[l][:k])
        rest = np.ones(vol.shape[0], bool)
        rest[lin[:k]] = False
        assert np.all(vol[rest] == MC.POISON) and np.all(rows[l][k:] == MC.POISON)


# ------------------------------------------------------------------------------------------------------------ the stream
def test_stream_constants():
    assert S.P_TOTAL == 132 and S.N_SCALE == 14 and S.WAVE_STREAM == 132 * 1024 + 4096
    assert S.PHASE_P0 == (0, 48, 96, 120, 132) and S.PHASE_S0 == (0, 4, 8, 12, 14)
    assert S.PACK_F32 == 333320 and S.PACK_SIZE == S.ABI_PACK_SIZE
    S.check_pack_size(S.ABI_PACK_SIZE)
    with pytest.raises(AssertionError, match="stream layout changed"):
        S.check_pack_size(S.ABI_PACK_SIZE + 4096)


def test_decoder_partitions_a_waves_share():
    n = S.attribution()
    assert n.shape == (3, S.WAVE_STREAM)
    assert np.all(n.sum(0) == 1), "every byte is piece data, a scale byte or padding, exactly once"
    assert int(n[0].sum()) == S.P_TOTAL * S.PIECE
    assert int(n[1].sum()) == 64 * sum(nb * 2 * mt for nb, mt in zip(S.PH_NB, S.PH_MT))
    assert int(n[2].sum()) == S.WAVE_STREAM - int(n[0].sum()) - int(n[1].sum())


def test_decoder_finds_every_weight_once_and_inverts_a_hand_packed_piece():
    """A zero stream decodes to zeros with every decoded place seen once; one fp16 written by hand where the packer's comment puts
    fc_1[64 w + 32 m + i][column of element 8 j + q of half-block ((b + w) & 3, kh)] comes back at that (row, column)."""
    z = np.zeros(S.N_WAVES * S.WAVE_STREAM, np.uint8)
    dec, free = S.decode(z)
    assert free.size == S.N_WAVES * int(S.attribution()[2].sum()) and not free.any()
    for ph, o in enumerate(dec):
        pc = S.phase_cols(ph)
        cols = np.unique(pc[pc >= 0])
        assert cols.size == (256 if ph < 3 else 90) and (ph < 3 or (cols.min() == 256 and cols.max() == 345))
        assert np.all(o["seen_h"][:, cols] == 1) and o["seen_h"].sum() == o["seen_h"].shape[0] * cols.size
        assert np.all(o["seen_c"][:, :, cols] == 1) and o["seen_c"].sum() == 2 * o["seen_h"].sum()
        pads = np.array([[np.all(pc[b, kh] < 0) for kh in range(2)] for b in range(S.PH_NB[ph])])
        assert np.all(o["seen_e"] == 1) and np.all(o["ex"] == -127)
        assert pads.sum() == (1 if ph == 3 else 0)
        assert o["pad_nonzero"] == 0
    w, b, j, m, lane, q = 3, 2, 1, 1, 37, 5
    piece = S.PHASE_P0[0] + b * S.block_pieces(2) + j * 2 + m
    z16 = z.view(np.uint16)
    z16[(w * S.WAVE_STREAM + piece * S.PIECE + lane * 16) // 2 + q] = np.float16(1.5).view(np.uint16)
    dec, _ = S.decode(z)
    row, col = 64 * w + 32 * m + (lane & 31), S.col_hidden(32 * ((b + w) & 3) + 8 * j + q, lane >> 5)
    assert dec[0]["heads"][row, col] == np.float16(1.5).view(np.uint16) and np.count_nonzero(dec[0]["heads"]) == 1


def test_stream_reference_on_the_edge_blocks():
    """expected() on the hand-made blocks of edge_params: the exponents and codes the docstring of edge_params promises."""
    p = MC.edge_params(5)
    exp = S.expected(S.phase_weights(p))[0]
    pc = S.phase_cols(0)

    def at(name):
        r, (b, kh) = MC.EDGE_BLOCKS[name]
        return r, b, kh, pc[b, kh]

    r, b, kh, c = at("head_midpoints")
    assert exp["ex"][0, r, b, kh] == 0 and np.array_equal(exp["code"][0][r, c[:16]], MC.EDGE_CODES) and not exp["code"][0][r, c[16:]].any()
    assert exp["ex"][1, r, b, kh] == 0 and not exp["code"][1][r, c].any()
    r, b, kh, c = at("rem_midpoints")
    assert np.all(exp["heads"][r, c] == np.float16(1.0).view(np.uint16))
    assert exp["ex"][1, r, b, kh] == -15 and np.array_equal(exp["code"][1][r, c[:16]], MC.EDGE_CODES)
    for name, e in (("amax_6", 3), ("amax_6_small", -9)):
        r, b, kh, c = at(name)
        assert exp["ex"][0, r, b, kh] == e and exp["code"][0][r, c[5]] == 15
        r, b, kh, c = at(name + "_up")
        assert exp["ex"][0, r, b, kh] == e + 1 and exp["code"][0][r, c[9]] == 5, "6 + one ulp under the next exponent is 3 + half an ulp"
    r, b, kh, c = at("zero")
    assert np.all(exp["ex"][:, r, b, kh] == 0) and not exp["code"][:, r, c].any() and not exp["heads"][r, c].any()
    r, b, kh, c = at("single")
    assert np.count_nonzero(exp["heads"][r, c]) == 1 and exp["ex"][0, r, b, kh] == -4 and exp["code"][0][r, c[13]] == 14
    r, b, kh, c = at("huge")
    assert np.all(exp["ex"][:, r, b, kh] == 0)
    assert exp["code"][0][r, c[4]] == 7 and exp["code"][0][r, c[20]] == 7 and exp["code"][1][r, c[4]] == 15
    assert exp["heads"][r, c[4]] == 0x7C00 and exp["heads"][r, c[20]] == 0x7C00


def test_fraction_counts_are_31_of_32():
    exp = S.expected(S.phase_weights(MC.fraction_params()))
    got = S.expected_stats(exp)
    assert got == MC.FRACTION_COUNTS
    assert got[0] * 32 == got[1] * 31 and got[2] * 32 == got[3] * 31 and got[4] * 346 == got[5] * 335


def test_fp64_sum_references():
    """The extended-precision references agree with a plain float64 product to float64's accuracy, the cancelling latent_b leaves a sum
    of ~2^-25 of its terms, and an fp32 accumulation of the same sum misses the bound the fp64 kernels are held to."""
    code = np.random.RandomState(8).standard_normal(128).astype(np.float32)
    p = MC.normal_params(7)
    ref, tot = MC.latent_bias_ref(p, code)
    x = np.concatenate([p["feature_b"], code]).astype(np.float64)
    plain = p["latent_b"].astype(np.float64) + p["latent_w"].astype(np.float64) @ x
    assert np.all(np.abs(plain - ref.astype(np.float64)) <= 2.0 ** -46 * tot.astype(np.float64))
    acc32 = p["latent_b"].copy()
    for k in range(384):
        acc32 = (acc32 + p["latent_w"][:, k] * x[k].astype(np.float32)).astype(np.float32)
    pc = MC.cancelling_params(7, code)
    cref, ctot = MC.latent_bias_ref(pc, code)
    assert np.all(np.abs(cref) <= 2.0 ** -24 * ctot) and np.median(np.abs(cref) / ctot) > 2.0 ** -30
    cacc = pc["latent_b"].copy()
    for k in range(384):
        cacc = (cacc + pc["latent_w"][:, k] * x[k].astype(np.float32)).astype(np.float32)
    bound = MC.fp64_sum_bound(cref, ctot).astype(np.float64)
    assert (np.abs(cacc - cref.astype(np.float64)) > bound).mean() > 0.9, "fp32 accumulation fails the cancelling case outright"
    assert (np.abs(acc32 - ref.astype(np.float64)) > MC.fp64_sum_bound(ref, tot).astype(np.float64)).mean() > 0.5
    vref, vtot = MC.view_bias_ref(p, code)
    assert vref.shape == (128,) and np.all(vtot >= np.abs(vref))
    assert math.isclose(float(vref[3]), float(p["view_b"][3] + p["view_w"][3, :256].astype(np.float64) @ plain), rel_tol=1e-12)
