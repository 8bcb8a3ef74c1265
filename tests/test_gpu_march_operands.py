"""The four kernels that prepare what the f16f6 march multiplies, each on its own against numpy / float64 (cases and references:
tests/march_operand_cases.py, tests/fold_stream_ref.py): nb_fold_build bit for bit on lattice inputs at every workgroup boundary, the
fp32 section of nb_mlp_pack_sections and nb_mlp_latent_bias through a layout discovered with probes, and the f16f6 weight stream
decoded back into heads, four-bit codes and block exponents.  The library is called through the C ABI on caller-owned, sentinel-filled
buffers; nothing here needs a scene, a renderer or a ray."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fold_stream_ref as S
from tests import march_operand_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_SENTINEL = -7777.0


def _stream_arg():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------ nb_fold_build
def _fold_call(case, rows, fc0, gathered, n_sat0, seed=9):
    """One nb_fold_build on a SENTINEL16-filled plane buffer with SLACK_ROWS rows behind the zero row.  Level l takes its rows compact
    (rows_lin NULL) or, where gathered[l], through rows_lin from a poisoned dense volume.  Returns (planes uint16, n_saturated)."""
    from neuralbody_amd import _lib

    scattered = MC.scatter_rows(rows, case, seed)
    bases, zero_row = MC.row_bases(case)
    v4, l4, n4, caps = (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_int32 * 4)()
    keep = []
    for l, (n, cap) in enumerate(case):
        if gathered[l]:
            vol, lin = (torch.from_numpy(a).to(DEV) for a in scattered[l])
            v4[l], l4[l] = vol.data_ptr(), lin.data_ptr()
            keep += [vol, lin]
        else:
            r = torch.from_numpy(rows[l]).to(DEV)
            v4[l], l4[l] = r.data_ptr(), None
            keep.append(r)
        cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
        keep.append(cnt)
        n4[l], caps[l] = cnt.data_ptr(), cap
    w = torch.from_numpy(np.ascontiguousarray(fc0)).to(DEV)
    planes = torch.full((zero_row + 1 + MC.SLACK_ROWS, 512), MC.SENTINEL16 - 65536, dtype=torch.int16, device=DEV)
    n_sat = torch.tensor([n_sat0], dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().nb_fold_build(v4, l4, n4, caps, _lib.ptr(w), _lib.ptr(planes), _lib.ptr(n_sat), _stream_arg()), "nb_fold_build")
    torch.cuda.synchronize()
    return planes.cpu().numpy().view(np.uint16), int(n_sat)


def _fold_twice(case, rows, fc0, gathered, n_sat0=0):
    got, n_sat = _fold_call(case, rows, fc0, gathered, n_sat0)
    again, n_again = _fold_call(case, rows, fc0, gathered, n_sat0)
    assert np.array_equal(got, again) and n_again == n_sat, "two calls give equal bits"
    return got, n_sat


def _assert_planes(got, want, nan=None):
    """Bit for bit: the live rows, the sentinel in [row_base + n, row_base + cap), the zero row, the sentinel behind it."""
    if nan is not None and nan.any():
        assert np.all(np.isnan(got.view(np.float16)[nan])), "a NaN product is a NaN in both planes"
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d entries differ, the first at plane row %d, column %d: got %#06x, want %#06x" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def _sources(swap):
    return [(l + swap) % 2 == 1 for l in range(4)]


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("c", range(len(MC.FOLD_CASES)))
def test_fold_lattice_rows_at_every_workgroup_boundary(c, swap):
    """EXACT.  Integer V, fc_0 on multiples of 2^-6: both planes bit for bit; the rows between count and capacity, the zero row and the
    rows behind it; levels alternate between compact rows and rows gathered through rows_lin (swap exchanges them).  The saturation
    counter is added to (it starts from 5 in the odd cases) and nothing is added."""
    case = MC.FOLD_CASES[c]
    fc0 = MC.lattice_fc0(100 + c)
    rows = MC.lattice_rows(case, 200 + c)
    want, _, n_off = MC.expected_planes(MC.fold_u64(rows, case, fc0), case)
    assert n_off == 0
    start = 5 * (c & 1)
    got, n_sat = _fold_twice(case, rows, fc0, _sources(swap), start)
    _assert_planes(got, want)
    assert n_sat == start


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("scale_log2", MC.LATTICE_SCALES[1:])
def test_fold_lattice_subnormal_planes(scale_log2, swap):
    """EXACT.  fc_0 scaled by 2^-14 (subnormal heads) and 2^-20 (remainders at and below half the subnormal quantum, ties included):
    both conversions round to nearest even into fp16 subnormals, as numpy's do."""
    case = MC.VALUE_CASE
    fc0 = MC.lattice_fc0(1, scale_log2)
    rows = MC.lattice_rows(case, 2)
    want, _, n_off = MC.expected_planes(MC.fold_u64(rows, case, fc0), case)
    got, n_sat = _fold_twice(case, rows, fc0, _sources(swap))
    _assert_planes(got, want)
    assert n_off == 0 and n_sat == 0


@pytest.mark.parametrize("swap", [0, 1])
def test_fold_saturation_is_clamped_and_counted(swap):
    """EXACT planes: +-65504 heads with zero remainders where the product left the fp16 range (a +inf voxel included), NaN where IEEE
    arithmetic gives one (the NaN voxel's row, and 0 . inf).  The counter: added to (from 5), not zero, at most the offending products
    (it counts the lanes that saw one)."""
    case = MC.VALUE_CASE
    fc0 = MC.lattice_fc0(1, 7)
    rows = MC.saturating_rows(case, 2, fc0)
    want, nan, n_off = MC.expected_planes(MC.fold_u64(rows, case, fc0), case)
    got, n_sat = _fold_twice(case, rows, fc0, _sources(swap), 5)
    _assert_planes(got, want, nan)
    print("saturation case: n_saturated = %d (5 before the call), %d offending products" % (n_sat, n_off))
    assert 5 < n_sat <= 5 + n_off


@pytest.mark.parametrize("swap", [0, 1])
def test_fold_counts_a_single_product_beyond_the_range(swap):
    """EXACT.  One product of 2^17 in the middle of a tile (march_operand_cases.single_offender): clamped, and the counter, zero before
    the call, is exactly 1 after it - zero iff no product left the range, whichever lane holds it."""
    case = MC.VALUE_CASE
    fc0, rows = MC.single_offender(case, 11)
    want, nan, n_off = MC.expected_planes(MC.fold_u64(rows, case, fc0), case)
    assert n_off == 1 and not nan.any()
    got, n_sat = _fold_twice(case, rows, fc0, _sources(swap))
    _assert_planes(got, want)
    l, r, f = MC.LONE_OFFENDER
    assert got[MC.row_bases(case)[0][l] + r, f] == np.float16(65504).view(np.uint16)
    assert n_sat == 1


@pytest.mark.parametrize("swap", [0, 1])
def test_fold_realistic_rows_against_float64(swap):
    """BOUNDED.  Post-ReLU normal V, normal fc_0:  |head + rem - u64| <= 2^-22 |u64| + 2^-25 + C_l 2^-24 sum_k |v_k w_k|  (two fp16
    roundings, half the fp16 subnormal quantum, an fp32 chain of C_l terms)."""
    case = MC.VALUE_CASE
    fc0 = MC.realistic_fc0(3)
    rows = MC.realistic_rows(case, 4)
    u64, s64 = MC.fold_u64(rows, case, fc0), MC.fold_abs64(rows, case, fc0)
    got, n_sat = _fold_twice(case, rows, fc0, _sources(swap))
    bases, zero_row = MC.row_bases(case)
    frame = got.copy()
    worst = 0.0
    for l, u in enumerate(u64):
        k = u.shape[0]
        err = np.abs(MC.planes_value(got[bases[l]:bases[l] + k]) - u)
        bound = 2.0 ** -22 * np.abs(u) + 2.0 ** -25 + MC.LEVEL_C[l] * 2.0 ** -24 * s64[l]
        worst = max(worst, float((err / bound).max()))
        assert np.count_nonzero(got[bases[l]:bases[l] + k, 256:]) > k * 128, "remainders carry the low bits"
        frame[bases[l]:bases[l] + k] = MC.SENTINEL16
    print("realistic fold rows: largest error / bound = %.3f" % worst)
    assert worst <= 1.0
    want = np.full(got.shape, MC.SENTINEL16, np.uint16)
    want[zero_row] = 0
    _assert_planes(frame, want)
    assert n_sat == 0


# ------------------------------------------------------------------------------------ nb_mlp_pack_sections (fp32), nb_mlp_latent_bias
def _dev(p):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in p.items()}


def _pack(p, precisions, fill):
    """nb_mlp_pack_sections into a caller-owned blob filled with `fill`; the whole blob as float32 numpy."""
    from neuralbody_amd import ops

    S.check_pack_size(ops.mlp_pack_size())
    out = torch.full((ops.mlp_pack_size(),), fill, dtype=torch.float32, device=DEV)
    ops.mlp_pack(_dev(p), out=out, precisions=precisions)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _f32_section(p):
    return _pack(p, ["f32"], F32_SENTINEL)[:S.PACK_F32]


def _latent_bias(p, code):
    from neuralbody_amd import ops

    out = torch.full((384,), F32_SENTINEL, dtype=torch.float32, device=DEV)
    ops.mlp_latent_bias(_dev(p), torch.from_numpy(code).to(DEV), out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _only(name, value):
    p = MC.zero_params()
    p[name] = value
    return p


def _permutation(values, n):
    """values = a permutation of 1 .. n -> the natural index at each position."""
    idx = values.astype(np.int64) - 1
    assert np.array_equal(values, idx + 1.0) and sorted(idx.tolist()) == list(range(n)), "not a permutation of the probe"
    return idx


def _nonzero_range(sec):
    nz = np.nonzero(sec)[0]
    return int(nz[0]), int(nz[-1]) + 1, nz


@pytest.fixture(scope="module")
def bias_order():
    """pi256 / pi128: the natural index of the bias at each fragment position, as nb_mlp_latent_bias lays them out."""
    zero = np.zeros(128, np.float32)
    a = _latent_bias(_only("latent_b", np.arange(1, 257, dtype=np.float32)), zero)
    assert not a[256:].any()
    b = _latent_bias(_only("view_b", np.arange(1, 129, dtype=np.float32)), zero)
    assert not b[:256].any()
    return _permutation(a[:256], 256), _permutation(b[256:], 128)


def test_every_bias_is_laid_out_in_the_one_fragment_order(bias_order):
    """EXACT.  The packer's fc_0 / fc_1 / fc_2 / view_fc biases sit, contiguous, in the order nb_mlp_latent_bias gives the folded ones:
    the kernels add all of them by the same fragment index."""
    pi256, pi128 = bias_order
    assert not np.array_equal(pi256, np.arange(256)), "fragment order is not natural order: the probe can tell them apart"
    ranges = []
    for name, pi in (("fc0_b", pi256), ("fc1_b", pi256), ("fc2_b", pi256), ("view_b", pi128)):
        n = pi.size
        sec = _f32_section(_only(name, np.arange(1, n + 1, dtype=np.float32)))
        lo, hi, nz = _nonzero_range(sec)
        assert nz.size == n and hi - lo == n, "%s: %d non-zeros over [%d, %d)" % (name, nz.size, lo, hi)
        assert np.array_equal(_permutation(sec[lo:hi], n), pi), name
        ranges.append((lo, hi))
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


@pytest.fixture(scope="module")
def weight_sections():
    """name -> (lo, hi) of the fp32 section that holds the tensor, found with a probe of distinct integers in that tensor alone (the
    merged layer: feature_w behind latent_w[:, :256] = I); checked on the way: the non-zeros are exactly the probe's multiset."""
    found = {}
    for i, name in enumerate(("fc0_w", "fc1_w", "fc2_w", "alpha_w", "view_w", "rgb_w", "merged")):
        p = MC.zero_params()
        key = "feature_w" if name == "merged" else name
        p[key] = MC.distinct_integers(p[key].shape, 40 + i)
        if name == "merged":
            p["latent_w"][:, :256] = np.eye(256, dtype=np.float32)
        sec = _f32_section(p)
        lo, hi, nz = _nonzero_range(sec)
        assert np.array_equal(np.sort(sec[nz]), np.arange(1, p[key].size + 1, dtype=np.float32)), "%s: not every weight exactly once" % name
        sigma = None
        if name == "merged":
            assert hi - lo == 65536
            flat = np.argsort(p[key].reshape(-1))  # value v sits at natural flat index flat[v - 1]
            sigma = flat[sec[lo:hi].astype(np.int64) - 1]
        found[name] = (lo, hi, sigma)
    return found


def test_every_weight_has_one_place_in_its_own_section(weight_sections):
    """EXACT.  Each tensor's entries appear exactly once (asserted while probing), inside one range, and no two ranges overlap."""
    spans = sorted((lo, hi, name) for name, (lo, hi, _) in weight_sections.items())
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(spans, spans[1:]):
        assert hi0 <= lo1, "%s [%d, %d) overlaps %s [%d, %d)" % (n0, lo0, hi0, n1, lo1, hi1)
    sizes = {name: hi - lo for name, (lo, hi, _) in weight_sections.items()}
    assert sizes["fc0_w"] == 256 * 352 and sizes["fc1_w"] == sizes["fc2_w"] == sizes["merged"] == 65536
    assert sizes["alpha_w"] == 256 and sizes["rgb_w"] == 384 and 128 * 346 <= sizes["view_w"] <= 4 * 44 * 256
    assert spans[-1][1] <= S.PACK_F32


@pytest.mark.parametrize("kind", ["normal", "cancelling"])
def test_fp64_sums_through_the_discovered_layout(bias_order, weight_sections, kind):
    """BOUNDED.  The merged layer's bias, the view layer's folded bias and the merged weights against extended-precision numpy:
    |got - ref| <= 2^-24 |ref| + 2^-50 sum |terms|  (one fp32 rounding of an fp64 sum, the order of that sum; for the view bias the terms
    are those of the expanded double sum).  `cancelling`: latent_b cancels the rest of its sum to the last fp32 bit."""
    pi256, pi128 = bias_order
    lo, hi, sigma = weight_sections["merged"]
    code = np.random.RandomState(8).standard_normal(128).astype(np.float32)
    p = MC.normal_params(7) if kind == "normal" else MC.cancelling_params(7, code)
    out = _latent_bias(p, code).astype(np.float64)
    sec = _f32_section(p).astype(np.float64)
    checks = (("merged bias", out[:256], MC.latent_bias_ref(p, code), pi256),
              ("view bias", out[256:], MC.view_bias_ref(p, code), pi128),
              ("merged weights", sec[lo:hi], tuple(a.reshape(-1) for a in MC.merged_ref(p)), sigma))
    worst = {}
    for name, got, (ref, tot), perm in checks:
        ref, tot = ref[perm], tot[perm]
        err = np.abs(got.astype(np.longdouble) - ref)
        worst[name] = float((err / MC.fp64_sum_bound(ref, tot)).max())
        if kind == "cancelling" and name == "merged bias":
            assert np.all(np.abs(ref) <= 2.0 ** -24 * tot)
    print("%s weights: largest error / bound: %s" % (kind, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_pack_leaves_unrequested_sections_alone_and_repeats_itself():
    """EXACT.  With precisions = ['f32'] the stream section and the statistic keep what the caller put there; two packs are bit-equal."""
    p = MC.normal_params(7)
    a = _pack(p, ["f32"], F32_SENTINEL)
    assert np.all(a[S.PACK_F32:] == np.float32(F32_SENTINEL)) and a.size == S.PACK_SIZE
    assert np.all(a[:S.PACK_F32] != np.float32(F32_SENTINEL)), "every element of the fp32 section is written"
    b, c = _pack(p, None, 0.0), _pack(p, None, 0.0)
    assert np.array_equal(b.view(np.uint32), c.view(np.uint32))
    assert np.array_equal(a[:S.PACK_F32].view(np.uint32), b[:S.PACK_F32].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ the f16f6 stream
def _packed_stream(p):
    """(decoded phases, unattributed bytes, the statistic's six integers, the packed blob on the device)."""
    from neuralbody_amd import _lib, ops

    S.check_pack_size(ops.mlp_pack_size())
    out = torch.zeros(ops.mlp_pack_size(), dtype=torch.float32, device=DEV)
    ops.mlp_pack(_dev(p), out=out, precisions=["f16f6"])
    torch.cuda.synchronize()
    blob = out.cpu().numpy()
    off = int(_lib.lib().nb_mlp_six_bit_stats_offset())
    assert off == S.PACK_F32 + S.STREAM_FLOATS
    dec, free = S.decode(blob[S.PACK_F32:off].view(np.uint8))
    stats = blob[off:].view(np.int32)
    assert not stats[6:].any()
    return dec, free, stats[:6].tolist(), out


def _assert_stream(dec, exp, skip_codes=()):
    """Heads, both terms' codes and block exponents of every phase, bit for bit; each found exactly once; padding zero."""
    names = ("fc_1", "fc_2", "colour head over the hidden units", "colour head over the encodings")
    for ph, (d, e) in enumerate(zip(dec, exp)):
        ok = e["valid"]
        assert np.all(d["seen_h"][ok] == 1) and not d["seen_h"][~ok].any() and np.all(d["seen_c"][:, ok] == 1) and np.all(d["seen_e"] == 1)
        assert d["pad_nonzero"] == 0, "%s: non-zero padding elements" % names[ph]
        bad = np.argwhere(d["heads"] != e["heads"])
        assert bad.size == 0, "%s: %d heads differ, the first at %s" % (names[ph], len(bad), bad[0])
        for k, term in enumerate(("W_h", "W_l")):
            bad = np.argwhere(d["ex"][k] != e["ex"][k])
            assert bad.size == 0, "%s %s: %d block exponents differ, the first at (row, block, half) %s: got %d, want %d" % (
                names[ph], term, len(bad), bad[0], d["ex"][k][tuple(bad[0])], e["ex"][k][tuple(bad[0])])
            diff = d["code"][k] != e["code"][k]
            for p_, r, c in skip_codes:
                if p_ == ph:
                    diff[r, c] = False
            bad = np.argwhere(diff)
            assert bad.size == 0, "%s %s: %d codes differ, the first at %s: got %d, want %d" % (
                names[ph], term, len(bad), bad[0], d["code"][k][tuple(bad[0])], e["code"][k][tuple(bad[0])])


@pytest.fixture(scope="module")
def normal_stream():
    p = MC.normal_params(5)
    return p, _packed_stream(p)


@pytest.mark.parametrize("by_row", [False, True])
def test_stream_has_a_place_for_every_weight(by_row):
    """EXACT.  Weights that name their column (1 + c), then their row (1 + r): the decoded heads are the input, the padding elements of
    the encodings are zero, and every byte that is neither piece data, a scale byte nor the statistic is zero."""
    p = MC.place_params(by_row)
    dec, free, stats, _ = _packed_stream(p)
    assert not free.any(), "%d stray bytes between the pieces and scales" % np.count_nonzero(free)
    want = [p["fc1_w"], p["fc2_w"], p["feature_w"][:128], p["view_w"]]
    for ph in range(4):
        cols = slice(256, 346) if ph == 3 else slice(0, 256)
        assert np.all(dec[ph]["seen_h"][:, cols] == 1)
        got = dec[ph]["heads"].view(np.float16).astype(np.float32)
        assert np.array_equal(got[:, cols], want[ph][:, cols]), "phase %d" % ph
        assert dec[ph]["pad_nonzero"] == 0
        assert not dec[ph]["code"][1].any() and np.all(dec[ph]["ex"][1] == 0), "no remainder: W_l is zero under scale byte 127"
    _assert_stream(dec, S.expected(S.phase_weights(p)))


def test_stream_heads_remainders_and_scales(normal_stream):
    """EXACT.  Normal weights: head = fp16(w); W_l = e2m1((w - head) 2^-ex) with ex the smallest exponent that brings the block's largest
    |w - head| to 6 or below; W_h = e2m1(head 2^-ex_h) likewise; the scale bytes are 127 + ex.  The folded colour head is
    view_w[:, :256] . (latent_w[:, :256] . feature_w), each product an fp64 sum rounded to fp32."""
    p, (dec, free, stats, _) = normal_stream
    exp = S.expected(S.phase_weights(p))
    assert not free.any()
    _assert_stream(dec, exp)
    assert all(np.count_nonzero(e["code"][1]) > 0.5 * e["valid"].sum() for e in exp) and len({int(x) for x in exp[0]["ex"][1].reshape(-1)}) > 2


def test_stream_quantiser_edges(normal_stream):
    """EXACT.  Blocks of fc_1 made by hand (march_operand_cases.edge_params): heads and remainders on every e2m1 midpoint with both
    signs, a largest head of 6 2^e exactly and one fp16 ulp above, an all-zero block, a single element, and a block with 3.2e38 and inf
    (exponents 0, saturated codes).  Every other block of the stream is what the same weights give without them."""
    p0, (dec0, _, _, _) = normal_stream
    p = MC.edge_params(5)
    dec, free, _, _ = _packed_stream(p)
    exp = S.expected(S.phase_weights(p))
    pc = S.phase_cols(0)
    r, (b, kh) = MC.EDGE_BLOCKS["huge"]
    nan_at = (0, r, pc[b, kh][20])  # inf - inf: the remainder of the inf weight is a NaN, its code is not pinned
    _assert_stream(dec, exp, skip_codes=[nan_at])
    assert not free.any()
    # spelled out, beside the reference: midpoints go to the even code under block exponents 0 and -15, the zero block, the huge block
    r, (b, kh) = MC.EDGE_BLOCKS["head_midpoints"]
    assert dec[0]["ex"][0, r, b, kh] == 0 and np.array_equal(dec[0]["code"][0][r, pc[b, kh][:16]], MC.EDGE_CODES)
    r, (b, kh) = MC.EDGE_BLOCKS["rem_midpoints"]
    assert dec[0]["ex"][1, r, b, kh] == -15 and np.array_equal(dec[0]["code"][1][r, pc[b, kh][:16]], MC.EDGE_CODES)
    r, (b, kh) = MC.EDGE_BLOCKS["zero"]
    assert np.all(dec[0]["ex"][:, r, b, kh] == 0) and not dec[0]["code"][:, r, pc[b, kh]].any()
    r, (b, kh) = MC.EDGE_BLOCKS["huge"]
    c = pc[b, kh]
    assert np.all(dec[0]["ex"][:, r, b, kh] == 0) and dec[0]["code"][0][r, c[4]] == 7 and dec[0]["code"][0][r, c[20]] == 7
    assert dec[0]["code"][1][r, c[4]] == 15
    # the rest of the stream: finite, and untouched by the edge blocks
    touched = np.zeros((256, 256), bool)
    for rr, (bb, kk) in MC.EDGE_BLOCKS.values():
        touched[rr, pc[bb, kk]] = True
    assert np.all(np.isfinite(dec[0]["heads"].view(np.float16)[~touched]))
    for key in ("heads", "code"):
        assert np.array_equal(dec[0][key][..., ~touched], dec0[0][key][..., ~touched])
        for ph in (1, 2, 3):
            assert np.array_equal(dec[ph][key], dec0[ph][key])
    for ph in (1, 2, 3):
        assert np.array_equal(dec[ph]["ex"], dec0[ph]["ex"]) and np.all(np.isfinite(dec[ph]["heads"].view(np.float16)))


def test_statistic_counts_the_small_heads(normal_stream):
    """EXACT.  The six integers behind the stream: per layer (fc_1, fc_2, both colour-head phases together) the non-zero heads below 1/8
    of their block's largest head, and the non-zero heads; ops.six_bit_small_fraction is their ratio.  Once with normal weights, once
    with blocks [1, 1/16, 1/16, ...] whose fraction is 31/32 by construction."""
    from neuralbody_amd import ops

    p, (dec, free, stats, blob) = normal_stream
    want = S.expected_stats(S.expected(S.phase_weights(p)))
    assert stats == want
    frac = ops.six_bit_small_fraction(blob).cpu().numpy().astype(np.float64)
    ratio = np.array([want[2 * i] / want[2 * i + 1] for i in range(3)])
    assert np.all(np.abs(frac - ratio) <= 2.0 ** -23 * ratio), "one fp32 division"
    assert all(0 < want[2 * i] < want[2 * i + 1] for i in range(3))
    dec, free, stats, blob = _packed_stream(MC.fraction_params())
    assert stats == MC.FRACTION_COUNTS
    frac = ops.six_bit_small_fraction(blob).cpu().numpy().astype(np.float64)
    ratio = np.array([31 / 32, 31 / 32, 335 / 346])
    assert np.all(np.abs(frac - ratio) <= 2.0 ** -23 * ratio) and frac[0] == 31 / 32
