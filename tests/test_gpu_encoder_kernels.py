"""Every sparse-convolution kernel of the encoder, and the BatchNorm kernels at their launch boundaries, against float64 references
built from oracle/spconv_rulebook.py (tests/spconv_cases.py) — through the public ops entry points only.

The forward kernel nb_enc_conv16 runs depends on the row CAPACITY, and a workgroup past the live rows leaves at once, so a few hundred
live rows under a large n_out_max reach every variant.  LATTICE inputs make the float64 answer exactly representable at every step of
an fp32 accumulation in any order: those cases are compared bit for bit (rows, gradients and the fp64 BatchNorm sums).  REALISTIC
inputs are held to the worst-case bound of each arithmetic, |got - ref| <= c * sum |a| |w| per element (spconv_cases' docstring); each
such case prints the ratio it observed.  Every test loops over live row counts at the tile edges by rewriting the device scalar."""
import math

import numpy as np
import pytest
import torch

from tests import spconv_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_GEO = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _count(n):
    return torch.tensor([int(n)], dtype=torch.int32, device=DEV)


def _geo(which, stride):
    """the geometry's index tensors on the device; the strided output set is the device's own (enc_downsample_index), checked against
    the rulebook's"""
    from neuralbody_amd import ops

    key = (which, stride)
    if key not in _GEO:
        geo = sc.geometry(which, stride)
        d = {"in_grid": _dev(geo.in_grid()), "in_lin": _dev(geo.in_lin), "n_in": _count(geo.n_in)}
        if stride == 1:
            d["out_grid"] = d["in_grid"]
        else:
            out_grid, out_lin, n_out, n_out_max, out_dhw = ops.enc_downsample_index(d["in_lin"], d["n_in"], geo.n_in, geo.in_dhw)
            assert tuple(out_dhw) == geo.out_dhw and int(n_out) == geo.n_out <= n_out_max
            assert np.array_equal(out_lin[:geo.n_out].cpu().numpy(), geo.out_lin)
            assert np.array_equal(out_grid.cpu().numpy(), geo.out_grid())
            d["out_grid"] = out_grid
        _GEO[key] = (geo, d)
    return _GEO[key]


def _report(what, ratio, bound):
    print("REALISTIC %s: max |got - ref| / S = %.3e (2^%.1f), bound %.3e (2^%.1f)"
          % (what, ratio, math.log2(ratio) if ratio > 0 else -math.inf, bound, math.log2(bound)))


def _assert_rows_and_sums(got, stats, ref, what):
    """lattice: the rows and the fp64 sums over exactly those rows, bit for bit"""
    c = ref.shape[1]
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), "%s: rows differ at %d entries, first %s" % (
        what, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
    assert float((ref ** 2).sum(0).max(initial=0.0)) * 2.0 ** 24 < 2.0 ** 53, "the sums of squares are exact in fp64"
    assert np.array_equal(stats[:c], ref.sum(0)), "%s: sum over the live rows" % what
    assert np.array_equal(stats[c:], (ref ** 2).sum(0)), "%s: sum of squares over the live rows" % what


# ----------------------------------------------------------------------------------------------------------------- (a) enc_conv
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", sc.ALL_PAIRS)
def test_fp32_convolution(cin, cout, stride):
    from neuralbody_amd import ops

    geo, d = _geo("small", stride)
    out_lin = _dev(geo.out_lin)
    for mode in ("lattice", "realistic"):
        rs = np.random.RandomState(100 + cin + 2 * cout + stride)
        if mode == "lattice":
            a, w = sc.lattice32(rs, (geo.n_in, cin)), sc.lattice32(rs, (3, 3, 3, cin, cout))
        else:
            a, w = sc.realistic_rows(rs, (geo.n_in, cin)), sc.realistic_weight(rs, cin, cout)
        ref, S = sc.conv_ref(geo, a, w), sc.conv_ref(geo, np.abs(a), np.abs(w))
        if mode == "lattice":
            sc.assert_lattice(S, 1.0)
        a_d, w_d = _dev(a), _dev(w)
        worst = 0.0
        for n in sc.row_counts(geo.n_out):
            rows, stats = ops.enc_conv(a_d, d["in_grid"], geo.in_dhw, out_lin, _count(n), geo.n_out, geo.out_dhw, stride, w_d)
            got, st = rows[:n].cpu().numpy(), stats.cpu().numpy()
            if mode == "lattice":
                _assert_rows_and_sums(got, st, ref[:n], "enc_conv %d -> %d stride %d, n = %d" % (cin, cout, stride, n))
            else:
                worst = max(worst, sc.worst_ratio(got, ref[:n], S[:n]))
        if mode == "realistic":
            _report("enc_conv %d -> %d stride %d" % (cin, cout, stride), worst, sc.c_fp32(cin))
            assert worst <= sc.c_fp32(cin)


# ----------------------------------------------------------------------------------------------------------------- (b), (c) enc_conv16
def _conv16_case(kind, conv_cin, conv_cout, cls, geo_rows, ref_of, gen_a, gen_w, prepare, call, what):
    """One 16-bit convolution case under one capacity class: lattice (exact, rows and sums) and realistic (bound).
    ref_of(a, w) -> float64 rows of the product on all output rows of the kernel; prepare(w, cap) -> what call(prepared, planes, n,
    cap) -> (rows, stats) needs beside the planes (the packed weight, the padded rows)."""
    from neuralbody_amd import ops

    cap = sc.capacity(sc.CAPACITIES[cls], geo_rows)
    variant = sc.VARIANTS[(conv_cin, conv_cout)][cls]
    assert ops.enc_conv16_variant(conv_cin, conv_cout, cap) == variant, "the capacity no longer reaches %s" % variant
    what = "%s, capacity %d (%s)" % (what, cap, variant)
    for mode in ("lattice", "realistic"):
        rs = np.random.RandomState(200 + conv_cin + 2 * conv_cout + cls)
        a, w = gen_a(rs, mode), gen_w(rs, mode)
        S = ref_of(np.abs(a), np.abs(w))
        if mode == "lattice":
            ref = sc.three_products(ref_of, sc.split(a, kind), sc.split(w, kind))
            sc.assert_lattice(S, sc.REM)
        else:
            ref = ref_of(a, w)
        planes, prepared = sc.split_planes(a, kind).to(DEV), prepare(_dev(w), cap)
        worst = 0.0
        for n in sc.row_counts(geo_rows):
            rows, stats = call(prepared, planes, n, cap)
            assert tuple(rows.shape) == (cap, conv_cout)
            got, st = rows[:n].cpu().numpy(), stats.cpu().numpy()
            if mode == "lattice":
                _assert_rows_and_sums(got, st, ref[:n], "%s, n = %d" % (what, n))
            else:
                worst = max(worst, sc.worst_ratio(got, ref[:n], S[:n]))
        if mode == "realistic":
            bound = sc.c_pairs16(kind, conv_cin)
            _report(what, worst, bound)
            assert worst <= bound


@pytest.mark.parametrize("cls", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,stride", sc.FORWARD16)
def test_fp16_pair_forward_convolution_in_every_variant(cin, cout, stride, cls):
    from neuralbody_amd import ops

    geo, d = _geo("small", stride)

    def prepare(w_d, cap):
        packed = ops.enc_conv_pack16(w_d)
        assert torch.equal(packed, ops.enc_conv_pack16_batch([(w_d, False)])[0]), "the batch pack gives other bits"
        return packed, _dev(sc.pad_lin(geo.out_lin, cap))

    def call(prepared, planes, n, cap):
        packed, out_lin = prepared
        return ops.enc_conv16(planes, d["in_grid"], geo.in_dhw, out_lin, _count(n), cap, geo.out_dhw, stride, packed, cin, cout)

    _conv16_case("fp16", cin, cout, cls, geo.n_out, lambda a, w: sc.conv_ref(geo, a, w),
                 lambda rs, mode: (sc.lattice16 if mode == "lattice" else sc.realistic_rows)(rs, (geo.n_in, cin)),
                 lambda rs, mode: sc.lattice16(rs, (3, 3, 3, cin, cout)) if mode == "lattice" else sc.realistic_weight(rs, cin, cout),
                 prepare, call, "enc_conv16 fp16 %d -> %d stride %d" % (cin, cout, stride))


@pytest.mark.parametrize("cls", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,stride", sc.BWD_INPUT16)
def test_bf16_pair_backward_input_convolution_in_every_variant(cin, cout, stride, cls):
    """The call training.encoder_backward makes: the layer's dx planes through the forward kernels' bf16 instantiation with a mode-1
    pack, a strided layer as the transposed gather (stride = -2) — against the scatter of dx @ W[o]^T over the FORWARD pairs.
    (cin, cout) are the layer's: the packed convolution runs cout -> cin."""
    from neuralbody_amd import ops

    geo, d = _geo("small", stride)

    def prepare(w_d, cap):
        packed = ops.enc_conv_pack16(w_d, backward_input=True)
        assert torch.equal(packed, ops.enc_conv_pack16_batch([(w_d, True)])[0]), "the batch pack gives other bits"
        return packed, _dev(sc.pad_lin(geo.in_lin, cap))

    def call(prepared, planes, n, cap):
        packed, in_lin = prepared
        return ops.enc_conv16(planes, d["out_grid"], geo.out_dhw, in_lin, _count(n), cap, geo.in_dhw, 1 if stride == 1 else -stride,
                              packed, cout, cin, bf16=True)

    _conv16_case("bf16", cout, cin, cls, geo.n_in, lambda dx, w: sc.bwd_input_ref(geo, dx, w),
                 lambda rs, mode: (sc.lattice16 if mode == "lattice" else sc.wide_gradients)(rs, (geo.n_out, cout)),
                 lambda rs, mode: sc.lattice16(rs, (3, 3, 3, cin, cout)) if mode == "lattice" else sc.realistic_weight(rs, cin, cout),
                 prepare, call, "enc_conv16 bf16 backward-input of %d -> %d stride %d" % (cin, cout, stride))


# ----------------------------------------------------------------------------------------------------------------- (d) enc_conv_bwd_input
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", sc.ALL_PAIRS)
def test_fp32_backward_input(cin, cout, stride):
    from neuralbody_amd import ops

    geo, d = _geo("small", stride)
    for mode in ("lattice", "realistic"):
        rs = np.random.RandomState(300 + cin + 2 * cout + stride)
        if mode == "lattice":
            dx, w = sc.lattice32(rs, (geo.n_out, cout)), sc.lattice32(rs, (3, 3, 3, cin, cout))
        else:
            dx, w = sc.wide_gradients(rs, (geo.n_out, cout)), sc.realistic_weight(rs, cin, cout)
        ref, S = sc.bwd_input_ref(geo, dx, w), sc.bwd_input_ref(geo, np.abs(dx), np.abs(w))
        if mode == "lattice":
            sc.assert_lattice(S, 1.0)
        dx_d, w_d = _dev(dx), _dev(w)
        worst = 0.0
        for n in sc.row_counts(geo.n_in):
            din = ops.enc_conv_bwd_input(dx_d, d["out_grid"], geo.out_dhw, d["in_lin"], _count(n), geo.n_in, geo.in_dhw, stride, w_d)
            got = din.cpu().numpy()
            assert not got[n:].any(), "rows beyond the live count were written"
            if mode == "lattice":
                assert np.array_equal(got[:n].astype(np.float64), ref[:n]), "enc_conv_bwd_input %d -> %d stride %d, n = %d" % (cin, cout, stride, n)
            else:
                worst = max(worst, sc.worst_ratio(got[:n], ref[:n], S[:n]))
        if mode == "realistic":  # the product reduces over the 27 offsets x Cout channels of dx: the fp32 bound with that count
            _report("enc_conv_bwd_input %d -> %d stride %d" % (cin, cout, stride), worst, sc.c_fp32(cout))
            assert worst <= sc.c_fp32(cout)


# ----------------------------------------------------------------------------------------------------------------- (e) enc_conv_bwd_weight
WEIGHT_COUNTS = (0, 1, 2, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025)  # ... and all 2049 rows (row_counts appends them)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout,split", [(ci, co, False) for ci, co in sc.ALL_PAIRS] + [(ci, co, True) for ci, co in sc.PAIRS16])
def test_weight_gradient(cin, cout, split, stride):
    """Live row counts round the K = 2 chunk with a lone last row, the 32-row double-buffered chunks, 256 rows per wave and 1024 rows
    per workgroup (the strided layer of this set has 288 output rows: the counts below that, and all of them); the neighbour table
    first built by the call, then reused — the same bits on the lattice, where the atomics add exactly."""
    from neuralbody_amd import ops

    geo, d = _geo("big", stride)
    out_lin = _dev(geo.out_lin)
    name = "enc_conv_bwd_weight %s %d -> %d stride %d" % ("bf16 pairs" if split else "fp32", cin, cout, stride)
    for mode in ("lattice", "realistic"):
        rs = np.random.RandomState(400 + cin + 2 * cout + stride + 7 * split)
        lat = sc.lattice16 if split else sc.lattice32
        if mode == "lattice":
            a, dx = lat(rs, (geo.n_in, cin)), lat(rs, (geo.n_out, cout))
        else:
            a, dx = sc.realistic_rows(rs, (geo.n_in, cin)), sc.wide_gradients(rs, (geo.n_out, cout))
        a_d, dx_d = _dev(a), _dev(dx)
        planes = sc.split_planes(dx, "bf16").to(DEV) if split else None
        ref, S, n_before = np.zeros((3, 3, 3, cin, cout)), np.zeros((3, 3, 3, cin, cout)), 0
        worst = (0.0, 0, 0.0)
        for n in sc.row_counts(geo.n_out, WEIGHT_COUNTS):
            rows = (n_before, n)  # the references grow by the rows this count adds
            S += sc.bwd_weight_ref(geo, np.abs(a), np.abs(dx), rows=rows)
            if mode == "lattice" and split:
                ref += sc.three_products(lambda p, q: sc.bwd_weight_ref(geo, p, q, rows=rows), sc.split(a, "bf16"), sc.split(dx, "bf16"))
            else:
                ref += sc.bwd_weight_ref(geo, a, dx, rows=rows)
            n_before = n
            cache = []
            n_out = _count(n)
            got = ops.enc_conv_bwd_weight(a_d, d["in_grid"], geo.in_dhw, out_lin, n_out, geo.n_out, geo.out_dhw, stride, dx_d, cin, cout,
                                          dx_split=planes, rulebook=cache)
            assert len(cache) == 1
            again = ops.enc_conv_bwd_weight(a_d, d["in_grid"], geo.in_dhw, out_lin, n_out, geo.n_out, geo.out_dhw, stride, dx_d, cin, cout,
                                            dx_split=planes, rulebook=cache)
            if mode == "lattice":  # exact sums: the order of the fp32 atomics cannot show, so both calls give the reference's bits
                sc.assert_lattice(S, sc.REM if split else 1.0)
                assert torch.equal(got, again), "%s, n = %d: a reused neighbour table gives other bits" % (name, n)
                got = got.cpu().numpy()
                assert np.array_equal(got.astype(np.float64), ref), "%s, n = %d: %d entries differ" % (name, n, int((got != ref).sum()))
            else:  # (rounded sums: three and more atomics per entry arrive in any order, the two calls agree within the bound only)
                bound = sc.c_weight16(n) if split else sc.c_weight32(n)
                for dw in (got, again):
                    ratio = sc.worst_ratio(dw.cpu().numpy(), ref, S)
                    assert ratio <= bound, "%s, n = %d: %.3e > %.3e" % (name, n, ratio, bound)
                    worst = max(worst, (ratio, n, bound))
        if mode == "realistic":
            _report("%s (worst at n = %d)" % (name, worst[1]), worst[0], worst[2])


# ----------------------------------------------------------------------------------------------------------------- (f) BatchNorm + ReLU
EPS = float(np.float32(1e-3))
MOMENTUM = float(np.float32(0.01))
BN_SIZES = [(c, cap) for c in (16, 128) for cap in (1, 255, 300)] + [(128, 16400)]  # the last: past the 2048 blocks of the launch


def _bn_inputs(rs, cap, c):
    x = (rs.standard_normal((cap, c)) * rs.uniform(0.5, 1.5, c) + rs.uniform(0.5, 2.0, c)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, c).astype(np.float32), rs.uniform(-0.5, 0.5, c).astype(np.float32)
    rmean, rvar = rs.uniform(0.5, 2.0, c).astype(np.float32), rs.uniform(0.5, 1.5, c).astype(np.float32)
    return x, gamma, beta, rmean, rvar


def _close(got, ref, terms, what):
    """|got - ref| <= 2^-22 |ref| + 2^-40 sum |terms|: fp32 roundings of the result, and the fp64 cancellation of its terms"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    over = np.abs(got - ref) - (2.0 ** -22 * np.abs(ref) + 2.0 ** -40 * np.asarray(terms, np.float64))
    assert got.shape == ref.shape and np.all(over <= 0), "%s: off by %.3e beyond the bound" % (what, float(over.max()))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("c,cap", BN_SIZES)
def test_batchnorm_relu_forward_at_its_launch_boundaries(c, cap, training):
    """enc_bn_relu (in place, and with rows_out) and enc_bn_relu_split (with and without rows_out), with `dense`, with the momentum
    bookkeeping: y against float64 relu(a x + b) within 2^-22 (|a x| + |b|) (a and b rounded once each, one fma), the planes against
    the CPU split of the returned y bit for bit, batch_stats and the running statistics at 2^-22 relative (the variance also within
    2^-40 of the two terms whose difference it is).  n = 0 writes nothing."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(500 + c + cap)
    x, gamma, beta, rmean, rvar = _bn_inputs(rs, cap, c)
    dhw = (5, 41, 80) if cap > 300 else (4, 9, 10)
    assert cap <= int(np.prod(dhw))
    lin = np.sort(rs.choice(int(np.prod(dhw)), cap, replace=False)).astype(np.int32)
    x_d, lin_d = _dev(x), _dev(lin)
    g_d, b_d = _dev(gamma), _dev(beta)
    for n in sorted({0, max(cap - 1, 0), cap}):
        x64 = x[:n].astype(np.float64)
        stats = np.concatenate([x64.sum(0), (x64 ** 2).sum(0)])
        if training and n > 0:
            mean, sq = stats[:c] / n, stats[c:] / n
            var = np.maximum(sq - mean * mean, 0.0)
        else:
            mean, sq, var = rmean.astype(np.float64), None, rvar.astype(np.float64)
        invstd = 1.0 / np.sqrt(var + EPS)
        a, b = invstd * gamma, beta - mean * invstd * gamma
        ref = np.maximum(x64 * a + b, 0.0)
        bound = 2.0 ** -22 * (np.abs(x64 * a) + np.abs(b))
        what = "C = %d, capacity %d, n = %d, %s" % (c, cap, n, "train" if training else "eval")

        def run(entry, with_rows_out, with_dense, momentum):
            rows = x_d.clone()
            rm, rv = _dev(rmean), _dev(rvar)
            rows_out = torch.full_like(rows, -7.0) if with_rows_out else None
            dense = torch.zeros(tuple(dhw) + (c,), dtype=torch.float32, device=DEV) if with_dense else None
            out = entry(rows, _count(n), cap, _dev(stats), g_d, b_d, rm, rv, training, EPS, rows_lin=lin_d if with_dense else None,
                        dense=dense, momentum=momentum, rows_out=rows_out)
            return rows, rows_out, dense, rm, rv, out

        def check_y(y, name):
            y = y.cpu().numpy()
            assert np.all(np.abs(y[:n].astype(np.float64) - ref) <= bound), "%s, %s: y beyond 2^-22 (|a x| + |b|)" % (what, name)
            return y

        def check_stats(bs, rm, rv, momentum, name):
            bs = bs.cpu().numpy()
            assert bs[2 * c] == n
            if training and n > 0:
                _close(bs[:c], mean, 0.0, what + ", batch mean")
                _close(bs[c:2 * c], var, sq + mean * mean, what + ", batch variance")
            else:
                assert not bs[:2 * c].any(), "%s, %s: batch_stats of a pass without batch statistics" % (what, name)
            if training and n > 0 and momentum >= 0:
                unb = var * (n / max(n - 1, 1))
                _close(rm.cpu().numpy(), (1 - momentum) * rmean + momentum * mean, 0.0, what + ", running mean")
                _close(rv.cpu().numpy(), (1 - momentum) * rvar + momentum * unb, sq + mean * mean, what + ", running variance")
            else:
                assert np.array_equal(rm.cpu().numpy(), rmean) and np.array_equal(rv.cpu().numpy(), rvar), "%s, %s: running statistics moved" % (what, name)

        # in place, no bookkeeping
        rows, _, _, rm, rv, bs = run(ops.enc_bn_relu, False, False, -1.0)
        y = check_y(rows, "in place")
        assert np.array_equal(y[n:], x[n:]), "%s: rows beyond the live count were written" % what
        check_stats(bs, rm, rv, -1.0, "in place")
        # rows_out + dense + momentum: the raw rows stay
        rows, rows_out, dense, rm, rv, bs = run(ops.enc_bn_relu, True, True, MOMENTUM)
        assert torch.equal(rows, x_d), "%s: rows_out given, yet the raw rows changed" % what
        y2 = check_y(rows_out, "rows_out")
        assert np.array_equal(y2[:n], y[:n]) and np.all(y2[n:] == -7.0)
        want_dense = np.zeros((int(np.prod(dhw)), c), np.float32)
        want_dense[lin[:n]] = y[:n]
        assert np.array_equal(dense.cpu().numpy().reshape(-1, c), want_dense), "%s: dense" % what
        check_stats(bs, rm, rv, MOMENTUM, "rows_out")
        # the split entry point, without and with rows_out
        for with_rows_out in (False, True):
            rows, rows_out, dense, rm, rv, (planes, bs) = run(ops.enc_bn_relu_split, with_rows_out, with_rows_out, MOMENTUM if with_rows_out else -1.0)
            assert torch.equal(rows, x_d), "%s: the split entry point only reads the rows" % what
            assert tuple(planes.shape) == (2, cap, c)
            want = sc.split_planes(y[:n], "fp16")
            assert torch.equal(planes[:, :n].cpu(), want[:, :n]), "%s: planes are not the fp16 split of y" % what
            if with_rows_out:
                assert np.array_equal(rows_out.cpu().numpy()[:n], y[:n]) and np.array_equal(dense.cpu().numpy().reshape(-1, c), want_dense)
            check_stats(bs, rm, rv, MOMENTUM if with_rows_out else -1.0, "split")


@pytest.mark.parametrize("c", [16, 128])
@pytest.mark.parametrize("cap,counts", [(256, (1, 63, 64, 65)), (257, (1, 63, 64, 65)), (65537, (1, 63, 64, 65, 300))])
def test_batchnorm_relu_backward_at_its_slab_boundaries(cap, counts, c):
    """enc_bn_relu_bwd against the float64 formula of nb_encoder_bwd.hip's header comment, from the same fp32 batch_stats:
      g = dy [y > 0];  dbeta = sum g;  dgamma = sum g xhat;  dx = invstd gamma (g - dbeta / n - xhat dgamma / n)
    each within 2^-22 |ref| + 2^-40 sum |terms|; dx_split = the bf16 split of the returned dx, bit for bit.  Capacity 256: one slab of
    the reduction; 257: two; 65537: the 256-slab cap, 300 live rows at two rows a slab."""
    from neuralbody_amd import ops

    rs = np.random.RandomState(600 + c + cap)
    rows = max(counts)
    x = np.zeros((cap, c), np.float32)
    x[:rows], gamma, beta, _, _ = _bn_inputs(rs, rows, c)
    dy = np.zeros((cap, c), np.float32)
    dy[:rows] = sc.wide_gradients(rs, (rows, c))
    x_d, dy_d, g_d = _dev(x), _dev(dy), _dev(gamma)
    for n in counts:
        x64 = x[:n].astype(np.float64)
        bstats = np.concatenate([x64.mean(0), x64.var(0), [n]]).astype(np.float32)
        mean, invstd = bstats[:c].astype(np.float64), 1.0 / np.sqrt(bstats[c:2 * c].astype(np.float64) + EPS)
        xhat = (x64 - mean) * invstd
        y = np.zeros((cap, c), np.float32)
        y[:n] = np.maximum(xhat * gamma + beta, 0.0)
        g = np.where(y[:n] > 0, dy[:n].astype(np.float64), 0.0)
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
        scale = invstd * gamma
        dx = scale * (g - dbeta / n - xhat * dgamma / n)
        dx_terms = np.abs(scale) * (np.abs(g) + np.abs(dbeta / n) + np.abs(xhat * dgamma / n))
        what = "C = %d, capacity %d, n = %d" % (c, cap, n)
        for want_split in (True, False):
            out = ops.enc_bn_relu_bwd(dy_d, _dev(y), x_d, _count(n), cap, _dev(bstats), EPS, g_d, want_split=want_split)
            _close(out[2].cpu().numpy(), dbeta, np.abs(g).sum(0), what + ", dbeta")
            _close(out[1].cpu().numpy(), dgamma, np.abs(g * xhat).sum(0), what + ", dgamma")
            got_dx = out[0][:n].cpu().numpy()
            _close(got_dx, dx, dx_terms + np.abs(scale) * (np.abs(g).sum(0) + np.abs(xhat) * np.abs(g * xhat).sum(0)) / n, what + ", dx")
            if want_split:
                assert tuple(out[3].shape) == (2, cap, c)
                assert torch.equal(out[3][:, :n].cpu(), sc.split_planes(got_dx, "bf16")), what + ": dx_split is not the bf16 split of dx"
