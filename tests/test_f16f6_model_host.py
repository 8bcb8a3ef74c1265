"""The float64 model of the f16f6 layer phases (tests/f16f6_model.py) and the preconditions of every case of
tests/f16f6_phase_cases.py, on the CPU: the quantisers against brute force, losslessness and the one-grid sums of the EXACT cases, no bf6
midpoints and the cross-term shift condition of the BOUNDED ones, and the model against the true float64 product."""
import math

import numpy as np
import pytest

from tests import f16f6_model as M
from tests import f16f6_phase_cases as C
from tests import fold_stream_ref as S
from tests import march_operand_cases as K


def _e3m2_decode(code):
    """An e3m2 code from its bit fields: sign | 3 exponent bits (bias 3) | 2 mantissa bits."""
    s, e, m = (code >> 5) & 1, (code >> 2) & 7, code & 3
    v = m / 4.0 * 2.0 ** -2 if e == 0 else (1.0 + m / 4.0) * 2.0 ** (e - 3)
    return -v if s else v


def test_e3m2_grid_and_quantiser_against_brute_force():
    vals = [_e3m2_decode(c) for c in range(32)]
    assert vals == list(M.E3M2_GRID) and vals[1] == 2.0 ** -4 and vals[31] == 28.0 and len(set(vals)) == 32
    assert (M.e3m2_value(np.arange(64)) == np.array([_e3m2_decode(c) for c in range(64)])).all()
    rs = np.random.RandomState(0)
    mids = [(a + b) / 2 for a, b in zip(vals[:-1], vals[1:])]
    x = np.concatenate([rs.uniform(-32, 32, 4000), rs.standard_normal(4000) * 0.2, vals, mids, [-v for v in mids], [28.0, 29.0, 1e9, -1e9, 0.0]])
    got = M.e3m2_code(x)
    for xi, ci in zip(x, got):
        a = min(abs(xi), 28.0)
        d = [abs(a - v) for v in vals]
        best = [c for c in range(32) if d[c] == min(d)]
        want = best[0] if len(best) == 1 else [c for c in best if c % 2 == 0][0]
        assert int(ci) == want + 32 * (xi < 0), (xi, ci, want)
    # ties to even: the midpoints 9, 11, 13, 15 of the heads' binade and 1.125, 1.375 of the remainders'
    assert list(M.bf6(np.array([9.0, 11.0, 13.0, 15.0, 1.125, 1.375, 2.25, 2.75]))) == [8.0, 12.0, 12.0, 16.0, 1.0, 1.5, 2.0, 3.0]
    assert M.is_e3m2_midpoint(np.array(mids)).all() and not M.is_e3m2_midpoint(np.array(vals)).any()


def test_block_exponent_is_the_kernels():
    for v in (0.0, 1e-30, 2.0 ** -112, 2.0 ** -111, 0.75, 1.0, 1.9999999, 2.0, 7.99, 8.0, 65504.0):
        t = int(M.block_exponent(np.float32(v)))
        e = (math.frexp(float(np.float32(v)))[1] - 1 + 127) if v > 0 else 0
        assert t == max(e, 15) - 3, (v, t)
        if v >= 2.0 ** -111:  # above the clamp: the largest element lands in [8, 16)
            assert 8.0 <= float(np.float32(v)) / 2.0 ** (t - 127) < 16.0


def test_split_activations_follows_the_half_blocks():
    rs = np.random.RandomState(1)
    x = (rs.standard_normal((256, 5)) * 3).astype(np.float32)
    s = M.split_activations(x, 0)
    pc = S.phase_cols(0)
    for b in range(4):
        for kh in range(2):
            for n in range(5):
                v = x[pc[b, kh], n]
                t = int(M.block_exponent(np.abs(v).max()))
                assert t == s["t"][b, kh, n]
                h = v.astype(np.float16).astype(np.float64)
                assert (s["xh"][pc[b, kh], n] == h).all()
                assert (s["xx"][pc[b, kh], n] == M.bf6(h / 2.0 ** (t - 127)) * 2.0 ** (t - 127)).all()
                assert (s["xl"][pc[b, kh], n] == M.bf6((v - h) / 2.0 ** (t - 138)) * 2.0 ** (t - 138)).all()


def _unit_exponent(p):
    """Exponent of the lowest set bit over the non-zero entries of p, along axis 1."""
    m, e = np.frexp(p)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi != 0, np.log2(np.maximum(low, 1)).astype(np.int64), 0)
    u = np.where(p != 0, e - 53 + tz, 10 ** 6)
    return u.min(1)


def _products(case, m):
    """The tested phase's products per (row, term and column, sample), non-zero columns only: [R, 3 x cols, N]."""
    ph = case.phase
    wh, q0, q1 = M.quantised_weights(S.phase_weights(case.params))[ph]
    s = m["phases"][ph]["split"]
    cols = np.nonzero((wh != 0).any(0))[0]
    return np.concatenate([wh[:, cols, None] * s["xh"][None, cols, :], q0[:, cols, None] * s["xl"][None, cols, :],
                           q1[:, cols, None] * s["xx"][None, cols, :]], 1)


@pytest.mark.parametrize("key", C.EXACT_KEYS + C.CORE_KEYS, ids=lambda k: "-".join(str(x) for x in k[1:]) + ("-core" if k[0] == "core" else ""))
def test_exact_case_preconditions(key):
    """Every quantisation of an EXACT case is lossless (the bf6 ties excepted: those round, to even), every layer's sum is an fp32
    number, and the tested phase's products lie on one grid per (row, sample) whose |.|-sum stays below 2^24 units."""
    case = C.get(key)
    m = case.model()
    assert all(m["exact"]), m["exact"]
    ph = case.phase
    w = S.phase_weights(case.params)[ph].astype(np.float64)
    wh, q0, q1 = M.quantised_weights(S.phase_weights(case.params))[ph]
    valid = S.expected(S.phase_weights(case.params))[ph]["valid"]
    assert (q0 == wh).all() and (q1[valid] == (w - wh)[valid]).all(), "a four-bit term of the weights is not lossless"
    assert (np.abs(w - wh)[wh != 0] < 2.0 ** -11 * np.abs(wh)[wh != 0]).all() and (np.sign(w - wh) * np.sign(wh) >= 0).all()
    s = m["phases"][ph]["split"]
    live = (wh != 0).any(0)  # every hidden column; of the encodings the x and v slots
    assert live[:256].all() or ph == 3
    s = dict((k, v[live] if k != "t" else v) for k, v in s.items())
    tie_h, tie_l = M.is_e3m2_midpoint(s["xx_scaled"]), M.is_e3m2_midpoint(s["xl_scaled"])
    assert (s["xx"] == s["xh"])[~tie_h].all() and (s["xl"] == s["rem"])[~tie_l].all(), "a bf6 form of the activations is not lossless"
    assert (s["rem"] >= 0).all()
    if case.variant == "ties":
        assert tie_h.mean() > 0.2 and (M.e3m2_code(s["xx_scaled"][tie_h]) % 2 == 0).all()
        if ph in (0, 3):
            assert tie_l.mean() > 0.2 and (M.e3m2_code(s["xl_scaled"][tie_l]) % 2 == 0).all()
        assert (s["xx"] != s["xh"])[tie_h].all() and (s["xl"] != s["rem"])[tie_l].all()  # a tie rounds: the model says where to
    else:
        assert not tie_h.any() and not tie_l.any()
    p = _products(case, m)
    y, ab = case.tested(m)
    most = 1.0
    for n in range(p.shape[2]):  # per sample: [R, terms]
        u = _unit_exponent(p[:, :, n])
        live = u < 10 ** 6
        most = max(most, float((np.abs(p[:, :, n]).sum(1)[live] / np.ldexp(1.0, u[live])).max(initial=0.0)))
    assert most < 2.0 ** 24, math.log2(most)
    ph_terms = m["phases"][ph]
    cross = np.abs(ph_terms["whxl"]) + np.abs(ph_terms["wlxh"])
    exp = case.expected(m)[case.rows]
    print("%s: %d x %d read-outs, %.0f%% non-zero, largest sum 2^%.1f units, cross terms %.1e of |y| (median)" % (
        case.name, exp.shape[0], exp.shape[1], 100.0 * (exp != 0).mean(), math.log2(most),
        float(np.median((cross / np.maximum(np.abs(y), 1e-300))[y != 0]))))
    assert (exp != 0).mean() > 0.3, "too few read-outs survive the ReLU"
    # what the variant is about
    if case.variant == "wl0":
        assert not ph_terms["wlxh"].any() and ph_terms["whxl"].any()
    if case.variant == "xl0":
        assert not ph_terms["whxl"].any() and ph_terms["wlxh"].any()
    if case.variant == "cancel":
        assert not ph_terms["main"].any() and ph_terms["whxl"].any() and ph_terms["wlxh"].any()
    if case.variant == "edge":
        t = s["t"]
        assert (t[1, 1] == 12).all() and not s["xh"][C.half_block_of(np.arange(256)) == 3].any()  # the all-zero half-block
        sub = s["xx_scaled"][(np.arange(256) // 64 == 2) & np.isin(np.arange(256) % 32, (2, 5))]
        assert (sub == 2.0 ** -4).all()  # bf6's subnormal step
        top = np.abs(s["xh"]).reshape(4, 64, -1).max(1)[:, 1::4]
        assert (np.frexp(top)[0] == 0.5).all()  # every fourth sample: a power of two on top of each block
    if case.variant == "full" and ph < 3:
        ex = S.expected(S.phase_weights(case.params))[ph]["ex"]
        assert all(len(set(ex[k, r].reshape(-1))) == 8 for k in range(2) for r in range(ex.shape[1])), "a row's scale bytes repeat"
        assert (ex[0] != ex[1]).all()
        t = m["phases"][ph]["split"]["t"].reshape(8, -1)
        assert all(len(set(t[:, n])) == 8 for n in range(t.shape[1])), "a sample's block exponents repeat"
        assert len(set(t[0])) >= 3, "the samples share one exponent"


@pytest.mark.parametrize("key", C.FOLD_KEYS, ids=lambda k: k[1])
def test_fold_case_preconditions(key):
    """The folded first layer's cases: H1 is an fp32 number (asserted where it is built), both heads' and remainders' planes are fp16
    numbers, and the layers behind it sum exactly."""
    case = C.get(key)
    m = case.model(density_only=True)
    assert all(m["exact"])
    u = case.volumes[0].reshape(-1, 32).astype(np.float64)[:, np.arange(256) % 32] * case.params["fc0_w"][np.arange(256), np.arange(256) % 32]
    planes, off = K.split_planes(u)
    assert not off.any() and (K.planes_value(planes) == u).all()
    rem = planes[:, 256:].view(np.float16)
    assert bool((rem != 0).any()) == (case.variant == "u_rem")
    th = np.float16(case.t).astype(np.float64)
    assert bool((th != case.t).any()) == (case.variant == "wt_rem") and (np.float16(case.t - th).astype(np.float64) == case.t - th).all()
    assert (case.expected(m)[case.rows] != 0).mean() > 0.9


def _shift_figures(case):
    m = case.model()
    y, ab = case.tested(m)
    rows = np.asarray(case.rows)
    out = {}
    for term in ("whxl", "wlxh"):
        y2, _ = case.tested(case.model(drop={case.phase: (term,)}))
        out[term] = np.abs(y2 - y)[rows]
    return y[rows], ab[rows], out


@pytest.mark.parametrize("key", C.BOUNDED_KEYS, ids=lambda k: "phase%d" % k[1])
def test_bounded_case_preconditions(key):
    """No input of the tested phase on a bf6 midpoint, a one-signed remainder, layers ahead exact; and the tolerance stays below
    2^-16 sum |terms| and below one eighth of the shift either cross term makes (median over the read-outs; the largest is printed)."""
    case = C.get(key)
    m = case.model()
    ph = case.phase
    assert all(m["exact"][:ph if ph < 3 else 2])
    s = m["phases"][ph]["split"]
    if ph == 3:  # of the encodings only the x and v slots carry weights
        s = dict((k, v[list(C.PE_X_COL + C.PE_V_COL)]) for k, v in s.items() if k != "t")
    assert not M.is_e3m2_midpoint(s["xx_scaled"]).any() and not M.is_e3m2_midpoint(s["xl_scaled"]).any()
    assert (s["rem"] >= 0).all() and (s["rem"] > 0).mean() > 0.9
    y, ab, shift = _shift_figures(case)
    unit = 2.0 ** -24 * ab
    for term, d in shift.items():
        r = d / unit
        print("%s: removing %s shifts the read-outs by %.1f (median) / %.1f (largest) x 2^-24 sum |terms|" % (
            case.name, term, float(np.median(r)), float(r.max())))
    assert C.BOUNDED_FACTOR == 4.0 * C.BOUNDED_MEASURED and C.BOUNDED_FACTOR < 2.0 ** 8
    for term, d in shift.items():
        assert C.BOUNDED_FACTOR < float(np.median(d / unit)) / 8.0, term


def test_model_against_the_true_product_on_normal_params():
    """On normal_params the model's layer differs from the float64 product W . x by what the four-bit cross terms lose: within
    2^-13 of the products' magnitudes per cross term."""
    p = K.normal_params(3)
    w = S.phase_weights(p)
    rs = np.random.RandomState(4)
    worst = 0.0
    for ph in range(3):
        x = np.maximum(rs.standard_normal((256, 64)), 0).astype(np.float32)
        L = M.layer(w, ph, x)
        true = w[ph].astype(np.float64) @ x.astype(np.float64)
        mag = np.abs(w[ph].astype(np.float64)) @ np.abs(x.astype(np.float64))
        rel = float((np.abs(L["y"] - true) / mag).max())
        rms = float(np.sqrt(((L["y"] - true) ** 2).mean() / (true ** 2).mean()))
        print("phase %d: model vs float64 product: %.2e of sum |w x| at worst (2^%.1f), %.2e rms of the output" % (ph, rel, math.log2(rel), rms))
        worst = max(worst, rel)
        assert rel <= 2 * 2.0 ** -13
        # and each cross term alone is worth about that: dropping one moves the output by more than the model's whole error
        for term in ("whxl", "wlxh"):
            assert float((np.abs(L[term]) / mag).max()) > rel
    print("worst: 2^%.1f" % math.log2(worst))
