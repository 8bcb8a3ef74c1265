"""A float64 model of the f16f6 layer phases of nb_march_fold_kernel (csrc/nb_march_fold.hip, csrc/nb_f6_ops.h), operand for operand.
CPU only; nothing here touches the library.

Per 64-column K block the kernel forms
    W . X  ~=  W_h . X_h (fp16 MFMA)  +  q4(W_h) . bf6(X_l)  +  q4(W_l) . bf6(X_h)   (scaled K = 64 MFMAs)
with fp32 accumulation.  The weight side (heads, four-bit codes, one block exponent per (row, half-block, term)) is what
tests/fold_stream_ref.expected() says the stream holds; this file adds the activation side — the fp16 head, the two bf6 (e3m2) forms
and the E8M0 block exponent t / t - 11 that make_operands6 and cvt_block6 form at run time per (sample, half-block of 32 columns) — and
chains the phases the way the kernel does: ReLU and a new split between the layers, alpha_fc and rgb_fc as plain sums.

Every product of the model is exact in float64 and so is every sum of the EXACT cases of tests/f16f6_phase_cases.py; for the others the
model's sum is the exactly rounded one and the kernel's fp32 accumulation is held to a multiple of 2^-24 sum |terms| (`abs`).
"""
import numpy as np

from tests import fold_stream_ref as S

# bf6 = fp6 e3m2: sign, three exponent bits of bias 3, two mantissa bits; subnormal step 2^-4, largest value 28, no inf / NaN
E3M2_GRID = tuple(m / 16.0 for m in range(4)) + tuple(2.0 ** (e - 3) * (1.0 + m / 4.0) for e in range(1, 8) for m in range(4))
E3M2_TOP = 28.0
REM_SHIFT = 11  # the remainder block's exponent is t - 11: |x - fp16(x)| <= 2^-11 |x|


def e3m2_code(x):
    """Code of the e3m2 number nearest to x, saturating at +-28, a tie to the even code (bit 5: the sign)."""
    return S._nearest_code(x, E3M2_GRID, E3M2_TOP)


def e3m2_value(code):
    code = np.asarray(code)
    return np.where(code & 32, -1.0, 1.0) * np.asarray(E3M2_GRID)[code & 31]


def bf6(x):
    """x rounded to e3m2, float64."""
    return e3m2_value(e3m2_code(x))


def is_e3m2_midpoint(x):
    """True where |x| lies exactly between two neighbouring e3m2 numbers (below the largest)."""
    a = np.abs(np.asarray(x, np.float64))
    g = np.asarray(E3M2_GRID)
    mid = 0.5 * (g[1:] + g[:-1])
    return (a[..., None] == mid).any(-1)


def block_exponent(amax):
    """nb_f6_ops.h block_exponent: max(biased fp32 exponent of max |v|, 15) - 3, as a BIASED E8M0 byte t; the head block is stored
    / 2^(t - 127) (its largest element lands in [8, 16) of e3m2's +-28), the remainder block / 2^(t - 11 - 127)."""
    bits = np.asarray(amax, np.float32).view(np.uint32).astype(np.int64)
    return np.maximum(bits >> 23, 15) - 3


def _phase_rows(x, ph):
    """x [PH_WIDTH, N] natural columns -> [NB, 2, 32, N]: the elements of every half-block in the order the kernel converts them
    (fold_stream_ref.phase_cols); padding elements are 0."""
    pc = S.phase_cols(ph)
    ok = pc >= 0
    out = np.zeros(pc.shape + (x.shape[1],), x.dtype)
    out[ok] = x[pc[ok]]
    return out, pc, ok


def split_activations(x, ph=0):
    """x: fp32 [PH_WIDTH[ph], N], the input of phase ph in natural column order (phase 3: view_fc's 346 columns, of which 256.. are the
    encodings).  Per (half-block, sample): t = block_exponent(max |x|); per element X_h = fp16(x) (round to nearest even),
    xx = bf6(X_h / 2^(t-127)) 2^(t-127), xl = bf6((x - X_h) / 2^(t-11-127)) 2^(t-11-127).  Returns a dict of float64 arrays in
    natural column order (columns the phase does not read: 0) — xh, xx, xl, the unrounded remainder rem — and t [NB, 2, N]."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[0] == S.PH_WIDTH[ph], (x.dtype, x.shape)
    assert float(np.abs(x).max(initial=0.0)) <= 65504.0, "beyond the fp16 range the kernel saturates: not modelled"
    v, pc, ok = _phase_rows(x, ph)
    t = block_exponent(np.abs(v).max(2))  # [NB, 2, N]
    sh = np.ldexp(1.0, (t - 127))[:, :, None, :]
    sl = np.ldexp(1.0, (t - REM_SHIFT - 127))[:, :, None, :]
    h = v.astype(np.float16).astype(np.float64)
    r = v.astype(np.float64) - h
    parts = dict(xh=h, rem=r, xx=bf6(h / sh) * sh, xl=bf6(r / sl) * sl, xx_scaled=h / sh, xl_scaled=r / sl)
    out = {}
    for k, a in parts.items():
        o = np.zeros(x.shape, np.float64)
        o[pc[ok]] = a[ok]
        out[k] = o
    out["t"] = t
    return out


_QCACHE = {}


def quantised_weights(weights):
    """Per phase (W_h, q4(W_h), q4(W_l)) as float64 [R, W] in natural order, from fold_stream_ref.expected: the fp16 heads, and the
    four-bit codes times 2^(block exponent of their (row, half-block, term)).  Kept per set of matrices (by content)."""
    key = tuple(hash(np.ascontiguousarray(w, np.float32).tobytes()) for w in weights)
    if key in _QCACHE:
        return _QCACHE[key]
    exp = S.expected(weights)
    out = []
    for ph in range(4):
        e, pc = exp[ph], S.phase_cols(ph)
        wh = np.where(e["valid"], np.ascontiguousarray(e["heads"]).view(np.float16).astype(np.float64), 0.0)
        q = [np.zeros(wh.shape), np.zeros(wh.shape)]
        for b in range(S.PH_NB[ph]):
            for kh in range(2):
                c = pc[b, kh]
                c = c[c >= 0]
                for k in range(2):
                    q[k][:, c] = S.e2m1_value(e["code"][k][:, c]) * np.ldexp(1.0, e["ex"][k, :, b, kh])[:, None]
        out.append((wh, q[0], q[1]))
    _QCACHE[key] = out
    return out


def layer(weights, ph, x, bias=None, drop=()):
    """One phase on the input x (fp32 [PH_WIDTH[ph], N]): the three products `main` = W_h . X_h, `whxl` = q4(W_h) . bf6(X_l),
    `wlxh` = q4(W_l) . bf6(X_h) ([R, N] float64; W_l . X_l is absent, as in the kernel), `abs` = |bias| + the sum of the magnitudes of
    every product, and `y` = bias + the three.  `drop` names terms left out of y (the sensitivity figures of the host tests)."""
    wh, q0, q1 = quantised_weights(weights)[ph]
    s = split_activations(x, ph)
    b = np.zeros(wh.shape[0]) if bias is None else np.asarray(bias, np.float64)
    out = dict(main=wh @ s["xh"], whxl=q0 @ s["xl"], wlxh=q1 @ s["xx"], split=s)
    out["abs"] = np.abs(b)[:, None] + np.abs(wh) @ np.abs(s["xh"]) + np.abs(q0) @ np.abs(s["xl"]) + np.abs(q1) @ np.abs(s["xx"])
    out["y"] = b[:, None] + sum(out[k] for k in ("main", "whxl", "wlxh") if k not in drop)
    return out


def positional_encoding(pts, viewdir):
    """view_fc's input columns 256..345 for points [N, 3] and view directions [N, 3] (fold_stream_ref.pe_slot_col): fp32 [346, N] with
    rows 0..255 zero.  The sines and cosines are float64 values rounded to fp32: the kernel's differ by ~2e-7, so a test may give them
    no weight and must keep them below the half-block's x and v (they only take part in the block maximum)."""
    pts, viewdir = np.asarray(pts, np.float32), np.asarray(viewdir, np.float32)
    out = np.zeros((S.PH_WIDTH[3], pts.shape[0]), np.float32)
    for a in range(3):
        for slot in range(30):
            c = S.pe_slot_col(a, slot)
            src = pts[:, a] if slot <= 20 else viewdir[:, a]
            k = -1 if slot in (0, 21) else ((slot - 1) >> 1 if slot <= 20 else (slot - 22) >> 1)
            is_cos = 0 if slot in (0, 21) else ((slot - 1) & 1 if slot <= 20 else (slot - 22) & 1)
            if k < 0:
                out[c] = src
            else:
                arg = src.astype(np.float64) * 2.0 ** k
                out[c] = (np.cos(arg) if is_cos else np.sin(arg)).astype(np.float32)
    return out


def relu32(y):
    """What the next phase reads: the fp32 accumulator, ReLU'd."""
    return np.maximum(np.asarray(y, np.float64).astype(np.float32), np.float32(0.0))


def decode(params, latent_bias, h1, pe=None, density_only=False, drop=None):
    """The decoder behind the folded first layer.  params: fc1_w .. rgb_b as numpy fp32 (tests/march_operand_cases.MLP_SHAPES),
    latent_bias: what nb_mlp_latent_bias returns (fp32 [384]: its second block [256:] is the colour head's bias), h1: fp32 [256, N],
    the first layer's output before its ReLU, pe: fp32 [346, N] from positional_encoding.  drop: {phase: (terms,)} left out.
    Returns sigma [N], rgb [3, N] (None with density_only), `phases`: the four layer() dicts, and `exact`: per phase whether y was an
    fp32 number (the EXACT cases assert it)."""
    drop = drop or {}
    w = S.phase_weights(params)
    h1 = np.asarray(h1)
    assert h1.dtype == np.float32
    phases, exact = [], []
    x = np.maximum(h1, np.float32(0.0))
    for ph, b in ((0, params["fc1_b"]), (1, params["fc2_b"])):
        L = layer(w, ph, x, b, drop.get(ph, ()))
        phases.append(L)
        exact.append(bool((L["y"].astype(np.float32).astype(np.float64) == L["y"]).all()))
        x = relu32(L["y"])
    sigma = np.asarray(params["alpha_w"], np.float64).reshape(-1) @ x.astype(np.float64) + float(np.asarray(params["alpha_b"]).reshape(-1)[0])
    if density_only:
        return dict(sigma=sigma, rgb=None, phases=phases, exact=exact, h3=x)
    xv = np.zeros((S.PH_WIDTH[3], x.shape[1]), np.float32) if pe is None else np.asarray(pe, np.float32)
    L2 = layer(w, 2, x, np.asarray(latent_bias, np.float32)[256:384], drop.get(2, ()))
    L3 = layer(w, 3, xv, None, drop.get(3, ()))
    y = L2["y"] + L3["y"]
    phases += [L2, L3]
    exact += [bool((y.astype(np.float32).astype(np.float64) == y).all())] * 2
    v = relu32(y)
    rgb = np.asarray(params["rgb_w"], np.float64) @ v.astype(np.float64) + np.asarray(params["rgb_b"], np.float64)[:, None]
    return dict(sigma=sigma, rgb=rgb, phases=phases, exact=exact, h3=x, view=v, y_colour=y, abs_colour=L2["abs"] + L3["abs"])
