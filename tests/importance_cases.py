"""Hierarchical sampling: the float64 model of the importance depths, the acceptance rule for a depth a kernel returns, fp32
restatements of the inversion in two arithmetics, and the input builders shared by tests/test_importance_host.py and
tests/test_gpu_importance.py.

The inversion, for a ray with S coarse depths z and weights w[0..S-1]: bins b_j = 0.5 (z_{j+1} + z_j), j = 0..K, K = S - 2;
v_i = fl32(w[i + 1] + 1e-5f); pdf_i = v_i / sum v; knots c_0 = 0, c_{i+1} = c_i + pdf_i; for u in [0, 1]: inds = #{j : c_j <= u},
below = max(inds - 1, 0), above = min(K, inds), denom = c_above - c_below (1 where < 1e-5), t = (u - c_below) / denom,
z = b_below + t (b_above - b_below).

Depths are ill-conditioned where a bin is nearly empty, so a returned depth is judged in the CDF domain (`accept`).  TAU = 2^-16:
the K - 1 additions of the sum, the K divisions and the K - 1 additions of the prefix are fp32 operations on values <= 1, each off
by at most 2^-24 and at most 64 of each kind deep in any order that a wave of 64 lanes sums in: three sources of at most
64 * 2^-24 = 2^-18, together under 2^-17, doubled."""
import numpy as np
import torch

TAU = 2.0 ** -16
FLOOR = 1e-5       # the reference's `denom < 1e-5 -> 1`
FLOOR_BAND = 2.0 ** -20


# ------------------------------------------------------------------------------------------------ float64 model
def bins_f32(z_coarse):
    """The S - 1 midpoints of fp32 coarse depths [n,S], formed in fp32 as the kernel and torch form them."""
    z = np.asarray(z_coarse, np.float32)
    return (np.float32(0.5) * (z[:, 1:] + z[:, :-1])).astype(np.float32)


def knots_f64(weights):
    """fp32 weights [n,S] -> (pdf [n,K], knots c [n,K+1]) in float64, from fl32(weights[:, 1:-1] + 1e-5f)."""
    v = (np.asarray(weights, np.float32)[:, 1:-1] + np.float32(1e-5)).astype(np.float32).astype(np.float64)
    pdf = v / v.sum(1, keepdims=True)
    c = np.concatenate([np.zeros((v.shape[0], 1)), np.cumsum(pdf, 1)], 1)
    return pdf, c


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _accept_bins(z, u, b, pdf, c, k):
    """The rule for candidate bins k (same shape as z, values in 0..K-1; b, pdf, c of the entry's ray already gathered per entry
    as [.., K+1], [.., K], [.., K+1])."""
    take = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]  # noqa: E731
    b0, b1, p, c0, c1 = take(b, k), take(b, k + 1), take(pdf, k), take(c, k), take(c, k + 1)
    width = b1 - b0
    ulp2 = 2.0 * np.maximum(_ulp(b0), _ulp(b1))
    in_u = (c0 - TAU <= u) & (u <= c1 + TAU)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(width > 0, (z - b0) / np.where(width > 0, width, 1.0), 0.0)
        slack = np.where(width > 0, p * 4.0 * 2.0 ** -24 * np.abs(b1) / np.where(width > 0, width, 1.0), np.inf)
    normal = (p >= FLOOR - FLOOR_BAND) & (z >= b0 - ulp2) & (z <= b1 + ulp2) & (np.abs(c0 + frac * p - u) <= 2 * TAU + slack)
    floor = (p <= FLOOR + FLOOR_BAND) & (np.abs(z - b0) <= (FLOOR + 2 * TAU) * width + ulp2)
    return in_u & (normal | floor)


def accept(z, u, bins, weights):
    """bool [n,N]: which returned depths z [n,N] (fp32) the rule admits for u [n,N] or [N], bins [n,K+1] (fp32) and the coarse
    weights [n,S] (fp32).  Candidate bins are the ones around the depth itself; an entry they do not admit is tried on every bin."""
    z = np.asarray(z, np.float32).astype(np.float64)
    n, N = z.shape
    u = np.broadcast_to(np.asarray(u, np.float32).astype(np.float64), (n, N))
    b = np.asarray(bins, np.float32).astype(np.float64)
    pdf, c = knots_f64(weights)
    K = pdf.shape[1]
    ok = np.zeros((n, N), bool)
    # the last-knot clause: u >= c_K - tau and z within 2 tau (b_K - b_{K-1}) + 2 ulp of b_K
    bK, bK1 = b[:, K:K + 1], b[:, K - 1:K]
    ok |= (u >= c[:, K:K + 1] - TAU) & (np.abs(z - bK) <= 2 * TAU * (bK - bK1) + 2.0 * _ulp(bK))
    kz = np.stack([np.searchsorted(b[r], z[r], side="right") - 1 for r in range(n)])
    be, pe, ce = (np.broadcast_to(a[:, None, :], (n, N, a.shape[1])) for a in (b, pdf, c))
    for d in (0, -1, 1, -2, 2):
        ok |= _accept_bins(z, u, be, pe, ce, np.clip(kz + d, 0, K - 1))
    for r, m in zip(*np.nonzero(~ok)):  # (few: bins of zero width, depths far from where they belong)
        k = np.arange(K)
        full = lambda a: np.broadcast_to(a[r], (K, a.shape[1]))  # noqa: E731
        ok[r, m] = bool(_accept_bins(np.full(K, z[r, m]), np.full(K, u[r, m]), full(b), full(pdf), full(c), k).any())
    return ok


def cdf_error(z, u, bins, weights):
    """|CDF(z) - u| in float64 [n,N], the CDF piecewise linear through (b_k, c_k): what the rule's 2 tau is compared with."""
    z = np.asarray(z, np.float32).astype(np.float64)
    n, N = z.shape
    u = np.broadcast_to(np.asarray(u, np.float32).astype(np.float64), (n, N))
    b = np.asarray(bins, np.float32).astype(np.float64)
    _, c = knots_f64(weights)
    return np.stack([np.abs(np.interp(z[r], b[r], c[r]) - u[r]) for r in range(n)])


# ------------------------------------------------------------------------------------------------ fp32 restatements
def sample_pdf_f32(bins, weights, u, arithmetic="sequential"):
    """The inversion in fp32 torch on the CPU, torch.searchsorted(right=True).  bins [n,K+1], weights [n,S] (the coarse pass's,
    cut to [1:-1] here), u [N] or [n,N] -> depths [n,N] fp32.  arithmetic: 'sequential' — sum and prefix by torch.sum / torch.cumsum in
    fp32; 'rounded_once' — sum and every prefix sum formed in float64 and rounded to fp32 once."""
    bins = torch.as_tensor(np.asarray(bins, np.float32))
    w = torch.as_tensor(np.asarray(weights, np.float32))[:, 1:-1] + torch.tensor(1e-5, dtype=torch.float32)
    n = w.shape[0]
    if arithmetic == "sequential":
        pdf = w / torch.sum(w, -1, keepdim=True)
        cdf = torch.cumsum(pdf, -1)
    elif arithmetic == "rounded_once":
        pdf = w / torch.sum(w.double(), -1, keepdim=True).float()
        cdf = torch.cumsum(pdf.double(), -1).float()
    else:
        raise ValueError(arithmetic)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    u = torch.as_tensor(np.asarray(u, np.float32))
    u = (u.expand(n, u.shape[-1]) if u.dim() == 1 else u).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = c1 - c0
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - c0) / denom
    return (b0 + t * (b1 - b0)).numpy()


# ------------------------------------------------------------------------------------------------ inputs
def t_vals(S):
    """torch.linspace(0, 1, S), the march's t_vals, as fp32 numpy."""
    return torch.linspace(0.0, 1.0, steps=int(S)).numpy()


def coarse_depths_f32(near, far, S):
    """near (1 - t) + far t in fp32, one rounding per operation (no jitter)."""
    t = t_vals(S)[None]
    near, far = np.asarray(near, np.float32)[:, None], np.asarray(far, np.float32)[:, None]
    return (near * (np.float32(1.0) - t) + far * t).astype(np.float32)


def make_rays(n, seed, flat_ray=None):
    """n rays: near in 3.5..4.5, far - near in 0.3..0.6, origins and directions of a camera a few metres away.  flat_ray: index of a
    ray with near == far == 4 (a power of two: near (1 - t) + near t is then exactly near in fp32, every depth of the ray with it)."""
    rs = np.random.RandomState(seed)
    near = rs.uniform(3.5, 4.5, n).astype(np.float32)
    far = (near + rs.uniform(0.3, 0.6, n).astype(np.float32)).astype(np.float32)
    ray_o = rs.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    ray_d = rs.standard_normal((n, 3)).astype(np.float32)
    ray_d[np.abs(ray_d).sum(1) < 0.1] = 1.0
    if flat_ray is not None and flat_ray < n:
        near[flat_ray] = far[flat_ray] = 4.0
    return ray_o, ray_d, near, far


KINDS = ("peaky", "zero", "first", "middle", "last", "lattice")


def make_weights(n, S, seed, first_kind=0):
    """Coarse weights [n,S] fp32, ray r of kind KINDS[(r + first_kind) % 6]: the composite of random peaky densities; all zero (a ray
    that misses: uniform depths); one non-zero interior bin at the first, a middle and the last position of weights[1:-1]; a dyadic
    lattice (multiples of 2^-8) with 70 % zeros."""
    rs = np.random.RandomState(seed)
    w = np.zeros((n, S), np.float64)
    s = np.arange(S)
    for r in range(n):
        kind = KINDS[(r + first_kind) % len(KINDS)]
        if kind == "peaky":
            sigma = np.zeros(S)
            for _ in range(rs.randint(1, 4)):
                sigma += rs.uniform(5.0, 200.0) * np.exp(-0.5 * ((s - rs.uniform(0, S - 1)) / rs.uniform(0.4, 3.0)) ** 2)
            alpha = 1.0 - np.exp(-sigma * (0.45 / S))
            w[r] = alpha * np.concatenate([[1.0], np.cumprod(1.0 - alpha + 1e-10)[:-1]])
        elif kind in ("first", "middle", "last"):
            w[r, {"first": 1, "middle": (S - 1) // 2 if S > 3 else 1, "last": S - 2}[kind]] = rs.uniform(0.2, 0.9)
        elif kind == "lattice":
            w[r] = rs.randint(1, 64, S) / 256.0 * (rs.uniform(0, 1, S) >= 0.7)
    return w.astype(np.float32)


def make_u(n, N, mode, seed):
    """'det': linspace(0, 1, N) shared by the rays (N = 1: [0]); 'rand': uniform [n,N] in [0, 1), unsorted."""
    if mode == "det":
        return torch.linspace(0.0, 1.0, steps=int(N)).numpy()
    return np.random.RandomState(seed).uniform(0.0, 1.0, (n, N)).astype(np.float32).clip(0.0, np.float32(1.0 - 2.0 ** -24))
