"""float64 restatement of the vanilla-NeRF baseline's mesh pass for the tests of NerfMeshRenderer (numpy only, nothing of the
package): the trunk of lib/networks/nerf_mesh.py:45-54 (pts_linears[0..7] with the skip, alpha_linear) with every pre-activation,
its analytic gradient by the point under given relu masks, and the lattice, the iso rule and the recipe the fixture
tests/golden/nerf_mesh.npz and the tests share.  Builds on tests/nerf_ref.py (the embedding, the weight recipe)."""
import numpy as np

from tests import nerf_ref

AXES = (np.linspace(-0.6, 0.6, 16, dtype=np.float32), np.linspace(-0.5, 0.5, 14, dtype=np.float32),
        np.linspace(-0.4, 0.4, 12, dtype=np.float32))  # three distinct lengths: an axis swap shows
SEMI = (0.58, 0.47, 0.37)
PAD = 10
N_GRAD = 96  # the gradient reference covers the first 96 inside points
ISO_MARGIN = 1e-3  # 10 x the RAW_TOL of tests/golden/make_golden_nerf.py


def lattice():
    """-> (pts [16,14,12,3] float32, inside [16,14,12] bool): the meshgrid of AXES and the ellipsoid of semi-axes SEMI."""
    pts = np.stack(np.meshgrid(*AXES, indexing="ij"), -1).astype(np.float32)
    inside = ((pts.astype(np.float64) / np.array(SEMI)) ** 2).sum(-1) <= 1.0
    return pts, inside


def _params(sd, module):
    return {k[len(module) + 1:]: np.asarray(v, np.float64) for k, v in sd.items() if k.startswith(module + ".")}


def trunk(sd, module, pts):
    """pts [n,3] -> (alpha [n] float64, z: the eight pre-activations [n,256] of pts_linears[0..7]).  The model is evaluated AT the
    points given: fp32 arrays for what the fp32 programs see, float64 ones for finite differences."""
    p = _params(sd, module)
    e = nerf_ref.embed(np.asarray(pts, np.float64).reshape(-1, 3), nerf_ref.XYZ_RES)
    h, z = e, []
    for i in range(8):
        z.append(h @ p["pts_linears.%d.weight" % i].T + p["pts_linears.%d.bias" % i])
        h = np.maximum(z[-1], 0.0)
        if i == 4:
            h = np.concatenate([e, h], -1)  # nerf_mesh.py:52: the input first
    alpha = h @ p["alpha_linear.weight"].T + p["alpha_linear.bias"]
    return alpha[:, 0], z


def embed_gradient(emb, d_emb):
    """The gradient by the point from the gradient by the 63 embedding columns: [n,63] each -> [n,3] (float64)."""
    emb, d_emb = np.asarray(emb, np.float64), np.asarray(d_emb, np.float64)
    g = d_emb[:, 0:3].copy()
    for f in range(nerf_ref.XYZ_RES):
        s, c = slice(3 + 6 * f, 6 + 6 * f), slice(6 + 6 * f, 9 + 6 * f)
        g += 2.0 ** f * (d_emb[:, s] * emb[:, c] - d_emb[:, c] * emb[:, s])
    return g


def trunk_gradient(sd, module, pts, masks=None):
    """d alpha / d p [n,3] in float64: the analytic chain through the trunk with the relu masks `masks` (eight bool [n,256]: unit
    passes; None: the float64 model's own, z > 0)."""
    p = _params(sd, module)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    if masks is None:
        masks = [z > 0 for z in trunk(sd, module, pts)[1]]
    d_emb = np.zeros((pts.shape[0], 63))
    dz = p["alpha_linear.weight"] * masks[7]
    for i in range(7, 0, -1):
        w = p["pts_linears.%d.weight" % i]
        if i == 5:
            d_emb += dz @ w[:, :63]
            w = w[:, 63:]
        dz = (dz @ w) * masks[i - 1]
    d_emb += dz @ p["pts_linears.0.weight"]
    return embed_gradient(nerf_ref.embed(pts, nerf_ref.XYZ_RES), d_emb)


def centred_state_dict(pts_inside):
    """The fixture's recipe: make_state_dict with, per module, the alpha_shift that puts the median density of these points at 0.
    -> (state dict, alpha_shift [2] float32)"""
    base = nerf_ref.make_state_dict((0.0, 0.0))
    shift = [float(np.float32(-np.median(trunk(base, m, pts_inside)[0] / 20.0))) for m in nerf_ref.MODULES]
    return nerf_ref.make_state_dict(shift), np.array(shift, np.float32)


def pick_iso(values):
    """The multiple of 1/64 (zero excluded: the cube is 0 outside `inside`) that leaves 10-90 % of `values` above it and is farthest
    from every one of them.  -> (iso, that distance)"""
    values = np.asarray(values, np.float64)
    best = (None, -1.0)
    for k in range(int(np.floor(values.min() * 64)), int(np.ceil(values.max() * 64)) + 1):
        iso = k / 64.0
        if k == 0 or not 0.1 <= np.mean(values > iso) <= 0.9:
            continue
        dist = min(float(np.abs(values - iso).min()), abs(iso))  # (the 0 outside `inside` is a lattice value too)
        if dist > best[1]:
            best = (iso, dist)
    return best


def band_limited(sd, n_freq=3):
    """The same weights with the embedding's frequencies 2^n_freq and above switched off in pts_linears[0] and in the skip layer:
    a field the 16 x 14 x 12 lattice resolves (2^2 x 0.08 = 0.32 rad per step)."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for m in nerf_ref.MODULES:
        for name in ("pts_linears.0", "pts_linears.5"):
            out["%s.%s.weight" % (m, name)][:, 3 + 6 * n_freq:63] = 0.0
    return out


def lattice_agreement(sd, module):
    """The share of the lattice's interior inside points at which the analytic gradient sides with the lattice's own central
    differences of the density (float64): what a comparison of field normals with face normals can show at best."""
    pts, inside = lattice()
    alpha = trunk(sd, module, pts.reshape(-1, 3))[0].reshape(pts.shape[:3])
    diff = np.stack(np.gradient(alpha, *[float(a[1] - a[0]) for a in AXES]), -1)
    grad = trunk_gradient(sd, module, pts.reshape(-1, 3)).reshape(pts.shape)
    sel = inside.copy()
    sel[[0, -1]] = sel[:, [0, -1]] = sel[:, :, [0, -1]] = False
    return float(np.mean((diff[sel] * grad[sel]).sum(-1) > 0))


def crossing_emulation(sd, module, iso):
    """Marching cubes' vertices without marching cubes, in float64: every lattice edge of the padded cube (the density inside, 0
    elsewhere) whose ends lie on different sides of `iso` carries one vertex, linearly interpolated.  -> (inner [V] bool: both ends
    inside, so the vertex belongs to the field and not to the cut the carving makes; sides [V] bool: the analytic gradient at the
    vertex sides with the central differences of the cube there, the stand-in for a face normal)."""
    pts, inside = lattice()
    steps = [float(a[1] - a[0]) for a in AXES]
    alpha = trunk(sd, module, pts.reshape(-1, 3))[0].reshape(pts.shape[:3])
    cube, ins = np.pad(np.where(inside, alpha, 0.0), 2), np.pad(inside, 2)
    diff = np.stack(np.gradient(cube, *steps), -1)
    idx = np.stack(np.meshgrid(*[np.arange(-2, n + 2) for n in inside.shape], indexing="ij"), -1)
    pos = np.array([a[0] for a in AXES], np.float64) + idx * np.array(steps)
    where, normal, inner = [], [], []
    for ax in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = (cube[a] > iso) != (cube[b] > iso)
        t = ((iso - cube[a][cross]) / (cube[b][cross] - cube[a][cross]))[:, None]
        where.append(pos[a][cross] * (1 - t) + pos[b][cross] * t)
        normal.append(diff[a][cross] * (1 - t) + diff[b][cross] * t)
        inner.append(ins[a][cross] & ins[b][cross])
    where, normal, inner = np.concatenate(where), np.concatenate(normal), np.concatenate(inner)
    return inner, (trunk_gradient(sd, module, where) * normal).sum(-1) > 0
