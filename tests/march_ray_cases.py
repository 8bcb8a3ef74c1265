"""The ray loop of the two march kernels (nb_march_kernel, nb_march_fold_kernel<0, CULL>) restated on the CPU, and the inputs of
tests/test_march_rays_host.py and tests/test_gpu_march_rays.py.  CPU only; nothing here touches the library.

A. The integrator.  z_vals_f32 forms the sample depths operation for operation as z_lin / z_at do (single IEEE float32 operations:
bit-exact by construction); composite_f64 is raw2outputs in float64 on the decoder output the kernel itself composited, so that only
the ray loop's own roundings remain between the two; composite_f32_restated is the same recurrence in float32 in RayAccum::add's
order, used on the CPU alone to show that tol(S) leaves a float32 integrator a factor of two.

B. The sample positions.  sample_points_f32: p = fadd(o, fmul(d, z)) per axis and v = d / |d|, float32.

C. ray_case: the lattice scene of tests/f16f6_phase_cases.py marched by 64 rays whose samples are voxel centres or midpoints between
two voxels, every depth, position and trilinear weight exact, so that the operand-exact model of tests/f16f6_model.py gives the
decoder output of every (ray, step) bit for bit — through the pipelined preparation of the f16f6 kernel.
"""
import numpy as np

from tests import f16f6_phase_cases as C
from tests import march_operand_cases as K

F32 = np.float32
U24 = 2.0 ** -24
# |got - composite_f64| of weights, rgb and acc (depth: times the ray's largest z).  Whence: the float32 restatement below against
# composite_f64 on 4096 rays per case (normal logits of sigma 3, densities of sigma 20 and 1, jitter on) gave 2.5, 4.8, 6.3, 7.6,
# 11.9 and 16.5 units of 2^-24 at S = 2, 9, 16, 24, 64 and 128: about sqrt(S), and 8 + S / 2 is at least twice that at every S.
# tests/test_march_rays_host.py holds the restatement to HALF of it on the GPU test's own rays (largest: 0.31 of tol, rgb at S = 9).
# That restatement rounds expf correctly; with numpy's own float32 exp, which is allowed several ulp, it reaches 0.55 of tol (weights at
# S = 24) — the device's expf is a 1-ulp function, and the kernels stay well inside:
# MEASURED_RATIO: the largest |error| / tolerance of the unmutated kernels on the MI355X over the cases of A_CASES (the test prints
# them per case), fp32 / f16f6 (with and without the fix-up alike).  The bound was not touched.
MEASURED_RATIO = {"weights": (0.373, 0.390), "rgb": (0.204, 0.181), "acc": (0.253, 0.253), "depth": (0.251, 0.251),
                  "acc_sum": (0.068, 0.080), "disp": (0.344, 0.343)}
DISP_RTOL = 4.0 * U24  # two correctly rounded divisions, with margin


def tol(S):
    return (8.0 + S / 2.0) * U24


assert tol(64) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- A: depths
def z_lin_f32(near, far, t):
    """near (1 - t) + far t, uncontracted float32: [n, S] of near, far [n] and t [S]."""
    near, far, t = np.asarray(near, F32)[:, None], np.asarray(far, F32)[:, None], np.asarray(t, F32)[None, :]
    return near * (F32(1.0) - t) + far * t


def z_vals_f32(near, far, t_vals, t_rand=None):
    """The sample depths [n, S] as z_at forms them.  With jitter: lower = zc at s == 0, else 0.5 (zc + zc[s - 1]); upper = zc at
    s == S - 1, else 0.5 (zc[s + 1] + zc); z = lower + (upper - lower) t_rand."""
    zc = z_lin_f32(near, far, t_vals)
    assert zc.dtype == F32
    if t_rand is None:
        return zc
    t_rand = np.asarray(t_rand, F32)
    lower, upper = zc.copy(), zc.copy()
    lower[:, 1:] = F32(0.5) * (zc[:, 1:] + zc[:, :-1])
    upper[:, :-1] = F32(0.5) * (zc[:, 1:] + zc[:, :-1])
    z = lower + (upper - lower) * t_rand
    assert z.dtype == F32
    return z


def ray_norm_f32(ray_d):
    """|d| as the kernels form it: the float32 square root of the uncontracted float32 sum of squares."""
    d = np.asarray(ray_d, F32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def sample_points_f32(ray_o, ray_d, z):
    """p [n, S, 3] = fadd(o, fmul(d, z)) per axis and the view direction v [n, 3] = d / |d|, float32."""
    o, d = np.asarray(ray_o, F32), np.asarray(ray_d, F32)
    p = o[:, None, :] + d[:, None, :] * np.asarray(z, F32)[:, :, None]
    v = d / ray_norm_f32(d)[:, None]
    assert p.dtype == F32 and v.dtype == F32
    return p, v


# ------------------------------------------------------------------------------------------------------------ A: compositing
def composite_f64(raw, z, ray_d, white_bkgd=False):
    """raw2outputs in float64 of raw [n, S, 4] (float32 values), z [n, S] and ray_d [n, 3]: the last interval is 1e10, the factor
    1 - alpha + 1e-10, |d| the kernel's float32 one.  -> dict of weights [n, S], rgb [n, 3], acc [n], depth [n] (no disp: it is
    checked against the kernel's own depth and acc, disp_f64)."""
    raw, z = np.asarray(raw, np.float64), np.asarray(z, np.float64)
    n, S = z.shape
    dn = ray_norm_f32(ray_d).astype(np.float64)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10)], 1) * dn[:, None]
    alpha = -np.expm1(-np.maximum(raw[..., 3], 0.0) * dist)
    T = np.cumprod(np.concatenate([np.ones((n, 1)), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * T
    rgb = (w[..., None] / (1.0 + np.exp(-raw[..., :3]))).sum(1)
    acc = w.sum(1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc)[:, None]
    return dict(weights=w, rgb=rgb, acc=acc, depth=(w * z).sum(1))


def _fma32(a, b, c):
    """fmaf emulated through float64: the product of two float32 numbers is exact there."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _exp32(x):
    """expf as a correctly rounded float32 function of its float32 argument (numpy's own float32 exp is allowed several ulp)."""
    return np.exp(x.astype(np.float64)).astype(F32)


def composite_f32_restated(raw, z, ray_d, white_bkgd=False):
    """The same recurrence in numpy float32, in RayAccum::add's order (expf: correctly rounded)."""
    raw, z = np.asarray(raw, F32), np.asarray(z, F32)
    n, S = z.shape
    dn = ray_norm_f32(ray_d)
    one = F32(1.0)
    T, acc, depth = np.ones(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    c = [np.zeros(n, F32) for _ in range(3)]
    w_out = np.zeros((n, S), F32)
    for s in range(S):
        d = (z[:, s + 1] - z[:, s]) if s + 1 < S else np.full(n, 1e10, F32)
        dist = d * dn
        sig = np.maximum(raw[:, s, 3], F32(0.0))
        alpha = one - _exp32(-sig * dist)
        w = alpha * T
        T = T * ((one - alpha) + F32(1e-10))
        for ch in range(3):
            c[ch] = _fma32(w, one / (one + _exp32(-raw[:, s, ch])), c[ch])
        depth = _fma32(w, z[:, s], depth)
        acc = acc + w
        w_out[:, s] = w
    rgb = np.stack(c, 1)
    if white_bkgd:
        rgb = rgb + (one - acc)[:, None]
    assert rgb.dtype == F32 and acc.dtype == F32 and depth.dtype == F32
    return dict(weights=w_out, rgb=rgb, acc=acc, depth=depth)


def disp_f64(depth, acc):
    """1 / max(1e-10, depth / acc) in float64 of the kernel's own float32 depth and acc; acc == 0 gives NaN."""
    depth, acc = np.asarray(depth, F32).astype(np.float64), np.asarray(acc, F32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = depth / acc
        return 1.0 / np.where(np.isnan(q), q, np.maximum(float(F32(1e-10)), q))


def integrator_ratios(got, raw, z, ray_d, white_bkgd):
    """The largest |got - composite_f64| / tolerance per output of one march: got holds float32 weights, rgb_map, acc_map,
    depth_map and disp_map (numpy).  Also 'acc_sum' (acc against the float64 sum of the stored weights) and 'disp' (against disp_f64,
    relative, in units of DISP_RTOL; inf when the NaN patterns differ)."""
    S = z.shape[1]
    ref = composite_f64(raw, z, ray_d, white_bkgd)
    t = tol(S)
    g = dict((k, np.asarray(v, np.float64)) for k, v in got.items())
    zmax = np.abs(np.asarray(z, np.float64)).max(1)
    out = dict(weights=np.abs(g["weights"] - ref["weights"]).max() / t, rgb=np.abs(g["rgb_map"] - ref["rgb"]).max() / t,
               acc=np.abs(g["acc_map"] - ref["acc"]).max() / t, depth=(np.abs(g["depth_map"] - ref["depth"]) / zmax).max() / t,
               acc_sum=np.abs(g["acc_map"] - g["weights"].sum(1)).max() / t)
    want = disp_f64(got["depth_map"], got["acc_map"])
    nan_g, nan_w = np.isnan(g["disp_map"]), np.isnan(want)
    if not np.array_equal(nan_g, nan_w) or not np.array_equal(nan_w, g["acc_map"] == 0):
        out["disp"] = float("inf")
    else:
        ok = ~nan_w
        out["disp"] = float((np.abs(g["disp_map"][ok] - want[ok]) / np.abs(want[ok])).max(initial=0.0)) / DISP_RTOL
    return dict((k, float(v)) for k, v in out.items())


# ------------------------------------------------------------------------------------------------------------------- culling
def cull_project_f32(p, RT, Kc):
    """One view's projection of cull_inside (cull_project of nb_march_common.h) in float32, the FMA chains of
    tests/cull_cases.py::project: p [..., 3], RT [3, 4], Kc [3, 3] -> the pixel coordinates (x, y) before rounding."""
    from tests import cull_cases

    p = np.asarray(p, F32)
    x, y = cull_cases.project(dict(RT=RT, K=Kc), p.reshape(-1, 3), "chain")
    return x.reshape(p.shape[:-1]), y.reshape(p.shape[:-1])


def cull_inside_f32(p, RT, Kc, mask):
    """cull_inside for one view: rint (half to even), clamp to the mask [H, W], look up."""
    x, y = cull_project_f32(p, RT, Kc)
    assert x.dtype == F32
    H, W = mask.shape
    xi = np.clip(np.rint(x), 0, W - 1).astype(np.int64)
    yi = np.clip(np.rint(y), 0, H - 1).astype(np.int64)
    return mask[yi, xi] != 0


def cull_project_f64(p, RT, Kc):
    p = np.asarray(p, np.float64)
    t = p @ np.asarray(RT, np.float64)[:, :3].T + np.asarray(RT, np.float64)[:, 3]
    q = t @ np.asarray(Kc, np.float64).T
    return q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]


# --------------------------------------------------------------------------------------------------- A, B: the scene's rays
N_RAYS = 200   # the last wave, the last 64-ray group and the last 128-ray workgroup are ragged
RAY0 = 236     # rays RAY0 .. RAY0 + N_RAYS of the 'small_dense' scene: image rows through the body, where at every S below more
               # than a third of the rays end between 0.05 and 0.95 opacity and a fifth hit nothing at all (the oracle says)
SAMPLE_COUNTS = (2, 9, 16, 24, 64)
JITTER = (None, "rand", "zeros", "ones")
# stripes across the scene, one pixel (1 / 32 of a world unit along x + y + z) wide, every other one cut away: a ray crosses several
STRIPE_RT = np.array([[1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1]], F32)
STRIPE_K = np.array([[32, 0, 0], [0, 32, 0], [0, 0, 1]], F32)
STRIPE_W = 256

# (name, S, jitter, white_bkgd, ray_order, cull)
A_CASES = tuple(
    [("S%d%s" % (S, "-jit" if j else ""), S, j, bool((i + k) & 1), False, False)
     for i, S in enumerate(SAMPLE_COUNTS) for k, j in enumerate((None, "rand"))] +
    [("S16-t0", 16, "zeros", False, False, False), ("S16-t1", 16, "ones", True, False, False),
     ("S16-jit-order", 16, "rand", False, True, False), ("S24-order", 24, None, True, True, False), ("S9-jit-order", 9, "rand", True, True, False),
     ("S16-cull", 16, None, True, False, True), ("S16-jit-cull", 16, "rand", False, False, True), ("S9-cull", 9, None, False, False, True),
     ("S24-jit-cull", 24, "rand", True, False, True), ("S64-jit-cull-order", 64, "rand", True, True, True)])
B_CASES = tuple(c for c in A_CASES if c[0] in ("S16", "S16-jit", "S16-cull", "S16-jit-cull"))


def linear_t_vals(S):
    return (np.arange(S, dtype=np.float64) / (S - 1)).astype(F32)


def t_rand_of(kind, n, S, seed=77):
    if kind is None:
        return None
    if kind == "zeros":
        return np.zeros((n, S), F32)
    if kind == "ones":
        return np.full((n, S), 1.0 - 2.0 ** -24, F32)
    u = np.random.RandomState(seed + S).uniform(0, 1, (n, S)).astype(F32)
    return np.minimum(u, F32(1.0 - 2.0 ** -24))


_RAYS = {}


def scene_rays():
    """ray_o, ray_d [N_RAYS, 3], near, far [N_RAYS] of the 'small_dense' scene (float32, never written to)."""
    if "rays" not in _RAYS:
        from tests.golden import scenes

        batch = scenes.build("small_dense")[3]
        sel = slice(RAY0, RAY0 + N_RAYS)
        out = tuple(np.ascontiguousarray(batch[k][0, sel], F32) for k in ("ray_o", "ray_d", "near", "far"))
        for a in out:
            a.setflags(write=False)
        _RAYS["rays"] = out
    return _RAYS["rays"]


def slot_list(n):
    """The slot list of test_march_edge_cases (a dead group, the rays reversed, padding slots that march the last listed ray again)
    with the last seven rays left out: they have no slot and must read 0.  -> (int32 slots, bool [n]: the ray has a slot)."""
    listed = n - 7
    perm = np.arange(listed - 1, -1, -1, dtype=np.int32)
    pad = np.full((-listed) % 64, -(int(perm[-1]) + 1), np.int32)
    dead = np.full(64, -2 ** 31, np.int32)
    has = np.zeros(n, bool)
    has[:listed] = True
    return np.concatenate([dead, perm, pad]), has


def stripe_mask():
    m = np.zeros((1, STRIPE_W), np.uint8)
    m[0, ::2] = 1
    return m


def a_inputs(case):
    """The CPU side of one case of A_CASES: dict of ray_o, ray_d, near, far, t_vals, t_rand (or None), z [n, S], p [n, S, 3],
    v [n, 3], inside (bool [n, S] or None), slots / has_slot (or None)."""
    name, S, jit, white, order, cull = case
    ray_o, ray_d, near, far = scene_rays()
    t_vals = linear_t_vals(S)
    t_rand = t_rand_of(jit, N_RAYS, S)
    z = z_vals_f32(near, far, t_vals, t_rand)
    p, v = sample_points_f32(ray_o, ray_d, z)
    d = dict(name=name, S=S, white=white, ray_o=ray_o, ray_d=ray_d, near=near, far=far, t_vals=t_vals, t_rand=t_rand, z=z, p=p, v=v,
             inside=None, slots=None, has_slot=np.ones(N_RAYS, bool))
    if cull:
        # the stripes start at the scene's own lowest x + y + z: every sample lands on a pixel of the mask
        RT = STRIPE_RT.copy()
        RT[0, 3] = -np.floor(float((p.astype(np.float64).sum(-1)).min()) * 32.0) / 32.0 + 1.0
        d.update(cull_RT=RT, cull_K=STRIPE_K, cull_mask=stripe_mask())
        d["inside"] = cull_inside_f32(p, RT, STRIPE_K, d["cull_mask"][0][None, :])
    if order:
        d["slots"], d["has_slot"] = slot_list(N_RAYS)
    return d


def fixture_figures(weights, acc, has_slot):
    """What the fixture conditions of A are asserted on: the fraction of (listed) rays with 0.05 < acc < 0.95, the number with
    acc == 0, and — over the rays with acc > 0.05 — the fraction of neighbouring weights that differ, among all pairs and among the
    pairs in which either weight is not zero."""
    w, a = np.asarray(weights)[has_slot], np.asarray(acc)[has_slot]
    rows = a > 0.05
    pairs_differ = w[rows][:, 1:] != w[rows][:, :-1]
    live = (w[rows][:, 1:] != 0) | (w[rows][:, :-1] != 0)
    return dict(mid=float(((a > 0.05) & (a < 0.95)).mean()), zero=int((a == 0).sum()), distinct_all=float(pairs_differ.mean()),
                distinct_live=float(pairs_differ[live].mean()) if live.any() else 0.0)


# ------------------------------------------------------------------------------------------------------------ C: lattice rays
RAY_KINDS = ("whole", "half", "leave", "ybundle", "cull", "narrow")
CULL_RT = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 2.0 ** 10]], F32)  # a camera looking along +y from 2^10 away
CULL_K = np.array([[2.0 ** 15, 0, 0], [0, 2.0 ** 15, 0], [0, 0, 1]], F32)    # pixel = (x, z) 2^15 / (y + 2^10): column = step, row = z_r
CULL_DEAD_COLUMNS = (2, 3, 8)  # whole depth steps without a surviving sample: two in a row, and the last one


def _trilinear64(vol0, idx):
    """vol0 [D, H, W, C] sampled at voxel coordinates idx [..., 3] (x, y, z) in float64 with zero padding; also the eight weights."""
    f = np.floor(idx)
    t = idx - f
    i0 = f.astype(np.int64)
    out = np.zeros(idx.shape[:-1] + (vol0.shape[3],))
    ws = []
    D, H, W = vol0.shape[:3]
    for corner in range(8):
        dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
        w = (t[..., 0] if dx else 1 - t[..., 0]) * (t[..., 1] if dy else 1 - t[..., 1]) * (t[..., 2] if dz else 1 - t[..., 2])
        x, y, z = i0[..., 0] + dx, i0[..., 1] + dy, i0[..., 2] + dz
        inb = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (z >= 0) & (z < D)
        w = np.where(inb, w, 0.0)
        out += w[..., None] * vol0[np.clip(z, 0, D - 1), np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.float64)
        ws.append(w)
    return out, np.stack(ws, -1)


def ray_case(kind, colour=False, seed=0):
    """64 rays (one workgroup: 64 samples per depth step) through the lattice scene, direction 2^-5 along an axis, near = 0,
    far = 8, so that z[s] is exactly s (t_vals = s / 8, S = 9) or s / 2 (t_vals = s / 16, S = 16), every p exact, |d| = 2^-5 and the
    view direction a unit vector.  The whole 9^3 level-0 volume holds lattice values: the EXACT recipe (heads {4 .. 7} 2^e, a
    quarter halved, remainders {1, 2, 3} 2^(e - 13), e per voxel) where the samples are voxel centres, fold_case('u_rem')'s
    (heads {4 .. 7}, remainders {1, 2, 3} 2^-13) where a trilinear weight of 1/2 is used.
       whole    S = 9: ray r from voxel (0, r & 7, r >> 3) along +x; sample (r, s) reads voxel (z_r, y_r, s): the 64 samples of a step
                all differ and the boxes move every step
       half     S = 16, half-voxel steps: odd steps blend two voxels with weights 1/2; the 16-step weight store
       leave    half-voxel steps from x = 3: x = 8.5 reads V[8] / 2 (zero padding), x >= 9 nothing: there the bias path alone is
                left — half-block (1, 1) has no gain and an fc_0 bias on the lattice instead
       ybundle  half-voxel steps along +y from the x - z face: the (wave, level) boxes move along another axis
       cull     'whole' under the camera CULL_RT / CULL_K (pixel column = step, row = z_r) and a mask without the columns
                CULL_DEAD_COLUMNS and without eight single pixels
       narrow   'whole' from an 8 x 4 face (rays r and r + 32 share their voxels): the step's voxel list fits one pass, so the
                next step's table is looked up inside the running step
    colour: the colour head's weights of f16f6_phase_cases' ('core', 2) behind the identity layers, read through rgb_fc ('whole').
    -> f16f6_phase_cases.Case with pts / viewdir / h1 per (ray, step) in ray-major order, and ray_o, ray_d, near, far, t_vals, S,
    idx (voxel coordinates [64, S, 3]), tri_w (the eight trilinear weights), inside (bool [64, S]) and cull = (mask, RT, K) or None."""
    assert kind in RAY_KINDS and (not colour or kind == "whole")
    rs = np.random.RandomState(9000 + 31 * RAY_KINDS.index(kind) + seed)
    whole = kind in ("whole", "cull", "narrow")
    f = np.arange(256)
    hb = C.half_block_of(f)
    gexp = np.asarray(C.GAIN_HB)[hb]
    gain_on = np.ones(256, bool)
    shape = (C.N0, C.N0, C.N0, 32)
    mh = rs.choice([4.0, 5.0, 6.0, 7.0], size=shape)
    ml = rs.choice([1.0, 2.0, 3.0], size=shape)
    e = np.zeros(shape[:3] + (1,), np.int64)
    if whole:
        mh = np.where(rs.rand(*shape) < 0.25, mh / 2, mh)
        e = rs.randint(-1, 2, size=shape[:3] + (1,))
    v64 = (mh + ml * 2.0 ** -13) * np.ldexp(1.0, e)
    vol0 = v64.astype(F32)
    assert (vol0.astype(np.float64) == v64).all()
    # the rays
    r = np.arange(64)
    S = 9 if whole else 16
    o = np.zeros((64, 3))
    axis = 1 if kind == "ybundle" else 0
    if kind == "ybundle":
        o[:, 0], o[:, 2] = r & 7, r >> 3
    else:
        o[:, 1], o[:, 2] = r & 7, (r >> 3) & 3 if kind == "narrow" else r >> 3
        o[:, 0] = 3 if kind == "leave" else 0
    ray_o = (o * C.VS_HIDDEN).astype(F32)
    ray_d = np.zeros((64, 3), F32)
    ray_d[:, axis] = C.VS_HIDDEN
    near, far = np.zeros(64, F32), np.full(64, 8.0, F32)
    t_vals = (np.arange(S) / (8.0 if whole else 16.0)).astype(F32)
    z = z_vals_f32(near, far, t_vals)
    p, v = sample_points_f32(ray_o, ray_d, z)
    idx = p.astype(np.float64) / C.VS_HIDDEN  # voxel coordinates (x, y, z)
    chan, tri_w = _trilinear64(vol0, idx)     # [64, S, 32]
    # fc_0: the selection with power-of-two gains; 'leave': half-block (1, 1) carries a bias instead
    p_ = C.base_params()
    b0 = np.zeros(256)
    if kind == "leave":
        gain_on[hb == 3] = False
        b0[hb == 3] = ((rs.choice([4.0, 5.0, 6.0, 7.0], size=256) + rs.choice([1.0, 2.0, 3.0], size=256) * 2.0 ** -13) * np.ldexp(1.0, gexp))[hb == 3]
    fc0 = np.zeros((256, 352), F32)
    fc0[f, f % 32] = np.where(gain_on, np.ldexp(1.0, gexp), 0.0)
    p_["fc0_w"] = fc0
    p_["fc0_b"] = b0.astype(F32)
    assert (p_["fc0_b"].astype(np.float64) == b0).all()
    N = 64 * S
    h1 = b0[:, None] + fc0[f, f % 32].astype(np.float64)[:, None] * chan.reshape(N, 32)[:, f % 32].T
    h32 = h1.astype(F32)
    assert (h32.astype(np.float64) == h1).all()
    phase, rows = 1, list(C.VARIANT_ROWS[1])
    if colour:
        p_["feature_w"] = C.get(("core", 2)).params["feature_w"].copy()
        phase, rows = 2, list(C.VARIANT_ROWS[2])
    inside, cull = np.ones((64, S), bool), None
    if kind == "cull":
        mask = np.ones((1, 8, S), np.uint8)
        mask[0, :, list(CULL_DEAD_COLUMNS)] = 0
        free = [c for c in range(S) if c not in CULL_DEAD_COLUMNS]
        for k in range(8):  # single pixels: single samples of a step that is marched
            mask[0, rs.randint(0, 8), free[k % len(free)]] = 0
        cull = (mask, CULL_RT, CULL_K)
        inside = cull_inside_f32(p, CULL_RT, CULL_K, mask[0])
    vols = [vol0] + [np.zeros(s + (c,), F32) for s, c in zip(C.LEVEL_SHAPES[1:], K.LEVEL_C[1:])]
    return C.Case(name="rays-%s%s" % (kind, "-colour" if colour else ""), phase=phase, kind="exact", variant=kind, params=p_, volumes=vols,
                  voxel_size=C.VS_HIDDEN, pts=np.ascontiguousarray(p.reshape(N, 3)), viewdir=np.ascontiguousarray(np.repeat(v, S, 0)),
                  h1=h32, rows=rows, ray_o=ray_o, ray_d=ray_d, near=near, far=far, t_vals=t_vals, S=S, z=z, idx=idx, tri_w=tri_w,
                  inside=inside, cull=cull, colour=colour)


RAY_KEYS = tuple((k, False) for k in RAY_KINDS) + (("whole", True),)
_CACHE = {}


def get(key):
    """ray_case(kind, colour) by key, built once."""
    if key not in _CACHE:
        _CACHE[key] = ray_case(*key)
    return _CACHE[key]


def ray_expected(case):
    """What the read-outs of a ray case show, [rows, 64, S] float64 (the model's value of every (ray, step) behind its ReLU, 0 on a
    culled sample), and the model."""
    m = case.model(density_only=not case.colour)
    exp = case.expected(m)[case.rows].reshape(len(case.rows), 64, case.S)
    return np.where(case.inside[None], exp, 0.0), m
