"""Edge cases of the ray / box stage (csrc/nb_ray.h) and its float32 restatement, numpy only.

image_rays32 restates nb_raygen's per-pixel work operation for operation: pixel_ray_f64 in float64 (train_rays_ref.pixel_rays),
one cast, then get_near_far (if_nerf_data_utils.py:54-69) with every intermediate a float32.  Like the reference it keeps a pixel
whenever tn < tf, whatever the signs: a box BEHIND the camera gives near < far < 0 and is kept (that is the reference's
behaviour, not a choice made here), a camera inside the box gives near < 0 < far.

CASES are (name, H, W, K, R, T, bounds).  None of them is decided by rounding: tests/test_ray_cases_host.py holds every pixel
to tn == tf from bit-identical operands (TIES) or |tn - tf| >= 16 ulps (decision_margin)."""
import math

import numpy as np

from tests import synthetic as syn
from tests import train_rays_ref as trr

F32 = np.float32
TILE = 1024  # nbscan::TILE, as in tests/test_gpu_compact.py
EPS_POS, EPS_NEG = 1e-10, 1e-5  # a direction component in (-EPS_POS, EPS_NEG) becomes +EPS_NEG, then one in (-EPS_NEG, EPS_POS) -EPS_NEG


def _f32(*arrays):
    for a in arrays:
        assert isinstance(a, (np.ndarray, np.floating)) and a.dtype == F32, getattr(a, "dtype", type(a))
    return arrays[0] if len(arrays) == 1 else arrays


def slab32(bounds, o, d, swap=False, le=False, symmetric=False):
    """float32 get_near_far on cast rays o [3], d [n,3] -> (tn, tf, n, hit), all pixels kept.  The three switches are the mutations
    of tests/test_ray_cases_host.py (lines :58 and :59 swapped; <= for <; both thresholds 1e-10): never set by a caller that
    wants the kernel's result."""
    b = np.ascontiguousarray(bounds, F32).reshape(2, 3)
    _f32(o, d)
    n = _f32(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    v = _f32(d / n[:, None])
    big = F32(EPS_POS if symmetric else EPS_NEG)
    first = lambda v: (v < big) & (v > -F32(EPS_POS))  # noqa: E731  if_nerf_data_utils.py:58
    second = lambda v: (v > -big) & (v < F32(EPS_POS))  # noqa: E731  :59
    for cond, value in ((second, -F32(EPS_NEG)), (first, F32(EPS_NEG))) if swap else ((first, F32(EPS_NEG)), (second, -F32(EPS_NEG))):
        v[cond(v)] = value
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = _f32((b[:1] - o[None]) / v, (b[1:2] - o[None]) / v)
    tn, tf = _f32(np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1))
    return tn, tf, n, (tn <= tf if le else tn < tf)


def cast_rays(H, W, K, R, T):
    """(o [3], d [H*W,3]) float32, row-major pixels: pixel_ray_f64 and the one cast."""
    p = np.arange(H * W)
    o, d = trr.pixel_rays(K, R, T, p // W, p % W)
    return _f32(o.astype(F32), d.astype(F32))


def image_rays32(H, W, K, R, T, bounds, **mutation):
    """-> (o [3], d [H*W,3], near, far [H*W], hit [H*W] bool) for ALL pixels in row-major order, float32 in the kernel's
    operation order; near and far of a missed pixel are what the kernel computes and does not store."""
    o, d = cast_rays(H, W, K, R, T)
    tn, tf, n, hit = slab32(bounds, o, d, **mutation)
    with np.errstate(invalid="ignore"):
        near, far = _f32(tn / n, tf / n)
    return o, d, near, far, hit


def decision_margin(case):
    """|tn - tf| of every pixel in ulps of the larger magnitude (float32)."""
    _, H, W, K, R, T, bounds = case
    o, d = cast_rays(H, W, K, R, T)
    tn, tf, _, _ = slab32(bounds, o, d)
    big = np.maximum(np.abs(tn), np.abs(tf))
    return np.abs(tn.astype(np.float64) - tf.astype(np.float64)) / np.spacing(big).astype(np.float64)


def class_of(v):
    """Which substitution a direction component meets: 'plus' (-> +1e-5), 'minus' (-> -1e-5) or 'none'."""
    if -EPS_POS < v < EPS_NEG:
        return "plus"
    if -EPS_NEG < v < EPS_POS:
        return "minus"
    return "none"


# ------------------------------------------------------------------------------------------- the slab cameras
SLAB_H, SLAB_W, SLAB_CENTRE = 9, 17, 4 * 17 + 8  # pixel (x, y) = (8, 4)
SLAB_BOX = np.array([[-1.5e-5, -0.25, 1.0], [1.2e-5, 0.25, 2.0]], F32)
# name -> (cx - 8, class of the centre pixel's v_x = -(cx - 8) / 64, does it hit, its far)
SLAB = {
    "slab_zero": (0.0, "plus", True, 1.2),
    "slab_p30": (2.0 ** -30, "plus", True, 1.2),  # a tiny negative becomes +1e-5
    "slab_m30": (-2.0 ** -30, "plus", True, 1.2),
    "slab_p14": (2.0 ** -14, "minus", True, 1.5),
    "slab_m14": (-2.0 ** -14, "plus", True, 1.2),
    "slab_p655": (0.655 * 2.0 ** -10, "minus", True, 1.5),  # 9.99e-6: just inside the threshold
    "slab_m655": (-0.655 * 2.0 ** -10, "plus", True, 1.2),
    "slab_p8": (2.0 ** -8, "none", False, None),  # the whole image misses
    "slab_m8": (-2.0 ** -8, "none", False, None),
}


def slab_camera(dcx):
    """R = I, T = 0 and power-of-two focal lengths: every float64 product of pixel_ray_f64 is exact."""
    return np.array([[64.0, 0, 8.0 + dcx], [0, 64.0, 4.0], [0, 0, 1.0]]), np.eye(3), np.zeros((3, 1))


def _slab_cases():
    return [(name, SLAB_H, SLAB_W) + slab_camera(dcx) + (SLAB_BOX,) for name, (dcx, _, _, _) in SLAB.items()]


# ------------------------------------------------------------------------------------------- tie, inside, behind
TIE_NAMED = ((1, 1), (2, 2))  # (x, y): next to hits on both sides
# case -> pixels with tn == tf, bit for bit, in row-major order: the diagonal, and (1, 4), where v_y is 4 v_x exactly (a power of two
# scales a float32 quotient exactly) and the y-slab's exit 4 / v_y is the x-slab's entry 1 / v_x
TIES = {"tie": tuple(y * 6 + x for x, y in ((1, 1), (2, 2), (3, 3), (1, 4), (4, 4), (5, 5)))}


def _fixed_cases():
    """tie: d = (x, y, 1), so on the diagonal v_x and v_y are the same bits and the x-slab's exit 2 / v_x is the y-slab's entry
    2 / v_y: tn == tf, a miss under the strict comparison (TIES has one more such pixel).  Hits are the pixels with x < y < 4 x, eight of them."""
    eye, zero = np.eye(3), np.zeros((3, 1))
    K16 = np.array([[32.0, 0, 8.0], [0, 32.0, 8.0], [0, 0, 1.0]])
    return [("tie", 6, 6, np.eye(3), eye, zero, np.array([[1, 2, -8], [2, 4, 8]], F32)),
            ("inside", 16, 16, K16, eye, zero, np.array([[-1, -1, -1], [1, 1, 1]], F32)),
            ("behind", 16, 16, K16, eye, zero, np.array([[-4, -4, -2], [4, 4, -1]], F32))]


# ------------------------------------------------------------------------------------------- oblique cameras
OBLIQUE_BOX = np.array([[-0.12, -0.35, -0.1], [0.16, 0.3, 0.12]], F32)


def oblique_camera(H, W, size=None, **kw):
    """synthetic.make_camera at OBLIQUE_BOX for a size x size image, the principal point moved to the middle of H x W."""
    size = size or max(H, W)
    K, R, T = syn.make_camera({"can_bounds": OBLIQUE_BOX}, size, size, **dict(dict(focal_factor=1.5, distance=1.6, yaw=0.5, pitch=0.2), **kw))
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return K, R, T


SIZES = ((15, 17), (16, 16), (1, 257), (31, 33), (32, 32), (25, 41), (3, 683))  # 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 TILE + 1
assert [h * w for h, w in SIZES] == [255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def _oblique_cases():
    """W1 and H1: a single column and a single row of a 300 x 300 view.  sizes_*: the block (256) and scan tile (1024) edges; the
    box's silhouette covers the middle of every row it meets, so hits and misses alternate in row-major order."""
    out = [("W1", 300, 1) + oblique_camera(300, 1) + (OBLIQUE_BOX,), ("H1", 1, 300) + oblique_camera(1, 300) + (OBLIQUE_BOX,)]
    for H, W in SIZES:
        out.append(("sizes_%d" % (H * W), H, W) + oblique_camera(H, W) + (OBLIQUE_BOX,))
    return out


# ------------------------------------------------------------------------------------------- rotated cameras
ROT_ANGLES = (("3e-11", 3e-11), ("5e-7", 5e-7), ("2e-5", 2e-5))
# the two axis-aligned poses (world -> camera), their translations and the sense of the rotation about y
ROT_POSES = {"rotA": (np.eye(3), np.array([0.3, -0.2, 0.7]), 1.0), "rotB": (np.diag([-1.0, -1.0, 1.0]), np.array([-0.45, 0.15, -0.6]), -1.0)}
# case -> class of the centre pixel's v_x
ROT_CLASS = {"rotA_3e-11": "plus", "rotA_5e-7": "plus", "rotA_2e-5": "none", "rotB_3e-11": "plus", "rotB_5e-7": "minus", "rotB_2e-5": "none"}


def _rotated_cases():
    """The slab camera's K at an axis-aligned pose turned about y by a tiny angle, T != 0: the centre pixel's v_x is -+sin(angle)
    reached through the cancellation in pw - o.  The thin slab hangs on the camera centre as SLAB_BOX does on the origin."""
    out = []
    for pose, (base, T, sense) in ROT_POSES.items():
        for tag, angle in ROT_ANGLES:
            c, s = math.cos(sense * angle), math.sin(sense * angle)
            R = base @ np.array([[c, 0, -s], [0, 1.0, 0], [s, 0, c]])  # the optical axis in the world is R[2] = (s, 0, c)
            T = T.reshape(3, 1)
            K = slab_camera(0.0)[0]
            o = trr.camera_origin(R, T)
            bounds = (o[None] + SLAB_BOX.astype(np.float64)).astype(F32)
            name = "%s_%s" % (pose, tag)
            _, d = trr.pixel_rays(K, R, T, [4], [8])
            v_x = float(d[0, 0] / np.sqrt((d[0] * d[0]).sum()))
            assert abs(abs(v_x) - angle) <= 1e-3 * angle and class_of(v_x) == ROT_CLASS[name], (name, v_x)
            assert class_of(float(F32(v_x))) == ROT_CLASS[name]
            out.append((name, SLAB_H, SLAB_W, K, R, T, bounds))
    return out


EDGE_CASES = _slab_cases() + _fixed_cases() + _rotated_cases()  # what the training path and the reference fixture also see
CASES = EDGE_CASES + _oblique_cases()
BY_NAME = {c[0]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def full_hull(H, W):
    """The CCW hull (x, y) of the whole image."""
    return np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]])


def ulp_diff(a, b):
    """Largest distance of two float32 arrays in units in the last place, on the number line: -0.0 and +0.0 are 0 apart."""
    def line(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == F32 and b.dtype == F32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return int(np.abs(line(a) - line(b)).max(initial=0))
