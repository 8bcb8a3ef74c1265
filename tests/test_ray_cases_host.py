"""tests/ray_cases.py on the host: the float32 restatement of csrc/nb_ray.h against the numpy oracle and the reference's own
fixture, every case in the class it was built for, no case decided by rounding, and the mutations the cases exist to catch."""
import os

import numpy as np
import pytest

from oracle import neuralbody_oracle as orc
from tests import ray_cases as rc
from tests import synthetic as syn
from tests import train_rays_ref as trr

NAMES = [c[0] for c in rc.CASES]
MIN_MARGIN = 16  # ulps between tn and tf wherever they are not the same bits


def _against(o, d, near, far, hit, ro, rd, rnear, rfar, rmask, what):
    assert hit.dtype == bool and np.array_equal(hit, rmask), what
    assert rc.ulp_diff(np.tile(o, (int(hit.sum()), 1)), np.ascontiguousarray(ro)) == 0, what
    assert rc.ulp_diff(d[hit], rd) == 0 and rc.ulp_diff(near[hit], rnear) == 0 and rc.ulp_diff(far[hit], rfar) == 0, what


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle(name):
    _, H, W, K, R, T, bounds = rc.BY_NAME[name]
    out = rc.image_rays32(H, W, K, R, T, bounds)
    assert [a.dtype for a in out[:4]] == [np.float32] * 4 and out[1].shape == (H * W, 3)
    _against(*out, *orc.image_rays(H, W, K, R, T, bounds), name)


def test_restatement_equals_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "raygen.npz"))
    for tag, body_kw, H, W, ff in (("a", dict(seed=3, box=(0.9, 1.7, 0.35), rh=(0.2, 0.4, 0.0), th=(0.3, 0.1, 0.2)), 40, 56, 1.1),
                                   ("b", dict(seed=4, box=(0.3, 0.5, 0.2)), 33, 17, 3.0)):
        body = syn.make_body(**body_kw)
        K, R, T = syn.make_camera(body, H, W, focal_factor=ff, distance=2.2, yaw=-0.6, pitch=0.25)
        o, d, near, far, hit = rc.image_rays32(H, W, K, R, T, body["can_bounds"])
        n = int(hit.sum())
        _against(o, d, near, far, hit, np.tile(g[tag + "_ray_o"], (n, 1)), g[tag + "_img_ray_d"], g[tag + "_img_near"],
                 g[tag + "_img_far"], g[tag + "_mask"], tag)
        assert rc.ulp_diff(d, g[tag + "_ray_d"].reshape(-1, 3)) == 0  # the missed pixels' directions too


@pytest.mark.parametrize("name", list(rc.SLAB))
def test_slab_case_is_in_its_interval_and_gives_the_tables_outcome(name):
    dcx, cls, hits, far_want = rc.SLAB[name]
    _, H, W, K, R, T, bounds = rc.BY_NAME[name]
    held = K[0, 2] - 8.0  # what cx holds of the offset (0.655 * 2^-10 loses its last bits next to 8)
    assert abs(held - dcx) <= 2.0 ** -50
    o, d, near, far, hit = rc.image_rays32(H, W, K, R, T, bounds)
    c = rc.SLAB_CENTRE
    assert d[c, 1] == 0 and d[c, 2] == 1 and d[c, 0] == np.float32(-held / 64)  # n = 1: v_x = d_x, every float64 step exact
    assert rc.class_of(float(d[c, 0])) == cls
    assert bool(hit[c]) == hits
    if hits:
        assert near[c] == 1 and abs(float(far[c]) - far_want) <= 1e-6 * far_want
        assert int(hit.sum()) == H and hit.reshape(H, W)[:, 8].all()  # the centre column and nothing else
    else:
        assert not hit.any()
    assert np.all(np.signbit(o)) and np.all(o == 0)  # -R^T T with T = 0 is -0.0


def test_tie_pixels_have_bit_equal_tn_and_tf_and_are_out():
    _, H, W, K, R, T, bounds = rc.BY_NAME["tie"]
    o, d = rc.cast_rays(H, W, K, R, T)
    tn, tf, n, hit = rc.slab32(bounds, o, d)
    assert int(hit.sum()) == 8 and {(p % W, p // W) for p in np.nonzero(hit)[0]} == {(x, y) for x in range(6) for y in range(6) if x < y < 4 * x}
    assert set(rc.TIE_NAMED) <= {(p % W, p // W) for p in rc.TIES["tie"]}
    for p in rc.TIES["tie"]:
        assert tn[p].tobytes() == tf[p].tobytes() and np.isfinite(tn[p]) and not hit[p], p
        assert d[p, 0].tobytes() == d[p, 1].tobytes() or (p == 4 * 6 + 1 and d[p, 1] == 4 * d[p, 0])
    assert np.array_equal(np.nonzero(tn == tf)[0], rc.TIES["tie"])


def test_inside_and_behind_keep_every_pixel():
    for name, sign in (("inside", 1), ("behind", -1)):
        _, H, W, K, R, T, bounds = rc.BY_NAME[name]
        _, _, near, far, hit = rc.image_rays32(H, W, K, R, T, bounds)
        assert hit.all() and np.all(near < 0) and np.all(near < far) and np.all(sign * far > 0), name


@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_decided_by_rounding(name):
    """Every pixel is a listed tie or has tn and tf at least 16 ulps apart: a device division or square root that is 1 ulp off
    (each of tn and tf then moves by a few ulps at most) cannot change a mask the GPU tests compare exactly."""
    m = rc.decision_margin(rc.BY_NAME[name])
    ties = np.zeros(m.size, bool)
    ties[list(rc.TIES.get(name, ()))] = True
    assert np.all(m[ties] == 0) and np.isfinite(m).all()
    assert m[~ties].min() >= MIN_MARGIN, (name, float(m[~ties].min()), int(np.argmin(np.where(ties, np.inf, m))))


@pytest.mark.parametrize("name", NAMES)
def test_float64_and_float32_paths_agree_on_the_mask(name):
    _, H, W, K, R, T, bounds = rc.BY_NAME[name]
    p = np.arange(H * W)
    o, d = trr.pixel_rays(K, R, T, p // W, p % W)
    _, _, hit64 = trr.near_far64(bounds, o, d)
    assert np.array_equal(hit64, rc.image_rays32(H, W, K, R, T, bounds)[4])


def _changed_by(mutation):
    """Names of the cases whose expected output (mask, or near / far of the kept pixels) the mutated restatement changes."""
    out = set()
    for name, H, W, K, R, T, bounds in rc.CASES:
        _, _, near, far, hit = rc.image_rays32(H, W, K, R, T, bounds)
        _, _, near_m, far_m, hit_m = rc.image_rays32(H, W, K, R, T, bounds, **{mutation: True})
        if not (np.array_equal(hit, hit_m) and np.array_equal(near[hit], near_m[hit]) and np.array_equal(far[hit], far_m[hit])):
            out.add(name)
    return out


def test_mutation_swapped_substitution_lines_is_caught():
    """:59 before :58 turns a component in (-1e-10, 1e-10) into -1e-5: the centre pixel's far becomes 1.5."""
    assert _changed_by("swap") == {"slab_zero", "slab_p30", "slab_m30", "rotA_3e-11", "rotB_3e-11"}
    _, H, W, K, R, T, bounds = rc.BY_NAME["slab_zero"]
    assert abs(float(rc.image_rays32(H, W, K, R, T, bounds, swap=True)[3][rc.SLAB_CENTRE]) - 1.5) < 1e-6


def test_mutation_non_strict_comparison_is_caught():
    """tn <= tf lets the tied pixels of `tie` in, and nothing else anywhere."""
    assert _changed_by("le") == {"tie"}
    _, H, W, K, R, T, bounds = rc.BY_NAME["tie"]
    hit, hit_le = rc.image_rays32(H, W, K, R, T, bounds)[4], rc.image_rays32(H, W, K, R, T, bounds, le=True)[4]
    assert np.array_equal(np.nonzero(hit != hit_le)[0], rc.TIES["tie"])


def test_mutation_symmetric_thresholds_is_caught():
    """With (-1e-10, 1e-10) in both lines a component of 9.5e-7 or 9.99e-6 is left alone and the thin slab is missed or left early."""
    assert _changed_by("symmetric") == {"slab_p14", "slab_m14", "slab_p655", "slab_m655", "rotA_5e-7", "rotB_5e-7"}


def test_rotated_cases_reach_their_class_through_cancellation():
    """T != 0: pw and o are O(1) and their difference's x component is the tiny one (the builder asserts its class)."""
    for name, cls in rc.ROT_CLASS.items():
        _, H, W, K, R, T, bounds = rc.BY_NAME[name]
        o, d = trr.pixel_rays(K, R, T, [4], [8])
        assert abs(o[0]) > 0.1 and abs(d[0, 0]) < 3e-5 and rc.class_of(float(d[0, 0] / np.linalg.norm(d[0]))) == cls
        hit = rc.image_rays32(H, W, K, R, T, bounds)[4]
        assert bool(hit[rc.SLAB_CENTRE]) == (cls != "none")
