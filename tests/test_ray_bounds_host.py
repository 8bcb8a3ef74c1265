"""The ray bounds' definitions (tests/ray_bounds_ref.py) checked on the host, before the device is held to them bit for bit
(tests/test_gpu_ray_bounds.py): coverage is the silhouette's, a view that does not bound says so, no point of the surface leaves its
pixel's widened interval, and the cases tell the definitions apart from three mutants."""
import numpy as np
import pytest

from tests import ray_bounds_ref as rb
from tests import silhouette_ref as sil

N_POINTS = 20000
DEPTH_TOL = 1e-5  # metres: the fp32 rounding of a camera depth below 10 m (half an ulp is 4.8e-7) with room for the chain's three terms


def _views(c):
    return [(f, v) for f in range(c["verts"].shape[0]) for v in range(c["Ks"].shape[0])]


@pytest.mark.parametrize("name", rb.CASES)
def test_coverage_is_the_silhouettes_and_a_view_that_does_not_bound_is_unbounded(name):
    c, r = rb.case_ranges(name)
    assert r.shape == (2, 3, c["H"], c["W"], 2) and r.dtype == np.float32 and not np.isnan(r).any()
    unbounded = 0
    for f, v in _views(c):
        mask = sil.snapped_mask(c["verts"][f], c["faces"], c["Ks"][v], c["RTs"][v], c["H"], c["W"])
        if sil.view_culls(c["verts"][f], c["Ks"][v], c["RTs"][v]):
            assert np.array_equal(r[f, v, ..., 0] <= r[f, v, ..., 1], mask.astype(bool)), (f, v)
            empty = mask == 0
            assert (r[f, v][empty] == np.array(rb.EMPTY)).all() and np.isfinite(r[f, v][~empty]).all()
            assert (r[f, v][~empty] >= np.float32(sil.MIN_DEPTH)).all()
        else:
            unbounded += 1
            assert mask.all() and (r[f, v] == np.array(rb.UNBOUNDED)).all(), (f, v)
    assert unbounded == (0 if name == "paths" else 1)


@pytest.mark.parametrize("name", rb.CASES)
def test_no_point_of_the_surface_leaves_its_pixels_widened_interval(name):
    """Points of the unsnapped surface, projected in float64 and rounded to their pixel: the snap moves a triangle by 2.8e-3 px, so the
    3 x 3 window holds a pixel the point's own snapped triangle covers, whose interval holds the point's depth; blocks only widen."""
    c, r = rb.case_ranges(name)
    H, W = c["H"], c["W"]
    wide = {tile: rb.widen(r, 3, tile) for tile in (1, 8, 16)}
    checked = 0
    for f, v in _views(c):
        if not sil.view_culls(c["verts"][f], c["Ks"][v], c["RTs"][v]):
            continue
        pts = sil.surface_points(c["verts"][f], c["faces"], N_POINTS, seed=11 + 3 * f + v)
        uv, depth = sil.project(pts, c["Ks"][v], c["RTs"][v])
        x, y = np.rint(uv[:, 0]).astype(np.int64), np.rint(uv[:, 1]).astype(np.int64)
        on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        for tile, w in wide.items():
            lo, hi = w[f, v, y[on], x[on], 0].astype(np.float64), w[f, v, y[on], x[on], 1].astype(np.float64)
            bad = (depth[on] < lo - DEPTH_TOL) | (depth[on] > hi + DEPTH_TOL)
            assert not bad.any(), (name, f, v, tile, int(bad.sum()))
        checked += int(on.sum())
    print("%s: %d surface points on the image checked" % (name, checked))
    assert checked > N_POINTS


def test_the_cases_tell_the_definition_from_its_mutants():
    for name in rb.CASES:
        c, r = rb.case_ranges(name)
        kw = dict(verts=c["verts"], faces=c["faces"], Ks=c["Ks"], RTs=c["RTs"], H=c["H"], W=c["W"])
        centre = rb.depth_range_stack(coverage="centre", **kw)
        bary = rb.depth_range_stack(depth="barycentric", **kw)
        wrap = rb.widen(r, 3, 1, wrap=True)
        want = rb.widen(r, 3, 1)
        n = [int((m != d).any(axis=-1).sum()) for m, d in ((centre, r), (bary, r), (wrap, want))]
        print("%s: pixels that differ from the definition: centre coverage %d, barycentric depth %d, wrapping window %d" % (name, *n))
        assert min(n[:2]) > 0, name
        # pixel-centre coverage loses pixels the surface reaches; the wrapping window differs only where the body leaves the image
        assert ((centre[..., 0] <= centre[..., 1]) <= (r[..., 0] <= r[..., 1])).all()
        assert (n[2] > 0) == (name != "paths" or bool((r[..., 0] <= r[..., 1])[..., [0, -1], :].any())), name


def test_widen_and_cut_by_hand():
    r = np.empty((3, 4, 2), np.float32)
    r[...] = rb.EMPTY
    r[0, 0] = (2.0, 3.0)
    r[2, 3] = (1.0, 1.5)
    w = rb.widen(r, 3, 1)
    assert (w[1, 1] == (2.0, 3.0)).all() and (w[1, 2] == (1.0, 1.5)).all() and (w[0, 2] == rb.EMPTY).all()
    assert (w[1, 3] == (1.0, 1.5)).all() and (w[2, 0] == rb.EMPTY).all()  # no wrap
    assert (rb.widen(r, 3, 1, wrap=True)[2, 0] == (1.0, 3.0)).all()  # rows 1, 2, 0 and columns 3, 0, 1: both
    assert (rb.widen(r, 1, 1) == r).all()
    t = rb.widen(r, 1, 2)
    assert (t[:2, :2] == (2.0, 3.0)).all() and (t[2:, 2:] == (1.0, 1.5)).all() and (t[:2, 2:] == rb.EMPTY).all()
    assert (rb.widen(r, 1, 4)[..., 0] == 1.0).all() and (rb.widen(r, 1, 4)[..., 1] == 3.0).all()
    near, far = np.array([1.0, 1.0, 1.0, 1.0], np.float32), np.array([2.0, 2.0, 2.0, 2.0], np.float32)
    lo = np.array([-np.inf, 1.5, np.inf, 2.0], np.float32)
    hi = np.array([np.inf, 1.75, -np.inf, 2.5], np.float32)
    n2, f2, keep = rb.body_cut(near, far, lo, hi, 0.0)
    assert keep.tolist() == [True, True, False, False] and n2[:2].tolist() == [1.0, 1.5] and f2[:2].tolist() == [2.0, 1.75]
    assert rb.body_cut(near, far, lo, hi, 0.25)[2].tolist() == [True, True, False, True]
