"""CPU checks of tests/cull_cases.py against tests/golden/cull_edges.npz (the unmodified reference's three sample culls on the same
points): `chain` is what the reference computes, at every point; each mutant restatement is told apart from it; the plain cases are
looked up at their stated pixels; the rays of the device test carry the case points exactly."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import cull_cases as cc
from tests import march_ray_cases as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cull_edges.npz")
FUNCTIONS = ("inside_mmsk", "inside_msk", "inside_mesh")


def _gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fma32_is_correctly_rounded():
    """fma32 against rational arithmetic on random operands, on operands built so that the float64 sum lands on a float32 midpoint
    with a remainder on either side (where rounding the float64 sum again goes wrong), and on cancelling sums."""
    rs = np.random.RandomState(5)
    a = rs.standard_normal(3000).astype(np.float32)
    b = rs.standard_normal(3000).astype(np.float32)
    c = (rs.standard_normal(3000) * 10.0 ** rs.randint(-3, 4, 3000)).astype(np.float32)
    c[:500] = (-(a[:500].astype(np.float64) * b[:500])).astype(np.float32)  # cancellation: the result is the product's rounding error
    # a b = 64 - 2^-40.  2^30 + 128 + a b lies just BELOW the midpoint 2^30 + 192 of two float32 numbers; the float64 sum is the
    # midpoint itself, and rounding that again goes up to the even 2^30 + 256.  -(2^30 + 128) + a b: the mirror image
    a = np.concatenate([a, np.array([8.0 * (1.0 + 2.0 ** -23)] * 2, np.float32)])
    b = np.concatenate([b, np.array([8.0 * (1.0 - 2.0 ** -23)] * 2, np.float32)])
    c = np.concatenate([c, np.array([2.0 ** 30 + 128.0, -(2.0 ** 30 + 128.0)], np.float32)])
    got = cc.fma32(a, b, c)
    assert got[-2] == np.float32(2.0 ** 30 + 128.0) and got[-1] == np.float32(-(2.0 ** 30 + 128.0))
    assert got.dtype == np.float32
    double_rounded = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    n_hard = 0
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = Fraction(float(got[i]))
        lo, hi = (Fraction(float(np.nextafter(got[i], np.float32(s)))) for s in (-np.inf, np.inf))
        # nearest: no neighbour is closer; a tie goes to the even significand
        assert abs(g - exact) <= abs(lo - exact) and abs(g - exact) <= abs(hi - exact), (i, a[i], b[i], c[i])
        if abs(g - exact) == abs(lo - exact) or abs(g - exact) == abs(hi - exact):
            assert (got[i : i + 1].view(np.uint32)[0] & 1) == 0
        n_hard += int(double_rounded[i] != got[i])
    print("fma32: %d operands, %d on which float64 arithmetic rounded again differs" % (len(a), n_hard))
    assert n_hard >= 2


@pytest.mark.parametrize("name", cc.SET_NAMES)
def test_chain_is_what_the_reference_computes(name):
    """`chain` equals the fixture at EVERY point, for each of the reference's functions the set went through: 0 differing.  The
    fixture's points are the ones cull_cases builds, and each call had more than 7 rows."""
    g = _gold()
    p, cam = cc.points(name), cc.camera(name)
    assert np.array_equal(g[name + "/points"].view(np.uint32), p.view(np.uint32)), "the fixture was made on other points"
    assert int(g[name + "/rows"]) > 7 and int(g[name + "/rows"]) >= len(p)
    want = cc.inside(cc.views(name), p, "chain")
    seen = 0
    for fn in FUNCTIONS:
        key = "%s/%s" % (name, fn)
        if key not in g:
            continue
        seen += 1
        ok = cc.mesh_comparable(cam, p) if fn == "inside_mesh" else np.ones(len(p), bool)
        differ = np.flatnonzero((g[key].astype(bool) != want) & ok)
        print("%s: %d points (%d rows in the call), chain differs from the reference at %d" % (key, int(ok.sum()), int(g[name + "/rows"]), len(differ)))
        assert len(differ) == 0, "%s: chain differs at points %s" % (key, differ[:20].tolist())
    assert seen == (1 if name == "pre" else 2)


@pytest.mark.parametrize("name", cc.EDGE_SETS)
def test_every_mutant_is_told_apart_from_the_fixture(name):
    """The fixture condition: per camera at least 32 case points where chain and unfused pick different pixels and at least 8 where
    chain and contract_first do — and each of those mutants then disagrees with the REFERENCE's answer on at least as many (the
    checkerboard turns every other pixel into another answer).  The rounding mutants differ on the edge points too."""
    g = _gold()
    p = cc.points(name)
    counts = cc.fixture_counts(name)
    fn = "inside_msk" if name == "pre" else "inside_mmsk"
    ref = g["%s/%s" % (name, fn)].astype(bool)
    vs_ref = dict((m, np.flatnonzero(cc.inside(cc.views(name), p, m) != ref)) for m in cc.MUTANTS)
    print("%s: %d points; pixels differ from chain: %s; answers differ from the reference: %s" % (
        name, len(p), ", ".join("%s %d" % kv for kv in sorted(counts.items())), ", ".join("%s %d" % (m, len(v)) for m, v in sorted(vs_ref.items()))))
    assert counts["unfused"] >= cc.MIN_CHAIN_VS_UNFUSED and counts["contract_first"] >= cc.MIN_CHAIN_VS_CONTRACT_FIRST
    assert len(vs_ref["unfused"]) >= cc.MIN_CHAIN_VS_UNFUSED and len(vs_ref["contract_first"]) >= cc.MIN_CHAIN_VS_CONTRACT_FIRST
    assert len(vs_ref["floor_half"]) >= cc.MIN_CHAIN_VS_CONTRACT_FIRST and len(vs_ref["trunc"]) >= cc.MIN_CHAIN_VS_UNFUSED
    # the edge points straddle their edges: both neighbouring pixels occur on every line, within a pixel of the edge in float64
    cam = cc.camera(name)
    for ln in cc.lines(name):
        u = cc.project_f64(cam, ln["points"])[ln["axis"]]
        assert np.abs(u - ln["edge"]).max() < 1e-3
        got = cc.pixels(cam, ln["points"])[ln["axis"]]
        assert (got == ln["edge"] - 0.5).any() and (got == ln["edge"] + 0.5).any() and len(ln["coords"]) >= 17 * 24
        assert np.abs(ln["points"] - cc.CENTRE).max() <= cc.HALF + 1e-6


def test_plain_cases_are_looked_up_at_their_stated_pixels():
    """Ties go to the even pixel, a point behind the camera is projected like any other, inf and NaN read pixel 0, coordinates off the
    image clamp to its border, and a coordinate beyond the int64 range reads pixel 0 — in `chain` and in the reference (fixture);
    floor(x + .5) and truncation miss the named ties."""
    g = _gold()
    p = cc.points("pow2")
    x, y = cc.pixels(cc.POW2, p)
    board = cc.checkerboard()
    wrong = {"floor_half": [], "trunc": []}
    for i, (name, _, (wx, wy)) in enumerate(cc.PLAIN):
        assert (int(x[i]), int(y[i])) == (wx, wy), name
        assert bool(g["pow2/inside_mmsk"][i]) == bool(board[wy, wx]), name
        for m in wrong:
            mx, my = cc.pixels(cc.POW2, p[i : i + 1], m)
            if (int(mx[0]), int(my[0])) != (wx, wy):
                wrong[m].append(name)
    print("plain cases missed by the rounding mutants:", wrong)
    assert {"tie-x-10", "tie-x-300", "tie-y-20", "tie-y-400", "tie-xy"} <= set(wrong["floor_half"])
    assert {"tie-x-11", "tie-x-301", "tie-y-21", "tie-y-401", "tie-xy"} <= set(wrong["trunc"])
    # the arithmetic mutants cannot differ here: every product is exact
    for m in ("unfused", "contract_first"):
        mx, my = cc.pixels(cc.POW2, p, m)
        assert np.array_equal(mx, x) and np.array_equal(my, y)


def test_silhouette_case_tells_the_chain_from_the_unfused_projection():
    from tests import silhouette_ref as sil

    c = cc.silhouette_case()
    masks = dict((a, np.stack([sil.snapped_mask(c["verts"][0], c["faces"], c["Ks"][v], c["RTs"][v], c["H"], c["W"], a) for v in range(3)]))
                 for a in ("chain", "unfused"))
    differ = (masks["chain"] != masks["unfused"]).reshape(3, -1).sum(1)
    print("silhouette case: pixels that differ between chain and unfused per view: %s; covered %s" % (differ.tolist(), masks["chain"].reshape(3, -1).sum(1).tolist()))
    assert differ.sum() >= 1 and all(sil.view_culls(c["verts"][0], c["Ks"][v], c["RTs"][v]) for v in range(3))
    assert 0 < masks["chain"].mean() < 1


@pytest.mark.parametrize("names,n_rays", [(("cam0",), 64), (("cam1",), 200), (("cam0", "cam1", "cam2"), 64), (("cam0", "cam1", "cam2"), 200),
                                          (("pre",), 64), (("pre",), 200)])
def test_march_rays_carry_the_case_points_exactly(names, n_rays):
    """z_lin and ray_point (numpy float32, one rounding per operation: what the kernels do) give the two chosen case points of every
    ray bit for bit, and the rays keep enough points on which the candidates disagree."""
    d = cc.march_rays(names, n_rays)
    z = R.z_vals_f32(d["near"], d["far"], d["t_vals"])
    assert np.array_equal(z[:, 0].view(np.uint32), d["near"].view(np.uint32)) and np.array_equal(z[:, 1].view(np.uint32), d["far"].view(np.uint32))
    p, _ = R.sample_points_f32(d["ray_o"], d["ray_d"], z)
    assert np.array_equal(p.view(np.uint32), d["points"].view(np.uint32))
    pts = d["points"].reshape(-1, 3)
    cams = [cc.camera(n) for n in names]
    want = cc.inside(cams, pts, "chain")
    missed = dict((m, int((cc.inside(cams, pts, m) != want).sum())) for m in cc.MUTANTS)
    print("%s, %d rays: %d of %d samples kept; answers that differ from chain: %s" % ("+".join(names), n_rays, int(want.sum()), len(want), missed))
    assert 0 < want.sum() < len(want)
    assert missed["unfused"] >= 8 and missed["contract_first"] >= 4
