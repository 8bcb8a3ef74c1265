"""The sample cull (cull_project / cull_inside / cull_pixel, csrc/nb_march_common.h) on the device at pixel edges, in every kernel it
is compiled into, against tests/cull_cases.py::chain — the restatement tests/test_cull_cases_host.py holds to the unmodified
reference's answers (tests/golden/cull_edges.npz) at every point.  The mask is a checkerboard, so a pixel off by one in x or y is
another answer; the points sit within 8 float32 steps of a pixel edge, where the candidate arithmetics (FMA chain, unfused,
another contraction; rint, floor(x + .5), truncation) disagree on hundreds of them.  Every comparison is exact: 0 differing points.

  nb_lattice_carve                       each line of case points as an [n, 1, 1] / [1, n, 1] lattice: the narrowest probe
  nb_march_kernel, nb_march_fold_kernel  rays of two samples that ARE two case points; a culled sample has raw == 0
  ... with the _msk pre-affine           through RendererMsk.make_cull and the scene's own pose
  nb_smpl_silhouette                     a mesh on which the FMA chain and the unfused projection snap a vertex differently

What the device matched before the projection was written as FMA chains (this file run once on the parent commit, MI355X): the
same eight `__fmul_rn / __fadd_rn` lines came out as THREE arithmetics, one per kernel, 16 of these tests failing.
  nb_lattice_carve       no restatement: != chain at 116 / 138 / 90 of the 3587 / 3587 / 3400 points of cam0 / cam1 / cam2
                         (!= contract_first at 54 / 75 / 41, != unfused at 239 / 157 / 153)
  nb_march_fold_kernel   contract_first, exactly (0 of 400 points; != chain at 69, != unfused at 208), with the pre-affine none
                         (!= chain at 85 of 400, != contract_first at 51)
  nb_march_kernel        no restatement: != chain at 102 of 400 points (cam1), 119 of 400 with the pre-affine
  nb_smpl_silhouette     the one pixel of the case below came out as chain's
Now every line above reads 0 for chain.
"""
import numpy as np
import pytest
import torch

from tests import cull_cases as cc
from tests import silhouette_ref as sil
from tests.test_gpu_march_rays import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _make_cull(cams):
    from neuralbody_amd import ops

    board = cc.checkerboard()
    return ops.make_cull(_dev(np.stack([board] * len(cams))), _dev(np.stack([c["RT"] for c in cams])), _dev(np.stack([c["K"] for c in cams])))


def _report(what, got, p, cams):
    """got: bool [n] from the device.  Prints how many points each restatement misses and asserts chain misses none."""
    want = cc.inside(cams, p, "chain")
    missed = dict((m, int((cc.inside(cams, p, m) != got).sum())) for m in cc.RESTATEMENTS)
    print("%s: %d points, %d inside; device differs from: %s" % (what, len(p), int(got.sum()), ", ".join("%s %d" % kv for kv in sorted(missed.items()))))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: the device differs from chain at %d of %d points, first %s" % (what, len(bad), len(p), p[bad[:3]].tolist())
    return missed


# ------------------------------------------------------------------------------------------------------------- nb_lattice_carve
def _carve_line(ln, cull):
    from neuralbody_amd import ops

    axes = [_dev(np.array([v], np.float32)) for v in (0.0, 0.0, 0.0)]
    others = [a for a in range(3) if a != ln["axis"]]
    axes[ln["axis"]] = _dev(ln["coords"])
    axes[others[0]], axes[others[1]] = _dev(ln["fixed"][:1]), _dev(ln["fixed"][1:])
    dims = [int(a.shape[0]) for a in axes]
    inside = torch.full(dims, 0xAB, dtype=torch.uint8, device=DEV)  # poisoned: every flag and the count must be written
    n_inside = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ops.lattice_carve(axes, cull[0], inside=inside, n_inside=n_inside)
    torch.cuda.synchronize()
    got = inside.cpu().numpy().reshape(-1)
    assert set(np.unique(got)) <= {0, 1} and int(n_inside.item()) == int(got.sum())
    return got.astype(bool)


@pytest.mark.parametrize("names", [("cam0",), ("cam1",), ("cam2",), ("cam0", "cam1", "cam2")], ids="+".join)
def test_carve_equals_the_chain_at_every_edge_point(names):
    cams = [cc.camera(n) for n in names]
    cull = _make_cull(cams)
    got, pts = [], []
    for n in names:
        for ln in cc.lines(n):
            got.append(_carve_line(ln, cull))
            pts.append(ln["points"])
    got, pts = np.concatenate(got), np.concatenate(pts)
    missed = _report("carve " + "+".join(names), got, pts, cams)
    # the fixture tells the device's arithmetic from the mutants': each of them misses points the device gets right
    assert missed["unfused"] >= 8 and missed["contract_first"] >= 4 and missed["floor_half"] >= 1 and missed["trunc"] >= 8


def test_carve_looks_the_plain_cases_up_at_their_stated_pixels():
    """Ties (half to even), a point behind the camera, inf and NaN (pixel 0), the clamp, beyond the int64 range (pixel 0): each
    plain case as a 1 x 1 x 1 lattice against the checkerboard and against a mask that holds the stated pixel alone."""
    from neuralbody_amd import ops

    board = cc.checkerboard()
    p = cc.points("pow2")
    cull = _make_cull([cc.POW2])
    inside = torch.full((len(p),), 0xAB, dtype=torch.uint8, device=DEV)
    single = torch.full((len(p),), 0xAB, dtype=torch.uint8, device=DEV)
    n_inside = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    masks = np.zeros((len(p), cc.H, cc.W), np.uint8)
    for i, (_, _, (x, y)) in enumerate(cc.PLAIN):
        masks[i, y, x] = 255
    masks_d = _dev(masks)
    RT, K = _dev(cc.POW2["RT"][None]), _dev(cc.POW2["K"][None])
    keep = []
    for i in range(len(p)):
        axes = [_dev(p[i, a : a + 1]) for a in range(3)]
        ops.lattice_carve(axes, cull[0], inside=inside[i : i + 1].view(1, 1, 1), n_inside=n_inside)
        one = ops.make_cull(masks_d[i : i + 1], RT, K)
        keep.append(one)
        ops.lattice_carve(axes, one[0], inside=single[i : i + 1].view(1, 1, 1), n_inside=n_inside)
    torch.cuda.synchronize()
    got, got_single = inside.cpu().numpy(), single.cpu().numpy()
    for i, (name, _, (x, y)) in enumerate(cc.PLAIN):
        assert got_single[i] == 1, "%s is not looked up at pixel (%d, %d)" % (name, x, y)
        assert got[i] == board[y, x], name
    assert np.array_equal(got.astype(bool), cc.inside([cc.POW2], p, "chain"))


# ------------------------------------------------------------------------------------------------------------------ the marches
_RAYS = {}


def _rays(names, n_rays):
    key = (names, n_rays)
    if key not in _RAYS:
        d = cc.march_rays(names, n_rays)
        _RAYS[key] = (d, [_dev(d[k]) for k in ("ray_o", "ray_d", "near", "far", "t_vals")])
    return _RAYS[key]


def _march_raw(precision, rays, cull):
    from neuralbody_amd import ops

    sc = _scene()
    with torch.no_grad():
        out = ops.march(sc["scene"][precision], sc["packed"][precision], sc["lb"], *rays, None, want_raw=True, precision=precision, cull=cull)
    torch.cuda.synchronize()
    return out["raw"].cpu().numpy()


def _march_case(names, n_rays, precision, cull, cams):
    d, rays = _rays(names, n_rays)
    free = _march_raw(precision, rays, None)
    assert free.shape == (n_rays, 2, 4)
    assert (free != 0).any(-1).all(), "a case point decodes to raw == 0 without culling: kept and culled could not be told apart"
    raw = _march_raw(precision, rays, cull)
    kept = (raw != 0).any(-1)
    assert not raw[~kept].any()
    # a kept sample is the sample of the march without culling (fp32: the same decode; f16f6: the grouping may differ)
    if precision == "f32":
        assert np.array_equal(raw[kept].view(np.uint32), free[kept].view(np.uint32))
    return _report("march %s %s, %d rays" % ("+".join(names), precision, n_rays), kept.reshape(-1), d["points"].reshape(-1, 3), cams)


@pytest.mark.parametrize("precision", ["f32", "f16f6"])
@pytest.mark.parametrize("n_rays", [64, 200])
@pytest.mark.parametrize("names", [("cam1",), ("cam0", "cam1", "cam2")], ids="+".join)
def test_march_keeps_exactly_the_samples_the_chain_keeps(names, n_rays, precision):
    """Rays of two samples whose positions are two case points exactly (the host test asserts it): the kept / culled pattern of
    nb_march_kernel (f32) and nb_march_fold_kernel<0, true> (f16f6) equals chain's, one view and three."""
    cams = [cc.camera(n) for n in names]
    missed = _march_case(names, n_rays, precision, _make_cull(cams), cams)
    assert missed["unfused"] >= 8 and missed["contract_first"] >= 4


@pytest.mark.parametrize("precision", ["f32", "f16f6"])
@pytest.mark.parametrize("n_rays", [64, 200])
def test_march_with_the_msk_pre_affine_keeps_what_the_chain_keeps(n_rays, precision):
    """The _msk renderer's cull: world -> SMPL space of the scene's pose -> the snapshot frame's world -> its camera.  The cull is
    the one RendererMsk.make_cull builds from the batch; R and Th come from the scene the march is given."""
    from neuralbody_amd.renderer import RendererMsk

    cam = cc.camera("pre")
    batch = dict(msk=_dev(cc.checkerboard()[None]), RT=_dev(cam["RT"][None]), K=_dev(cam["K"][None]), R0_snap=_dev(cam["R0"][None]),
                 Th0_snap=_dev(cam["Th0"][None]))
    cull = RendererMsk(_scene()["net"]).make_cull(batch)
    assert cull[0].pre_affine == 1
    missed = _march_case(("pre",), n_rays, precision, cull, [cam])
    assert missed["unfused"] >= 8 and missed["contract_first"] >= 4


# ------------------------------------------------------------------------------------------------------------ nb_smpl_silhouette
def test_silhouette_equals_the_chain_where_the_unfused_projection_snaps_another_mask():
    """cull_cases.silhouette_case: a placement of the ico1280 mesh at 96 x 128 found by search on the CPU, where snapped_mask under
    `unfused` and under `chain` differ in a pixel of view 0; the device masks (poisoned buffer) equal the chain ones bit for bit."""
    from neuralbody_amd import ops

    c = cc.silhouette_case()
    want = sil.snapped_stack(c["verts"], c["faces"], c["Ks"], c["RTs"], c["H"], c["W"])
    other = np.stack([np.stack([sil.snapped_mask(c["verts"][f], c["faces"], c["Ks"][v], c["RTs"][v], c["H"], c["W"], "unfused")
                                for v in range(len(c["Ks"]))]) for f in range(len(c["verts"]))])
    assert (want != other).any(), "the case does not tell chain from unfused"
    out = torch.full(want.shape, 0xAB, dtype=torch.uint8, device=DEV)
    got = ops.smpl_silhouette(_dev(c["verts"]), _dev(c["faces"]), _dev(c["RTs"]), _dev(c["Ks"]), c["H"], c["W"], out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    print("silhouette: %d pixels differ between chain and unfused; device != chain at %d, != unfused at %d" % (
        int((want != other).sum()), int((got != want).sum()), int((got != other).sum())))
    assert np.array_equal(got, want)
