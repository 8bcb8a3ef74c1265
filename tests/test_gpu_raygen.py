"""nb_raygen and nb_train_rays on the edge cases of tests/ray_cases.py: direction components at and around zero (the two
substitution lines of get_near_far), tn == tf, a camera inside the box, a box behind it, images that miss or hit as a whole,
one-pixel-wide images, and the launch and scan-tile edges.  Expected values are the float32 restatement image_rays32 (held to
the reference and the oracle bit for bit by tests/test_ray_cases_host.py and tests/test_oracle_golden.py) and, for the training
path, train_rays_ref.sample.  No case is decided by rounding (test_no_case_is_decided_by_rounding), so masks compare exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import ray_cases as rc
from tests import synthetic as syn
from tests import train_rays_ref as trr
from tests.test_gpu_train_rays import _assert_same, _dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR_FAR_ULP = 0  # see test_raygen_on_every_case
_WANT = {}


def _want(name):
    """image_rays32 of a case, computed once and left alone."""
    if name not in _WANT:
        _, Hh, Ww, K, R, T, bounds = rc.BY_NAME[name]
        _WANT[name] = rc.image_rays32(Hh, Ww, K, R, T, bounds)
        for a in _WANT[name]:
            a.setflags(write=False)
    return _WANT[name]


def _poisoned(n):
    """Outputs of an n-pixel nb_raygen call filled with NaN (floats) and 0xFF bytes (mask, count)."""
    nan = float("nan")
    return dict(ray_o=torch.full((n, 3), nan, device=DEV), ray_d=torch.full((n, 3), nan, device=DEV), near=torch.full((n,), nan, device=DEV),
                far=torch.full((n,), nan, device=DEV), mask=torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV),
                n_rays=torch.full((1,), -1, dtype=torch.int32, device=DEV))


def _call(Hh, Ww, K, R, T, bounds, out, scratch, null=None):
    from neuralbody_amd import _lib

    p = {k: (None if k == null else _lib.ptr(v)) for k, v in out.items()}
    K, R = (np.asarray(m, np.float64).reshape(9) for m in (K, R))
    return _lib.lib().nb_raygen(Hh, Ww, (C.c_double * 9)(*K), (C.c_double * 9)(*R), (C.c_double * 3)(*np.asarray(T, np.float64).reshape(3)),
                                (C.c_float * 6)(*np.asarray(bounds, np.float32).reshape(6)), p["ray_o"], p["ray_d"], p["near"], p["far"],
                                p["mask"], p["n_rays"], _lib.ptr(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _raygen(case):
    from neuralbody_amd import _lib, ops

    _, Hh, Ww, K, R, T, bounds = case
    out = _poisoned(Hh * Ww)
    _lib.check(_call(Hh, Ww, K, R, T, bounds, out, ops.scan_scratch(Hh * Ww, DEV)), "nb_raygen")
    torch.cuda.synchronize()
    return out


def _compare(got, want, what, bound):
    """Device outputs (dict of numpy arrays) against (o, d, near, far, hit) of all pixels -> measured (near, far) ulp."""
    o, d, near, far, hit = want
    n = int(hit.sum())
    assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], hit.astype(np.uint8)), what  # 0 / 1 bytes, no 0xFF left
    assert int(got["n_rays"][0]) == n, what
    # the first n rows are the hit pixels in row-major order: their directions are those pixels' own
    assert rc.ulp_diff(got["ray_d"][:n], d[hit]) == 0, what
    assert rc.ulp_diff(got["ray_o"][:n], np.tile(o, (n, 1))) == 0, what
    assert np.array_equal(np.signbit(got["ray_o"][:n]), np.tile(np.signbit(o), (n, 1))), what
    assert np.array_equal(np.signbit(got["ray_d"][:n]), np.signbit(d[hit])), what
    ulps = rc.ulp_diff(got["near"][:n], near[hit]), rc.ulp_diff(got["far"][:n], far[hit])
    print("%s: %d of %d pixels hit; near %d ulp, far %d ulp" % (what, n, hit.size, ulps[0], ulps[1]))
    assert max(ulps) <= bound, (what, ulps)
    return ulps


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", [c[0] for c in rc.CASES])
def test_raygen_on_every_case(name):
    """Mask, count and row order exactly; ray_o and ray_d at 0 ulp with numpy's signs of zero; near and far within NEAR_FAR_ULP.
    Every operation of the float32 slab test is meant to be one IEEE operation, so 0 ulp is what to expect.  Measured on an MI355X:
    first up to 2 ulp (near of sizes_2049; 1 ulp on H1 and five of the sizes_* cases, 0 on the rest), over the "at most 1 ulp" the
    project had recorded against the reference fixture (tests/test_gpu_train_rays.py, case D): the `_rn` intrinsics of csrc/nb_ray.h
    were contracted and the norm was fma(dx, dx, dy * dy) + dz * dz.  With the header's arithmetic under `fp contract(off)` the
    measured maximum is 0 ulp of near and of far on every case and on both fixture cameras, so the bound is 0."""
    case = rc.BY_NAME[name]
    got = _host(_raygen(case))
    want = _want(name)
    _compare(got, want, name, NEAR_FAR_ULP)
    o, _, _, _, hit = want
    n = int(hit.sum())
    if np.all(np.asarray(case[5]) == 0) and n:
        assert np.all(got["ray_o"][:n] == 0) and np.all(np.signbit(got["ray_o"][:n]))  # -R^T T = -0.0, as in numpy
    if name in ("slab_p8", "slab_m8", "rotA_2e-5", "rotB_2e-5"):
        assert n == 0 and not got["mask"].any()
    if name in ("inside", "behind"):
        assert n == hit.size and got["mask"].all()


def test_raygen_on_the_reference_fixture_cameras():
    """The two cameras of tests/golden/raygen.npz with the comparison above, against the restatement and the fixture itself."""
    g = np.load(H.GOLDEN + "/raygen.npz")
    for tag, body_kw, Hh, Ww, ff in (("a", dict(seed=3, box=(0.9, 1.7, 0.35), rh=(0.2, 0.4, 0.0), th=(0.3, 0.1, 0.2)), 40, 56, 1.1),
                                     ("b", dict(seed=4, box=(0.3, 0.5, 0.2)), 33, 17, 3.0)):
        body = syn.make_body(**body_kw)
        K, R, T = syn.make_camera(body, Hh, Ww, focal_factor=ff, distance=2.2, yaw=-0.6, pitch=0.25)
        got = _host(_raygen((tag, Hh, Ww, K, R, T, body["can_bounds"])))
        _compare(got, rc.image_rays32(Hh, Ww, K, R, T, body["can_bounds"]), "golden " + tag, NEAR_FAR_ULP)
        n = int(got["n_rays"][0])
        assert np.array_equal(got["mask"].astype(bool), g[tag + "_mask"]) and rc.ulp_diff(got["ray_d"][:n], g[tag + "_img_ray_d"]) == 0
        assert max(rc.ulp_diff(got["near"][:n], g[tag + "_img_near"]), rc.ulp_diff(got["far"][:n], g[tag + "_img_far"])) <= NEAR_FAR_ULP


@pytest.mark.parametrize("name", ["slab_zero", "slab_p8", "tie", "sizes_%d" % (2 * rc.TILE + 1)])
def test_raygen_repeats_bit_for_bit(name):
    """Through ops.raygen, which allocates outputs and scratch itself: the valid rows, the mask and the count, byte for byte."""
    from neuralbody_amd import ops

    keys = ("ray_o", "ray_d", "near", "far", "mask", "n_rays")
    first = dict(zip(keys, ops.raygen(*rc.BY_NAME[name][1:], DEV)))
    torch.empty(1 << 22, device=DEV).normal_()  # other work in between: the second call's buffers are not the first's
    second = dict(zip(keys, ops.raygen(*rc.BY_NAME[name][1:], DEV)))
    torch.cuda.synchronize()
    n = int(first["n_rays"])
    assert n == int(second["n_rays"])
    assert torch.equal(first["mask"], second["mask"])
    for k in ("ray_o", "ray_d", "near", "far"):
        assert torch.equal(first[k][:n].view(torch.uint8).reshape(-1), second[k][:n].view(torch.uint8).reshape(-1)), k
    _compare(_host(first), _want(name), "ops.raygen " + name, NEAR_FAR_ULP)


@pytest.mark.parametrize("name", [c[0] for c in rc.EDGE_CASES])
def test_train_rays_on_the_edge_cases(name):
    """The float64 path of the same header: every pixel a candidate (full-image hull, msk of ones, plain mode), 64 rays, 4 rounds.
    With the zero and +2^-14 slab cameras only the centre column hits and the batch stays short at 12 rays; with 2^-8 nothing
    hits, the batch is padding from row 0 on."""
    from neuralbody_amd.train_rays import TrainRaySampler

    _, Hh, Ww, K, R, T, bounds = rc.BY_NAME[name]
    rs = np.random.RandomState(1)
    u = rs.uniform(0, 1, (4, 64)).astype(np.float32)
    c = dict(img=rs.uniform(0, 1, (Hh, Ww, 3)).astype(np.float32), msk=np.ones((Hh, Ww), np.uint8), K=K, R=R, T=T, bounds=bounds,
             hull=rc.full_hull(Hh, Ww), mode="plain")
    want = trr.sample(u=u, body_ratio=0.5, **c)
    if name in ("slab_zero", "slab_p14"):
        assert want["status"].tolist() == [12, 4, Hh * Ww, Hh * Ww]
    if name == "slab_p8":
        assert want["status"].tolist() == [0, 4, Hh * Ww, Hh * Ww] and (want["pixel"] == -1).all()
    if name in ("inside", "behind"):
        assert want["status"].tolist() == [64, 1, Hh * Ww, Hh * Ww]
    s = TrainRaySampler(Hh, Ww, 64, mode="plain", device=DEV)
    out = s.sample(_dev(c["img"]), _dev(c["msk"]), K, R, T, bounds, u=_dev(u), hull=c["hull"])
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _assert_same(got, want, "train " + name)
    n = int(want["status"][0])
    pix = got["pixel"][:n]
    assert _want(name)[4][pix[:, 0] * Ww + pix[:, 1]].all()  # the float64 path keeps pixels the float32 path keeps
    assert s.check() == tuple(int(v) for v in want["status"])


@pytest.mark.parametrize("what", ["singular K", "H = 0", "W = 0", "NULL ray_d", "NULL n_rays"])
def test_raygen_refuses_bad_arguments_and_launches_nothing(what):
    from neuralbody_amd import _lib, ops

    _, Hh, Ww, K, R, T, bounds = rc.BY_NAME["inside"]  # every pixel would be written
    out = _poisoned(Hh * Ww)
    before = {k: v.clone() for k, v in out.items()}
    scratch = ops.scan_scratch(Hh * Ww, DEV)
    torch.cuda.synchronize()
    if what == "singular K":
        rc_ = _call(Hh, Ww, np.array([[32.0, 0, 8], [64.0, 0, 16], [0, 0, 1]]), R, T, bounds, out, scratch)
    elif what == "H = 0":
        rc_ = _call(0, Ww, K, R, T, bounds, out, scratch)
    elif what == "W = 0":
        rc_ = _call(Hh, 0, K, R, T, bounds, out, scratch)
    else:
        rc_ = _call(Hh, Ww, K, R, T, bounds, out, scratch, null=what.split()[1])
    with pytest.raises(_lib.NbError, match="nb_raygen"):
        _lib.check(rc_, "nb_raygen")
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k].view(torch.uint8).reshape(-1), before[k].view(torch.uint8).reshape(-1)), k
