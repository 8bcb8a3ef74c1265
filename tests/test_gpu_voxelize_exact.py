"""nb_smpl_voxelize (csrc/nb_smpl.hip) against its operation-by-operation restatement smpl_ref.voxelize_f32, with no band and no
tolerance: every entry of coord, bounds, out_sh and summary, on the cases of tests/voxelize_cases.py (which the host test
tests/test_voxelize_cases_host.py shows to tell the restatement's mutants apart).

The restatement is fed the DEVICE's own R: the kernel forms it with the device's fp64 sin and cos, which may differ from libm in the
last bit, so R is first held to 1 ulp of the host's cv2-style matrix and then taken as given.  Everything after R is float32
arithmetic in a stated order (fmaf chains, one subtraction), a float64 division and rint / ceil: nothing is left to round another
way."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import smpl_ref as sr
from tests import voxelize_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -7
KEYS = ("coord", "out_sh", "bounds", "R", "summary")


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)  # (the cases are read-only)


def _voxelize(case, voxel_size):
    from neuralbody_amd import ops

    out = ops.smpl_voxelize(_dev(case["verts"]), _dev(case["Rh"]), _dev(case["Th"]), voxel_size, case["pad"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_is_restatement(got, case, voxel_size, what):
    """got: host arrays with the frames leading (coord [F,V,3], out_sh [F,3], bounds [F,2,3], R [F,3,3], summary [F,9])."""
    F, V = case["verts"].shape[:2]
    assert got["coord"].shape == (F, V, 3) and got["coord"].dtype == np.int32
    for f in range(F):
        R = got["R"][f]
        want_R = vc.host_R(case["Rh"][f])
        assert bool((np.abs(R.astype(np.float64) - want_R.astype(np.float64)) <= np.spacing(np.abs(want_R))).all()), (what, f, "R")
        want = sr.voxelize_f32(case["verts"][f], R, case["Th"][f], voxel_size, case["pad"])
        diff = int((got["coord"][f] != want["coord"]).sum())
        assert diff == 0, "%s frame %d: coord differs at %d of %d entries, first at %s" % (
            what, f, diff, want["coord"].size, np.argwhere(got["coord"][f] != want["coord"])[0].tolist())
        assert np.array_equal(got["bounds"][f].view(np.uint32), want["bounds"].view(np.uint32)), (what, f, "bounds")
        assert np.array_equal(got["out_sh"][f], want["out_sh"]), (what, f, "out_sh", got["out_sh"][f].tolist(), want["out_sh"].tolist())
        assert np.array_equal(got["summary"][f], want["summary"]), (what, f, "summary")
        assert got["coord"][f].min() >= 0 and (got["coord"][f].max(axis=0) < got["out_sh"][f]).all(), (what, f)


# ---------------------------------------------------------------------------------------------------------- 1. fixture cases
@pytest.mark.parametrize("size", sorted(vc.VOXEL_SIZES))
@pytest.mark.parametrize("name,pad", sr.VOXEL_CASES)
def test_fixture_cases_bit_for_bit(name, pad, size):
    case, vs = vc.fixture_case(name, pad), vc.VOXEL_SIZES[size]
    got = _voxelize(case, vs)
    _assert_is_restatement(got, case, vs, "%s %s %s" % (name, pad, size))
    if size == "aniso":
        assert len(set(got["out_sh"][0].tolist())) > 1


# ---------------------------------------------------------------------------------------------------------- 2. block edges
@pytest.mark.parametrize("pad", sorted(sr.PADS))
@pytest.mark.parametrize("V", vc.EDGE_V)
def test_block_edges_with_guard_rows(V, pad):
    """Straight through the library with every output over-allocated by two frames and pre-filled: the F frames are the
    restatement's, everything behind them is untouched."""
    from neuralbody_amd import _lib

    case = vc.edge_case(V, pad)
    F, extra = vc.EDGE_FRAMES, 2
    verts, Rh, Th = _dev(case["verts"]), _dev(case["Rh"]), _dev(case["Th"])
    per_frame = {"coord": 3 * V, "out_sh": 3, "bounds": 6, "R": 9, "summary": 9}
    dtype = {"coord": torch.int32, "out_sh": torch.int32, "bounds": torch.float32, "R": torch.float32, "summary": torch.int32}
    out = {k: torch.full(((F + extra) * per_frame[k],), GUARD, dtype=dtype[k], device=DEV) for k in KEYS}
    _lib.check(_lib.lib().nb_smpl_voxelize(_lib.ptr(verts), V, F, _lib.ptr(Rh), _lib.ptr(Th), 3, (C.c_double * 3)(*vc.ANISO),
                                           _lib.PAD_MODES[pad], _lib.ptr(out["coord"]), _lib.ptr(out["out_sh"]), _lib.ptr(out["bounds"]),
                                           _lib.ptr(out["R"]), _lib.ptr(out["summary"]),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nb_smpl_voxelize")
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        tail = host[k][F * per_frame[k]:]
        assert tail.size == extra * per_frame[k] and bool((tail == GUARD).all()), (k, "written behind the %d frames" % F)
    shapes = {"coord": (F, V, 3), "out_sh": (F, 3), "bounds": (F, 2, 3), "R": (F, 3, 3), "summary": (F, 9)}
    got = {k: host[k][:F * per_frame[k]].reshape(shapes[k]) for k in KEYS}
    _assert_is_restatement(got, case, vc.ANISO, "V %d %s" % (V, pad))
    if V >= 2:
        assert not np.array_equal(got["bounds"][0], got["bounds"][1])


# ---------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("pad", vc.EXACT_PADS)
def test_ties_round_half_to_even(pad):
    """Exact inputs: on the unpadded axes (s - lo) / vs is an exact multiple of 1/2, and the expected voxel is integer arithmetic:
    0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4."""
    case = vc.tie_case(pad)
    got = _voxelize(case, vc.EXACT_VS)
    assert np.array_equal(got["R"][0], np.eye(3, dtype=np.float32))
    for a, want in case["expect"].items():
        col = got["coord"][0][:, 2 - a]
        assert np.array_equal(col, want), (pad, "xyz"[a], dict(zip(case["halves"][a], col.tolist())))
        lo = (vc.BASE[a] * vc.UNIT, (vc.BASE[a] + max(case["halves"][a]) * vc.half_voxel_units(a)) * vc.UNIT)
        assert (float(got["bounds"][0][0, a]), float(got["bounds"][0][1, a])) == lo
    _assert_is_restatement(got, case, vc.EXACT_VS, "ties %s" % pad)


# ---------------------------------------------------------------------------------------------------------- 4. out_sh edges
@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("pad", vc.EXACT_PADS)
def test_out_sh_at_exact_multiples_of_32_voxels(pad, single):
    """Extents of exactly 0 (one vertex), 31, 31.5, 32, 33 and 64 voxels -> 32, 32, 64, 64, 64, 96."""
    case = vc.out_sh_case(pad, single)
    got = _voxelize(case, vc.EXACT_VS)
    for f, want in enumerate(case["expect"]):
        assert {a: int(got["out_sh"][f][2 - a]) for a in want} == want, (pad, f)
        assert np.array_equal(got["summary"][f][6:], got["out_sh"][f])
    _assert_is_restatement(got, case, vc.EXACT_VS, "out_sh %s" % pad)
