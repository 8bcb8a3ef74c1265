"""The operation-by-operation restatement of nb_smpl_voxelize (smpl_ref.voxelize_f32) against the package's host frames, and the
cases of tests/voxelize_cases.py against the restatement's mutants: each mutant must change something on a case the GPU suite runs,
or the suite would pass a kernel that computes the mutant.  CPU only; nothing here touches a device."""
import numpy as np
import pytest

from tests import smpl_ref as sr
from tests import voxelize_cases as vc

HOST_FRAME_CASES = [c for c in sr.VOXEL_CASES if c[1] != "snapshot"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("size", sorted(vc.VOXEL_SIZES))
@pytest.mark.parametrize("name,pad", HOST_FRAME_CASES)
def test_restatement_is_the_host_frame(name, pad, size):
    """multi_view_frame at every coordinate, the ones within the band of a half-integer included, and every bit of bounds and
    can_bounds.  ('snapshot' stays with the banded comparison: rotate_smpl_frame moves the vertices to the centroid and back
    through float32, tests/test_gpu_smpl_pose.py says what that does to the last bit.)"""
    c, vs = vc.fixture_case(name, pad), vc.VOXEL_SIZES[size]
    host = sr.host_frame(c["verts"][0], c["Rh"][0], c["Th"][0], pad, vs)
    assert np.array_equal(_bits(host["R"]), _bits(vc.host_R(c["Rh"][0])))
    got = sr.voxelize_f32(c["verts"][0], host["R"], host["Th"], vs, pad)
    band = sr.near_band(sr.coord_f64(c["verts"][0], host["R"], host["Th"], pad, vs)[0])
    diff = int((got["coord"] != host["coord"]).sum())
    print("%s %s %s: out_sh %s, %d of %d coordinates differ (%d of them lie in the band)" % (
        name, pad, size, got["out_sh"].tolist(), diff, band.size, int(band.sum())))
    assert got["coord"].dtype == np.int32 and got["coord"].shape == host["coord"].shape and diff == 0
    assert np.array_equal(_bits(got["bounds"]), _bits(host["bounds"]))
    assert np.array_equal(got["out_sh"], host["out_sh"]) and np.array_equal(got["summary"][6:], host["out_sh"])
    assert np.array_equal(got["summary"][:6].view(np.uint32), _bits(host["can_bounds"]).reshape(-1))
    if size == "aniso":
        assert len(set(got["out_sh"].tolist())) > 1


def test_exact_cases_are_what_integer_arithmetic_says():
    """The tie and out_sh cases carry their own expectations; the restatement has to meet them before a device is held to either."""
    for pad in vc.EXACT_PADS:
        c = vc.tie_case(pad)
        got = sr.voxelize_f32(c["verts"][0], np.eye(3, dtype=np.float32), c["Th"][0], vc.EXACT_VS, pad)
        for a, want in c["expect"].items():
            assert np.array_equal(got["coord"][:, 2 - a], want), (pad, a)
            odd = np.array(c["halves"][a]) % 2 == 1
            assert odd.sum() >= 6 and set((want[odd] % 2).tolist()) == {0}  # a tie goes to the even voxel, up and down
            assert len({(h // 2) % 2 for h, o in zip(c["halves"][a], odd) if o}) == 2
        for single in (True, False):
            c = vc.out_sh_case(pad, single)
            for f, want in enumerate(c["expect"]):
                got = sr.voxelize_f32(c["verts"][f], np.eye(3, dtype=np.float32), c["Th"][f], vc.EXACT_VS, pad)
                assert {a: int(got["out_sh"][2 - a]) for a in want} == want, (pad, single, f)
    assert sorted(vc.OUT_SH_OF_HALVES.values()) == [32, 32, 64, 64, 64, 96]


# the cases that have to tell a mutant from the restatement, by the prefix of their names (voxelize_cases.suite)
KILLED_BY = {
    # (one vertex under 'snapshot' has no extent but the pad's 0.2 m along y, the middle entry either way)
    "vs_reversed": tuple("edge-%d-" % V for V in vc.EDGE_V if V >= 2) + ("tie-", "out_sh-zju", "out_sh-snapshot") + tuple(
        "fixture-%s-%s-aniso" % c for c in sr.VOXEL_CASES),
    "half_away": ("tie-",),
    "unfused": ("fixture-smpl6890_new-big_box-",),
    "floor_plus_1": ("out_sh-zju", "out_sh-snapshot"),
}


def test_every_mutant_is_told_apart_by_the_gpu_suite():
    suite = vc.suite()
    assert len(suite) == 12 + 3 * len(vc.EDGE_V) + 6 and set(KILLED_BY) == set(sr.VOXEL_MUTANTS)
    counts = {m: {} for m in sr.VOXEL_MUTANTS}
    for name, c, vs in suite:
        for f in range(c["verts"].shape[0]):
            R = vc.host_R(c["Rh"][f])
            exact = sr.voxelize_f32(c["verts"][f], R, c["Th"][f], vs, c["pad"])
            for m in sr.VOXEL_MUTANTS:
                n = vc.entries_changed(sr.voxelize_f32(c["verts"][f], R, c["Th"][f], vs, c["pad"], m), exact)
                counts[m][name] = counts[m].get(name, 0) + n
    for m in sr.VOXEL_MUTANTS:
        told = {k: n for k, n in counts[m].items() if n > 0}
        print("%s: changes entries (coord, bounds, out_sh, summary) on %d of %d cases" % (m, len(told), len(suite)))
        for k, n in told.items():
            print("    %-44s %d" % (k, n))
        must = [k for k in counts[m] if k.startswith(KILLED_BY[m])]
        assert must and all(counts[m][k] >= 1 for k in must), (m, {k: counts[m][k] for k in must})
    # an isotropic size cannot see the order of voxel_size: what the suite was blind to
    assert all(n == 0 for k, n in counts["vs_reversed"].items() if k.endswith("-iso"))


def test_lattice_axes_step_by_the_first_entry_along_x():
    """multi_view_mesh_dataset.py:150-156: voxel_size is read in xyz order there, entry 0 is the step along x."""
    from neuralbody_amd.mesh_lattice import lattice_axes

    can_bounds = np.array([[-0.31, -0.87, 0.11], [0.42, 0.953, 0.53]], np.float32)
    axes = lattice_axes(can_bounds, vc.ANISO)
    for a in range(3):
        want = np.arange(can_bounds[0, a], can_bounds[1, a] + vc.ANISO[a], vc.ANISO[a]).astype(np.float32)
        assert np.array_equal(axes[a], want), a
        step = np.diff(axes[a].astype(np.float64))
        assert axes[a][0] == can_bounds[0, a] and float(np.abs(step - vc.ANISO[a]).max()) < 1e-6
    # x: 0.73 m in steps of 4 mm, y: 1.823 m in steps of 5 mm, z: 0.42 m in steps of 8 mm
    assert [len(x) for x in axes] == [184, 366, 54]
    reversed_axes = lattice_axes(can_bounds, vc.ANISO[::-1])
    assert len(reversed_axes[0]) != len(axes[0]) and len(reversed_axes[2]) != len(axes[2])
