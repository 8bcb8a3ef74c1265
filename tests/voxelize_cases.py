"""The cases nb_smpl_voxelize is held to bit for bit (tests/test_gpu_voxelize_exact.py) and the host test that shows they tell the
mutants of smpl_ref.VOXELIZERS apart (tests/test_voxelize_cases_host.py).  CPU only; nothing here touches the library.

    fixture   the six smpl_ref.VOXEL_CASES (the reference layer's vertices, V = 321 and 6890), isotropic and ANISO
    edge      seeded clouds of V vertices around the voxeliser's workgroup of 1024 threads and the skinning's blocks of 64, three
              frames a call, each with its own cloud and pose, ANISO, every pad
    tie       exact inputs (R = I, dyadic Th, vertices on multiples of 2^-10, power-of-two voxel sizes): on an unpadded axis
              (s - lo) / vs is exact, so half-integers are TIES and the expected coordinate is integer arithmetic
    out_sh    the same exact inputs with extents of exactly 0, 31, 31.5, 32, 33 and 64 voxels on the unpadded axes
"""
import functools
import os

import numpy as np

from tests import smpl_ref as sr

ANISO = (0.004, 0.005, 0.008)  # dhw
VOXEL_SIZES = {"iso": sr.VOXEL_SIZE, "aniso": ANISO}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_pose.npz")
EDGE_V = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
EDGE_FRAMES = 3
BOX = (0.7, 1.8, 0.3)


def host_R(Rh):
    """cv2.Rodrigues(Rh)[0].astype(np.float32) as the package's host frames form it."""
    from neuralbody_amd.train_rays import rodrigues

    return rodrigues(np.asarray(Rh, np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


@functools.lru_cache(maxsize=None)
def fixture_case(name, pad):
    """-> dict(verts [1,V,3], Rh [1,3], Th [1,3]) of a smpl_ref.VOXEL_CASES entry (one frame)."""
    g = _gold()
    return _frozen(verts=g[name + "/verts"][None].copy(), Rh=g[name + "/Rh"][None].copy(), Th=g[name + "/Th"][None].copy(), pad=pad)


@functools.lru_cache(maxsize=None)
def edge_case(V, pad):
    """EDGE_FRAMES frames of V vertices: uniform in BOX (SMPL space), moved to the world by a non-zero Rh and Th of the frame's own."""
    rs = np.random.RandomState(5000 + 7 * V + sorted(sr.PADS).index(pad))
    verts, Rhs, Ths = [], [], []
    for _ in range(EDGE_FRAMES):
        smpl = (rs.uniform(-0.5, 0.5, (V, 3)) * np.array(BOX)).astype(np.float32)
        Rh = rs.uniform(-1.5, 1.5, 3).astype(np.float32)
        Th = rs.uniform(-1.0, 1.0, 3).astype(np.float32)
        verts.append((np.matmul(smpl, host_R(Rh).T) + Th[None]).astype(np.float32))
        Rhs.append(Rh)
        Ths.append(Th)
    return _frozen(verts=np.stack(verts), Rh=np.stack(Rhs), Th=np.stack(Ths), pad=pad)


# ------------------------------------------------------------------------------------------- exact inputs
EXACT_VS = (2.0 ** -7, 2.0 ** -8, 2.0 ** -6)  # dhw: z, y, x
EXACT_TH = np.array([0.25, -0.5, 0.125], np.float32)
EXACT_PADS = ("zju", "snapshot")
UNIT = 2.0 ** -10                              # every SMPL-space coordinate is a multiple of it
BASE = np.array([-37, 211, -90])              # the minimum of each axis (xyz), in UNIT
# offsets from the minimum in HALF voxels: the ties 0.5, 1.5, 2.5, 3.5 (and two more of either parity), and whole voxels
TIE_HALVES = (0, 1, 3, 5, 7, 2, 4, 6, 8, 13, 15, 80, 21, 23)
EXTENT_HALVES = (62, 63, 64, 66, 128)          # 31, 31.5, 32, 33, 64 voxels
OUT_SH_OF_HALVES = {0: 32, 62: 32, 63: 64, 64: 64, 66: 64, 128: 96}


def rint_halves(h):
    """Round h / 2 to the nearest integer, half to even, in integer arithmetic."""
    q, r = divmod(int(h), 2)
    return q if r == 0 else q + (q & 1)


def unpadded_axes(pad):
    return [a for a in range(3) if sr.PADS[pad][a] == 0.0]


def half_voxel_units(axis):
    """Half a voxel of xyz axis `axis` in UNIT (voxel_size is dhw)."""
    u = 0.5 * EXACT_VS[2 - axis] / UNIT
    assert u == int(u) and u >= 1
    return int(u)


def _exact_frame(halves_by_axis, pad, filler):
    """SMPL-space vertices at BASE + the given half-voxel offsets on the unpadded axes and at `filler` (UNIT) on the others, moved
    by EXACT_TH -> world vertices [V,3] float32, exactly."""
    V = len(next(iter(halves_by_axis.values())))
    s = np.zeros((V, 3), np.int64)
    for a in range(3):
        s[:, a] = BASE[a] + (np.array(halves_by_axis[a]) * half_voxel_units(a) if a in halves_by_axis else np.resize(filler, V))
    world64 = s * UNIT + EXACT_TH.astype(np.float64)[None]
    world = world64.astype(np.float32)
    assert np.array_equal(world.astype(np.float64), world64) and np.array_equal((world - EXACT_TH[None]).astype(np.float64), s * UNIT)
    return world


@functools.lru_cache(maxsize=None)
def tie_case(pad):
    """One frame -> dict(verts [1,V,3], Rh, Th, pad, halves {axis: offsets in half voxels}, expect {axis: coordinate [V]})."""
    axes = unpadded_axes(pad)
    halves = {axes[0]: list(TIE_HALVES), axes[1]: list(TIE_HALVES[::-1])}
    verts = _exact_frame(halves, pad, filler=[0, 17, 5, 300, 41, 42, 7])
    expect = {a: np.array([rint_halves(h) for h in halves[a]], np.int32) for a in axes}
    return _frozen(verts=verts[None], Rh=np.zeros((1, 3), np.float32), Th=EXACT_TH[None].copy(), pad=pad, halves=halves, expect=expect)


@functools.lru_cache(maxsize=None)
def out_sh_case(pad, single=False):
    """single: one frame of ONE vertex (every unpadded extent is 0).  Otherwise five frames of three vertices: frame f spans
    EXTENT_HALVES[f] on the first unpadded axis and EXTENT_HALVES[(f + 2) % 5] on the second
    -> dict(verts [F,V,3], Rh, Th, pad, expect [F] of {axis: out_sh entry})."""
    axes = unpadded_axes(pad)
    if single:
        frames, expect = [_exact_frame({a: [0] for a in axes}, pad, filler=[9])], [{a: OUT_SH_OF_HALVES[0] for a in axes}]
    else:
        frames, expect = [], []
        for f in range(len(EXTENT_HALVES)):
            e = {axes[0]: EXTENT_HALVES[f], axes[1]: EXTENT_HALVES[(f + 2) % len(EXTENT_HALVES)]}
            frames.append(_exact_frame({a: [e[a], 0, 5] for a in axes}, pad, filler=[3, 120, 64]))
            expect.append({a: OUT_SH_OF_HALVES[e[a]] for a in axes})
    F = len(frames)
    return _frozen(verts=np.stack(frames), Rh=np.zeros((F, 3), np.float32), Th=np.repeat(EXACT_TH[None], F, 0), pad=pad, expect=expect)


# ------------------------------------------------------------------------------------------- the whole suite, for the host test
def suite():
    """Every (name, case, voxel_size) tests/test_gpu_voxelize_exact.py runs."""
    out = []
    for name, pad in sr.VOXEL_CASES:
        for tag, vs in VOXEL_SIZES.items():
            out.append(("fixture-%s-%s-%s" % (name, pad, tag), fixture_case(name, pad), vs))
    for V in EDGE_V:
        for pad in sorted(sr.PADS):
            out.append(("edge-%d-%s" % (V, pad), edge_case(V, pad), ANISO))
    for pad in EXACT_PADS:
        out.append(("tie-%s" % pad, tie_case(pad), EXACT_VS))
        out.append(("out_sh-one-%s" % pad, out_sh_case(pad, True), EXACT_VS))
        out.append(("out_sh-%s" % pad, out_sh_case(pad), EXACT_VS))
    return out


def entries_changed(a, b):
    """The number of output entries (coord, bounds' bits, out_sh, summary) on which two voxelisations differ."""
    return int(sum((np.asarray(a[k]).view(np.int32) != np.asarray(b[k]).view(np.int32)).sum() for k in ("coord", "bounds", "out_sh", "summary")))
