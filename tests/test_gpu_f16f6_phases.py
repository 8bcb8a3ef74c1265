"""The f16f6 layer phases of nb_march_fold_kernel against the operand-exact float64 model of tests/f16f6_model.py, through the product
ABI alone (ops.mlp_pack, mlp_latent_bias, fold_build, make_scene, decode_points, march): known activations are driven into one phase
at a time and its accumulators read back through one-hot heads (tests/f16f6_phase_cases.py says how).

EXACT cases are compared bit for bit: every quantisation in them is lossless (or a bf6 tie, which must go to the even code) and every
sum stays on one grid below 2^24 units, so a dropped or doubled cross term, a wrong scale byte, t - 10 for t - 11, a fragment of the
other N tile or of another sample all change the answer, and no summation order does.  BOUNDED cases (realistic magnitudes) hold the
phases whose accumulators a VALU head reads in fp32 to a multiple of 2^-24 sum |terms| measured on the device."""
import time

import numpy as np
import pytest
import torch

from tests import f16f6_phase_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("points", "density", "march", "cull")  # the four instantiations of the kernel: <1, false>, <2, false>, <0, false>, <0, true>


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Rig(object):
    """A case on the device: the folded planes and the scene (built once), the parameters, and read-outs through one-hot heads."""

    def __init__(self, case):
        from neuralbody_amd import ops

        self.ops, self.case = ops, case
        self.vols = [_dev(v) for v in case.volumes]
        self.sparse = [ops.sparsify(v) for v in self.vols]
        self.params = dict((k, _dev(v)) for k, v in case.params.items())
        self.fold = ops.fold_build(self.vols, self.sparse, self.params["fc0_w"])
        self.pose = ops.make_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), device=DEV)
        self.scene = ops.make_scene(self.vols, self.pose, (case.voxel_size,) * 3, C.OUT_SH, fold=self.fold)
        self.lb = ops.mlp_latent_bias(self.params, torch.zeros(128, device=DEV))
        self.pts, self.vd = _dev(case.pts), _dev(case.viewdir)
        n = case.pts.shape[0]
        self.zeros_n = torch.zeros(n, device=DEV)
        self.t_vals = torch.zeros(1, device=DEV)
        # the all-inside cull: one 8 x 8 mask of ones seen by a camera in front of the volume (pixel = (x, y) / (z + 1) + 4)
        RT = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1]]], device=DEV)
        Km = torch.tensor([[[1.0, 0, 4], [0, 1, 4], [0, 0, 1]]], device=DEV)
        self.cull = ops.make_cull(torch.ones((1, 8, 8), dtype=torch.uint8, device=DEV), RT, Km)

    def raw(self, mode):
        """[N, 4] (density: [N, 1]) of the current parameters through one instantiation of the kernel."""
        ops = self.ops
        packed = ops.mlp_pack(self.params, precisions=("f16f6",))
        if mode == "points":
            return ops.decode_points(self.scene, packed, self.lb, self.pts, self.vd, precision="f16f6")
        if mode == "density":
            return ops.decode_points(self.scene, packed, None, self.pts, None, density_only=True, precision="f16f6")
        # one-sample rays whose sample point is the lattice point: origin = the point, near = far = 0
        out = ops.march(self.scene, packed, self.lb, self.pts, self.vd, self.zeros_n, self.zeros_n, self.t_vals, want_raw=True,
                        precision="f16f6", fixup=False, cull=self.cull if mode == "cull" else None)
        return out["raw"][:, 0]

    def read(self, mode, rows=None):
        """got [len(rows), N] float64: the accumulators of the case's phase behind their ReLU, one read-out per row (colour head: per
        three rows)."""
        case = self.case
        rows = list(case.rows if rows is None else rows)
        got = np.full((len(rows), case.pts.shape[0]), np.nan)
        head = "alpha_w" if case.phase < 2 else "rgb_w"
        for start, pairs in C.readout_rows(case.phase, rows):
            self.params[head] = _dev(C.observe(case.params, case.phase, start)[head])
            out = self.raw(mode).double().cpu().numpy()
            for col, r in pairs:
                got[rows.index(r)] = out[:, 0 if mode == "density" else col]
        assert not np.isnan(got).any()
        return got


_RIGS = {}


def _rig(key):
    if key not in _RIGS:
        _RIGS[key] = Rig(C.get(key))
    return _RIGS[key]


_MODELS = {}


def _model(key):
    """The model's read-outs of a case, computed once and shared (never written to)."""
    if key not in _MODELS:
        case = C.get(key)
        m = case.model()
        exp = case.expected(m)
        exp.setflags(write=False)
        _MODELS[key] = (m, exp)
    return _MODELS[key]


def _assert_exact(key, mode, rows=None):
    case = C.get(key)
    rows = list(case.rows if rows is None else rows)
    t0 = time.time()
    got = _rig(key).read(mode, rows)
    torch.cuda.synchronize()
    want = _model(key)[1][rows]
    bad = got != want
    print("%s %s: %d x %d read-outs in %.2f s, %d differ, largest |difference| %.3e of %.3e" % (
        case.name, mode, got.shape[0], got.shape[1], time.time() - t0, int(bad.sum()), float(np.abs(got - want).max()), float(np.abs(want).max())))
    assert (want != 0).mean() > 0.3
    if bad.any():
        r, n = np.argwhere(bad)[0]
        raise AssertionError("%s through %s: %d of %d read-outs differ from the model; first: row %d sample %d got %r, model %r" % (
            case.name, mode, int(bad.sum()), bad.size, rows[r], n, got[r, n], want[r, n]))


@pytest.mark.parametrize("key", C.EXACT_KEYS, ids=lambda k: "%s-%s" % (("fc1", "fc2", "colour", "pe")[k[1]], k[2]))
def test_exact_phase_through_decode_points(key):
    """Every EXACT case through nb_decode_points, bit for bit.  The 'full' cases read every output row — every (wave, tile, half,
    accumulator register) of the phase; the variants (one cross term at a time, cancelling main products, edge blocks, bf6 ties) a
    row of every wave, tile and half."""
    _assert_exact(key, "points")


def test_fc2_every_row_through_density_only():
    """Density-only mode reads all 256 rows of fc_2's accumulators straight from registers, in fp32, without a publish."""
    _assert_exact(("exact", 1, "full"), "density")


@pytest.mark.parametrize("variant", [v for v in C.EXACT_VARIANTS if v != "full"])
@pytest.mark.parametrize("phase", [0, 1])
def test_exact_variants_through_density_only(phase, variant):
    _assert_exact(("exact", phase, variant), "density")


# density-only stops behind alpha_fc: it has no colour head
@pytest.mark.parametrize("phase,mode", [(ph, mo) for ph in (0, 1, 2) for mo in MODES if not (ph == 2 and mo == "density")])
def test_core_through_every_instantiation(phase, mode):
    """The same small core (the 'full' recipe on 64 samples, 16 rows; the colour head: 12) through the four instantiations of the
    kernel: points, density only (fc_1 and fc_2), the march on one-sample rays whose sample points are the lattice points (raw
    output), and the culled march with an all-inside cull."""
    _assert_exact(("core", phase), mode)


@pytest.mark.parametrize("mode", ["points", "density", "march"])
@pytest.mark.parametrize("kind", ["u_rem", "wt_rem"])
def test_folded_first_layer(kind, mode):
    """U_h . Wt_h + U_h . Wt_l + U_l . Wt_h: points offset along one axis (the two trilinear weights exact products), U with a
    remainder under dyadic weights, and a weight with a remainder (1/2 + 2^-13) under head-only U; read through identity layers."""
    _assert_exact(("fold", kind), mode)


@pytest.mark.parametrize("key", C.BOUNDED_KEYS, ids=lambda k: ("fc1", "fc2", "colour", "pe")[k[1]])
def test_bounded_phase(key):
    """Realistic magnitudes: |got - model| <= BOUNDED_FACTOR 2^-24 sum |terms| for fc_2 and both colour-head phases (the figure and
    how it was set: tests/f16f6_phase_cases.py)."""
    case = C.get(key)
    m = _model(key)[0]
    rows = list(case.rows)
    y, ab = case.tested(m)
    t0 = time.time()
    got = _rig(key).read("density" if case.phase == 1 else "points")
    torch.cuda.synchronize()
    ratio = np.abs(got - np.maximum(y[rows], 0.0)) / (2.0 ** -24 * ab[rows])
    print("%s: %d x %d read-outs in %.2f s: largest |got - model| = %.3f x 2^-24 sum |terms| (median %.3f), |y| up to %.3f" % (
        case.name, got.shape[0], got.shape[1], time.time() - t0, float(ratio.max()), float(np.median(ratio)), float(np.abs(y[rows]).max())))
    assert float(ratio.max()) <= C.BOUNDED_FACTOR, float(ratio.max())
