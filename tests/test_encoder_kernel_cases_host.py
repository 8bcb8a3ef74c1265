"""Host-side checks of what tests/test_gpu_encoder_kernels.py stands on (tests/spconv_cases.py): the generators meet the lattice
precondition for every case the GPU file runs, the capacities it uses reach every kernel nb_enc_conv16 can pick, and the float64
references agree with torch's dense conv3d and its autograd."""
import numpy as np
import pytest
import torch

from neuralbody_amd import build, ops
from tests import spconv_cases as sc


def test_active_sets_hold_what_the_kernels_can_get_wrong():
    geo = sc.geometry("small", 1)
    coord = sc.active_set()
    assert 280 <= geo.n_in <= 320 and geo.n_in % 32 != 0, "about 300 rows, a partial last tile"
    have = {tuple(c) for c in coord}
    D, H, W = sc.GRID
    assert all((z, y, x) in have for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)), "the eight corners"
    live = np.zeros((geo.n_out, 27), bool)
    for o, p in enumerate(geo.pairs):
        live[p[:, 1], o] = True
    iso = int(np.nonzero(geo.in_lin == np.ravel_multi_index(sc.ISOLATED, sc.GRID))[0][0])
    assert live[iso].tolist() == [o == 13 for o in range(27)], "the isolated voxel: only the centre offset"
    assert (live.sum(1) == 27).any(), "a voxel with all 27 neighbours (inside the dense block)"
    assert all((z, 7, 2) in have for z in range(D)), "the line"
    # per 32-row tile, which offsets are live: some tile has whole offsets dead that another tile has live
    tiles = np.stack([live[r:r + 32].any(0) for r in range(0, geo.n_out, 32)])
    assert (tiles.any(0) & ~tiles.all(0)).any(), "an offset dead for a whole tile and live in another"
    # ... and within the first 128-row workgroup of the LDS kernels: dead for one of its waves, live for another
    assert (tiles[:4].any(0) & ~tiles[:4].all(0)).any()
    big = sc.geometry("big", 1)
    assert big.n_in == 2049 and int(np.prod(sc.BIG_GRID)) == 2160
    for which in ("small", "big"):
        g2 = sc.geometry(which, 2)
        assert g2.out_dhw == tuple((s - 1) // 2 + 1 for s in g2.in_dhw) and 0 < g2.n_out <= int(np.prod(g2.out_dhw))
        fed = np.unique(np.concatenate([p[:, 0] for p in g2.pairs if len(p)]))
        assert np.array_equal(fed, np.arange(g2.n_in)), "every input row feeds an output"


def test_pad_lin_repeats_valid_voxels_only():
    geo = sc.geometry("small", 2)
    lin = sc.pad_lin(geo.out_lin, 4224)
    assert lin.shape == (4224,) and np.array_equal(lin[:geo.n_out], geo.out_lin) and set(lin.tolist()) == set(geo.out_lin.tolist())
    assert np.array_equal(sc.pad_lin(geo.out_lin, 3), geo.out_lin)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_lattice_values_split_into_a_unit_head_and_a_2_to_the_minus_12_remainder(kind):
    rs = np.random.RandomState(1)
    x = sc.lattice16(rs, (4096, 8))
    assert set(np.unique(x).tolist()) == {0.0, 1.0, -1.0, 1.0 + sc.REM, 1.0 - sc.REM, -1.0 + sc.REM, -1.0 - sc.REM}
    assert 0.2 < float((x == 0).mean()) < 0.3, "about a quarter zeros"
    h, l = sc.split(x, kind)
    assert set(np.unique(h).tolist()) == {0.0, 1.0, -1.0} and set(np.unique(l).tolist()) == {0.0, sc.REM, -sc.REM}
    assert not np.any((l != 0) & (h == 0)), "a remainder only beside a head"
    assert np.array_equal(h + l, x.astype(np.float64))
    planes = sc.split_planes(x, kind, cap=4100)
    ph, pl = sc.planes_to_float(planes, kind)
    assert np.array_equal(ph[:4096].double().numpy(), h) and np.array_equal(pl[:4096].double().numpy(), l)
    assert bool(torch.isnan(ph[4096:]).all()) and planes.dtype == torch.int16 and tuple(planes.shape) == (2, 4100, 8)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_cpu_splits_reproduce_realistic_values_to_the_pair_precision(kind):
    rs = np.random.RandomState(2)
    x = np.concatenate([sc.realistic_rows(rs, (512, 8)), sc.wide_gradients(rs, (512, 8))])
    h, l = sc.split(x, kind)
    # head + remainder is the value up to the remainder's own rounding (fp16: its subnormal spacing 2^-24 at the least)
    bound = np.maximum(np.abs(x) * (2.0 ** -21 if kind == "fp16" else 2.0 ** -16), 2.0 ** -25 if kind == "fp16" else 0.0)
    assert np.all(np.abs(h + l - x) <= bound)
    g = sc.wide_gradients(rs, (4096,))
    assert 2.0 ** -20 <= float(np.abs(g).min()) < 2.0 ** -19 and 2.0 ** 3 < float(np.abs(g).max()) <= 2.0 ** 4


def _exact_in_fp32_in_any_order(terms, rs):
    """a shuffled fp32 accumulation of `terms` equals their float64 sum"""
    t = terms[rs.permutation(len(terms))].astype(np.float32)
    acc = np.float32(0)
    for v in t:
        acc = np.float32(acc + v)
    return float(acc) == float(np.sum(terms.astype(np.float64)))


def test_lattice_precondition_holds_for_every_case_the_gpu_file_runs():
    rs = np.random.RandomState(3)
    # forward and backward-input products: the largest sum is 27 offsets x 128 channels of the densest voxel
    for stride in (1, 2):
        geo = sc.geometry("small", stride)
        for cin, cout in sc.ALL_PAIRS:
            a16, w16 = sc.lattice16(rs, (geo.n_in, cin)), sc.lattice16(rs, (3, 3, 3, cin, cout))
            sc.assert_lattice(sc.conv_ref(geo, np.abs(a16), np.abs(w16)), sc.REM)
            sc.assert_lattice(sc.bwd_input_ref(geo, np.abs(sc.lattice16(rs, (geo.n_out, cout))), np.abs(w16)), sc.REM)
            a32, w32 = sc.lattice32(rs, (geo.n_in, cin)), sc.lattice32(rs, (3, 3, 3, cin, cout))
            sc.assert_lattice(sc.conv_ref(geo, np.abs(a32), np.abs(w32)), 1.0)
            sc.assert_lattice(sc.bwd_input_ref(geo, np.abs(sc.lattice32(rs, (geo.n_out, cout))), np.abs(w32)), 1.0)
        big = sc.geometry("big", stride)
        a16, d16 = sc.lattice16(rs, (big.n_in, 32)), sc.lattice16(rs, (big.n_out, 32))
        sc.assert_lattice(sc.bwd_weight_ref(big, np.abs(a16), np.abs(d16)), sc.REM)
        sc.assert_lattice(sc.bwd_weight_ref(big, np.abs(sc.lattice32(rs, (big.n_in, 16))), np.abs(sc.lattice32(rs, (big.n_out, 16)))), 1.0)
    assert 3456 * (1 + 2 * sc.REM) < 2 ** 12 and 3456 * 9 < 2 ** 24 and 2049 * (1 + sc.REM) ** 2 < 2 ** 12
    # ... and what the precondition promises, on the terms of the largest sum: any order of fp32 additions is exact
    a, w = sc.lattice16(rs, (3456,)), sc.lattice16(rs, (3456,))
    (ah, al), (wh, wl) = sc.split(a, "fp16"), sc.split(w, "fp16")
    assert _exact_in_fp32_in_any_order(np.concatenate([ah * wh, ah * wl, al * wh]), rs)
    assert _exact_in_fp32_in_any_order((sc.lattice32(rs, (3456,)) * sc.lattice32(rs, (3456,))).astype(np.float64), rs)


def test_the_three_capacities_reach_every_kernel_the_dispatch_can_pick():
    """nb_enc_conv16_variant over capacities 1 .. 2^18 (steps of 128 and both sides of every change): the kernels a pair can run are
    exactly those tests/spconv_cases.py names for the three capacity classes — a moved threshold fails here instead of silently
    leaving a kernel untested."""
    build.build(verbose=False)
    assert ops.enc_conv16_variant(16, 32, 100) is None and ops.enc_conv16_variant(32, 16, 100) is None
    assert ops.enc_conv16_variant(48, 32, 100) is None
    live = max(sc.geometry("small", s).n_out for s in (1, 2))
    assert live <= 4096
    assert set(sc.VARIANTS) == set(sc.PAIRS16 + sc.REVERSED16)
    seen_all = set()
    for (cin, cout), named in sc.VARIANTS.items():
        caps = list(range(1, 2 ** 18 + 1, 128)) + [2 ** 18]
        kinds = [ops.enc_conv16_variant(cin, cout, c) for c in caps]
        seen = set(kinds)
        for c0, c1, k0, k1 in zip(caps, caps[1:], kinds, kinds[1:]):
            if k0 != k1:  # walk the step: every capacity between the two
                seen |= {ops.enc_conv16_variant(cin, cout, c) for c in range(c0, c1 + 1)}
        assert None not in seen
        used = [ops.enc_conv16_variant(cin, cout, sc.capacity(cls, live)) for cls in sc.CAPACITIES]
        assert tuple(used) == named, (cin, cout, used)
        assert seen == set(named), "%d -> %d can run %s, the tests reach %s" % (cin, cout, sorted(seen), sorted(set(named)))
        seen_all |= seen
    assert seen_all == set(ops.CONV16_VARIANTS)
    forward = {(ci, co) for ci, co, _ in sc.FORWARD16}
    backward = {(co, ci) for ci, co, _ in sc.BWD_INPUT16}
    assert forward == set(sc.PAIRS16) and forward | backward == set(sc.VARIANTS)


@pytest.mark.parametrize("stride", [1, 2])
def test_references_agree_with_dense_conv3d_and_its_autograd(stride):
    geo = sc.geometry("small", stride)
    cin, cout = 16, 32
    rs = np.random.RandomState(4 + stride)
    a = rs.standard_normal((geo.n_in, cin))
    w = rs.standard_normal((3, 3, 3, cin, cout))
    dx = rs.standard_normal((geo.n_out, cout))
    n = 129 if stride == 1 else 33
    assert n < geo.n_out
    D, H, W = geo.in_dhw
    a_t = torch.from_numpy(a).requires_grad_(True)
    w_t = torch.from_numpy(w).requires_grad_(True)
    dense = torch.zeros(D * H * W, cin, dtype=torch.float64).index_put((torch.from_numpy(geo.in_lin.astype(np.int64)),), a_t)
    y = torch.nn.functional.conv3d(dense.reshape(1, D, H, W, cin).permute(0, 4, 1, 2, 3), w_t.permute(4, 3, 0, 1, 2), stride=stride, padding=1)
    assert tuple(y.shape[2:]) == geo.out_dhw
    y_flat = y[0].reshape(cout, -1).t()
    rows = y_flat[torch.from_numpy(geo.out_lin.astype(np.int64))]
    if stride == 2:  # (a submanifold layer keeps the input's set; the strided layer's set is where a dense result can be non-zero)
        off = np.ones(int(np.prod(geo.out_dhw)), bool)
        off[geo.out_lin] = False
        assert float(y_flat.detach()[torch.from_numpy(off)].abs().sum()) == 0.0
    scale = float(rows.detach().abs().max())
    np.testing.assert_allclose(sc.conv_ref(geo, a, w), rows.detach().numpy(), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(sc.conv_ref(geo, a, w, n), rows[:n].detach().numpy(), rtol=0, atol=1e-12 * scale)
    # all output rows: d in and dW; a prefix of the output rows: dW
    gi, gw = torch.autograd.grad((rows * torch.from_numpy(dx)).sum(), (a_t, w_t), retain_graph=True)
    np.testing.assert_allclose(sc.bwd_input_ref(geo, dx, w), gi.numpy(), rtol=0, atol=1e-12 * float(gi.abs().max()))
    np.testing.assert_allclose(sc.bwd_input_ref(geo, dx, w, n), gi[:n].numpy(), rtol=0, atol=1e-12 * float(gi.abs().max()))
    np.testing.assert_allclose(sc.bwd_weight_ref(geo, a, dx), gw.numpy(), rtol=0, atol=1e-12 * float(gw.abs().max()))
    gw_n, = torch.autograd.grad((rows[:n] * torch.from_numpy(dx[:n])).sum(), (w_t,))
    np.testing.assert_allclose(sc.bwd_weight_ref(geo, a, dx, n), gw_n.numpy(), rtol=0, atol=1e-12 * float(gw_n.abs().max()))
    # the three-product form is linear in each operand: on whole values split exactly it is the product minus remainder x remainder
    (ah, al), (wh, wl) = sc.split(sc.lattice16(rs, (geo.n_in, cin)), "fp16"), sc.split(sc.lattice16(rs, (3, 3, 3, cin, cout)), "bf16")
    three = sc.three_products(lambda p, q: sc.conv_ref(geo, p, q), (ah, al), (wh, wl))
    assert np.array_equal(three, sc.conv_ref(geo, ah + al, wh + wl) - sc.conv_ref(geo, al, wl))
