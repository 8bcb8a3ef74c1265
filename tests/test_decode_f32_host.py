"""The preconditions and the sensitivity of tests/test_gpu_decode_f32.py, on the CPU: every lattice precondition, the path every
(case, wave, level) takes by the predicate of tests/decode_f32_cases.py, the ReLU shares, and for each part a list of mistakes applied
to the float64 reference, each of which must change a compared element (the exact cases) or push a ratio above 1 (the bounded ones)."""
import itertools

import numpy as np
import pytest
import torch

from tests import bwd_cases as bc
from tests import decode_f32_cases as dc
from tests import fold_stream_ref as FS
from tests import march_ray_cases as R
from tests import spconv_cases as sc

F32 = np.float32
CASES = dc.a_cases()
TILE_CASES = ("cell", "fit-L0", "fit-L1", "fit-L2", "fit-L3", "divisors", "mixed", "workgroups", "edges-clustered")


def _ref(case, pose="identity", mutate=None):
    _, g = dc.case_grid(case.q, pose)
    paths, boxes = dc.wave_paths(g)
    return dc.gather_f64(g.astype(np.float64), dc.distinct_volumes(), mutate=mutate, boxes=boxes, paths=paths)


# ------------------------------------------------------------------------------------------------------------------------- A
def test_volumes_hold_distinct_integers():
    for v, shape, c in zip(dc.distinct_volumes(), dc.SHAPES, dc.LEVEL_C):
        assert v.shape == tuple(shape) + (c,) and v.dtype == F32
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 255
        assert not dc._violations(v).any(), "two corners of a cell or two neighbouring channels agree"
        assert len(np.unique(v)) > 500
    assert 255 * bc.tri_weight_denominator(3) < 2 ** 23


def test_reference_is_grid_sample():
    """gather_f64 against float64 F.grid_sample (align_corners=True, zeros padding) on a random scene with points outside"""
    g, _, grids = bc.random_tri_scene()
    rs = np.random.RandomState(1)
    vols = [rs.standard_normal(tuple(gr.shape) + (c,)) for gr, c in zip(grids, dc.LEVEL_C)]
    F, S, _ = dc.gather_f64(g, vols)
    gt = torch.from_numpy(g)[None, None, None]
    for l, v in enumerate(vols):
        want = torch.nn.functional.grid_sample(torch.from_numpy(v).permute(3, 0, 1, 2)[None], gt, padding_mode="zeros",
                                               align_corners=True)[0, :, 0, 0].t().numpy()
        got = F[:, dc.CHAN_BASE[l]:dc.CHAN_BASE[l] + dc.LEVEL_C[l]]
        assert np.abs(got - want).max() < 1e-12
    assert np.all(S >= np.abs(F) - 1e-12)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_coordinates_are_exact_under_both_poses(case):
    """the world points are fp32 numbers; grid_coords in fp32 gives the same bits under either pose, the bits of bwd_cases.fp32_grid
    under the identity, and the float64 coordinates themselves wherever the point is within reach"""
    w0, g0 = dc.case_grid(case.q, "identity")
    w1, g1 = dc.case_grid(case.q, "permuted")
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32)) and not np.array_equal(w0, w1)
    assert np.array_equal(g0, bc.fp32_grid(w0, (0.0, 0.0, 0.0), dc.VOXEL, dc.OUT_SH))
    near = np.abs(case.q).max(1) < 1e6
    for w, name in ((w0, "identity"), (w1, "permuted")):
        p = dc.POSES[name]
        g64 = dc.grid_coords64(w, p["R"], p["Th"], p["bmin"])
        assert np.array_equal(g64[near], g0[near].astype(np.float64))
    assert len(case.q) % 32 == 0 or case.name == "tri-scene"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_wave_and_level_takes_the_stated_path(case):
    _, g = dc.case_grid(case.q, "identity")
    paths, boxes = dc.wave_paths(g)
    assert tuple(paths) == case.paths
    for (wave, level), dims in case.dims.items():
        assert tuple(boxes[wave, level, 1] - boxes[wave, level, 0] + 1) == tuple(dims), (wave, level)


def test_fit_boxes_sit_on_the_threshold():
    for l, (fit, over, _) in enumerate(dc.FIT_BOXES):
        cap = dc.MAX_TILE_VOXELS[l]
        assert int(np.prod(fit)) <= cap < int(np.prod(over))
        assert int(np.prod(over)) - int(np.prod(fit)) == int(np.prod(over)) // max(o for o, f in zip(over, fit) if o != f), "one plane more"
        D, H, W = dc.SHAPES[l]
        if l < 3:
            assert int(np.prod(fit)) == cap and int(np.prod(fit)) * dc.LEVEL_C[l] // 4 == dc.TILE_PIECES
        else:  # no box of the 5 x 3 x 3 volume has 32 voxels: 30 is the largest that fits
            sizes = [a * b * c for a in range(1, W + 1) for b in range(1, H + 1) for c in range(1, D + 1)]
            assert max(s for s in sizes if s <= cap) == int(np.prod(fit)) and cap not in sizes
    assert dc.MAX_TILE_VOXELS == (128, 64, 32, 32)
    divs = set()
    for (nx, ny, nz), _ in dc.DIVISOR_BOXES:
        divs |= {nx, nx * ny}
    assert {3, 5, 6, 7} <= divs


def test_tile_fill_quotients_survive_a_reciprocal_one_ulp_off():
    """v / (nx ny) and r / nx as the tile fill forms them, (int)((v + 0.5) rcp), with the reciprocal one ulp either side: right for
    every divisor up to 128 and every voxel number a tile can hold"""
    v = np.arange(0, 1024, dtype=np.int64)
    for d in range(1, 129):
        exact = F32(1.0) / F32(d)
        for rcp in (np.nextafter(exact, F32(0)), exact, np.nextafter(exact, F32(2))):
            got = ((v.astype(F32) + F32(0.5)) * rcp).astype(np.int64)
            assert np.array_equal(got, v // d), d


def test_row_counts_padding_lanes_do_not_widen_the_box():
    q = dc.rows_case()
    _, g = dc.case_grid(q, "identity")
    counts = sc.row_counts(len(q), dc.ROW_COUNTS)
    assert counts == [1, 31, 32, 33, 127, 128, 129, 192]
    for n in counts:
        paths, _ = dc.wave_paths(g, n)
        assert paths[-1] == dc.ROWS_LAST_WAVE[n], n
        assert len(paths) == (n + 31) // 32
    assert dc.wave_paths(g)[0][0] == "PPPP" and dc.wave_paths(g, 1)[0][0] == "TTTT"


def test_odd_points_leave_the_box_in_range():
    """the NaN point drops out of the box; the +inf one stretches it to the last plane in x and makes the lane's y and z NaN"""
    odd, plain, (i_nan, i_inf) = dc.odd_case()
    w, g = dc.case_grid(odd, "identity")
    assert np.isnan(g[i_nan]).all() and np.isposinf(g[i_inf, 0]) and np.isnan(g[i_inf, 1:]).all()
    paths, boxes = dc.wave_paths(g)
    assert paths == ["TTTT", "TTTT"]
    assert tuple(boxes[0, 0, 1] - boxes[0, 0, 0] + 1) == (25, 2, 2) and boxes[0, 0, 1, 0] == dc.SHAPES[0][2] - 1
    assert dc.wave_paths(dc.case_grid(plain, "identity")[1])[0] == ["TTTT", "TTTT"]
    F, _, _ = dc.gather_f64(g.astype(np.float64), dc.distinct_volumes())
    assert not F[[i_nan, i_inf]].any()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gather_lattice_precondition_and_something_to_poison(case):
    F, S, touched = _ref(case)
    dc.assert_gather_lattice(S)
    assert np.array_equal(F.astype(F32).astype(np.float64), F)
    assert all(0 < t.sum() for t in touched) and not touched[0].all()
    pois = dc.poisoned(dc.distinct_volumes(), touched)
    _, g = dc.case_grid(case.q, "identity")
    F2, _, _ = dc.gather_f64(g.astype(np.float64), pois)
    assert np.array_equal(F, F2)


A_MUTANT_CASES = {"drop_corner": [c.name for c in CASES], "clamp_last_plane": ["edges-clustered", "edges-scattered", "tri-scene"],
                  "box_short": TILE_CASES, "tile_shift": TILE_CASES, "swap_levels_23": [c.name for c in CASES],
                  "swap_halves": [c.name for c in CASES]}


@pytest.mark.parametrize("mutate", dc.A_MUTANTS)
def test_gather_mutants_show_on_the_lattice(mutate):
    for name in A_MUTANT_CASES[mutate]:
        case = dc.a_case(name)
        assert not np.array_equal(_ref(case)[0], _ref(case, mutate=mutate)[0]), name


def test_gather_mutants_leave_the_realistic_bound():
    s = dc.realistic_scene()
    paths, _ = dc.wave_paths(s["g"], shapes=s["shapes"])
    for l in range(4):
        kinds = {p[l] for p in paths}
        assert kinds == {"T", "P"}, "level %d: both paths" % l
    F, S, _ = dc.gather_f64(s["g"], s["vols"], index_dtype=F32)
    assert (S.sum(1) > 0).mean() > 0.9
    for m in ("drop_corner", "swap_levels_23", "swap_halves"):
        Fm, _, _ = dc.gather_f64(s["g"], s["vols"], index_dtype=F32, mutate=m)
        assert max(dc.gather_ratios(Fm, F, S)) > 1, m
    # ... and so does an index coordinate that is not rounded as the kernel rounds it
    p = s["pose"]
    F64, _, _ = dc.gather_f64(dc.grid_coords64(s["pts"], p["R"], p["Th"], p["bmin"], s["voxel"], s["out_sh"]), s["vols"])
    assert max(dc.gather_ratios(F64, F, S)) > 1


def test_pose_mutants_show():
    """R transposed, every other signed permutation, and bounds_min read in another order each move at least one point's features"""
    case = dc.a_case("scattered")
    pose = dc.POSES["permuted"]
    w, g = dc.case_grid(case.q, "permuted")
    vols = dc.distinct_volumes()
    ref, _, _ = dc.gather_f64(dc.grid_coords64(w, pose["R"], pose["Th"], pose["bmin"]), vols)
    assert np.array_equal(ref, _ref(case)[0])
    others = [m for m in dc.signed_permutations() if not np.array_equal(m, pose["R"])]
    assert len(others) == 47 and any(np.array_equal(m, pose["R"].T) for m in others)
    for m in others:
        got, _, _ = dc.gather_f64(dc.grid_coords64(w, m, pose["Th"], pose["bmin"]), vols)
        assert not np.array_equal(got, ref), m
    for order in itertools.permutations(range(3)):
        if order != (0, 1, 2):
            got, _, _ = dc.gather_f64(dc.grid_coords64(w, pose["R"], pose["Th"], pose["bmin"], bmin_order=order), vols)
            assert not np.array_equal(got, ref), order
    assert len(set(pose["bmin"].tolist())) == 3 and np.all(np.log2(np.abs(pose["Th"])) % 1 == 0)


# ------------------------------------------------------------------------------------------------------------------------- B
def _exact_chain(mutate=None):
    p, code = dc.exact_params()
    q, v, vols = dc.exact_points()
    w, g = dc.case_grid(q, dc.B_POSE)
    F, _, _ = dc.gather_f64(g.astype(np.float64), vols)
    return p, F, dc.layer_chain(p, code, F, dc.raw_encodings(w, v), mutate=mutate)


def test_exact_weights_cover_every_column_and_every_tile_has_distinct_biases():
    p, code = dc.exact_params()
    for name in ("fc0", "fc1", "fc2", "alpha", "rgb"):
        assert (p[name + "_w"] != 0).any(0).all(), name
    assert (p["latent_w"] != 0).any(0).all()
    assert (p["view_w"][:, :256] != 0).any(0).all() and (p["view_w"][:, list(dc.RAW_COLS)] != 0).any(0).all()
    sines = [c for c in range(256, 346) if c not in dc.RAW_COLS]
    assert len(sines) == 84 and not p["view_w"][:, sines].any()
    for name in ("fc0_b", "fc1_b", "fc2_b", "latent_b", "view_b"):
        b = p[name]
        for t in range(len(b) // 32):
            assert len(set(b[32 * t:32 * t + 32].tolist())) == 32, (name, t)
    for w in p.values():
        assert np.array_equal(w, np.round(w))
    m = dc.merged64(p)
    assert np.array_equal(m, np.round(m)) and (m != 0).any(0).all()
    assert np.abs(p["feature_w"]).sum(0).tolist() == [1.0] * 256 and np.abs(p["feature_w"]).sum(1).tolist() == [1.0] * 256
    assert np.array_equal(dc.latent_bias64(p, code), np.round(dc.latent_bias64(p, code))) and code.any()


def test_exact_chain_is_a_lattice_with_live_relus():
    p, F, chain = _exact_chain()
    assert np.array_equal(F, np.round(F)) and np.abs(F).max() <= 7 and (np.abs(F).sum(1) > 0).all()
    for stage in dc.STAGES:
        val, S = chain[stage]
        sc.assert_lattice(S / dc.EXACT_UNIT[stage], 1.0)
        assert np.array_equal(val / dc.EXACT_UNIT[stage], np.round(val / dc.EXACT_UNIT[stage]))
        assert np.array_equal(val.astype(F32).astype(np.float64), val)
        if stage in ("h1", "h2", "h3", "V"):
            zeros = float((val == 0).mean())
            assert 0.2 <= zeros <= 0.8, (stage, zeros)
    q, v, _ = dc.exact_points()
    assert len(q) == dc.B_N and len(np.unique(q, axis=0)) == 45 and np.abs(v).max() == 2.0


B_FIRST_STAGE = {"tile_bias": "h2", "swap_kchunks": "h2", "pf_tail": "h3", "drop_encoding_column": "V", "swap_rgb": "rgb", "no_relu_V": "V"}


@pytest.mark.parametrize("mutate", dc.B_MUTANTS)
def test_layer_mutants_show_in_the_exact_chain(mutate):
    _, _, ref = _exact_chain()
    _, _, mut = _exact_chain(mutate)
    first = B_FIRST_STAGE[mutate]
    for stage in dc.STAGES[:dc.STAGES.index(first)]:
        if not (stage == "sigma" and first in ("V", "rgb", "G")):
            assert np.array_equal(ref[stage][0], mut[stage][0]), stage
    assert not np.array_equal(ref[first][0], mut[first][0])


def test_fragment_columns_partition_every_layer():
    for kind, groups, width in (("feat", dc.G0, 352), ("hidden", dc.GH, 256)):
        cols = sorted(c for g in range(groups) for c in dc.fragment_cols(kind, g))
        assert cols == list(range(width)), kind
    cols = [c for g in range(dc.GV) for c in dc.fragment_cols("view", g)]
    assert sorted(c for c in cols if c >= 0) == list(range(346)) and cols.count(-1) == 8 * dc.GV - 346
    assert [FS.col_hidden(q, 0) for q in range(4)] == [0, 1, 2, 3] and FS.col_hidden(0, 1) == 4


def _realistic_chain():
    s = dc.realistic_scene()
    n = 256
    p, code = dc.realistic_params()
    rs = np.random.RandomState(3)
    v = rs.standard_normal((n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    F, _, _ = dc.gather_f64(s["g"][:n], s["vols"], index_dtype=F32)
    pe = dc.encodings_f64(s["pts"][:n], v)
    ref = dc.layer_chain(p, code, F, pe)
    inputs = {"h1": F, "h2": ref["h1"][0], "h3": ref["h2"][0], "sigma": ref["h3"][0], "G": ref["h3"][0], "V": ref["G"][0],
              "rgb": ref["V"][0]}
    return p, code, F, pe, ref, inputs


def test_layer_mutants_leave_the_realistic_bound():
    p, code, F, pe, ref, inputs = _realistic_chain()
    for stage in ("h1", "h2", "h3", "V"):
        zeros = float((ref[stage][0] == 0).mean())
        assert 0.2 <= zeros <= 0.8, (stage, zeros)
    V = dc.layer_chain(dc.rgb_tie(p, 0)[0], code, F, pe)["V"][0]
    assert (V > 0).any(0).all() and len(np.unique(V.astype(F32), axis=1).T) == 128, "the rgb tie reads 128 live, different columns"
    for m in dc.B_MUTANTS:
        mut = dc.layer_chain(p, code, F, pe, mutate=m, inputs=inputs)
        stage = B_FIRST_STAGE[m]
        ratio = float((np.abs(mut[stage][0] - ref[stage][0]) / dc.layer_bound(stage, ref[stage][1])).max())
        assert ratio > 1, (m, ratio)


def test_tie_weights():
    for sign in (1.0, -1.0):
        p = dc.pe_tie_params(sign)
        assert np.count_nonzero(p["view_w"]) == 90 and all(p["view_w"][r, 256 + r] == sign for r in range(90))
        assert not any(v.any() for k, v in p.items() if k != "view_w")
    seen = set()
    base, _ = dc.exact_params()
    for t in range(43):
        p, cols, signs = dc.rgb_tie(base, t)
        assert np.count_nonzero(p["rgb_w"]) == 3 and not p["rgb_b"].any()
        seen |= set(cols.tolist())
    assert seen == set(range(128))


# ------------------------------------------------------------------------------------------------------------------------- C
def test_encoding_arguments_and_mutants():
    pts, dirs = dc.pe_points()
    assert pts.dtype == F32 and pts.shape == dirs.shape and len(pts) <= 512
    assert np.abs(pts).max() == 64.0 and (pts == 64.0).any() and (pts == -64.0).any()
    assert (np.signbit(pts) & (pts == 0)).any() and ((pts == 0) & ~np.signbit(pts)).any()
    for k in range(1, 13):
        assert (pts == F32(2.0 ** -k)).any() and (pts == F32(-2.0 ** -k)).any()
    assert ((dirs == 1.0).any() and (dirs == -1.0).any() and (dirs == 0.0).any())
    norms = np.linalg.norm(dirs.astype(np.float64), axis=1)
    assert (np.abs(norms - 1.0) > 0.5).mean() > 0.5, "unnormalised directions"
    half, quarter = dc.seam_hits(pts, 10)
    assert half >= 20 and quarter >= 20, (half, quarter)
    half, quarter = dc.seam_hits(dirs, 4)
    assert half >= 10 and quarter >= 10, (half, quarter)
    assert float(np.abs(pts).max()) * 2.0 ** 9 == 2.0 ** 15
    ref = dc.encodings_f64(pts, dirs)
    assert ref.shape == (len(pts), 90) and len(np.unique(ref.astype(F32), axis=1).T) == 90, "no two encoding columns agree"
    assert np.array_equal(ref[:, 0:3], dirs.astype(np.float64)) and np.array_equal(ref[:, 27:30], pts.astype(np.float64))
    for m in ("cos_for_sin", "next_frequency"):
        assert np.abs(dc.encodings_f64(pts, dirs, m) - ref).max() > dc.PE_TOL, m
    # the column order is col_pe's: slot c of half hi
    for c in range(dc.N_PE):
        for hi in (0, 1):
            col = dc.col_pe(c, hi) - 256
            a = c % 3
            if c < 12:
                want = (np.cos if hi else np.sin)(dirs[:, a].astype(np.float64) * 2.0 ** (c // 3))
            elif c < 42:
                want = (np.cos if hi else np.sin)(pts[:, a].astype(np.float64) * 2.0 ** ((c - 12) // 3))
            else:
                want = (pts if hi else dirs)[:, a].astype(np.float64)
            assert np.array_equal(ref[:, col], want), (c, hi)


# ------------------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("S", dc.COMPOSITE_S)
def test_composite_scan_restated_stays_within_half_the_bound(S):
    for n in dc.COMPOSITE_N:
        raw, z, d, kinds = dc.composite_inputs(S, n)
        assert raw.shape == (n, S, 4) and z.shape == (n, S) and d.shape == (n, 3)
        for white in (False, True):
            ref = R.composite_f64(raw, z, d, white)
            twin = dc.composite_f64_mutant(raw, z, d, white)
            assert all(np.array_equal(ref[k], twin[k]) for k in ref), "the twin is composite_f64"
            got = dc.composite_scan_f32(raw, z, d, white)
            ratios = R.integrator_ratios(got, raw, z, d, white)
            assert max(ratios.values()) <= 0.5, (n, white, ratios)
            assert np.all(got["weights"] >= 0) and np.isfinite(got["weights"]).all()


def test_composite_rays_cover_every_kind_at_every_n():
    for n in dc.COMPOSITE_N:
        seen = set()
        for S in dc.COMPOSITE_S:
            seen |= set(dc.composite_inputs(S, n)[3])
        assert seen == set(dc.RAY_KINDS), n
    raw, z, d, kinds = dc.composite_inputs(64, 9)
    assert list(kinds) == list(dc.RAY_KINDS)
    ref = R.composite_f64(raw, z, d)
    k = dict((name, i) for i, name in enumerate(kinds))
    assert ref["acc"][k["no_density"]] == 0 and ref["acc"][k["sigma_zero"]] == 0 and ref["acc"][k["zero_direction"]] == 0
    assert ref["weights"][k["saturated_from_first"], 0] == 1.0 and ref["weights"][k["saturated_from_first"], 5] < 1e-40
    assert ref["weights"][k["saturates_at_third"], 64 // 3 + 1:].max() < 1e-9
    assert z[k["equal_depths"], 32] == z[k["equal_depths"], 31] and np.abs(raw[k["logits_30"], :, :3]).min() == 30.0


@pytest.mark.parametrize("S", dc.COMPOSITE_S)
def test_composite_mutants_leave_the_bound(S):
    raw, z, d, kinds = dc.composite_inputs(S, 9)
    for mutate in dc.D_MUTANTS:
        if mutate == "no_carry" and S <= 64:
            continue
        mu = dc.composite_f64_mutant(raw, z, d, False, mutate)
        got = dict(weights=mu["weights"].astype(F32), rgb_map=mu["rgb"].astype(F32), acc_map=mu["acc"].astype(F32),
                   depth_map=mu["depth"].astype(F32))
        got["disp_map"] = R.disp_f64(got["depth_map"], got["acc_map"]).astype(F32)
        ratios = R.integrator_ratios(got, raw, z, d, False)
        assert max(ratios.values()) > 1, (mutate, ratios)
