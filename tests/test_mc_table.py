"""The marching-cubes case table (tools/gen_mc_table.py -> neuralbody_amd/csrc/nb_mc_table.h): reproducible, complete,
crack-free across shared faces, and oriented from inside to outside.  Positions: edge mid points in half-cell units (integers)."""
import collections
import re

import pytest

from tests import mc_ref

G = mc_ref.load_generator()


@pytest.fixture(scope="module")
def table():
    return G.build_table()


def test_generator_reproduces_committed_header(table):
    with open(G.HEADER) as f:
        committed = f.read()
    assert G.render_header(table) == committed
    m = re.search(r"#define NB_MC_MAX_TRI (\d+)", committed)
    assert int(m.group(1)) == max(len(t) for t in table)


def _sides(tris):
    return [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]


def test_every_case_uses_the_crossed_edges_and_closes_up_to_the_faces(table):
    assert table[0] == [] and table[255] == []
    for case in range(256):
        tris = table[case]
        crossed = {e for e in range(12) if G.crossed(case, e)}
        assert {e for t in tris for e in t} == crossed, case
        assert all(len(set(t)) == 3 for t in tris), case
        count = collections.Counter(_sides(tris))
        assert set(count.values()) <= {1}, case  # no directed side twice
        segments = {s for f in G.FACES for s in G.face_segments(case, f)}
        for (a, b) in count:
            if G.edges_share_face(a, b):  # the side lies in a cell face: once, and it is that face's segment
                assert (b, a) not in count and (a, b) in segments, (case, a, b)
            else:  # interior: twice, in opposite directions
                assert (b, a) in count, (case, a, b)
        assert segments <= set(count), case


def test_face_segments_depend_on_the_face_signs_only(table):
    for face in G.FACES:
        corners = G.face_corners(face)
        by_signs = {}
        for case in range(256):
            key = tuple(G.inside(case, k) for k in corners)
            segs = sorted(G.face_segments(case, face))
            assert by_signs.setdefault(key, segs) == segs, (face, case)
        assert len(by_signs) == 16


def _shifted(e, axis, delta):
    """Edge id -> doubled mid point with the cell moved by `delta` cells along `axis`."""
    m = list(G.EDGE_MID2[e])
    m[axis] += 2 * delta
    return tuple(m)


@pytest.mark.parametrize("axis,lows", [(0, None), (1, (0, 37, 90, 105, 150, 165, 255)), (2, (0, 37, 90, 105, 150, 165, 255))])
def test_shared_face_segments_cancel(table, axis, lows):
    """Two cells side by side along `axis`: the low cell's face axis = 1 and the high cell's face axis = 0 hold the same four
    lattice points; for every compatible pair of cases the directed triangle sides in that face cancel.  All 256 x 256 pairs
    (filtered to the compatible ones) on axis 0; all high cases against a spread of low cases on axes 1 and 2."""
    hi_face, lo_face = (axis, 0), (axis, 1)
    bit = 4 >> axis
    pairs = 0
    for lo in (range(256) if lows is None else lows):
        for hi in range(256):
            # corner k of the high cell with axis bit 0 is corner k | bit of the low cell
            if any(G.inside(hi, k) != G.inside(lo, k | bit) for k in G.face_corners(hi_face)):
                continue
            pairs += 1
            lo_edges, hi_edges = set(G.face_edges(lo_face)), set(G.face_edges(hi_face))
            side_lo = collections.Counter((_shifted(a, axis, 0), _shifted(b, axis, 0)) for a, b in _sides(table[lo])
                                          if a in lo_edges and b in lo_edges)
            side_hi = collections.Counter((_shifted(b, axis, 1), _shifted(a, axis, 1)) for a, b in _sides(table[hi])
                                          if a in hi_edges and b in hi_edges)  # reversed
            assert side_lo == side_hi, (axis, lo, hi)
    assert pairs == (256 * 16 if lows is None else len(lows) * 16)


def test_triangle_normals_point_from_inside_to_outside(table):
    """Predicate, in exact integer arithmetic: with P the doubled edge mid points of a triangle, n = (P1 - P0) x (P2 - P0) and
    g = P0 + P1 + P2 (three times the doubled centroid), there is an OUTSIDE corner c with n . (6 c - g) > 0 and an INSIDE corner
    c with n . (6 c - g) < 0."""
    for case, tris in enumerate(table):
        for t in tris:
            P = [G.EDGE_MID2[e] for e in t]
            n = G._cross(G._sub(P[1], P[0]), G._sub(P[2], P[0]))
            g = tuple(sum(p[i] for p in P) for i in range(3))
            assert n != (0, 0, 0), (case, t)
            side = [G._dot(n, G._sub(tuple(6 * x for x in G.corner_pos(k)), g)) for k in range(8)]
            assert any(s > 0 for k, s in enumerate(side) if not G.inside(case, k)), (case, t)
            assert any(s < 0 for k, s in enumerate(side) if G.inside(case, k)), (case, t)


def test_complementary_cases_mirror_the_unambiguous_ones(table):
    """A case without an ambiguous face and its complement cut the same edges; only the orientation flips."""
    for case in range(256):
        ambiguous = any(len([e for e in G.face_edges(f) if G.crossed(case, e)]) == 4 for f in G.FACES)
        if not ambiguous:
            a = {frozenset(s) for s in _sides(table[case]) if G.edges_share_face(*s)}
            b = {frozenset(s) for s in _sides(table[255 - case]) if G.edges_share_face(*s)}
            assert a == b, case
