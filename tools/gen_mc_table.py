"""Derives the 256-case marching-cubes triangle table from first principles and writes neuralbody_amd/csrc/nb_mc_table.h.

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit 1 when the committed header differs

Conventions (shared by csrc/nb_mesh.hip, tests/mc_ref.py and tests/test_mc_table.py):

  corner k of the cell at lattice point (i, j, l) is (i + (k >> 2 & 1), j + (k >> 1 & 1), l + (k & 1));
  a corner is INSIDE iff value > iso (equal and NaN are outside); case index = bit mask of the inside corners (bit k = corner k);
  edge e = 4 * a + 2 * u + v runs along axis a (0 = x, 1 = y, 2 = z) from the corner whose axis-a bit is 0 to the one whose bit is
  1; (u, v) are the corner bits of the two other axes in increasing axis order.  The vertex of an edge belongs to the edge's
  lower corner (EDGE_CORNERS[e][0]) and to axis a.

Construction, per case:

  1. On each of the six faces the crossed edges are joined into directed segments.  Two crossed edges: one segment.  Four crossed
     edges (the two inside corners sit on a diagonal): one segment per inside corner, joining the two face edges that meet in it,
     so inside corners are never connected across a face.  The rule reads the four corner signs of the face and nothing else:
     two cells that share a face draw the same segments in it, and the surface has no cracks.
  2. Every segment is directed so that, looking at the face from outside the cell, the inside corners lie to its RIGHT.  The
     segments are then the boundary of the inside region of the cell's surface, run clockwise as seen from outside; each
     crossed edge is the head of one segment and the tail of one other, so following them gives closed loops.
  3. Every loop is fan-triangulated.  With the direction of step 2 the triangle normals ((b - a) x (c - a)) point from the
     inside (high values) to the outside.  The fan's apex is the loop vertex that keeps every diagonal off the cell's faces
     (lowest edge id among those; a diagonal inside a face would coincide with nothing in the neighbouring cell).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "neuralbody_amd", "csrc", "nb_mc_table.h")


def corner_pos(k):
    return (k >> 2 & 1, k >> 1 & 1, k & 1)


def _edge_corners():
    out = []
    for a in range(3):
        others = [b for b in range(3) if b != a]
        for u in range(2):
            for v in range(2):
                p = [0, 0, 0]
                p[others[0]], p[others[1]] = u, v
                q = list(p)
                q[a] = 1
                out.append((p[0] * 4 + p[1] * 2 + p[2], q[0] * 4 + q[1] * 2 + q[2]))
    return out


EDGE_CORNERS = _edge_corners()  # [12] (lower corner, upper corner)
EDGE_AXIS = [e // 4 for e in range(12)]
# edge mid points in half-cell units (exact integers)
EDGE_MID2 = [tuple(a + b for a, b in zip(corner_pos(c0), corner_pos(c1))) for c0, c1 in EDGE_CORNERS]
# faces: (axis, side) -> corners and edges lying in the plane x_axis = side
FACES = [(a, s) for a in range(3) for s in range(2)]


def face_corners(face):
    a, s = face
    return [k for k in range(8) if corner_pos(k)[a] == s]


def face_edges(face):
    fc = set(face_corners(face))
    return [e for e in range(12) if EDGE_CORNERS[e][0] in fc and EDGE_CORNERS[e][1] in fc]


def edges_share_face(e0, e1):
    return any(e0 in face_edges(f) and e1 in face_edges(f) for f in FACES)


def inside(case, k):
    return bool(case >> k & 1)


def crossed(case, e):
    c0, c1 = EDGE_CORNERS[e]
    return inside(case, c0) != inside(case, c1)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _direct(face, e0, e1, corner):
    """(e0, e1) or (e1, e0): the inside `corner` lies to the right of the segment as seen from outside the cell."""
    a, s = face
    n = [0, 0, 0]
    n[a] = 2 * s - 1  # outward normal of the face
    p, q = EDGE_MID2[e0], EDGE_MID2[e1]
    c = tuple(2 * x for x in corner_pos(corner))
    side = _dot(_cross(_sub(q, p), _sub(c, p)), n)
    assert side != 0
    return (e0, e1) if side < 0 else (e1, e0)


def face_segments(case, face):
    """Directed segments (tail edge, head edge) the case draws in one face; depends on the face's four corner signs only."""
    fe = [e for e in face_edges(face) if crossed(case, e)]
    ins = [k for k in face_corners(face) if inside(case, k)]
    if not fe:
        return []
    if len(fe) == 2:
        return [_direct(face, fe[0], fe[1], ins[0])]
    assert len(fe) == 4 and len(ins) == 2
    segs = []
    for k in ins:  # one segment per inside corner: the two face edges that meet in it
        e0, e1 = [e for e in fe if k in EDGE_CORNERS[e]]
        segs.append(_direct(face, e0, e1, k))
    return segs


def case_loops(case):
    nxt = {}
    for f in FACES:
        for t, h in face_segments(case, f):
            assert t not in nxt
            nxt[t] = h
    assert sorted(nxt) == sorted(nxt.values()) == [e for e in range(12) if crossed(case, e)]
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def _fan(loop):
    """Fan triangulation; apex: the first rotation (starting at the lowest edge id) none of whose diagonals lies in a face."""
    n = len(loop)
    start = loop.index(min(loop))
    for r in range(n):
        rot = loop[(start + r) % n:] + loop[:(start + r) % n]
        if all(not edges_share_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no fan apex keeps the diagonals of loop %s off the faces" % (loop,))


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        tris += _fan(loop)
    return tris


def build_table():
    return [case_triangles(c) for c in range(256)]


def render_header(table):
    max_tri = max(len(t) for t in table)
    row = 3 * max_tri
    L = []
    L.append("// GENERATED by tools/gen_mc_table.py — do not edit; tests/test_mc_table.py regenerates and compares it byte for byte.")
    L.append("// Marching-cubes case table derived from first principles (no copied table).")
    L.append("//   corner k of a cell = lower lattice point + (k >> 2 & 1, k >> 1 & 1, k & 1); case bit k = corner k is inside (v > iso)")
    L.append("//   edge e = 4 * axis + 2 * u + v, (u, v) = corner bits of the other two axes in increasing axis order; the edge's vertex")
    L.append("//   belongs to lattice point (lower cell point + NB_MC_EDGE_OWNER[e]) and to axis e / 4")
    L.append("//   ambiguous faces: each segment cuts off ONE inside corner (a function of the face's four signs only: no cracks)")
    L.append("//   triangle normals ((b - a) x (c - a)) point from inside (v > iso) to outside")
    L.append("// Maximum number of triangles per case found by the generator: %d" % max_tri)
    L.append("#pragma once")
    L.append("")
    L.append("#ifndef NB_MC_TABLE_QUAL")
    L.append("#define NB_MC_TABLE_QUAL static const")
    L.append("#endif")
    L.append("")
    L.append("#define NB_MC_MAX_TRI %d" % max_tri)
    L.append("#define NB_MC_ROW %d  // edge ids per row: 3 * NB_MC_MAX_TRI, -1 padded" % row)
    L.append("")
    L.append("// offset (dx, dy, dz) of the lattice point that owns edge e's vertex, relative to the cell's lower point")
    L.append("NB_MC_TABLE_QUAL signed char NB_MC_EDGE_OWNER[12][3] = {")
    L.append("    " + ", ".join("{%d, %d, %d}" % corner_pos(EDGE_CORNERS[e][0]) for e in range(12)) + "};")
    L.append("")
    L.append("NB_MC_TABLE_QUAL unsigned char NB_MC_NTRI[256] = {")
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    L.append("};")
    L.append("")
    L.append("NB_MC_TABLE_QUAL signed char NB_MC_TRI[256][NB_MC_ROW] = {")
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (row - len(flat))
        L.append("    {" + ", ".join("%2d" % e for e in flat) + "},  // %3d" % c)
    L.append("};")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    table = build_table()
    text = render_header(table)
    print("marching cubes table: max %d triangles per case, %d triangles in all" % (
        max(len(t) for t in table), sum(len(t) for t in table)))
    if args.check:
        with open(HEADER) as f:
            same = f.read() == text
        print("header %s" % ("matches" if same else "DIFFERS"))
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main())
