"""Vectorised numpy restatement of nb_marching_cubes (include/nb_hip.h): same inside rule (value > iso), same case table
(loaded from tools/gen_mc_table.py, not from the C header), fp64 interpolation rounded once to fp32, and the same output order:
vertices by (owner point in C order, axis), triangles by (cell in C order, place in the table row).  Plus the mesh predicates
the tests share (manifoldness, Euler characteristic, signed volume) and the test fields."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TABLE = None


def table():
    """(ntri [256], rows [256, 3 * max] with -1 padding, owner offsets [12, 3]) from the generator."""
    global _TABLE
    if _TABLE is None:
        g = load_generator()
        tris = g.build_table()
        width = 3 * max(len(t) for t in tris)
        rows = -np.ones((256, width), np.int64)
        for c, t in enumerate(tris):
            flat = [e for tri in t for e in tri]
            rows[c, :len(flat)] = flat
        owner = np.array([g.corner_pos(g.EDGE_CORNERS[e][0]) for e in range(12)], np.int64)
        _TABLE = (np.array([len(t) for t in tris], np.int64), rows, owner)
    return _TABLE


def case_index(cube, iso):
    """[X-1, Y-1, Z-1] case numbers: bit k = corner (k >> 2 & 1, k >> 1 & 1, k & 1) is inside."""
    ins = np.asarray(cube, np.float32) > np.float32(iso)
    X, Y, Z = ins.shape
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for k in range(8):
        dx, dy, dz = k >> 2 & 1, k >> 1 & 1, k & 1
        case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << k
    return case


def marching_cubes(cube, iso):
    """-> (vertices [V,3] float32 in lattice index units, triangles [T,3] int32)."""
    cube = np.ascontiguousarray(cube, np.float32)
    iso = np.float32(iso)
    X, Y, Z = cube.shape
    assert min(X, Y, Z) >= 2
    ntri, rows, owner = table()
    ins = cube > iso  # NaN and equality: outside
    flags = np.zeros((X, Y, Z, 3), bool)
    flags[:-1, :, :, 0] = ins[:-1] != ins[1:]
    flags[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    flags[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    flat = flags.reshape(-1)
    epos = np.cumsum(flat, dtype=np.int64) - flat  # exclusive scan
    idx = np.flatnonzero(flat)
    p, a = idx // 3, idx % 3
    stride = np.array([Y * Z, Z, 1], np.int64)
    v0 = cube.reshape(-1)[p].astype(np.float64)
    v1 = cube.reshape(-1)[p + stride[a]].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.float64(iso) - v0) / (v1 - v0)
    verts = np.stack(np.unravel_index(p, (X, Y, Z)), 1).astype(np.float64)
    verts[np.arange(len(p)), a] += t
    vertices = verts.astype(np.float32).reshape(-1, 3)

    case = case_index(cube, iso).reshape(-1)
    cells = np.flatnonzero(ntri[case] > 0)  # C order of the cell grid == C order of the cells' lower points
    ci, cj, cl = np.unravel_index(cells, (X - 1, Y - 1, Z - 1))
    r = rows[case[cells]]
    used = np.arange(rows.shape[1])[None, :] < 3 * ntri[case[cells]][:, None]
    e = r[used]  # row-major: by cell, then place in the row
    rep = np.repeat(np.arange(len(cells)), 3 * ntri[case[cells]])
    lin = ((ci[rep] + owner[e, 0]) * Y + cj[rep] + owner[e, 1]) * Z + cl[rep] + owner[e, 2]
    assert flat[3 * lin + e // 4].all()
    triangles = epos[3 * lin + e // 4].astype(np.int32).reshape(-1, 3)
    return vertices, triangles


# ------------------------------------------------------------------------------------------ mesh predicates
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented_manifold(triangles):
    """Every undirected edge lies in exactly two triangles, once per direction."""
    d = directed_edges(triangles)
    if len(d) == 0:
        return True
    n = int(d.max()) + 1
    key = d[:, 0] * n + d[:, 1]
    rev = d[:, 1] * n + d[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((d[:, 0] != d[:, 1]).all() and (counts == 1).all() and np.array_equal(uniq, np.unique(rev)))


def euler_characteristic(vertices, triangles):
    d = directed_edges(triangles)
    und = np.unique(np.sort(d, 1), axis=0)
    return len(vertices) - len(und) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------ fields
SPHERE = dict(shape=(40, 36, 44), c=(19.3, 17.6, 21.2), R=13.7)
TORUS = dict(shape=(48, 48, 24), c=(23.4, 23.7, 11.6), R=14.2, r=5.3)
NOISE_SEED, NOISE_SIDE, NOISE_ISO = 7, 24, 0.5


def _grid(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def sphere_field(shape=SPHERE["shape"], c=SPHERE["c"], R=SPHERE["R"]):
    """f = R - |p - c| in fp64, rounded to fp32; iso 0."""
    x, y, z = _grid(shape)
    return (R - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def torus_field(shape=TORUS["shape"], c=TORUS["c"], R=TORUS["R"], r=TORUS["r"]):
    x, y, z = _grid(shape)
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return (r - np.sqrt(q ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def noise_field():
    """24^3 uniform fp32 noise, zero-padded by one; at iso 0.5 every one of the 254 non-empty cases occurs (asserted in
    tests/test_mesh_host.py)."""
    rng = np.random.RandomState(NOISE_SEED)
    return np.pad(rng.rand(NOISE_SIDE, NOISE_SIDE, NOISE_SIDE).astype(np.float32), 1)


def golden_cube():
    return np.load(os.path.join(ROOT, "tests", "golden", "mesh_cube.npz"))["cube"].astype(np.float32)


def fields():
    """name -> (fp32 cube, iso): the four fields the host and the GPU tests share."""
    return {"sphere": (sphere_field(), 0.0), "torus": (torus_field(), 0.0), "golden": (golden_cube(), 5.0),
            "noise": (noise_field(), NOISE_ISO)}
