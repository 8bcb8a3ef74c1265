"""The mesh clean-up of csrc/nb_mesh_clean.hip restated with numpy and scipy, by the rules include/nb_hip.h states: labels from
scipy.sparse.csgraph.connected_components re-labelled to each component's smallest vertex, the select rule, the order-preserving
compaction; and the mesh cases both test files use."""
import functools

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

EINTERNAL = -4


def valid_faces(faces, V):
    """bool [T]: the faces whose three indices lie in 0..V-1 (the others are skipped everywhere)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < V)).all(axis=1)


def components(faces, V):
    """int32 [V]: the smallest vertex index of every vertex's connected component."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    f = faces[valid_faces(faces, V)]
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = scipy.sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V))
    _, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    smallest = np.full(comp.max(initial=-1) + 1, V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    return smallest[comp].astype(np.int32)


def select(label, faces, min_fraction):
    """-> (keep uint8 [V], stats int32 [4] = {components with a face, components kept, faces of the largest, faces kept})."""
    label = np.asarray(label, np.int64)
    V = len(label)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    count = np.bincount(label[faces[valid_faces(faces, V), 0]], minlength=V) if V else np.zeros(0, np.int64)
    roots = np.flatnonzero(count > 0)
    if len(roots) == 0:
        return np.zeros(V, np.uint8), np.zeros(4, np.int32)
    largest = int(count.max())
    winner = int(roots[count[roots] == largest].min())  # a tie goes to the smaller label
    if min_fraction >= 1.0:
        kept = np.array([winner])
    else:
        need = max(int(np.ceil(np.float64(np.float32(min_fraction)) * largest)), 1)
        kept = roots[count[roots] >= need]
    keep = np.isin(label, kept).astype(np.uint8)
    return keep, np.array([len(roots), len(kept), largest, int(count[kept].sum())], np.int32)


def compact(verts, faces, keep, attr=None):
    """-> (verts', faces'[, attr']): kept vertices and faces in their order; a face is kept iff it is valid and its first vertex is
    kept; an index of a dropped vertex becomes -1."""
    verts, faces, keep = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(keep) != 0
    V = len(verts)
    vpos = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    fkeep = valid_faces(faces, V)
    fkeep[fkeep] = keep[faces[fkeep, 0]]
    out = (verts[keep], vpos[faces[fkeep]].reshape(-1, 3).astype(np.int32))
    return out if attr is None else out + (np.asarray(attr, np.float32)[keep],)


def n_components_with_faces(faces, V):
    label = components(faces, V)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return len(np.unique(label[faces[valid_faces(faces, V), 0]]))


# ------------------------------------------------------------------------------------------------------------------ cases
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def strip(n_tri, perm=None):
    """A strip of n_tri triangles over n_tri + 2 vertices, triangle i = (i, i + 1, i + 2) along the strip, the vertices numbered
    through `perm` (position along the strip -> vertex index)."""
    i = np.arange(n_tri)
    f = np.stack([i, i + 1, i + 2], 1)
    return (f if perm is None else np.asarray(perm)[f]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (faces int32 [T,3], V).  Read-only: copy before changing."""
    out = {"two_tetrahedra": (np.concatenate([TETRA, TETRA + 4]), 8)}
    n = 4096
    rng = np.random.RandomState(7)
    perm = np.concatenate([rng.permutation(np.arange(1, n + 2)), [0]])  # vertex 0 at the far end of the strip
    out["strip_permuted"] = (strip(n, perm), n + 2)
    out["strip_ascending"] = (strip(n), n + 2)
    # 300 components of 1 to 40 faces (strips), 50 unused vertices in between
    sizes = rng.randint(1, 41, 300)
    gaps = set(rng.choice(299, 50, replace=False).tolist())
    faces, base = [], 0
    for k, s in enumerate(sizes):
        faces.append(strip(int(s)) + base)
        base += int(s) + 2 + (1 if k in gaps else 0)
    many = np.concatenate(faces)
    many = many[rng.permutation(len(many))]  # the components' faces interleaved
    out["many_components"] = (many.astype(np.int32), base)
    # 5 faces with an index of -1 or V between two tetrahedra: they neither connect nor survive
    bad = np.array([[0, 4, -1], [8, 1, 5], [-1, -1, -1], [3, 8, 7], [2, 6, 8]], np.int32)
    both = np.concatenate([TETRA, TETRA + 4])
    out["bad_faces"] = (np.concatenate([both[:3], bad[:2], both[3:6], bad[2:], both[6:]]), 8)
    out["no_faces"] = (np.zeros((0, 3), np.int32), 5)
    out["one_vertex"] = (np.zeros((0, 3), np.int32), 1)
    out["one_vertex_one_face"] = (np.zeros((1, 3), np.int32), 1)
    for f, _ in out.values():
        f.setflags(write=False)
    return out


def sized_components(sizes, gap=0):
    """Strips of the given face counts one after another (`gap` unused vertices behind each) -> (faces, V)."""
    faces, base = [], 0
    for s in sizes:
        faces.append(strip(int(s)) + base)
        base += int(s) + 2 + gap
    return np.concatenate(faces).astype(np.int32), base
