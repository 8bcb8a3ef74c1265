"""`TriMesh` — what RendererMesh.render returns as `mesh` where trimesh is not installed: the vertices, the faces and the one method
the reference's mesh visualizer calls on it (lib/visualizers/if_nerf_mesh.py:26-34, `mesh.export(path)`); optionally a colour per
vertex (cfg.mesh_color), which the reference's meshes never have."""
import numpy as np


class TriMesh:
    def __init__(self, vertices, faces, vertex_colors=None, vertex_normals=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        self.vertex_colors = None  # uint8 [V,3] RGB, or None: a mesh without colours
        if vertex_colors is not None:
            colors = np.asarray(vertex_colors)
            if colors.dtype != np.uint8 or colors.shape != (len(self.vertices), 3):
                raise ValueError("vertex_colors must be uint8 [%d,3], got %s %s" % (len(self.vertices), colors.dtype, colors.shape))
            self.vertex_colors = np.ascontiguousarray(colors)
        self.vertex_normals = None  # float32 [V,3], or None: a mesh without normals of its own (cfg.mesh_normals: field gives them)
        if vertex_normals is not None:
            normals = np.asarray(vertex_normals)
            if normals.dtype.kind != "f" or normals.shape != (len(self.vertices), 3):
                raise ValueError("vertex_normals must be float [%d,3], got %s %s" % (len(self.vertices), normals.dtype, normals.shape))
            self.vertex_normals = np.ascontiguousarray(normals, dtype=np.float32)

    def export(self, path):
        r"""Binary little-endian PLY: float32 vertices, triangles as `list uchar int` (what trimesh writes for a `.ply` path); with
        vertex_colors, `property uchar red / green / blue` behind x y z (what trimesh writes for a coloured mesh, without alpha).
        With vertex_normals, `property float nx / ny / nz` between the two (trimesh's order).  Without either the header is
            "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (V, T)
        followed by V x 3 little-endian float32 and T records of (uchar 3, 3 little-endian int32)."""
        path = str(path)
        if not path.lower().endswith(".ply"):
            raise ValueError("TriMesh.export writes PLY only (got %r); install trimesh for other formats" % path)
        nv, nf = len(self.vertices), len(self.faces)
        colors = "" if self.vertex_colors is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        normals = "" if self.vertex_normals is None else "property float nx\nproperty float ny\nproperty float nz\n"
        header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s%s"
                  "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (nv, normals, colors, nf))
        faces = np.empty(nf, dtype=[("n", "u1"), ("v", "<i4", (3,))])
        faces["n"] = 3
        faces["v"] = self.faces
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            if self.vertex_colors is None and self.vertex_normals is None:
                f.write(self.vertices.astype("<f4").tobytes())
            else:
                fields = [("p", "<f4", (3,))] + ([] if self.vertex_normals is None else [("n", "<f4", (3,))]) + \
                    ([] if self.vertex_colors is None else [("c", "u1", (3,))])
                verts = np.empty(nv, dtype=fields)
                verts["p"] = self.vertices
                if self.vertex_normals is not None:
                    verts["n"] = self.vertex_normals
                if self.vertex_colors is not None:
                    verts["c"] = self.vertex_colors
                f.write(verts.tobytes())
            f.write(faces.tobytes())
        return path

    _SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
                "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
                "double": "<f8", "float64": "<f8"}

    @classmethod
    def load_ply(cls, path):
        """Reads what `export` and trimesh write: binary little-endian PLY, a vertex element with float or double x / y / z
        (uchar red / green / blue, when all three are there, come back as vertex_colors, float nx / ny / nz as vertex_normals; further
        scalar properties are skipped), then
        a face element of `list uchar int|uint` triangles.  Anything else is
        refused with what was found."""
        with open(str(path), "rb") as f:
            data = f.read()
        end = data.find(b"end_header\n")
        if not data.startswith(b"ply") or end < 0:
            raise ValueError("%s is not a PLY file (starts with %r)" % (path, data[:16]))
        lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()[1:]]
        lines = [ln for ln in lines if ln and ln[0] not in ("comment", "obj_info")]
        if not lines or lines[0][:2] != ["format", "binary_little_endian"]:
            raise ValueError("%s: only binary_little_endian PLY is read, found %r" % (path, " ".join(lines[0]) if lines else ""))
        elements = []
        for ln in lines[1:]:
            if ln[0] == "element" and len(ln) == 3:
                elements.append((ln[1], int(ln[2]), []))
            elif ln[0] == "property" and elements:
                elements[-1][2].append(ln[1:])
            else:
                raise ValueError("%s: unexpected header line %r" % (path, " ".join(ln)))
        if [e[0] for e in elements] != ["vertex", "face"]:
            raise ValueError("%s: expected the elements vertex, face; found %s" % (path, [e[0] for e in elements]))
        (_, nv, vprops), (_, nf, fprops) = elements
        if any(len(p) != 2 or p[0] not in cls._SCALARS for p in vprops):
            raise ValueError("%s: vertex properties must be scalars, found %s" % (path, [" ".join(p) for p in vprops]))
        vdtype = np.dtype([(p[1], cls._SCALARS[p[0]]) for p in vprops])
        if any(k not in vdtype.names or vdtype[k].kind != "f" or vdtype[k].itemsize < 4 for k in "xyz"):
            raise ValueError("%s: x, y, z must be float or double vertex properties, found %s" % (path, [" ".join(p) for p in vprops]))
        if len(fprops) != 1 or len(fprops[0]) != 4 or fprops[0][0] != "list" or cls._SCALARS.get(fprops[0][1]) != "u1" or \
                cls._SCALARS.get(fprops[0][2]) not in ("<i4", "<u4"):
            raise ValueError("%s: faces must be one `list uchar int|uint` property, found %s" % (path, [" ".join(p) for p in fprops]))
        fdtype = np.dtype([("n", "u1"), ("v", cls._SCALARS[fprops[0][2]], (3,))])
        body = end + len(b"end_header\n")
        need = nv * vdtype.itemsize + nf * fdtype.itemsize
        if len(data) - body < need:
            raise ValueError("%s: %d bytes after the header, %d vertices and %d triangles need %d" % (path, len(data) - body, nv, nf, need))
        verts = np.frombuffer(data, vdtype, nv, body)
        faces = np.frombuffer(data, fdtype, nf, body + nv * vdtype.itemsize)
        if nf and (faces["n"] != 3).any():
            raise ValueError("%s: only triangles are read, found a face of %d vertices" % (path, int(faces["n"][faces["n"] != 3][0])))
        colors = None
        if all(k in vdtype.names and vdtype[k] == np.uint8 for k in ("red", "green", "blue")):
            colors = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
        normals = None
        if all(k in vdtype.names and vdtype[k].kind == "f" for k in ("nx", "ny", "nz")):
            normals = np.stack([verts["nx"], verts["ny"], verts["nz"]], 1).astype(np.float32)
        return cls(np.stack([verts["x"], verts["y"], verts["z"]], 1), faces["v"], colors, normals)
