"""`TriMesh` — what RendererMesh.render returns as `mesh` where trimesh is not installed: the vertices, the faces and the one method
the reference's mesh visualizer calls on it (lib/visualizers/if_nerf_mesh.py:26-34, `mesh.export(path)`)."""
import numpy as np


class TriMesh:
    def __init__(self, vertices, faces):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)

    def export(self, path):
        """Binary little-endian PLY: float32 vertices, triangles as `list uchar int` (what trimesh writes for a `.ply` path)."""
        path = str(path)
        if not path.lower().endswith(".ply"):
            raise ValueError("TriMesh.export writes PLY only (got %r); install trimesh for other formats" % path)
        nv, nf = len(self.vertices), len(self.faces)
        header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (nv, nf))
        faces = np.empty(nf, dtype=[("n", "u1"), ("v", "<i4", (3,))])
        faces["n"] = 3
        faces["v"] = self.faces
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(self.vertices.astype("<f4").tobytes())
            f.write(faces.tobytes())
        return path
