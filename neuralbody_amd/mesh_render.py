"""`MeshTurntable` — the normal-shaded turntable of an extracted mesh on the device: what zju3dv/neuralbody's
`python tools/render_mesh.py --exp_name ... --dataset ...` draws with an OpenGL context (tools/render/*), for nodes that have none.

tools/render_mesh.py:120-170 per view k = 0 .. 90: the vertices go through rot = [[1,0,0],[0,0,1],[0,-1,0]] and the dataset's
rotation (identity for zju_mocap, Rz(90) Ry(90) otherwise), are centred on the bounding box of the result, divided by its y extent
and rotated by Ry(-(90 + 4 (k + 1)) degrees).  The camera (tools/render/camera.py:160-190 with ortho_ratio = 1.2, width 1, height
H / W, eye on +z; glm.py:114-123) is orthographic; worked through its matrices, for p the transformed vertex
    x_px = (p.x / 1.2 + 1/2) W,    y_px = H / 2 - p.y W / 1.2  (row 0 on top after the reference's np.flip),    depth = -p.z,
the smaller depth nearer (GL_LESS).  The vertex colour is 0.5 n' + 0.5 with n' the vertex normal of the rotated mesh; rotation and
uniform scale commute with compute_normal, so the normals are computed once in object space (ops.mesh_vertex_normals) and rotated
per view inside ops.mesh_render.  `turntable_cams` composes both maps in float64; tests/test_mesh_render_host.py holds it to the
reference's chain of GL matrices."""
import math
import os

import numpy as np
import torch

from . import ops

ROT = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # render_mesh.py:132


def _rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def object_rotation(dataset="zju_mocap"):
    """float64 [3,3]: rot, then the dataset's rotation (render_mesh.py:113-116, 132-136)."""
    return ROT.copy() if dataset == "zju_mocap" else _rot_z(90.0) @ _rot_y(90.0) @ ROT


def turntable_cams(lo, hi, H, W, dataset="zju_mocap", n_views=91, step_deg=4.0, ortho_ratio=1.2):
    """lo, hi: the bounding box of the vertices after `object_rotation(dataset)` -> float64 [n_views,24], per view the 3 x 4
    affine from an object-space vertex to (x_px, y_px, depth), the 3 x 3 rotation of the normals and 3 zeros (ops.mesh_render
    takes it rounded to float32)."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    H, W, n_views = int(H), int(W), int(n_views)
    extent = hi[1] - lo[1]
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and extent > 0.0):
        raise ValueError("the mesh's bounding box %s .. %s has no y extent to scale by" % (lo.tolist(), hi.tolist()))
    if H < 1 or W < 1 or n_views < 1:
        raise ValueError("H = %d, W = %d, n_views = %d must be positive" % (H, W, n_views))
    A = object_rotation(dataset)
    centre = 0.5 * (hi + lo)
    cams = np.zeros((n_views, ops.MESH_CAM_FLOATS), np.float64)
    R, step = _rot_y(-90.0), _rot_y(-step_deg)
    for k in range(n_views):
        R = step @ R                       # Ry(-(90 + step_deg (k + 1))), accumulated as render_mesh.py:148-158 accumulates it
        L = R @ A / extent                 # p = L v + t
        t = -(R @ centre) / extent
        M = np.stack([np.append(L[0], t[0]) * (W / ortho_ratio) + np.array([0.0, 0.0, 0.0, 0.5 * W]),
                      np.append(L[1], t[1]) * (-W / ortho_ratio) + np.array([0.0, 0.0, 0.0, 0.5 * H]),
                      -np.append(L[2], t[2])])
        cams[k, :12] = M.reshape(-1)
        cams[k, 12:21] = (R @ A).reshape(-1)
    return cams


def to_bgr8(images):
    """What the reference hands cv2.imwrite (render_mesh.py:165-169): the channels in BGR order, 255 * img rounded half to even
    and saturated -> uint8 [...,3] host array."""
    img = images.detach().float().cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images, np.float32)
    if img.shape[-1] != 3:
        raise ValueError("images must end in 3 channels, got %s" % (img.shape,))
    return np.clip(np.rint(255.0 * img[..., ::-1].astype(np.float64)), 0, 255).astype(np.uint8)


def _jpeg_writer():
    try:
        from cv2 import imwrite  # also an ImportError for a cv2 that is only a stub in sys.modules

        return lambda path, bgr: imwrite(path, bgr)
    except ImportError:
        pass
    try:
        from PIL import Image

        return lambda path, bgr: Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path, quality=95)  # cv2's default quality
    except ImportError:
        raise ImportError("MeshTurntable.save needs cv2 (opencv-python) or PIL (pillow) to write JPEG files; neither imports")


class MeshTurntable:
    """render(vertices, triangles) -> device float32 [n_views,H,W,3] RGB in 0..1; save(images, directory) -> `%d.jpg`.
    render(..., colors=...) draws the mesh in its vertex colours instead of the normal shading: the same cameras, coverage and
    depth test (ops.mesh_render_attr)."""

    def __init__(self, H=512, W=512, dataset="zju_mocap", views_per_call=16, device="cuda:0", n_views=91, step_deg=4.0,
                 ortho_ratio=1.2):
        self.H, self.W, self.dataset, self.device = int(H), int(W), dataset, torch.device(device)
        self.views_per_call, self.n_views, self.step_deg, self.ortho_ratio = int(views_per_call), int(n_views), step_deg, ortho_ratio
        if self.views_per_call < 1:
            raise ValueError("views_per_call must be positive, got %d" % self.views_per_call)

    def _mesh(self, vertices, triangles):
        if triangles is None:  # a host mesh: trimesh.Trimesh or mesh.TriMesh
            vertices, triangles = vertices.vertices, vertices.faces
        v = torch.as_tensor(np.asarray(vertices) if not isinstance(vertices, torch.Tensor) else vertices)
        t = torch.as_tensor(np.asarray(triangles) if not isinstance(triangles, torch.Tensor) else triangles)
        v = v.detach().to(self.device, torch.float32).reshape(-1, 3).contiguous()
        t = t.detach().to(self.device, torch.int32).reshape(-1, 3).contiguous()
        if v.shape[0] < 1:
            raise ValueError("the mesh has no vertices")
        return v, t

    def cams(self, vertices):
        """The views' float32 [n_views,24] on the device; the bounding box is the one read-back (six floats)."""
        A = torch.from_numpy(object_rotation(self.dataset).astype(np.float32)).to(vertices.device)
        turned = vertices @ A.T
        box = torch.stack([turned.amin(0), turned.amax(0)]).double().cpu().numpy()
        cams = turntable_cams(box[0], box[1], self.H, self.W, self.dataset, self.n_views, self.step_deg, self.ortho_ratio)
        return torch.from_numpy(cams.astype(np.float32)).to(vertices.device)

    def _colors(self, colors, mesh, V):
        """float32 [V,3] in 0..1 on the device from `colors`: True (the host mesh's own vertex_colors), a uint8 array or tensor
        (divided by 255) or a float one (taken as it is: RendererMesh.extract_mesh's rgb_f)."""
        if colors is True:
            colors = getattr(mesh, "vertex_colors", None)
            if colors is None:
                raise ValueError("colors=True needs a mesh that carries vertex_colors")
        c = torch.as_tensor(np.asarray(colors) if not isinstance(colors, torch.Tensor) else colors).detach().to(self.device)
        c = c.float() / 255.0 if c.dtype == torch.uint8 else c.float()
        if tuple(c.shape) != (V, 3):
            raise ValueError("colors has shape %s, the mesh has %d vertices" % (tuple(c.shape), V))
        return c.contiguous()

    def render(self, vertices, triangles=None, normals=None, colors=False):
        v, t = self._mesh(vertices, triangles)
        draw = ops.mesh_render
        if colors is not False and colors is not None:
            draw, normals = ops.mesh_render_attr, self._colors(colors, vertices, v.shape[0])
        elif normals is None:
            normals = ops.mesh_vertex_normals(v, t)
        cams = self.cams(v)
        n = min(self.views_per_call, self.n_views)
        scratch = ops.mesh_render_scratch(n, self.H, self.W, t.shape[0], v.device)  # the keys stay at views_per_call H W 8 bytes
        out = torch.empty((self.n_views, self.H, self.W, 3), dtype=torch.float32, device=v.device)
        for k in range(0, self.n_views, n):
            draw(v, normals, t, cams[k:k + n], self.H, self.W, out=out[k:k + n], scratch=scratch)
        return out

    def save(self, images, directory):
        """`directory/%d.jpg` per view, as render_mesh.py:169 -> the paths."""
        write = _jpeg_writer()
        os.makedirs(directory, exist_ok=True)
        bgr = to_bgr8(images)
        paths = []
        for k in range(bgr.shape[0]):
            paths.append(os.path.join(directory, "%d.jpg" % k))
            write(paths[-1], bgr[k])
        return paths
