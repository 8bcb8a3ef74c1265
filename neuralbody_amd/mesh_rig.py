"""An animatable mesh: the mesh extracted for one frame bound to the SMPL body it clothes, and reposed on the device.

    bind frame's poses | shapes | Rh | Th --> nb_smpl_pose (the body, posed) --> nb_mesh_closest (per mesh vertex the closest
    point of the body's surface) --> nb_mesh_rig_bind (weights and shape directions there, the inverse skin to the rest pose)

The inverse skin is the reference's ppts_to_pts (lib/utils/blend_utils.py:73-82), which it applies to sample points in its T-pose
variant; it has no mesh counterpart.  A bound mesh IS an SMPL-shaped model of V = its vertex count (`RiggedMesh`, a `SmplModel`):
PoseDriver(rig).vertices reposes it with the kernel that poses the body, .silhouettes gives CLOTHED cull masks, and `animate`
draws a clip with the turntable's renderer.  What is transferred: skinning weights, shape directions.  What is not: pose blend
shapes (a rig is driven with new_params = False; a bind frame posed with new_params = True has its corrective offsets baked into
the template), and the network's latent codes — a rig is geometry only, PoseDriver.frames / views refuse it."""
import numpy as np
import torch

from . import _lib, ops
from .smpl_pose import PoseDriver, SmplModel, pack_params

RIG_KEYS = ("v_template", "weights", "shapedirs")


def _tensor(a, dtype):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(dtype).contiguous()


class RiggedMesh(SmplModel):
    """A bound mesh as an SMPL-shaped model.  v_template [P,3], weights [24,P], shapedirs [10,3P] fp32 and faces int32 [T,3] (the
    MESH's triangles) are tensors on `body.device` (bind_mesh) or on the host (`load`; uploaded on the first `native()`); the
    joints (j_template, j_shapedirs, parents) are the body's own tensors, shared.  `vertex_colors`: uint8 [P,3] or None.
    `bind`: dict(face int32 [P], bary fp32 [P,3], params fp32 [88], new_params bool) — where and in which frame it was bound."""

    has_codes = False  # PoseDriver.frames / views: the network holds one code per BODY vertex

    def __init__(self, body, v_template, weights, shapedirs, faces, vertex_colors=None, bind=None):
        if not isinstance(body, SmplModel) or isinstance(body, RiggedMesh):
            raise TypeError("body must be the SmplModel the mesh is bound to")
        self.body, self.device, self.parents = body, body.device, list(body.parents)
        self._t = {"v_template": _tensor(v_template, torch.float32), "weights": _tensor(weights, torch.float32),
                   "shapedirs": _tensor(shapedirs, torch.float32), "faces": _tensor(faces, torch.int32)}
        P = int(self._t["v_template"].shape[0]) if self._t["v_template"].dim() == 2 else -1
        want = {"v_template": (P, 3), "weights": (_lib.SMPL_JOINTS, P), "shapedirs": (_lib.SMPL_BETAS, 3 * P)}
        for k, shape in want.items():
            if P < 1 or tuple(self._t[k].shape) != shape:
                raise ValueError("%s has shape %s; a rig of %d vertices needs %s" % (k, tuple(self._t[k].shape), P, shape))
        if self._t["faces"].dim() != 2 or self._t["faces"].shape[1] != 3 or self._t["faces"].shape[0] < 1:
            raise ValueError("faces must be [T,3] with T >= 1, got %s" % (tuple(self._t["faces"].shape),))
        self.n_verts = P
        self.vertex_colors = None
        if vertex_colors is not None:
            c = vertex_colors if isinstance(vertex_colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertex_colors))
            if c.dtype != torch.uint8 or tuple(c.shape) != (P, 3):
                raise ValueError("vertex_colors must be uint8 [%d,3], got %s %s" % (P, c.dtype, tuple(c.shape)))
            self.vertex_colors = c.detach().contiguous()
        self.bind = bind
        self._dev = None

    # SmplModel's host-side attributes, materialised only when asked for (save)
    @property
    def host(self):
        return {k: self._t[k].cpu().numpy() for k in RIG_KEYS}

    @property
    def faces(self):
        return self._t["faces"].cpu().numpy()

    def native(self):
        """(NbSmplModel of P vertices without posedirs, device tensors); the joints are the body's."""
        if self._dev is None:
            if self.device.type != "cuda":
                raise ops.NbError("the rig must live on a HIP device (got %s); the HIP path has no CPU fallback" % (self.device,))
            _, body = self.body.native()
            tensors = {k: v.to(self.device) for k, v in self._t.items()}
            tensors.update(j_template=body["j_template"], j_shapedirs=body["j_shapedirs"])
            self._t = {k: tensors[k] for k in self._t}
            self._dev = ops.make_smpl_model(tensors, self.parents) + (tensors,)
        return self._dev[0], self._dev[2]

    def faces_device(self):
        return self.native()[1]["faces"]

    def colors_device(self):
        """float32 [P,3] in 0..1 on the device, what ops.mesh_render_attr draws."""
        if self.vertex_colors is None:
            raise ValueError("the rig carries no vertex colours (the bound mesh had none)")
        return (self.vertex_colors.to(self.device).float() / 255.0).contiguous()

    def save(self, path):
        """One .npz: the template, weights, shape directions, faces, colours, face / bary and the bind parameters."""
        out = dict(self.host, faces=self.faces)
        if self.vertex_colors is not None:
            out["vertex_colors"] = self.vertex_colors.cpu().numpy()
        if self.bind is not None:
            out.update(bind_face=_tensor(self.bind["face"], torch.int32).cpu().numpy(),
                       bind_bary=_tensor(self.bind["bary"], torch.float32).cpu().numpy(),
                       bind_params=_tensor(self.bind["params"], torch.float32).cpu().numpy().reshape(-1),
                       bind_new_params=np.array(bool(self.bind["new_params"])))
        path = str(path)
        np.savez(path, **out)
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path, body):
        """The rig `save` wrote, on `body`'s joints.  Nothing is regressed: the joints do not depend on the mesh."""
        with np.load(str(path)) as z:
            bind = None
            if "bind_face" in z:
                bind = {"face": z["bind_face"], "bary": z["bind_bary"], "params": z["bind_params"], "new_params": bool(z["bind_new_params"])}
            return cls(body, z["v_template"], z["weights"], z["shapedirs"], z["faces"], z["vertex_colors"] if "vertex_colors" in z else None,
                       bind)


def bind_mesh(model, mesh_or_vertices, triangles, poses, shapes, Rh, Th, new_params=False):
    """Binds a mesh to `model` (a SmplModel with a triangle list) in the frame poses [72], shapes [10], Rh, Th [3] -> RiggedMesh.
    `mesh_or_vertices`: a host mesh with .vertices / .faces (and maybe .vertex_colors) when `triangles` is None, else vertices
    [P,3] with triangles [T,3], arrays or tensors.  One upload; the stream carries one nb_smpl_pose, the closest query and the
    bind; one read-back, of the bind's status.  NbError when a vertex found no face of the body to bind to."""
    if isinstance(model, RiggedMesh) or not isinstance(model, SmplModel):
        raise TypeError("model must be the body's SmplModel")
    if model.faces is None:
        raise ops.NbError("the SMPL model has no triangle list (no 'f' or 'faces' among its arrays): a mesh binds to its surface")
    colors = None
    if triangles is None:
        colors = getattr(mesh_or_vertices, "vertex_colors", None)
        mesh_or_vertices, triangles = mesh_or_vertices.vertices, mesh_or_vertices.faces
    if model.device.type != "cuda":
        raise ops.NbError("the SMPL model must live on a HIP device (got %s); the HIP path has no CPU fallback" % (model.device,))
    rows = pack_params(poses, shapes, Rh, Th, pin=True)
    if rows.shape[0] != 1:
        raise ValueError("a mesh is bound in ONE frame, got parameters of %d" % rows.shape[0])
    with torch.cuda.device(model.device):
        native, body = model.native()
        points = _tensor(mesh_or_vertices, torch.float32).reshape(-1, 3).to(model.device)
        faces = _tensor(triangles, torch.int32).reshape(-1, 3).to(model.device)
        params = rows.to(model.device, non_blocking=True)
        ws = torch.empty((1, _lib.SMPL_WS_FLOATS), dtype=torch.float32, device=model.device)
        verts, _ = ops.smpl_pose(native, params, new_params, ws=ws)
        face, bary, _ = ops.mesh_closest(points, verts[0], body["faces"])
        weights, shapedirs, v_template, status = ops.mesh_rig_bind(native, params[0], ws[0], body["faces"], points, face, bary)
        unbound, degenerate = (int(v) for v in status[:2].cpu())
    if unbound:
        raise ops.NbError("%d of %d mesh vertices found no face of the body to bind to (a non-finite vertex, or a body whose "
                          "faces are all degenerate)" % (unbound, points.shape[0]))
    rig = RiggedMesh(model, v_template, weights, shapedirs, faces, colors,
                     {"face": face, "bary": bary, "params": params[0], "new_params": bool(new_params)})
    rig.n_degenerate = degenerate
    return rig


def animate(rig, poses, shapes, Rh, Th, turntable, colors=False, frames_per_call=16, view=0, spin=False):
    """A clip of the rig: poses [F,72], shapes [F,10] or [1,10], Rh, Th [F,3] -> device fp32 [F,H,W,3] RGB in 0..1, frame f seen by
    view `view` of `turntable` (a mesh_render.MeshTurntable; with `spin`, by view (view + f) mod n_views).  ONE camera set for the
    clip, from the bounds of all its frames (one read-back), so the body moves in the picture instead of the picture following
    it.  Normals per frame (ops.mesh_vertex_normals), or the rig's vertex colours with `colors`.  The frames are posed in chunks
    of `frames_per_call`, twice (bounds, then pictures): F x P vertices never have to fit at once."""
    from .mesh_render import object_rotation, turntable_cams

    if not isinstance(rig, RiggedMesh):
        raise TypeError("animate draws a RiggedMesh")
    rows = pack_params(poses, shapes, Rh, Th)
    F, n = int(rows.shape[0]), int(frames_per_call)
    if n < 1:
        raise ValueError("frames_per_call must be positive, got %d" % n)
    if not 0 <= int(view) < turntable.n_views:
        raise ValueError("view = %d, the turntable has %d" % (view, turntable.n_views))
    driver, dev = PoseDriver(rig), rig.device
    with driver._on_device():
        faces = rig.faces_device()
        attr = rig.colors_device() if colors else None
        A = torch.from_numpy(object_rotation(turntable.dataset).astype(np.float32)).to(dev)
        lo = torch.full((3,), float("inf"), device=dev)
        hi = -lo
        for a in range(0, F, n):
            turned = driver.vertices(*_chunk(rows, a, n)).reshape(-1, 3) @ A.T
            lo, hi = torch.minimum(lo, turned.amin(0)), torch.maximum(hi, turned.amax(0))
        box = torch.stack([lo, hi]).double().cpu().numpy()
        cams = turntable_cams(box[0], box[1], turntable.H, turntable.W, turntable.dataset, turntable.n_views, turntable.step_deg,
                              turntable.ortho_ratio)
        cams = torch.from_numpy(cams.astype(np.float32)).to(dev)
        out = torch.empty((F, turntable.H, turntable.W, 3), dtype=torch.float32, device=dev)
        scratch = ops.mesh_render_scratch(1, turntable.H, turntable.W, faces.shape[0], dev)
        acc = torch.empty((rig.n_verts, 3), dtype=torch.int32, device=dev)
        normals = torch.empty((rig.n_verts, 3), dtype=torch.float32, device=dev)
        for a in range(0, F, n):
            verts = driver.vertices(*_chunk(rows, a, n))
            for f in range(verts.shape[0]):
                k = (int(view) + a + f) % turntable.n_views if spin else int(view)
                if colors:
                    ops.mesh_render_attr(verts[f], attr, faces, cams[k:k + 1], turntable.H, turntable.W, out=out[a + f:a + f + 1],
                                         scratch=scratch)
                else:
                    ops.mesh_vertex_normals(verts[f], faces, out=normals, scratch=acc)
                    ops.mesh_render(verts[f], normals, faces, cams[k:k + 1], turntable.H, turntable.W, out=out[a + f:a + f + 1],
                                    scratch=scratch)
    return out


def _chunk(rows, a, n):
    r = rows[a:a + n].numpy()
    return r[:, :72], r[:, 72:82], r[:, 82:85], r[:, 85:88]
