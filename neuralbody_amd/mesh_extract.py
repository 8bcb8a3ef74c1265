"""What the two mesh renderers share (`renderer.RendererMesh` over the Neural Body network, `nerf.NerfMeshRenderer` over the
vanilla-NeRF baseline): the density cube of a lattice batch and everything behind the cube: marching cubes, the clean-up of stray
components, the normals, the colour query and the `{"cube", "mesh"}` dict of the reference's mesh renderers.  A renderer supplies its
three field queries as a `FieldQueries`; nothing here knows which network answers them."""
import collections

import torch

from . import ops

PAD = 10  # np.pad(cube, 10): if_mesh_renderer.py:46, volume_mesh_renderer.py:101


class ColoredMesh(collections.namedtuple("ColoredMesh", "vertices triangles rgb_f rgb_u8 wpts viewdir normals")):
    """extract_mesh(colors=True): device tensors; the first two are what it returns without colours."""


class FieldQueries(collections.namedtuple("FieldQueries", "density raw gradient")):
    """The three questions a mesh asks its field, each a callable on device tensors:
    density(wpts [n,3]) -> alpha, n values along one dimension (any shape with one long dimension, any stride);
    raw(wpts [1,V,3], viewdir [1,V,3]) -> raw, V x 4 values (three colour logits and the density);
    gradient(wpts [V,3]) -> d density / d p [V,3]."""


def lattice_axes(batch):
    """The lattice's three axis vectors of a collated batch (batch size 1, like `pts[0]`)."""
    axes = [batch[k] for k in ("axis_x", "axis_y", "axis_z")]
    if any(a.dim() != 2 or a.shape[0] != 1 for a in axes):
        raise ValueError("axis_x / axis_y / axis_z must be [1, n] (test.batch_size 1), got %s" % (
            [tuple(a.shape) for a in axes],))
    return [a[0].contiguous() for a in axes]


def lattice_cube(batch, pad, density):
    """-> DEVICE float32 [X+2*pad, Y+2*pad, Z+2*pad]: `density` at the lattice points flagged `inside`, 0 elsewhere.
    A batch with `pts` is the reference dataset's (multi_view_mesh_dataset.py:142-158).  A batch that carries the lattice's axes
    (`axis_x`, `axis_y`, `axis_z`: neuralbody_amd/mesh_lattice.py) never holds the [X,Y,Z,3] points: nb_lattice_gather -> density ->
    nb_lattice_scatter into the padded cube.  The count pass of the gather runs first (cap 0) and its 8-byte `n_out` is the one
    read-back: it sizes the point list, like `pts[0][inside]` does."""
    if "axis_x" not in batch:
        pts = batch["pts"]
        inside = batch["inside"][0].bool()
        alpha = density(pts[0][inside].contiguous())
        cube = torch.zeros(pts.shape[1:-1], dtype=torch.float32, device=pts.device)
        cube[inside] = alpha.reshape(-1)
        return torch.nn.functional.pad(cube, (pad,) * 6)
    axes = lattice_axes(batch)
    inside = batch["inside"][0]
    inside = (inside if inside.dtype == torch.uint8 else (inside != 0).to(torch.uint8)).contiguous()
    dims = [int(a.shape[0]) for a in axes]
    scratch = ops.lattice_scratch(dims, inside.device)
    total = int(ops.lattice_gather(axes, inside, scratch=scratch)[1].item())
    if total == 0:  # nothing to decode: the zero cube
        return torch.zeros([d + 2 * pad for d in dims], dtype=torch.float32, device=inside.device)
    wpts = torch.empty((total, 3), dtype=torch.float32, device=inside.device)
    lin = torch.empty(total, dtype=torch.int32, device=inside.device)
    ops.lattice_gather(axes, inside, wpts, lin, scratch=scratch)
    return ops.lattice_scatter(density(wpts), lin, dims, pad)


def world_frame(batch, like):
    """(step [3], origin [3]) of the lattice as tensors like `like`: the spacing read from the lattice and wbounds[0]."""
    if "pts" in batch:
        pts = batch["pts"]
        step = torch.stack([pts[0, 1, 0, 0, 0] - pts[0, 0, 0, 0, 0], pts[0, 0, 1, 0, 1] - pts[0, 0, 0, 0, 1],
                            pts[0, 0, 0, 1, 2] - pts[0, 0, 0, 0, 2]]).to(like)
    else:
        step = torch.stack([a[1] - a[0] for a in lattice_axes(batch)]).to(like)
    return step, batch["wbounds"][0, 0].to(like)


def to_world(vertices, batch, pad=PAD):
    """Lattice index units of the padded cube -> world units: (v - pad) * step + wbounds[0] (the two lines the reference
    leaves commented out, if_mesh_renderer.py:49-50, with the step read from the lattice instead of the literal 0.005)."""
    step, origin = world_frame(batch, vertices)
    return (vertices - float(pad)) * step + origin


def mesh_from_cube(batch, cube, iso, field, world=False, components="all", colors=False, normals="faces", pad=PAD):
    """Everything behind the cube: -> DEVICE (vertices [V,3] float32, triangles [T,3] int32) of the iso-surface cube == iso
    (ops.marching_cubes; the cube stays on the device), in index units of the padded cube like PyMCubes', or in world units.
    components: "all", "largest" or a fraction in (0, 1] (ops.mesh_components, mesh_component_select, mesh_compact).
    colors: a `ColoredMesh`: ONE field.raw call at the vertices of the (cleaned) mesh, seen along -normal from outside.
    normals (with colors): "faces", the area-weighted face normals of the WORLD vertices, or "field", -grad / |grad| of
    field.gradient there (nb_normal_composite with every vertex a ray of one sample); a vertex whose gradient is zero or not finite
    keeps its face normal.  `field` is a FieldQueries or a callable that makes one (called only when a query is needed)."""
    if normals not in ("faces", "field"):
        raise ValueError("normals must be 'faces' or 'field', got %r" % (normals,))
    vertices, triangles = ops.marching_cubes(cube.contiguous(), iso)
    if ops.mesh_components_fraction(components) is not None:
        scratch = ops.mesh_clean_scratch(vertices.shape[0], triangles.shape[0], vertices.device)
        label = ops.mesh_components(triangles, vertices.shape[0], scratch=scratch)
        keep, _ = ops.mesh_component_select(label, triangles, components, scratch=scratch)
        vertices, triangles = ops.mesh_compact(vertices, triangles, keep, scratch=scratch)
    if not colors:
        return (to_world(vertices, batch, pad) if world else vertices), triangles
    if not isinstance(field, FieldQueries):
        field = field()
    wverts = to_world(vertices, batch, pad)
    face_normals = ops.mesh_vertex_normals(wverts, triangles)
    if normals == "field" and wverts.shape[0]:
        grad = field.gradient(wverts)
        V = wverts.shape[0]
        unit, _ = ops.normal_composite(torch.arange(V, dtype=torch.int32, device=wverts.device), grad,
                                       torch.ones((V, 1), dtype=torch.float32, device=wverts.device))
        normals = torch.where((unit != 0).any(1, keepdim=True), unit, face_normals).contiguous()
    else:
        normals = face_normals
    step, origin = world_frame(batch, vertices)
    rgb_f, rgb_u8, wpts, viewdir = ops.mesh_vertex_colors(vertices, normals, step.contiguous(), origin.contiguous(), pad, field.raw)
    return ColoredMesh(wverts if world else vertices, triangles, rgb_f, rgb_u8, wpts, viewdir, normals)


def render_mesh(cfg, batch, cube_and_field):
    """if_mesh_renderer.py:26-54 / volume_mesh_renderer.py:84-107 -> {"cube", "mesh"}.  cube_and_field() -> (device cube,
    FieldQueries).  cfg.mesh_components / cfg.mesh_color / cfg.mesh_normals: field (YAML-only keys, absent = off) ask for
    `mesh_from_cube`'s clean-up, vertex colours and field normals (TriMesh.vertex_normals, written as nx ny nz and handed to the
    turntable): with any of them set the mesh is extracted on the device whatever cfg.mesh_backend says (PyMCubes has neither), and
    `mesh` is a mesh.TriMesh, the class that carries vertex_colors.  Otherwise the reference's host post-processing (PyMCubes,
    trimesh) runs wherever PyMCubes imports and cfg.mesh_backend does not say "device"."""
    backend = getattr(cfg, "mesh_backend", "auto")
    if backend not in ("auto", "device"):
        raise ValueError("mesh_backend must be 'auto' or 'device', got %r" % (backend,))
    components, colors = getattr(cfg, "mesh_components", "all"), bool(getattr(cfg, "mesh_color", False))
    normals = str(getattr(cfg, "mesh_normals", "faces"))
    if ops.mesh_components_fraction(components) is not None or colors or normals == "field":
        from .mesh import TriMesh

        cube_dev, field = cube_and_field()
        # (the field normals come with the colour query: the colour head is asked along them; the colours are kept only if asked for)
        mesh = mesh_from_cube(batch, cube_dev, cfg.mesh_th, field, components=components, colors=colors or normals == "field",
                              normals=normals)
        cube = cube_dev.double().cpu().numpy()
        return {"cube": cube, "mesh": TriMesh(mesh[0].double().cpu().numpy(), mesh[1].cpu().numpy(),
                                              vertex_colors=mesh.rgb_u8.cpu().numpy() if colors else None,
                                              vertex_normals=mesh.normals.cpu().numpy() if normals == "field" else None)}
    mcubes = None
    if backend == "auto":
        try:
            import mcubes  # CPU marching cubes, as in the reference (if_mesh_renderer.py:6,46)
        except ImportError:
            mcubes = None
    if mcubes is not None:
        import trimesh

        cube = cube_and_field()[0].double().cpu().numpy()
        vertices, triangles = mcubes.marching_cubes(cube, cfg.mesh_th)
        return {"cube": cube, "mesh": trimesh.Trimesh(vertices, triangles)}

    cube_dev, field = cube_and_field()
    vertices, triangles = mesh_from_cube(batch, cube_dev, cfg.mesh_th, field)
    cube = cube_dev.double().cpu().numpy()  # the float64 ndarray the reference's evaluator slices
    vertices, triangles = vertices.double().cpu().numpy(), triangles.cpu().numpy()
    try:
        import trimesh
    except ImportError:
        from .mesh import TriMesh

        return {"cube": cube, "mesh": TriMesh(vertices, triangles)}
    return {"cube": cube, "mesh": trimesh.Trimesh(vertices, triangles)}
