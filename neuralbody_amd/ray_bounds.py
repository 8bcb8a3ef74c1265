"""Ray bounds from the posed body: the rays of a rendered view cut to the body's own depth range instead of its box's.

nb_raygen keeps every pixel whose ray meets the SMPL bounding box and spreads N_samples between the box's entry and exit; the body
fills a small part of that box.  The posed triangles are on the device already (nb_smpl_pose), so for the camera that is rendered

    nb_body_depth_range   per pixel the camera-depth interval of the triangles that cover it (the silhouette's exact rasteriser)
    nb_depth_range_widen  a clothing margin in pixels and one interval per tile x tile block
    nb_raygen_body        nb_raygen with near / far cut to the interval -+ the margin in metres; rays left without one dropped

in front of the march, which is untouched: `near`, `far` and the ray list are its inputs.  get_rays does not
normalise ray_d, so with K's last row (0, 0, 1) a ray's parameter is its camera depth and the interval cuts [near, far] directly.
"""
import numpy as np
import torch

from . import ops
from .smpl_pose import cull_border


class BodyBounds:
    """`margin`: metres around the body's surface that stay inside the bounds (clothing, hair), in depth and, through
    smpl_pose.cull_border, in pixels; `tile`: the side of the pixel blocks that share one interval (1, 2, 4, 8 or 16; 8 is the
    march's ray tile)."""

    def __init__(self, margin=0.05, tile=8):
        self.margin, self.tile = float(margin), int(tile)
        if not 0.0 <= self.margin < float("inf"):
            raise ValueError("margin = %r m must be a finite length >= 0" % (margin,))
        if self.tile not in (1, 2, 4, 8, 16):
            raise ValueError("tile must be 1, 2, 4, 8 or 16, got %r" % (tile,))

    def depth_range(self, H, W, K, RT, can_bounds, verts, faces):
        """The widened range of one view, device fp32 [H,W,2].  verts: device fp32 [1,V,3] or [V,3] world vertices of any triangle
        mesh (the posed SMPL body, or a RiggedMesh's posed vertices for clothed bounds), faces: device int32 [Nf,3]."""
        K, RT = np.asarray(K, np.float64).reshape(3, 3), np.asarray(RT, np.float64)[:3]
        border = cull_border(can_bounds, K[None], RT[None], self.margin)  # raises like the cull masks' margin
        verts = verts if verts.dim() == 3 else verts[None]
        if verts.shape[0] != 1:
            raise ValueError("verts must hold one frame ([1,V,3] or [V,3]), got %s" % (tuple(verts.shape),))
        cam = torch.from_numpy(np.concatenate([RT.reshape(-1), K.reshape(-1)]).astype(np.float32))
        cam = (cam.pin_memory() if verts.is_cuda else cam).to(verts.device, non_blocking=True)
        raw = ops.body_depth_range(verts, faces, cam[:12].view(1, 3, 4), cam[12:].view(1, 3, 3), H, W)
        return ops.depth_range_widen(raw[0, 0], border, self.tile)

    def rays(self, H, W, K, RT, can_bounds, verts, faces, device=None):
        """-> ops.raygen's 6-tuple (ray_o, ray_d, near, far, mask_at_box, n_rays[1]) of the view, bounded by the body.  Three entries,
        nothing read back.  `device`: where verts and faces live (checked when given)."""
        if device is not None and torch.device(device) != verts.device:
            raise ValueError("verts live on %s, not on %s" % (verts.device, device))
        RT = np.asarray(RT, np.float64)
        rng = self.depth_range(H, W, K, RT, can_bounds, verts, faces)
        return ops.raygen_body(H, W, K, RT[:3, :3], RT[:3, 3], can_bounds, rng, self.margin)
