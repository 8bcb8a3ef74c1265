"""Inputs shared by tests/test_image_prep_host.py and tests/test_gpu_image_prep.py: cameras and distortion vectors, byte images,
label images of the three hand-checkable shapes, and a small ZJU-MoCap-shaped tree written with PIL and numpy (annots.npy,
PNG images, mask_cihp/, vertices/, params/).  Everything is generated from seeds; nothing here touches a device."""
import functools
import math
import os

import numpy as np

from tests import image_prep_ref as R
from tests import synthetic as syn

# 40 x 52 and 37 x 53 frames: principal point off the centre and off the pixel grid
K_40x52 = np.array([[60.0, 0.0, 25.3], [0.0, 58.0, 19.6], [0.0, 0.0, 1.0]])
K_37x53 = np.array([[71.5, 0.0, 27.9], [0.0, 69.0, 17.2], [0.0, 0.0, 1.0]])
# the strong pincushion pushes the source of the outer pixels off the image: at 40 x 52 with K_40x52, 27 % of the pixels have a
# tap outside and 22 % have all four outside (tests/test_image_prep_host.py asserts >= 5 % and >= 1 % on the CPU)
DISTORTIONS = {
    "strong5": np.array([0.9, 0.6, 0.02, -0.015, 0.3]),
    "rational8": np.array([-0.35, 0.12, 0.002, -0.001, 0.0, 0.05, -0.02, 0.01]),
    "zero": np.zeros(5),
}
# every source position inside the image (a barrel that pulls the samples towards the centre, integer principal point)
K_INWARD, D_INWARD = np.array([[60.0, 0.0, 26.0], [0.0, 58.0, 20.0], [0.0, 0.0, 1.0]]), np.array([-0.3, 0.0, 0.0, 0.0])


def cam(K, name):
    return R.camera_constants(K, DISTORTIONS[name])


def byte_image(H, W, seed):
    """A smooth ramp plus noise, every byte value present: uint8 [H,W,3]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([(5 * xx + 3 * yy) % 256, (7 * yy + 250 - 2 * xx) % 256, rng.randint(0, 256, (H, W))], axis=-1)
    img[0, 0], img[-1, -1] = 255, 0
    return np.ascontiguousarray(img.astype(np.uint8))


def byte_mask(H, W, seed):
    """A get_mask-like plane (0 / 1 with a band of 100) with a patch of arbitrary bytes, 255 included: uint8 [H,W]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    label = (((yy - 0.45 * H) / (0.38 * H)) ** 2 + ((xx - 0.55 * W) / (0.3 * W)) ** 2 < 1.0).astype(np.uint8)
    m = R.band(label[None], 5)[0]
    m[2:7, 3:11] = rng.randint(0, 256, (5, 8))
    m[3, 4] = 255
    return m


def band_labels(H=19, W=23):
    """[3,H,W] uint8: a body touching the top and the left border (labels 1..19, as CIHP numbers its parts), all zero, all one."""
    lab = np.zeros((3, H, W), np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lab[0] = np.where((yy < 11) & (xx < 9) | (yy + xx < 14), 1 + (yy * 3 + xx) % 19, 0)
    lab[0, 15, 20] = 7  # a lone pixel
    lab[2] = 1
    return lab


# ------------------------------------------------------------------------------------------- a tree on disk
TREE = dict(H=64, W=64, ratio=0.5, n_frames=2, n_cams=3, training_view=[0, 1], mask_bkgd=True, white_bkgd=False)


@functools.lru_cache(maxsize=None)
def tree_content():
    """The arrays of the tree, made once: per frame a body (vertices, Rh, Th), per camera K, D, R, T (T in millimetres, as
    annots.npy keeps it), per (frame, camera) an RGB byte image and a label image whose non-zero pixels are the projected,
    dilated vertices."""
    from scipy import ndimage

    H, W, nf, nc = TREE["H"], TREE["W"], TREE["n_frames"], TREE["n_cams"]
    bodies = [syn.make_body(seed=11 + f, rh=(0.1, 0.2 + 0.1 * f, 0.05), th=(0.02 * f, 0.0, 0.01), n_verts=400) for f in range(nf)]
    cams = {"K": [], "D": [], "R": [], "T": []}
    for c in range(nc):
        K, Rm, T = syn.make_camera(bodies[0], H, W, focal_factor=1.1, distance=2.4, yaw=0.4 + 2 * math.pi * c / nc,
                                   pitch=0.05 * (c % 2))
        K[0, 2] += 0.37 * (c + 1)
        K[1, 2] -= 0.21 * (c + 1)
        D = np.array([[-0.12 - 0.02 * c], [0.06], [0.0015 * (c + 1)], [-0.001], [0.01 * c]])  # [5,1], as the dataset stores it
        cams["K"].append(K)
        cams["D"].append(D)
        cams["R"].append(Rm)
        cams["T"].append(T * 1000.0)
    images, labels = {}, {}
    for f in range(nf):
        for c in range(nc):
            cam_pts = bodies[f]["world_verts"].astype(np.float64) @ cams["R"][c].T + cams["T"][c].ravel() / 1000.0
            uv = cam_pts @ cams["K"][c].T
            px = np.round(uv[:, :2] / uv[:, 2:]).astype(np.int64)
            ok = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
            m = np.zeros((H, W), bool)
            m[px[ok, 1], px[ok, 0]] = True
            m = ndimage.binary_dilation(m, structure=np.ones((5, 5), bool))
            yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            labels[f, c] = np.where(m, 1 + (yy // 8 + xx // 8) % 19, 0).astype(np.uint8)
            images[f, c] = byte_image(H, W, 100 + 10 * f + c)
    return dict(bodies=bodies, cams=cams, images=images, labels=labels)


def im_name(f, c):
    return "Camera_B%d/%06d.png" % (c + 1, f)


def write_tree(root):
    """Write the tree under `root` -> the path of annots.npy."""
    from PIL import Image

    t = tree_content()
    nf, nc = TREE["n_frames"], TREE["n_cams"]
    for d in ("vertices", "params"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for f in range(nf):
        b = t["bodies"][f]
        np.save(os.path.join(root, "vertices", "%d.npy" % f), b["world_verts"])
        np.save(os.path.join(root, "params", "%d.npy" % f), {"Rh": _rh(f), "Th": b["Th"]}, allow_pickle=True)
        for c in range(nc):
            for sub, arr in (("", t["images"][f, c]), ("mask_cihp", t["labels"][f, c])):
                path = os.path.join(root, sub, im_name(f, c))
                os.makedirs(os.path.dirname(path), exist_ok=True)
                Image.fromarray(arr).save(path)
    annots = {"cams": t["cams"], "ims": [{"ims": [im_name(f, c) for c in range(nc)]} for f in range(nf)]}
    ann_file = os.path.join(root, "annots.npy")
    np.save(ann_file, annots, allow_pickle=True)
    return ann_file


def _rh(f):
    return np.array([[0.1, 0.2 + 0.1 * f, 0.05]], np.float32)


def frame_items(split):
    """The tuples LightStageFrameSource.load returns for the tree, prepared with the numpy reference: the item list of
    multi_view_dataset.py:22-50 (frame-major over the split's views)."""
    t = tree_content()
    n = int(round(1.0 / TREE["ratio"]))
    views = TREE["training_view"] if split == "train" else [c for c in range(TREE["n_cams"]) if c not in TREE["training_view"]]
    fill = ("white" if TREE["white_bkgd"] else "black") if TREE["mask_bkgd"] else None
    items = []
    for f in range(TREE["n_frames"]):
        for c in views:
            K = np.array(t["cams"]["K"][c])
            msk = R.band(t["labels"][f, c][None], 5)[0]
            img, msk = R.frame(t["images"][f, c], msk, R.camera_constants(K, t["cams"]["D"][c]), n, fill)
            K[:2] = K[:2] * TREE["ratio"]
            b = t["bodies"][f]
            items.append((img, msk, K, np.array(t["cams"]["R"][c]), np.array(t["cams"]["T"][c]) / 1000.0, f, c, b["world_verts"],
                          _rh(f), b["Th"]))
    return items


def mesh_items():
    """(items, Ks, Rs, Ts) of a MemoryMeshSource for the tree: every view's (label != 0) undistorted by the numpy reference with
    the float32 cameras LightStageMeshSource keeps."""
    t = tree_content()
    nc = TREE["n_cams"]
    Ks = np.array(t["cams"]["K"]).astype(np.float32)
    Ds = np.array(t["cams"]["D"]).astype(np.float32)
    Rs = np.array(t["cams"]["R"]).astype(np.float32)
    Ts = np.array(t["cams"]["T"]).astype(np.float32) / 1000.0
    items = []
    for f in range(TREE["n_frames"]):
        msks = np.stack([R.undistort_u8((t["labels"][f, c] != 0).astype(np.uint8), R.camera_constants(Ks[c], Ds[c]))
                         for c in range(nc)])
        b = t["bodies"][f]
        items.append((msks, b["world_verts"], _rh(f), b["Th"]))
    return items, Ks, Rs, Ts
