"""Generate tests/golden/smpl_pose.npz by running the UNMODIFIED reference SMPL layer (zju_smpl/smplmodel/body_model.py::SMPLlayer
over zju_smpl/smplmodel/lbs.py, CPU torch, float32) on the seeded synthetic models of tests/smpl_ref.py.  Run from the repo root,
where the reference tree exists:
    python tests/golden/make_golden_smpl.py

Each model is written to a temporary pickle, which SMPLlayer loads as it would the SMPL file.  The fixture holds, per case of
smpl_ref.CASES: the parameters, the reference's float32 world vertices, the float64 checksums of the model's arrays (the models
are regenerated from their seeds by the tests, posedirs alone is 17 MB) and E_ref = max |reference float32 - float64 restatement|.
It also checks what the voxelisation tests need of these vertices: every raw extent at least 2 voxels from a multiple of 32, and
at most 1 % of the coordinates in the rounding band.  Data only."""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_harness import REF_ROOT  # noqa: E402
from tests import smpl_ref as sr  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smpl_pose.npz")


def main():
    sys.path.insert(0, os.path.join(REF_ROOT, "zju_smpl"))
    from smplmodel.body_model import SMPLlayer  # the reference's module, unmodified

    out = {"cases": np.array(sorted(sr.CASES))}
    layers = {}
    for name in sorted(sr.CASES):
        seed, V, tree, new_params, pseed, zero = sr.CASES[name]
        model = sr.case_model(name)
        if (seed, V) not in layers:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "model.pkl")
                with open(path, "wb") as f:
                    pickle.dump(model, f)
                layers[(seed, V)] = SMPLlayer(path, device=torch.device("cpu"))
        poses, shapes, Rh, Th = sr.case_params(name)
        with torch.no_grad():
            verts = layers[(seed, V)](poses[None], shapes[None], Rh=Rh[None], Th=Th[None], return_verts=True, return_tensor=True,
                                      new_params=new_params)
        verts = verts.numpy()
        assert verts.dtype == np.float32 and verts.shape == (V, 3)
        ref64 = sr.forward(model, poses, shapes, Rh, Th, new_params, np.float64)
        e_ref = float(np.abs(verts.astype(np.float64) - ref64).max())
        ext = np.ptp(verts, axis=0)
        print("%-14s V %5d new_params %d  E_ref %.3e  extent %s" % (name, V, new_params, e_ref, np.round(ext, 3)))
        assert e_ref < 2e-6 and ext.max() < 2.6, "the restatement does not follow the reference, or the body left its box"
        for k, v in (("poses", poses), ("shapes", shapes), ("Rh", Rh), ("Th", Th), ("verts", verts),
                     ("checksums", sr.checksums(model)), ("E_ref", np.float64(e_ref)), ("new_params", np.bool_(new_params)),
                     ("parents", np.array(sr.parents_of(model), np.int32))):
            out["%s/%s" % (name, k)] = v
    for name, pad in sr.VOXEL_CASES:
        info = sr.voxel_case_check(out["%s/verts" % name], out["%s/Rh" % name], out["%s/Th" % name], pad)
        print("%-14s %-8s raw extents %s (mod 32: %s), band %.3f %%" % (name, pad, info["raw"], info["raw"] % 32, 100 * info["band"]))
        assert info["ok"], "pick other parameters: an extent within 2 voxels of a multiple of 32, or the band above 1 %"
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
