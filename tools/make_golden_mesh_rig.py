"""Writes tests/golden/mesh_rig.npz: what the reference's own ppts_to_pts (lib/utils/blend_utils.py:73-82, torch, float32) returns
for the inputs of tests/mesh_rig_ref.py::fixture_case.  The function is imported from a checkout of zju3dv/neuralbody at run time:

    python tools/make_golden_mesh_rig.py --reference /path/to/neuralbody

The fixture holds the inputs beside the output, so the host suite can tell when fixture_case has drifted from what was recorded."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mesh_rig_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of zju3dv/neuralbody")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mesh_rig.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_blend_utils", os.path.join(args.reference, "lib", "utils", "blend_utils.py"))
    blend_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(blend_utils)
    y, w, A = ref.fixture_case()
    with torch.no_grad():
        out = blend_utils.ppts_to_pts(torch.from_numpy(y)[None], torch.from_numpy(np.ascontiguousarray(w.T))[None], torch.from_numpy(A)[None])
    out = out[0].numpy()
    assert out.dtype == np.float32 and out.shape == y.shape
    np.savez(args.out, y=y, w=w, A=A, pts=out)
    print("%s: %d points, %d bytes" % (args.out, y.shape[0], os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
