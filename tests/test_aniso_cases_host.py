"""The anisotropic scene of tests/aniso_cases.py discriminates: the oracle, given the same batch, renders another picture when it
reads voxel_size in the reverse order -- by far more than the tolerance the device is held to.  CPU only."""
import numpy as np

from tests import aniso_cases as ac
from tests import helpers as H


def test_reversed_voxel_size_is_another_picture():
    s = ac.scene()
    assert tuple(ac.ANISO) == (0.004, 0.005, 0.008) and len(set(s["out_sh"])) == 3
    assert np.array_equal(s["batch"]["out_sh"][0], s["out_sh"]) and int(s["batch"]["coord"].max()) < max(s["out_sh"])
    right, wrong = ac.oracle_render(ac.ANISO), ac.oracle_render(ac.ANISO[::-1])
    d = float(np.abs(right["rgb_map"] - wrong["rgb_map"]).max())
    print("out_sh %s: max |rgb(ANISO) - rgb(reversed)| = %.3e = %.0f x RGB_TOL over %d rays" % (
        s["out_sh"], d, d / H.RGB_TOL, right["rgb_map"].shape[1]))
    assert float(right["rgb_map"].max()) > 0.01 and float(right["acc_map"].max()) > 0.01
    assert d >= 100.0 * H.RGB_TOL
