"""Runs one GEMM case of tests/bwd_cases.py on the device and compares it with its float64 reference; shared by
tests/test_gpu_backward_kernels.py and the NB_BWD_SPLIT=0 child (`python -m tests.bwd_device`, one fresh process: the switch is read
once per process).  Everything goes through ops.sgemm / ops.gemm_variant."""
import json
import sys

import numpy as np
import torch

from tests import bwd_cases as bc
from tests import spconv_cases as sc

DEV = "cuda:0"
LEFT = 3  # guard columns in front of a destination slice (the slice itself is off the 16-byte grid: the kernels store scalars)


def dev(x):
    x = np.ascontiguousarray(x)
    if x.size == 0:  # numpy gives an empty array zero strides; the wrappers want a row stride
        return torch.zeros(x.shape, dtype=torch.from_numpy(x).dtype, device=DEV)
    return torch.from_numpy(x).to(DEV)


def same_numbers(got, ref64):
    """got (fp32) equals the float64 reference element for element; the reference is an fp32 number (the lattice's promise)"""
    ref32 = ref64.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref64), "the reference is not an fp32 number: the case is no lattice case"
    return bool(np.array_equal(got, ref32))  # a NaN anywhere is a difference


def prepare(case, lattice, rs, remainders="both", arithmetic=None):
    """operands on the host and the device, the float64 product of the arithmetic the kernel is to use, sum |a| |b|; an integer C0
    and the ReLU mask's values, which the launches of this case share"""
    variant, ta, tb, m, k, n, (oa, ob) = case
    a, b = bc.operands(case, lattice, rs, remainders)
    prod, S = bc.product(case, a, b, arithmetic or bc.arithmetic_of(variant))
    A, B = dev(bc.widen(a.x, oa, fill=np.nan)), dev(bc.widen(b.x, ob, fill=np.nan))  # NaN beside the operands: nothing may read them in
    prep = {"case": case, "lattice": lattice, "prod": prod, "S": S, "a": A[:, oa:oa + a.x.shape[1]], "b": B[:, ob:ob + b.x.shape[1]],
            "c0": sc.lattice32(rs, (m, n))}
    if not ta:
        prep["y"] = bc.mask_values(rs, (m, n))
        prep["y_dev"] = dev(bc.widen(prep["y"], 5))[:, 5:5 + n]
    return prep


def run(prep, rs, alpha=1.0, beta=0.0, mask=False, colsum=False, expect=None):
    """one launch -> dict(variant, exact, guards, colsum_exact / colsum_ratio).  beta = 0 runs over a destination filled with NaN,
    beta = 1 over integers; the destination is a slice between guard columns; the column sums start from integers where they are
    compared bit for bit and from zero where they are held to bc.colsum_bound."""
    from neuralbody_amd import ops

    variant, ta, tb, m, k, n, _ = prep["case"]
    lattice, c0 = prep["lattice"], prep["c0"]
    y = prep["y"] if mask else None
    C, cs, Sout = bc.epilogue(prep["prod"], prep["S"], alpha, beta, c0, y)
    bc.assert_case_lattice(prep["S"], Sout, lattice, alpha)
    got_variant = ops.gemm_variant(prep["a"], prep["b"], trans_a=ta, trans_b=tb)
    res = {"case": list(prep["case"][:6]), "lattice": lattice, "variant": got_variant}
    if expect is not None:
        assert got_variant == expect, "%s runs on %s, the case is meant for %s" % (prep["case"], got_variant, expect)
    wide = dev(bc.widen(c0 if beta else np.full((m, n), np.nan, np.float32), LEFT, fill=bc.GUARD))
    out = wide[:, LEFT:LEFT + n]
    exact_cs = colsum and bc.colsum_exact(Sout + 3.0 / max(m, 1), bc.UNIT[lattice] * alpha)
    assert exact_cs or not colsum or lattice != "int", "integer column sums are always compared bit for bit"
    cs0 = sc.lattice32(rs, (n,)) if exact_cs else np.zeros(n, np.float32)
    csd = dev(cs0) if colsum else None
    ops.sgemm(prep["a"], prep["b"], trans_a=ta, trans_b=tb, out=out, alpha=alpha, beta=beta, relu_mask=prep["y_dev"] if mask else None,
              colsum=csd)
    got = wide.cpu().numpy()
    res["guards"] = bool(np.all(got[:, :LEFT] == np.float32(bc.GUARD)) and np.all(got[:, LEFT + n:] == np.float32(bc.GUARD)))
    res["exact"] = same_numbers(got[:, LEFT:LEFT + n], C)
    if not res["exact"]:
        bad = got[:, LEFT:LEFT + n] != C.astype(np.float32)
        res["n_wrong"] = int(bad.sum())
        res["max_diff"] = float(np.nanmax(np.abs(got[:, LEFT:LEFT + n].astype(np.float64) - C))) if bad.any() else 0.0
    if colsum:
        got_cs = csd.cpu().numpy()
        if exact_cs:
            res["colsum_exact"] = same_numbers(got_cs, cs0.astype(np.float64) + cs)
        else:
            bound = bc.colsum_bound(C)
            err = np.abs(got_cs.astype(np.float64) - cs)
            assert np.all(got_cs[bound == 0] == 0)
            res["colsum_ratio"] = float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))
    return res


def main():
    """the NB_BWD_SPLIT=0 child: the large shapes on the fp32 kernels, against the FULL product; one JSON line per launch"""
    from neuralbody_amd import build

    build.build(verbose=False)
    rs = np.random.RandomState(77)
    for i, case in enumerate(bc.split_off_cases()):
        for lattice in ("sparse", "int"):
            prep = prepare(case, lattice, rs, arithmetic="fp32")
            if case[1]:
                res = run(prep, rs, alpha=0.5, beta=1.0)
            else:
                res = run(prep, rs, alpha=1.0, beta=float(i % 2), mask=True, colsum=True)
            print(json.dumps(res))
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
