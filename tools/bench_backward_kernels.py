"""Times the seven backward matrix kernels (csrc/nb_backward.hip: the six kernels behind nb_gemm_fused; csrc/nb_encoder_bwd.hip: the two
weight-gradient kernels of the sparse convolution) at the shapes one training step of `bench.py --mode train` gives them, for TWO
builds of the library — a parent commit's and the working tree's — and writes profiles/backward_tile_refactor.json.

    python tools/bench_backward_kernels.py --build-parent [REV]    # anywhere with git: lib/libnb_hip_parent.so from REV (default HEAD~1)
    python tools/bench_backward_kernels.py [--rounds 3] [--reps 30] [--out profiles/backward_tile_refactor.json]     # on an MI355X

The shapes are read, not guessed: a worker runs one step of bench.train_bench with ops.sgemm and ops.enc_conv_bwd_weight wrapped,
groups the products by ops.gemm_variant and replays each distinct one (same sizes, row strides, 16-byte alignment and epilogue) on
random operands; the weight gradients run on the tensors of every encoder layer of that step, each layer on both kernels its channel
count allows.  gemm_rows_fast_kernel<false> is reached by the step only with one row; a second worker under NB_BWD_SPLIT=0 times it
at the shapes the default dispatch gives to gemm_rows16_kernel.  Parent and branch alternate, `--rounds` rounds each, one fresh
process per library (NB_LIB_PATH), round and switch setting, each under its own `timeout`; the first process that fails ends the run.
HIP events per call after 3 warm-up calls (event_ms of tools/bench_mesh.py).

Condition, per kernel and shape (the one of profiles/raster_window_refactor.json): the mean of the branch's round means is at most
the mean of the parent's round means plus the spread (max - min) of the parent's round means.

Byte equality between the two libraries: C of the gemm_rows* kernels on the random operands (no atomics touch it); on exact-lattice
operands (tests/bwd_cases.py; integers on the encoder layers) every output, the atomically accumulated ones included — there every
partial sum is exact, so the order of the atomics cannot show.  The step time of `bench.py --mode train` is recorded for both
libraries, alternating, `--rounds` runs each, and held to the same condition.

The lattice operands and the device helpers are those of the test suite (tests/bwd_cases.py, tests/bwd_device.py,
tests/spconv_cases.py): this tool needs the repository's tests/ beside it.  Exit status 1 when any kernel misses the condition, so
that a chain of steps ends there.

The record names the tree it measured by `library_source_sha256`, the build stamp's digest (neuralbody_amd/build.py: sources, their
paths and the flags) as computed on the measuring machine, and by `head` / `parent` as given on the command line.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_mesh import _head, event_ms  # noqa: E402

LIB_DIR = os.path.join(ROOT, "neuralbody_amd", "lib")
PARENT_LIB = os.path.join(LIB_DIR, "libnb_hip_parent.so")
BRANCH_LIB = os.path.join(LIB_DIR, "libnb_hip.so")
KERNEL_OF = {"TN": "gemm_tn_kernel", "TN16": "gemm_tn16_kernel", "ROWS": "gemm_rows_kernel", "ROWS_FAST": "gemm_rows_fast_kernel<false>",
             "ROWS_FAST_T": "gemm_rows_fast_kernel<true>", "ROWS16": "gemm_rows16_kernel"}
GEMM_FIELDS = ("trans_a", "trans_b", "m", "n", "k", "lda", "ldb", "ldc", "a_off", "b_off", "c_off", "ldy", "y_off", "mask", "colsum", "alpha", "beta")
STEP_TIMEOUT = 300  # seconds, per child process


# ----------------------------------------------------------------------------------------------------------------- the parent's library
def build_parent(rev):
    """the sources of `rev` in a scratch directory, built there by that commit's own build.py under NB_LIB_SUFFIX=_parent"""
    os.makedirs(LIB_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.check_output(["git", "archive", rev, "neuralbody_amd/csrc", "neuralbody_amd/build.py", "include"], cwd=ROOT)
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        subprocess.check_call([sys.executable, os.path.join(d, "neuralbody_amd", "build.py")], cwd=d, env=dict(os.environ, NB_LIB_SUFFIX="_parent"),
                              stdout=subprocess.DEVNULL)
        shutil.copyfile(os.path.join(d, "neuralbody_amd", "lib", "libnb_hip_parent.so"), PARENT_LIB)
    print("built %s from %s" % (PARENT_LIB, subprocess.check_output(["git", "rev-parse", "--short", rev], cwd=ROOT).decode().strip()))


# ----------------------------------------------------------------------------------------------------------------- one recorded step
def _off(t):
    return (t.data_ptr() % 16) // 4  # floats off the 16-byte grid


def record_step(dev):
    """one step of bench.train_bench -> (the distinct GEMMs as dicts of GEMM_FIELDS + variant, the weight-gradient calls with their tensors)"""
    import bench
    from neuralbody_amd import ops

    gemms, convs = {}, []
    sgemm, conv_w = ops.sgemm, ops.enc_conv_bwd_weight

    def rec_sgemm(a, b, trans_a=False, trans_b=False, out=None, alpha=1.0, beta=0.0, relu_mask=None, colsum=None):
        res = sgemm(a, b, trans_a=trans_a, trans_b=trans_b, out=out, alpha=alpha, beta=beta, relu_mask=relu_mask, colsum=colsum)
        m, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
        g = dict(trans_a=bool(trans_a), trans_b=bool(trans_b), m=int(m), n=int(res.shape[1]), k=int(k), lda=int(a.stride(0)), ldb=int(b.stride(0)),
                 ldc=int(res.stride(0)), a_off=_off(a), b_off=_off(b), c_off=_off(res), ldy=int(relu_mask.stride(0)) if relu_mask is not None else 0,
                 y_off=_off(relu_mask) if relu_mask is not None else 0, mask=relu_mask is not None, colsum=colsum is not None,
                 alpha=float(alpha), beta=float(beta) if out is not None else 0.0)
        g["variant"] = ops.gemm_variant(a, b, trans_a=trans_a, trans_b=trans_b)
        gemms.setdefault(tuple(g[f] for f in GEMM_FIELDS), g)
        return res

    def rec_conv(in_rows, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, dx, cin, cout, dx_split=None, out=None, rulebook=None):
        convs.append(dict(in_rows=in_rows.clone(), in_grid=in_grid, in_dhw=tuple(int(v) for v in in_dhw), out_lin=out_lin, n_out=n_out,
                          n_out_max=int(n_out_max), out_dhw=tuple(int(v) for v in out_dhw), stride=int(stride), dx=dx.clone(), cin=int(cin),
                          cout=int(cout), dx_split=None if dx_split is None else dx_split.clone()))
        return conv_w(in_rows, in_grid, in_dhw, out_lin, n_out, n_out_max, out_dhw, stride, dx, cin, cout, dx_split=dx_split, out=out,
                      rulebook=rulebook)

    ops.sgemm, ops.enc_conv_bwd_weight = rec_sgemm, rec_conv
    try:
        bench.train_bench(argparse.Namespace(size=512, samples=64, warmup=0, steps=1), dev)
    finally:
        ops.sgemm, ops.enc_conv_bwd_weight = sgemm, conv_w
    return list(gemms.values()), convs


# ----------------------------------------------------------------------------------------------------------------- replay
def _strided(rows, cols, ld, off, gen, dev):
    """a [rows, cols] matrix of normals of row stride ld whose first element lies `off` floats off a 64-byte boundary"""
    import torch

    flat = torch.randn(rows * max(ld, cols) + off + 4, generator=gen).to(dev)
    return torch.as_strided(flat, (rows, cols), (ld, 1), off)


def gemm_key(g):
    return "%s %s m=%d n=%d k=%d%s%s%s%s" % (KERNEL_OF[g["variant"]], "A^T.B" if g["trans_a"] else ("A.B^T" if g["trans_b"] else "A.B"), g["m"], g["n"],
                                               g["k"], " mask" if g["mask"] else "", " colsum" if g["colsum"] else "",
                                               " beta=%g" % g["beta"] if g["beta"] else "", " ld=%d,%d,%d" % (g["lda"], g["ldb"], g["ldc"]))


def replay_gemm(g, reps, dev):
    """-> (timing, sha256 of C after one call from a fixed destination — meaningful for the gemm_rows* kernels only)"""
    import torch
    from neuralbody_amd import ops

    gen = torch.Generator().manual_seed(1234)
    sa = (g["k"], g["m"]) if g["trans_a"] else (g["m"], g["k"])
    sb = (g["n"], g["k"]) if g["trans_b"] else (g["k"], g["n"])
    a, b = _strided(sa[0], sa[1], g["lda"], g["a_off"], gen, dev), _strided(sb[0], sb[1], g["ldb"], g["b_off"], gen, dev)
    c = _strided(g["m"], g["n"], g["ldc"], g["c_off"], gen, dev)
    y = _strided(g["m"], g["n"], g["ldy"], g["y_off"], gen, dev) if g["mask"] else None
    cs = torch.zeros(g["n"], device=dev) if g["colsum"] else None
    c0 = c.clone()

    def call():
        ops.sgemm(a, b, trans_a=g["trans_a"], trans_b=g["trans_b"], out=c, alpha=g["alpha"], beta=g["beta"], relu_mask=y, colsum=cs)

    assert ops.gemm_variant(a, b, trans_a=g["trans_a"], trans_b=g["trans_b"]) == g["variant"], g
    call()
    digest = hashlib.sha256(c.cpu().numpy().tobytes()).hexdigest()
    c.copy_(c0)
    return event_ms(call, reps, warmup=3), digest


def conv_key(kernel, cv):
    return "%s %d->%d stride %d rows<=%d" % (kernel, cv["cin"], cv["cout"], cv["stride"], cv["n_out_max"])


def replay_convs(convs, reps, lattice):
    """every distinct layer on conv_bwd_w_kernel and, for C_in >= 32, on conv_bwd_w16_kernel -> (timings, sha256 of dW on integer operands)"""
    import torch
    from neuralbody_amd import ops
    from tests import spconv_cases as sc

    times, digests, seen = {}, {}, set()
    for cv in convs:
        ident = (cv["cin"], cv["cout"], cv["stride"], cv["n_out_max"])
        if ident in seen:
            continue
        seen.add(ident)
        geo = (cv["in_grid"], cv["in_dhw"], cv["out_lin"], cv["n_out"], cv["n_out_max"], cv["out_dhw"], cv["stride"])
        cache = []
        ops.enc_conv_bwd_weight(cv["in_rows"], *geo, cv["dx"], cv["cin"], cv["cout"], rulebook=cache)  # fills the neighbour table
        planes = cv["dx_split"]
        if planes is None and cv["cin"] >= 32:
            planes = sc.split_planes(cv["dx"].cpu().numpy(), "bf16", cap=cv["dx"].shape[0]).to(cv["dx"].device)
        for kernel, split in (("conv_bwd_w_kernel", None), ("conv_bwd_w16_kernel", planes)):
            if kernel == "conv_bwd_w16_kernel" and cv["cin"] < 32:
                continue
            times[conv_key(kernel, cv)] = event_ms(lambda: ops.enc_conv_bwd_weight(cv["in_rows"], *geo, cv["dx"], cv["cin"], cv["cout"], dx_split=split,
                                                                                   rulebook=cache), reps, warmup=3)
            if lattice:  # integers -3 .. 3: bf16 numbers, and 9 x rows < 2^24, so every sum is exact on both kernels
                rs = np.random.RandomState(cv["cin"] + 2 * cv["cout"] + cv["stride"])
                ai, dxi = sc.lattice32(rs, tuple(cv["in_rows"].shape)), sc.lattice32(rs, tuple(cv["dx"].shape))
                dev = cv["dx"].device
                pl = None if split is None else sc.split_planes(dxi, "bf16").to(dev)
                dw = ops.enc_conv_bwd_weight(torch.from_numpy(ai).to(dev), *geo, torch.from_numpy(dxi).to(dev), cv["cin"], cv["cout"], dx_split=pl,
                                             rulebook=cache)
                digests[conv_key(kernel, cv)] = hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest()
    return times, digests


def lattice_gemm_digests(dev):
    """sha256 of the whole destination (guard columns included) and, on the integer lattice, of the column sums, for cases of
    tests/bwd_cases.py on both sides of every launch boundary of every variant, with every epilogue"""
    import torch
    from neuralbody_amd import ops
    from tests import bwd_cases as bc
    from tests import bwd_device as bd
    from tests import spconv_cases as sc

    cases = bc.rows_cases() + bc.fast_cases(False, 129) + bc.fast_cases(True, 1023) + bc.rows16_cases(1025) + bc.tn_cases(257) + \
        bc.tn_cases(2049) + bc.tn16_cases(1056) + bc.tn16_cases(3103)
    rs = np.random.RandomState(2025)
    out = {}
    for case in cases:
        variant, ta, tb, m, k, n, (oa, ob) = case
        for lattice in ("int", "sparse") + (("dense",) if bc.arithmetic_of(variant) == "pairs" else ()):
            a, b = bc.operands(case, lattice, rs)
            A, B = bd.dev(bc.widen(a.x, oa))[:, oa:oa + a.x.shape[1]], bd.dev(bc.widen(b.x, ob))[:, ob:ob + b.x.shape[1]]
            assert ops.gemm_variant(A, B, trans_a=ta, trans_b=tb) == variant, case
            c0, y = sc.lattice32(rs, (m, n)), bd.dev(bc.widen(bc.mask_values(rs, (m, n)), 5))[:, 5:5 + n]
            h = hashlib.sha256()
            for name in (("none",) if ta else bc.EPILOGUES):
                mask, colsum, alpha, beta = bc.epilogue_args(name) if not ta else (False, False, 0.5, 1.0)
                wide = bd.dev(bc.widen(c0 if beta else np.full((m, n), np.nan, np.float32), bd.LEFT, fill=bc.GUARD))
                cs = bd.dev(sc.lattice32(rs, (n,))) if colsum else None
                ops.sgemm(A, B, trans_a=ta, trans_b=tb, out=wide[:, bd.LEFT:bd.LEFT + n], alpha=alpha, beta=beta, relu_mask=y if mask else None, colsum=cs)
                h.update(wide.cpu().numpy().tobytes())
                if colsum and lattice == "int":  # (elsewhere the column sums round: the order of the atomics may show)
                    h.update(cs.cpu().numpy().tobytes())
            out["%s %s" % (list(case[:6]), lattice)] = h.hexdigest()
    torch.cuda.synchronize()
    return out


def worker(args):
    import torch
    from neuralbody_amd import ops

    dev = torch.device("cuda:0")
    res = {"lib": os.environ.get("NB_LIB_PATH", BRANCH_LIB), "split": os.environ.get("NB_BWD_SPLIT", "1"), "times": {}, "random_c_sha256": {},
           "lattice_sha256": {}}
    if args.shapes:  # the NB_BWD_SPLIT=0 worker: the recorded products that the switch moves to gemm_rows_fast_kernel<false>
        with open(args.shapes) as f:
            gemms = [g for g in json.load(f) if g["variant"] == "ROWS16"]
        for g in gemms:
            g["variant"] = "ROWS_FAST"
        convs = []
    else:
        gemms, convs = record_step(dev)
        missing = set(KERNEL_OF) - {g["variant"] for g in gemms}
        if missing - {"ROWS_FAST"}:
            raise SystemExit("the training step launches no %s product: nothing to time for it" % sorted(missing))
        res["gemms"] = gemms
    for g in gemms:
        t, digest = replay_gemm(g, args.reps, dev)
        res["times"][gemm_key(g)] = t
        if not g["trans_a"]:
            res["random_c_sha256"][gemm_key(g)] = digest
    if convs:
        t, digests = replay_convs(convs, args.reps, args.lattice)
        res["times"].update(t)
        res["lattice_sha256"].update(digests)
    if args.lattice and not args.shapes:
        res["lattice_sha256"].update(lattice_gemm_digests(dev))
    res["device"] = torch.cuda.get_device_name(0)
    torch.cuda.synchronize()
    with open(args.worker, "w") as f:
        json.dump(res, f)


# ----------------------------------------------------------------------------------------------------------------- the comparison
def child(cmd, env):
    """one step of the chain: its own time limit, and the run ends with the first step that fails"""
    full = ["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd
    out = subprocess.run(full, cwd=ROOT, env=env, capture_output=True, text=True)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("`%s` ended with status %d: nothing further is started" % (" ".join(cmd), out.returncode))
    return out.stdout


def verdict(parent_means, branch_means):
    p, b = np.array(parent_means), np.array(branch_means)
    spread = float(p.max() - p.min())
    return dict(parent_round_means_ms=parent_means, branch_round_means_ms=branch_means, parent_mean_ms=float(p.mean()), branch_mean_ms=float(b.mean()),
                parent_spread_ms=spread, passes=bool(b.mean() <= p.mean() + spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", nargs="?", const="HEAD~1", default=None, metavar="REV")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backward_tile_refactor.json"))
    ap.add_argument("--head", default=None)
    ap.add_argument("--parent-head", default=None, help="the parent commit's name, for the record")
    ap.add_argument("--worker", default=None, metavar="FILE", help=argparse.SUPPRESS)
    ap.add_argument("--shapes", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lattice", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.build_parent:
        build_parent(args.build_parent)
        return 0
    if args.worker:
        worker(args)
        return 0
    for lib in (PARENT_LIB, BRANCH_LIB):
        if not os.path.exists(lib):
            raise SystemExit("%s is missing: build it first (--build-parent; python -m neuralbody_amd.build)" % lib)
    libs = {"parent": PARENT_LIB, "branch": BRANCH_LIB}
    runs = {tag: [] for tag in libs}
    train = {}
    with tempfile.TemporaryDirectory() as d:
        for rnd in range(args.rounds):
            for tag, lib in libs.items():
                merged = None
                for split in ("1", "0"):
                    path = os.path.join(d, "%s_%d_%s.json" % (tag, rnd, split))
                    cmd = [sys.executable, os.path.abspath(__file__), "--worker", path, "--reps", str(args.reps)] + (["--lattice"] if rnd == 0 else [])
                    if split == "0":
                        shapes = os.path.join(d, "shapes.json")
                        with open(shapes, "w") as f:
                            json.dump(merged["gemms"], f)
                        cmd += ["--shapes", shapes]
                    child(cmd, dict(os.environ, NB_LIB_PATH=lib, NB_BWD_SPLIT=split))
                    with open(path) as f:
                        part = json.load(f)
                    if merged is None:
                        merged = part
                    else:
                        for k in ("times", "random_c_sha256", "lattice_sha256"):
                            merged[k].update({key + " (NB_BWD_SPLIT=0)": v for key, v in part[k].items()})
                runs[tag].append(merged)
                print("round %d %s: %d timings" % (rnd, tag, len(merged["times"])), flush=True)
        for rnd in range(args.rounds):  # the step itself
            for tag, lib in libs.items():
                line = child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", "train", "--steps", str(args.train_steps), "--warmup", "3"],
                             dict(os.environ, NB_LIB_PATH=lib)).strip().splitlines()[-1]
                train.setdefault(tag, []).append(json.loads(line)["value"])
    train = verdict(train["parent"], train["branch"])
    keys = sorted(runs["parent"][0]["times"])
    assert all(sorted(r["times"]) == keys for tag in libs for r in runs[tag]), "the runs timed different shapes"
    per_shape = {k: verdict([r["times"][k]["mean_ms"] for r in runs["parent"]], [r["times"][k]["mean_ms"] for r in runs["branch"]]) for k in keys}
    per_kernel = {}
    for k, v in per_shape.items():
        per_kernel[k.split(" ")[0]] = per_kernel.get(k.split(" ")[0], True) and v["passes"]

    def equal(field, rounds):
        ref = runs["parent"][0][field]
        return {k: all(r[field].get(k) == ref[k] for tag in libs for r in runs[tag][:rounds]) for k in sorted(ref)}

    from neuralbody_amd import build as nb_build

    rec = dict(tool="tools/bench_backward_kernels.py", head=args.head or _head(), parent=args.parent_head, library_source_sha256=nb_build._digest(),
               device=runs["branch"][0]["device"],
               what="parent and branch libraries alternating, %d rounds each, one fresh process per library, round and NB_BWD_SPLIT setting; HIP events "
                    "per call after 3 warm-up calls, %d calls; shapes recorded from one step of bench.py --mode train" % (args.rounds, args.reps),
               condition="per kernel and shape: mean over the branch's round means <= mean over the parent's round means + (max - min of the parent's round means)",
               kernels_meet_condition=per_kernel, meets_condition=bool(all(per_kernel.values())),
               bench_train_step_ms=train,
               c_of_gemm_rows_kernels_byte_equal_on_random_operands=equal("random_c_sha256", args.rounds),
               outputs_byte_equal_on_exact_lattices=equal("lattice_sha256", 1),
               verdict=per_shape, gemms_of_the_step=runs["branch"][0]["gemms"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"kernels_meet_condition": per_kernel, "bench_train_step_ms": train,
                      "random_c_all_equal": all(rec["c_of_gemm_rows_kernels_byte_equal_on_random_operands"].values()),
                      "lattice_all_equal": all(rec["outputs_byte_equal_on_exact_lattices"].values())}))
    print("wrote", args.out)
    return 0 if rec["meets_condition"] else 1


if __name__ == "__main__":
    sys.exit(main())
