"""Record the genuine rocALUTION library's MultiElimination for tests/golden/multielim/*.npz.

    python tools/gen_golden_multielim.py [outdir]

Compiles tests/drivers/multielim_probe.cpp (public header and installed library only, accelerator disabled, one OpenMP
thread) into a temporary directory and runs it on the operators of tests/golden/{gr3030,poisson8,lap2d7,lap27_6}.npz (with
the CG + MultiElimination(MultiColoredILU(0), 2, drop) run) and, without the Krylov run, on path9 (the 1-D chain of
gen_golden_rsamg.py) and rand300u (rand300 with its entries below the diagonal removed: structurally unsymmetric, and the
sweep's result is still a permutation).  One small .npz per operator holds the operator, the right-hand side of the
Solve records (the fixture's x; for path9 a fixed vector), the drop-off the probe derived, and what the probe dumped (see
its header).  The histories are stored with the digits the library's history file holds.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
KRYLOV = ["gr3030", "poisson8", "lap2d7", "lap27_6"]
EDGE = ["path9", "rand300u"]
INT32 = ("_rowptr", "_col", "perm", "perm_f32")


def operator(name):
    """-> (rowptr, col, val, rhs)"""
    if name == "path9":
        n = 9
        rp, ci, va = [0], [], []
        for i in range(n):
            for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
                if 0 <= j < n:
                    ci.append(j); va.append(v)
            rp.append(len(ci))
        return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va), 1.0 + (np.arange(n) * 7 % 5) / 4.0
    g = np.load(os.path.join(GOLDEN, ("rand300" if name == "rand300u" else name) + ".npz"))
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    if name == "rand300u":
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        keep = ci >= rows
        nrp = np.zeros(len(rp), np.int32)
        np.cumsum(np.bincount(rows[keep], minlength=len(rp) - 1), out=nrp[1:])
        rp, ci, va = nrp, ci[keep], va[keep]
    return rp.astype(np.int32), ci.astype(np.int32), va.astype(np.float64), g["x"].astype(np.float64)


def _read(d):
    out = {}
    for f in sorted(os.listdir(d)):
        p, key = os.path.join(d, f), f[:-4]
        if f.endswith("_hist.txt"):
            out[key] = np.array([float(t) for t in open(p).read().split()])
        elif f.endswith(".bin"):
            if key.endswith("_shape") or key.startswith("size") or "_sizes" in key:
                dt = np.int64
            elif key.endswith(INT32):
                dt = np.int32
            elif key.endswith("_f32") or (key.endswith("_val") and "_f32" in key):
                dt = np.float32
            else:
                dt = np.float64
            out[key] = np.fromfile(p, dtype=dt)
    return out


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "multielim")
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "multielim_probe")
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-I" + os.path.join(ROCM, "include"),
                               os.path.join(ROOT, "tests", "drivers", "multielim_probe.cpp"), "-L" + os.path.join(ROCM, "lib"),
                               "-lrocalution", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
        for name in KRYLOV + EDGE:
            rp, ci, va, rhs = operator(name)
            ind, outd = os.path.join(tmp, name + "_in"), os.path.join(tmp, name + "_out")
            os.makedirs(ind); os.makedirs(outd)
            np.array([len(rp) - 1, len(ci), 1 if name in KRYLOV else 0], dtype=np.int64).tofile(os.path.join(ind, "hdr.bin"))
            rp.tofile(os.path.join(ind, "rowptr.bin")); ci.tofile(os.path.join(ind, "col.bin"))
            va.tofile(os.path.join(ind, "val.bin")); rhs.tofile(os.path.join(ind, "rhs.bin"))
            subprocess.check_call([exe, ind, outd], env=dict(os.environ, OMP_NUM_THREADS="1"), stdout=subprocess.DEVNULL)
            d = _read(outd)
            d["rowptr"], d["col"], d["val"], d["rhs"] = rp, ci, va, rhs
            for sfx in ("", "_f32"):  # the positive drop-off removes some entries and not all of them
                assert 0 < d["aad" + sfx + "_shape"][2] < d["aa0" + sfx + "_shape"][2], name
            path = os.path.join(outdir, name + ".npz")
            np.savez_compressed(path, **d)
            print(name, os.path.getsize(path), "bytes; size", int(d["size"][0]), "drop", float(d["drop"][0]), "AA nnz",
                  int(d["aa0_shape"][2]), "->", int(d["aad_shape"][2]), "operator nnz", len(ci), "->", int(d["cmp_shape"][2]),
                  "CG+ME iterations", int(d["cg_me_meta"][0]) if "cg_me_meta" in d else "-")


if __name__ == "__main__":
    main()
