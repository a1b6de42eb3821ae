"""Record the genuine rocALUTION library's Ruge-Stueben AMG for tests/golden/rsamg/*.npz.

    python tools/gen_golden_rsamg.py [outdir]

Compiles tests/drivers/rsamg_probe.cpp (public header and installed library only, accelerator disabled, one OpenMP
thread) into a temporary directory, runs it on the operators of tests/golden/{gr3030,poisson8,lap2d7,lap27_6,rand300}.npz
and, primitives only, on three edge operators (diag40: a diagonal matrix; path9: a 1-D chain; rand300s: rand300 with
every third row negated), and writes one small .npz per operator with
what the probe dumped (see the probe's header for the list).  The histories are stored with the digits the library's
history file holds.  `pos_strong_fine_rows_<map>` counts the fine rows with a positive strong off-diagonal entry.  On rand300 it is 0: its
diagonals are positive, and then a strong entry is negative by the definition of S.  `sign_skips_<map>` therefore counts
what the sign tests of the extended+i weights actually leave out (entries of a strong fine neighbour's row at a column of
the row's set, or at the row itself, whose sign equals the diagonal's), with tests/_rsamg_ref.py: > 0 on rand300, so those
branches are taken there; rand300s has rows with a negative diagonal and positive strong entries as well.

Which interpolation reproduces the rsamg_pmis_* / cg_rsamg_* arrays already stored in tests/golden/{gr3030,poisson8,
lap2d7}.npz (recorded with PMIS and the library's default interpolation): Direct -- the script compares the arrays of
its PMIS + Direct runs with them and fails if they differ (iterations, status, history, x all equal).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _rsamg_ref import extpi  # noqa: E402
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
MATRICES = ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300"]
INT = ("_rowptr", "_col", "_cf", "_S")


def _edge(name):
    if name == "diag40":
        n = 40
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 + np.arange(n) % 3
    if name == "rand300s":  # rand300 with every third row negated: rows with a negative diagonal and positive strong entries
        g = np.load(os.path.join(GOLDEN, "rand300.npz"))
        rp, ci, va = g["rowptr"], g["col"], g["val"].copy()
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        va[rows % 3 == 0] *= -1.0
        return rp, ci, va
    n = 9  # path9
    rp, ci, va = [0], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                ci.append(j); va.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va)


def _read(d):
    out = {}
    for f in sorted(os.listdir(d)):
        p, key = os.path.join(d, f), f[:-4]
        if f.endswith("_hist.txt"):
            out[key] = np.array([float(t) for t in open(p).read().split()])
        elif f.endswith(".bin"):
            if key.endswith("_shape"):
                dt = np.int64
            elif key.endswith(INT):
                dt = np.int32
            elif key.endswith("_val") and "_f32" in key:
                dt = np.float32
            else:
                dt = np.float64
            out[key] = np.fromfile(p, dtype=dt)
    return out


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "rsamg")
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rsamg_probe")
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-I" + os.path.join(ROCM, "include"),
                               os.path.join(ROOT, "tests", "drivers", "rsamg_probe.cpp"), "-L" + os.path.join(ROCM, "lib"),
                               "-lrocalution", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
        for name in MATRICES + ["diag40", "path9", "rand300s"]:
            edge = name not in MATRICES
            if edge:
                rp, ci, va = _edge(name)
            else:
                g = np.load(os.path.join(GOLDEN, name + ".npz"))
                rp, ci, va = g["rowptr"], g["col"], g["val"]
            ind, outd = os.path.join(tmp, name + "_in"), os.path.join(tmp, name + "_out")
            os.makedirs(ind); os.makedirs(outd)
            np.array([len(rp) - 1, len(ci), 0 if edge else 1], dtype=np.int64).tofile(os.path.join(ind, "hdr.bin"))
            rp.astype(np.int32).tofile(os.path.join(ind, "rowptr.bin"))
            ci.astype(np.int32).tofile(os.path.join(ind, "col.bin"))
            va.astype(np.float64).tofile(os.path.join(ind, "val.bin"))
            subprocess.check_call([exe, ind, outd], env=dict(os.environ, OMP_NUM_THREADS="1"), stdout=subprocess.DEVNULL)
            d = _read(outd)
            d["rowptr"], d["col"], d["val"] = rp.astype(np.int32), ci.astype(np.int32), va.astype(np.float64)
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
            for m in ("greedy", "pmis"):
                hit = (d[m + "_S"] == 1) & (va > 0) & (d[m + "_cf"][rows] == 2)
                d["pos_strong_fine_rows_" + m] = np.array([len(np.unique(rows[hit]))], dtype=np.int64)
                st = {}
                ref = extpi(rp, ci, va, d[m + "_cf"], d[m + "_S"], False, np.float64, st)
                assert ref[2].tobytes() == d["extpi_" + m + "_ff0_val"].tobytes() and np.array_equal(ref[1], d["extpi_" + m + "_ff0_col"])
                d["sign_skips_" + m] = np.array([st.get("sign_skips", 0)], dtype=np.int64)
            if not edge and "rsamg_pmis_meta" in g:
                for new, old in (("amg_pmis_direct", "rsamg_pmis"), ("cg_pmis_direct", "cg_rsamg")):
                    assert np.array_equal(d[new + "_meta"][:3], g[old + "_meta"]), (name, new)
                    assert np.array_equal(d[new + "_hist"], g[old + "_hist"]) and np.array_equal(d[new + "_x"], g[old + "_x"])
                assert d["amg_pmis_direct_meta"][3] == g["rsamg_levels"][0]
                assert np.array_equal(d["direct_pmis_val"], g["rs_P_val"]) and np.array_equal(d["pmis_cf"], g["rs_cf"])
            path = os.path.join(outdir, name + ".npz")
            np.savez_compressed(path, **d)
            print(name, os.path.getsize(path), "bytes; fine rows with a positive strong entry:",
                  int(d["pos_strong_fine_rows_greedy"][0]), int(d["pos_strong_fine_rows_pmis"][0]), "sign skips:",
                  int(d["sign_skips_greedy"][0]), int(d["sign_skips_pmis"][0]))


if __name__ == "__main__":
    main()
