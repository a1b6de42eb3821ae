"""Record the genuine rocALUTION library's aggregation-AMG setup for tests/golden/amg/*.npz.

    python tools/gen_golden_amg.py [outdir]

Compiles tests/drivers/amg_probe.cpp (public header and installed library only, accelerator disabled, one OpenMP thread)
into a temporary directory, runs it on operators this script generates itself (fixed seeds, or derived from committed
fixtures), and writes one .npz per operator.  Every file holds the input CSR (rowptr, col, val), `conn` (eps = 0.01; the
Greedy and the PMIS call return the same one), {greedy,pmis}_{agg,roots}, the unsmoothed prolongator ua_{greedy,pmis}_*
and the smoothed ones sa0_* (relax 2/3, lumping 0) and sa1_* (relax 0.5, lumping 1), each as _rowptr / _col / _val / _shape
(rows, columns, entries).  The library's float instantiation is reachable from the public header, so the fp32 run is
recorded too: the script checks that its connections, aggregates, root nodes and prolongator patterns equal the fp64 ones
on every operator here and stores the fp32 values alone, sa{0,1}_{greedy,pmis}_f32_val.  The archives are written with a
fixed time stamp: a second run gives the same bytes.

The operators, each for a branch; the script prints the counts that show the branch is taken (with tests/_amg_ref.py, on
what the library returned) and fails if one of them is 0:
  path9, diag40   the generators of gen_golden_rsamg.py.  diag40: no strong connection, every aggregate -2, P without entries.
  irr_sym         irregular and symmetric in values and pattern: (A + A^T) / 2 of tests/golden/rand300.npz (rand300 itself has
                  an unsymmetric pattern, hence an unsymmetric strong graph), 300 rows of 4 to 70 entries.  Rows owned through a
                  tentative claim; direct claims that overwrite a tentative claim of an earlier seed.
  irr_sym_rev     the same with every row stored in descending column order: unsorted columns, and where three or more
                  entries of a row fall into one aggregate another summation order in the smoothed prolongator.
  weakmix         irr_sym with a seeded tenth of the rows cut off (their off-diagonal entries, and the mirrored ones,
                  scaled by 1e-6): removed rows between live ones; five more rows lose their stored diagonal -- a zero
                  diagonal makes all their couplings strong and their lumped diagonal zero: infinite entries, and NaN where
                  infinities of both signs meet under one key.
  hub             row 0 coupled (seeded values in [-1.5, -0.5]) to every fourth row of a chain of 2049 rows behind it: a row of
                  514 entries that all fall into its own aggregate (one key, 514 terms); the rows between its neighbours
                  become seeds and take their neighbours back from it.
  unsym           irr_sym with the upper triangle scaled by 1e-3: the strong graph is not symmetric; strong entries point at
                  rows outside every aggregate.  The library's Greedy result is kept for the record: the device form refuses.
  level2          R A P of poisson8 with the stored smoothed prolongator amg_Ps (oracle.csr_transpose / csr_matmult): the
                  dense irregular kind of operator the second level sees.  An input only.
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _amg_ref as ref  # noqa: E402
from gen_golden_rsamg import _edge  # noqa: E402
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NAMES = ["path9", "diag40", "irr_sym", "irr_sym_rev", "weakmix", "hub", "unsym", "level2"]


def _csr(n, entries):
    """{(i, j): v} -> CSR with ascending columns"""
    rows = [[] for _ in range(n)]
    for (i, j), v in entries.items():
        rows[i].append((j, v))
    rp, ci, va = [0], [], []
    for r in rows:
        for j, v in sorted(r):
            ci.append(j); va.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


def _entries(rp, ci, va):
    return {(i, int(ci[j])): float(va[j]) for i in range(len(rp) - 1) for j in range(rp[i], rp[i + 1])}


def _irr_sym():
    g = np.load(os.path.join(GOLDEN, "rand300.npz"))
    e = _entries(g["rowptr"], g["col"], g["val"])
    sym = {}
    for (i, j), v in e.items():
        sym[(i, j)] = (v + e.get((j, i), 0.0)) / 2
        sym[(j, i)] = sym[(i, j)]
    return len(g["rowptr"]) - 1, sym


def operator(name):
    if name in ("path9", "diag40"):
        rp, ci, va = _edge(name)
        return rp.astype(np.int32), ci.astype(np.int32), np.asarray(va, np.float64)
    if name == "hub":
        n, rng, e = 2049, np.random.default_rng(2049), {(0, 0): 600.0}
        for i in range(1, n + 1):  # the chain: rows 1 .. 2049
            e[(i, i)] = 2.0
            if i > 1:
                e[(i, i - 1)] = e[(i - 1, i)] = -1.0
        for k in range(1, n + 1, 4):
            e[(0, k)] = e[(k, 0)] = -float(rng.uniform(0.5, 1.5))
        return _csr(n + 1, e)
    if name == "level2":
        from oracle import oracle as orc
        orc.build()
        orc.set_threads(1)
        g = np.load(os.path.join(GOLDEN, "poisson8.npz"))
        A = (g["rowptr"], g["col"], g["val"])
        P = (g["amg_Ps_rowptr"], g["amg_Ps_col"], g["amg_Ps_val"])
        nc = int(P[1].max()) + 1
        R = orc.csr_transpose(*P, ncol=nc)
        rp, ci, va = orc.csr_matmult(orc.csr_matmult(R, A), P, ncol_b=nc)
        return _csr(nc, _entries(rp, ci, va))
    n, e = _irr_sym()
    if name == "weakmix":
        rng = np.random.default_rng(300)
        pick = rng.permutation(n)
        for r in pick[:n // 10]:
            for (i, j) in list(e):
                if i != j and (i == r or j == r):
                    e[(i, j)] *= 1e-6
        for r in pick[n // 10:n // 10 + 5]:
            del e[(int(r), int(r))]
    if name == "unsym":
        for (i, j) in e:
            if j > i:
                e[(i, j)] *= 1e-3
    rp, ci, va = _csr(n, e)
    if name == "irr_sym_rev":
        for i in range(n):
            ci[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][::-1].copy()
            va[rp[i]:rp[i + 1]] = va[rp[i]:rp[i + 1]][::-1].copy()
    return rp, ci, va


def _read(d):
    out = {}
    for f in sorted(os.listdir(d)):
        key = f[:-4]
        if key.endswith("_shape"):
            dt = np.int64
        elif key.endswith("_val"):
            dt = np.float32 if "_f32" in key else np.float64
        else:
            dt = np.int32
        out[key] = np.fromfile(os.path.join(d, f), dtype=dt)
    return out


def save(path, d):
    """np.savez_compressed with a fixed time stamp and key order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "amg")
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "amg_probe")
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-I" + os.path.join(ROCM, "include"),
                               os.path.join(ROOT, "tests", "drivers", "amg_probe.cpp"), "-L" + os.path.join(ROCM, "lib"),
                               "-lrocalution", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
        for name in NAMES:
            rp, ci, va = operator(name)
            ind, outd = os.path.join(tmp, name + "_in"), os.path.join(tmp, name + "_out")
            os.makedirs(ind); os.makedirs(outd)
            np.array([len(rp) - 1, len(ci)], dtype=np.int64).tofile(os.path.join(ind, "hdr.bin"))
            rp.tofile(os.path.join(ind, "rowptr.bin")); ci.tofile(os.path.join(ind, "col.bin")); va.tofile(os.path.join(ind, "val.bin"))
            subprocess.check_call([exe, ind, outd], env=dict(os.environ, OMP_NUM_THREADS="1"), stdout=subprocess.DEVNULL)
            raw = _read(outd)
            assert np.array_equal(raw["greedy_conn"], raw["pmis_conn"])
            d = {"rowptr": rp, "col": ci, "val": va, "conn": raw["greedy_conn"]}
            for k, v in raw.items():
                if "_f32" in k:  # the fp32 run: same integers as the fp64 one, only the values are kept
                    if k.endswith("_val"):
                        if k.startswith("sa"):
                            d[k] = v
                    else:
                        assert np.array_equal(v, raw[k.replace("_f32", "")]), (name, k)
                elif not k.endswith("_conn"):
                    d[k] = v
            c = ref.branch_counts(d)
            ref.check_counts(name, c)
            path = os.path.join(outdir, name + ".npz")
            save(path, d)
            print(name, os.path.getsize(path), "bytes;", " ".join("%s=%d" % kv for kv in c.items()))


if __name__ == "__main__":
    main()
