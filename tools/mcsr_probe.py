"""MCSR product against the CSR products of the same matrix, in one process, alternating, timed with device events.

    python tools/mcsr_probe.py [--var 256] [--lap27 128] [--reps 30] [--rounds 9] [--copy-tbs 6.71] [--out FILE]

Operators: the 7-point operator with variable coefficients of tools/dia_probe.py (the pattern of the Poisson operator, seeded
symmetric weights, no two rows share their values, so no value pattern exists) and the 27-point Laplacian (constant
coefficients: the pattern kernels apply to its CSR form).

Per operator three matrices: CSR as the library picks its kernel (row patterns, value patterns, the lattice form), CSR with the
stored columns read (UseRowPatterns(False), i.e. ramd_mat_pattern_use(m, 0): k_csr_wr on rows of 16+ entries, k_csr_tr below),
MCSR.  Warm-up of all, then `rounds` rounds of `reps` products of each in turn; a product's time is the device-event pair the
library puts around the kernel (the SPMV channel of ramd_prof_enable / ramd_prof_result), a round's figure their average, and
the report the median, minimum and maximum over the rounds.  The MCSR product is compared with the CSR product first (another
summation order: equal to rounding, not to the bit).  Printed beside the times: the bytes an MCSR product has to move in fp64,
12 nnz - 4 n + 4 (n + 1) + 16 n, over the median time, and that rate over the copy rate of the machine (tools/membench.hip).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import rocalution_amd as ra  # noqa: E402
from rocalution_amd import capi  # noqa: E402
from dia_probe import variable_values  # noqa: E402


def timed(lib, A, x, y, reps):
    """average of the device-event times of `reps` products, in ms"""
    capi.check(lib.ramd_prof_enable(0, 1))
    for _ in range(reps):
        A.Apply(x, y)
    cnt, avg = C.c_int(0), C.c_double(0)
    capi.check(lib.ramd_prof_result(0, C.byref(cnt), C.byref(avg), None, None))
    capi.check(lib.ramd_prof_enable(0, 0))
    assert cnt.value == reps, (cnt.value, reps)
    return avg.value


def case(lib, tag, make, reps, rounds, copy_tbs, out):
    mats = {}
    A = make()
    n, nnz = A.GetM(), A.GetNnz()
    mats["csr"] = A
    for key in ("csr_cols", "mcsr"):
        B = ra.LocalMatrix(); B.CloneFrom(A)
        mats[key] = B
    mats["csr_cols"].UseRowPatterns(False)
    t0 = time.perf_counter()
    fmt = mats["mcsr"].ConvertToMCSR()
    ra.sync()
    t_conv = time.perf_counter() - t0
    assert fmt == ra.MCSR and mats["mcsr"].GetNnz() == nnz, "MCSR refused"
    x = ra.LocalVector(data=np.random.default_rng(1).uniform(-1.0, 1.0, n))
    ys = {}
    for key, M in mats.items():
        ys[key] = ra.LocalVector(); ys[key].Allocate("", n)
        for _ in range(5):
            M.Apply(x, ys[key])
    ra.sync()
    want, got = ys["csr"].numpy(), ys["mcsr"].numpy()
    assert np.array_equal(ys["csr_cols"].numpy(), want)
    differ = int(np.sum(want != got))
    max_rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    assert max_rel < 1e-12, max_rel
    t = {key: [] for key in mats}
    for _ in range(rounds):
        for key, M in mats.items():
            t[key].append(timed(lib, M, x, ys[key], reps))
    med = {key: float(np.median(v)) for key, v in t.items()}
    nbytes = 12 * nnz - 4 * n + 4 * (n + 1) + 16 * n
    rec = dict(case=tag, n=n, nnz=nnz, mcsr_differs_from_csr_in=differ, mcsr_max_rel_diff=max_rel, convert_s=round(t_conv, 4),
               ms={key: dict(median=med[key], min=min(v), max=max(v)) for key, v in t.items()},
               value_pattern_state=mats["csr"].ValuePatternState(),
               bytes_mcsr=nbytes, mcsr_tbs=nbytes / med["mcsr"] / 1e9, mcsr_share_of_copy_rate=nbytes / med["mcsr"] / 1e9 / copy_tbs,
               bytes_csr=12 * nnz + 4 * (n + 1) + 16 * n, csr_cols_share_of_copy_rate=(12 * nnz + 4 * (n + 1) + 16 * n) / med["csr_cols"] / 1e9 / copy_tbs,
               mcsr_over_csr=med["mcsr"] / med["csr"], mcsr_over_csr_cols=med["mcsr"] / med["csr_cols"], reps=reps, rounds=rounds)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--var", type=int, default=256)
    ap.add_argument("--lap27", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--copy-tbs", type=float, default=6.71, help="copy rate of the machine in TB/s (tools/membench.hip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ra.init_rocalution()
    lib = capi.load()

    def var7():
        A = ra.LocalMatrix(); A.GenPoisson7(args.var)
        rp, ci, _ = A.CopyToCSR()
        A.UpdateValuesCSR(variable_values(rp, ci, args.var, 20261020))
        return A

    def lap27():
        A = ra.LocalMatrix(); A.GenLaplace27(args.lap27)
        return A

    if args.var > 0:
        case(lib, "variable-coefficient 7-point %d^3" % args.var, var7, args.reps, args.rounds, args.copy_tbs, args.out)
    if args.lap27 > 0:
        case(lib, "laplace27 %d^3" % args.lap27, lap27, args.reps, args.rounds, args.copy_tbs, args.out)


if __name__ == "__main__":
    main()
