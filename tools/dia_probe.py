"""DIA product against the CSR and ELL products of the same matrix, in one process, alternating.

    python tools/dia_probe.py [--poisson 256] [--lap27 128] [--var 256] [--reps 30] [--rounds 9] [--copy-tbs 6.71] [--out FILE]

Operators: the 7-point Poisson operator (constant coefficients), the 27-point Laplacian, and a 7-point operator with variable
coefficients: the pattern of the Poisson operator, every edge (i, j) weighted -(1 + r_ij / 2) with r_ij from a seeded
generator, r_ij = r_ji, and the diagonal the sum of the row's weights plus 1/64 -- symmetric, diagonally dominant, and no two
rows share their values, so no value pattern exists.

Per operator four matrices: CSR as the library picks its kernel (row patterns, value patterns, the lattice form), CSR with the
stored columns read (UseRowPatterns(False): k_csr_tr / k_csr_wr), ELL, DIA.  Warm-up of all, then `rounds` rounds of (reps
products of one, synchronise) for each in turn, timed with the host clock around the synchronise; median, minimum and maximum
over the rounds of the time per product.  The products are compared first (DIA adds its padded zeros, so it equals CSR bit for
bit only where no diagonal is cut -- reported, not required).  Printed beside the times: the bytes a DIA product has to move,
(8 num_diag + 16) n in fp64, over the median time, and that rate over the copy rate of the machine (tools/membench.hip).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import rocalution_amd as ra  # noqa: E402


def timed(A, x, y, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        A.Apply(x, y)
    ra.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def variable_values(rp, ci, N, seed):
    """values for the 7-point pattern of an N^3 grid: see the module text"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    d = ci.astype(np.int64) - rows
    lo = np.minimum(rows, ci)
    direction = np.searchsorted(np.array([1, N, N * N]), np.abs(d))  # (the diagonal lands on 0 and is overwritten below)
    r = np.random.default_rng(seed).random((3, n))
    va = -(1.0 + 0.5 * r[np.minimum(direction, 2), lo])
    off = d != 0
    va[~off] = 0.0
    diag = np.add.reduceat(np.abs(va), rp[:-1].astype(np.int64)) + 1.0 / 64
    va[~off] = diag
    return va


def case(tag, make, reps, rounds, copy_tbs, out):
    mats = {}
    A = make()
    n, nnz = A.GetM(), A.GetNnz()
    mats["csr"] = A
    for key in ("csr_cols", "ell", "dia"):
        B = ra.LocalMatrix(); B.CloneFrom(A)
        mats[key] = B
    mats["csr_cols"].UseRowPatterns(False)
    assert mats["ell"].ConvertToELL() == ra.ELL, "ELL refused"
    t0 = time.perf_counter()
    fmt = mats["dia"].ConvertToDIA()
    ra.sync()
    t_conv = time.perf_counter() - t0
    assert fmt == ra.DIA, "DIA refused"
    nd = mats["dia"].GetNnz() // n
    x = ra.LocalVector(data=np.random.default_rng(1).uniform(-1.0, 1.0, n))
    ys = {}
    for key, M in mats.items():
        ys[key] = ra.LocalVector(); ys[key].Allocate("", n)
        for _ in range(5):
            M.Apply(x, ys[key])
    ra.sync()
    ref = ys["csr"].numpy()
    got = ys["dia"].numpy()
    bit_equal = bool(np.array_equal(ref, got))
    max_rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert max_rel < 1e-12, max_rel
    assert np.array_equal(ys["ell"].numpy(), ref) or np.allclose(ys["ell"].numpy(), ref, rtol=0, atol=1e-12 * np.max(np.abs(ref)))
    t = {key: [] for key in mats}
    for _ in range(rounds):
        for key, M in mats.items():
            t[key].append(timed(M, x, ys[key], reps))
    med = {key: float(np.median(v)) for key, v in t.items()}
    bytes_dia = (8 * nd + 16) * n
    rec = dict(case=tag, n=n, nnz_csr=nnz, num_diag=nd, fill=nd * n / nnz, dia_equals_csr_bitwise=bit_equal, dia_max_rel_diff=max_rel,
               convert_s=round(t_conv, 4),
               ms={key: dict(median=med[key], min=min(v), max=max(v)) for key, v in t.items()},
               value_pattern_state=mats["csr"].ValuePatternState(),
               bytes_dia=bytes_dia, dia_tbs=bytes_dia / med["dia"] / 1e9, dia_share_of_copy_rate=bytes_dia / med["dia"] / 1e9 / copy_tbs,
               dia_over_csr=med["dia"] / med["csr"], dia_over_csr_cols=med["dia"] / med["csr_cols"], dia_over_ell=med["dia"] / med["ell"],
               reps=reps, rounds=rounds)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poisson", type=int, default=256)
    ap.add_argument("--lap27", type=int, default=128)
    ap.add_argument("--var", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--copy-tbs", type=float, default=6.71, help="copy rate of the machine in TB/s (tools/membench.hip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ra.init_rocalution()

    def poisson():
        A = ra.LocalMatrix(); A.GenPoisson7(args.poisson)
        return A

    def lap27():
        A = ra.LocalMatrix(); A.GenLaplace27(args.lap27)
        return A

    def var7():
        A = ra.LocalMatrix(); A.GenPoisson7(args.var)
        rp, ci, _ = A.CopyToCSR()
        A.UpdateValuesCSR(variable_values(rp, ci, args.var, 20261020))
        return A

    if args.poisson > 0:
        case("poisson7 %d^3" % args.poisson, poisson, args.reps, args.rounds, args.copy_tbs, args.out)
    if args.lap27 > 0:
        case("laplace27 %d^3" % args.lap27, lap27, args.reps, args.rounds, args.copy_tbs, args.out)
    if args.var > 0:
        case("variable-coefficient 7-point %d^3" % args.var, var7, args.reps, args.rounds, args.copy_tbs, args.out)


if __name__ == "__main__":
    main()
