"""BCSR product against the CSR product of the same matrix, in one process, alternating.

    python tools/bcsr_probe.py [--shell-nx 549] [--poisson 256] [--reps 50] [--rounds 9] [--out FILE]

Cases: the shell surrogate (5 unknowns per mesh node, dense 5 x 5 blocks) with blockdim 5 -- no fill; the 7-point Poisson
operator with blockdim 2 and 4 -- BCSR stores the zeros of its blocks there.  Both matrices keep their default settings (row
patterns as the library picks them).  Per case: warm-up of both, then `rounds` rounds of (reps CSR products, synchronise, reps
BCSR products, synchronise) timed with the host clock around the synchronise; median, minimum and maximum over the rounds of
the time per product.  The moved-bytes model (what the kernel has to read and write once; x counted once) is printed beside
the times:
    CSR   12 nnz + 4 (n + 1) + 16 n                   (fp64 values, int32 columns and offsets, x and y)
    BCSR  8 nnzb d^2 + 4 nnzb + 4 (n / d + 1) + 16 n
The products are compared first: equal bit for bit where the CSR rows are sorted and x is finite (the padded entries add +0).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import rocalution_amd as ra  # noqa: E402
from rocalution_amd import generators as gen  # noqa: E402


def timed(A, x, y, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        A.Apply(x, y)
    ra.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def case(tag, make, d, reps, rounds, out):
    A = make()
    n, nnz = A.GetM(), A.GetNnz()
    B = ra.LocalMatrix(); B.CloneFrom(A)
    t0 = time.perf_counter()
    fmt = B.ConvertToBCSR(d)
    ra.sync()
    t_conv = time.perf_counter() - t0
    assert fmt == ra.BCSR, "conversion refused"
    nnzb = B.GetNnz() // (d * d)
    x = ra.LocalVector(data=np.random.default_rng(1).uniform(-1.0, 1.0, n))
    ya = ra.LocalVector(); ya.Allocate("", n)
    yb = ra.LocalVector(); yb.Allocate("", n)
    for _ in range(5):
        A.Apply(x, ya); B.Apply(x, yb)
    ra.sync()
    same = bool(np.array_equal(ya.numpy(), yb.numpy()))
    tc, tb = [], []
    for _ in range(rounds):
        tc.append(timed(A, x, ya, reps))
        tb.append(timed(B, x, yb, reps))
    bytes_csr = 12 * nnz + 4 * (n + 1) + 16 * n
    bytes_bcsr = 8 * nnzb * d * d + 4 * nnzb + 4 * (n // d + 1) + 16 * n
    rec = dict(case=tag, n=n, nnz_csr=nnz, blockdim=d, nnzb=nnzb, fill=nnzb * d * d / nnz, bit_equal=same,
               convert_s=round(t_conv, 4),
               csr_ms=dict(median=float(np.median(tc)), min=min(tc), max=max(tc)),
               bcsr_ms=dict(median=float(np.median(tb)), min=min(tb), max=max(tb)),
               bytes_csr=bytes_csr, bytes_bcsr=bytes_bcsr,
               csr_gbs=bytes_csr / np.median(tc) / 1e6, bcsr_gbs=bytes_bcsr / np.median(tb) / 1e6,
               bcsr_over_csr_time=float(np.median(tb) / np.median(tc)), reps=reps, rounds=rounds)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shell-nx", type=int, default=549)
    ap.add_argument("--poisson", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ra.init_rocalution()

    def shell():
        rp, ci, va = gen.shell_surrogate(args.shell_nx)
        A = ra.LocalMatrix(); A.SetDataPtrCSR(rp, ci, va)
        return A

    def poisson():
        A = ra.LocalMatrix(); A.GenPoisson7(args.poisson)
        return A

    if args.shell_nx > 0:
        case("shell %d^2 nodes" % args.shell_nx, shell, 5, args.reps, args.rounds, args.out)
    if args.poisson > 0:
        for d in (2, 4):
            if args.poisson ** 3 % d == 0:
                case("poisson7 %d^3" % args.poisson, poisson, d, args.reps, args.rounds, args.out)


if __name__ == "__main__":
    main()
