"""Measure one application of the BlockPreconditioner in its stepwise (0) and fused (1) form, fp64, Jacobi on every diagonal
block: the 7-point operator (default 256^3) with nb = 3, 16, 64 equal blocks, with the block forward substitution and with
SetDiagonalSolver().

    python tools/blockprec_measure.py [--grid 256] [--nb 3,16,64] [--rounds 3] [--reps 20] [--batches 5] [--out tables.md]

One process holds both forms of a configuration, built side by side on the one operator; they are timed in alternating order
(0 1, 1 0, ...) --rounds times: HIP events around batches of --reps applies after a warm-up batch, the median of --batches
batches per visit, the median over the visits with the spread beside it.  Launches and algorithmic bytes per apply are
computed from the plan's record (n rows, L entries, nb), not measured:
    stepwise  launches: nb slice copies + the ApplyAdd calls on non-empty blocks + nb Jacobi + nb slice copies
              bytes   : 16 n (slice copies in and out) + per ApplyAdd 12 entries + 4 rows + 16 rows (r_b read and written)
                        + 8 columns of x_j + 24 n (Jacobi: r, dinv read, z written)
    fused     launches: nb steps + nb Jacobi + 1 join
              bytes   : per step 12 entries + 4 rows + 16 rows (rhs read, r_b written) + gathers of z (counted once: 8 n at
                        most per step, here the distinct columns are not known and 0 is charged) + 24 n (Jacobi) + 16 n (join)
profiles/blockprec.md quotes the table next to hand-written text and is refused as a target.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ra, capi, fn, reps, batches):
    lib = capi.load()
    for _ in range(reps):
        fn()
    ra.sync()
    out = []
    for _ in range(batches):
        ms = C.c_double(0)
        capi.check(lib.ramd_timer_start())
        for _ in range(reps):
            fn()
        capi.check(lib.ramd_timer_stop(C.byref(ms)))
        out.append(ms.value / reps)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--nb", default="3,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out and os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "blockprec.md"):
        sys.exit("--out: profiles/blockprec.md holds hand-written sections; write the table elsewhere and paste it in")
    import rocalution_amd as ra
    from rocalution_amd import capi, solvers as S
    ra.init_rocalution()
    A = ra.LocalMatrix()
    A.GenPoisson7(args.grid)
    n = A.GetM()
    r = ra.LocalVector(data=np.random.default_rng(1).uniform(-1, 1, n))
    x = ra.LocalVector(); x.Allocate("", n)
    rows = ["### 7-point %d^3 (fp64, Jacobi on every block; one apply, medians of %d alternating visits, spread in brackets)"
            % (args.grid, args.rounds), "",
            "| nb | diagonal only | form | apply ms | launches | algorithmic MB | GB/s | L entries |", "|---|---|---|---|---|---|---|---|"]
    for nb in [int(v) for v in args.nb.split(",")]:
        sizes = [n // nb] * (nb - 1) + [n - (nb - 1) * (n // nb)]
        for diag in (False, True):
            built = {}
            for form in (0, 1):
                pc = S.BlockPreconditioner(sizes, S.Jacobi(), diagonal=diag); pc.SetForm(form)
                ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
                built[form] = (pc, ls)
            lnnz = 0 if diag else built[1][0].Info()["nnz_lower"]
            pairs = 0 if diag else min(nb * (nb - 1) // 2, 2 * (nb - 1))  # (the 7-point operator couples a block row to 2 earlier blocks at most)
            times = {0: [], 1: []}
            for rnd in range(args.rounds):
                for form in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                    ls = built[form][1]
                    times[form].append(timed(ra, capi, lambda: ls.PrecondApply(r, x), args.reps, args.batches))
            for form in (0, 1):
                assert built[form][0].Info()["form"] == form
                t = float(np.median(times[form]))
                if form == 0:
                    launches = 2 * nb + pairs + nb
                    mb = (16.0 * n + 12.0 * lnnz + 20.0 * n * (1 if lnnz else 0) + 24.0 * n) / 1e6
                else:
                    launches = 2 * nb + 1
                    mb = (12.0 * lnnz + 20.0 * n + 24.0 * n + 16.0 * n) / 1e6
                rows.append("| %d | %s | %d | %.3f [%.3f - %.3f] | %d | %.0f | %.0f | %d |" % (
                    nb, "yes" if diag else "no", form, t, min(times[form]), max(times[form]), launches, mb, mb / t, lnnz))
                print(rows[-1], flush=True)
            for form in (0, 1):
                built[form][1].Clear()
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
