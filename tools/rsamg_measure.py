"""Measure the Ruge-Stueben AMG setup and CG preconditioned by it on one MI355X; writes the table of profiles/rsamg.md.

    python tools/rsamg_measure.py <poisson:N | lap27:N> <pmis_direct | pmis_extpi | greedy_direct | saamg> [--out profiles/rsamg.md]

Each run appends one row to the file (and writes the table's head when the file does not exist yet); without --out the row
goes to stdout.  The series of profiles/rsamg.md: poisson:256 and lap27:128, the four cases each.

One case per process (run each under its own `timeout`, chained with &&, so that a fault ends the series).  For the RS cases
the hierarchy is built level by level with the LocalMatrix primitives (coarsening, interpolation, Transpose, TripleMatrix-
Product; coarsest level <= 300 rows) and every phase is timed by the host clock -- each entry drains its stream before it
returns.  Then CG + the preconditioner through the C solver table: Build() time, iterations to 1e-6 relative, it/s.
`saamg` runs CG + SAAMG(PMIS) only: the yardstick that exists at the same commit."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocalution_amd as ra  # noqa: E402
from rocalution_amd import solvers as S  # noqa: E402


def main():
    op, case = sys.argv[1], sys.argv[2]
    ra.init_rocalution()
    kind, N = op.split(":")
    A = ra.LocalMatrix()
    A.GenPoisson7(int(N)) if kind == "poisson" else A.GenLaplace27(int(N))
    n = A.GetM()
    line = "| %s | %s |" % (op, case)
    if case != "saamg":
        strat, interp = case.split("_")
        t = dict(coarsen=0.0, interp=0.0, transpose=0.0, triple=0.0)
        cur, rows, nnzs, info0 = A, [n], [A.GetNnz()], None
        while cur.GetM() > 300:
            t0 = time.perf_counter()
            cf, Sv = cur.RSPMISCoarsening(0.25) if strat == "pmis" else cur.RSCoarsening(0.25)
            t1 = time.perf_counter()
            P = ra.LocalMatrix()
            info = cur.RSExtPIInterpolation(cf, Sv, False, P) if interp == "extpi" else cur.RSDirectInterpolation(cf, Sv, P)
            info0 = info0 or info
            t2 = time.perf_counter()
            if P.GetN() == 0:
                break
            R, Ac = ra.LocalMatrix(), ra.LocalMatrix()
            P.Transpose(R)
            t3 = time.perf_counter()
            Ac.TripleMatrixProduct(R, cur, P)
            t4 = time.perf_counter()
            t["coarsen"] += t1 - t0; t["interp"] += t2 - t1; t["transpose"] += t3 - t2; t["triple"] += t4 - t3
            cur = Ac
            rows.append(cur.GetM()); nnzs.append(cur.GetNnz())
        line += " %.3f | %.3f | %.3f | %.3f | %d | %.3f |" % (t["coarsen"], t["interp"], t["transpose"], t["triple"], len(rows),
                                                             sum(nnzs) / nnzs[0])
        if info0:
            line += " lds %d scratch %d |" % (info0["lds_rows"], info0["scratch_rows"])
        else:
            line += " - |"
        pc = S.RugeStuebenAMG()
        pc.SetCoarseningStrategy(S.PMIS if strat == "pmis" else S.Greedy)
        pc.SetInterpolationType(S.ExtPI if interp == "extpi" else S.Direct)
    else:
        line += " - | - | - | - | - | - | - |"
        pc = S.SAAMG()
    ones = ra.LocalVector(data=np.ones(n))
    rhs = ra.LocalVector(); rhs.Allocate("rhs", n)
    A.Apply(ones, rhs)
    x = ra.LocalVector(); x.Allocate("x", n)
    ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Init(1e-15, 1e-6, 1e8, 500)
    t0 = time.perf_counter()
    ls.Build()
    t1 = time.perf_counter()
    ls.Solve(rhs, x)
    x.numpy()
    t2 = time.perf_counter()
    it = ls.GetIterationCount()
    line += " %.3f | %d | %d | %.1f |" % (t1 - t0, it, ls.GetSolverStatus(), it / (t2 - t1))
    head = ("| operator | case | coarsening s | interpolation s | transpose s | triple product s | levels | operator complexity |"
            " ExtPI rows of the first level: LDS / scratch table | CG Build() s | CG iterations | status | it/s |\n"
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        new = not os.path.exists(path)
        with open(path, "a") as f:
            f.write((head if new else "") + line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
