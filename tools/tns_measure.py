"""Measure the TNS preconditioner next to Jacobi and MultiColoredSGS on the 7-point and the 27-point operator (fp64, one process):
time per apply, Build() time, CG iterations and wall time to the default tolerances (1e-6 relative).

    python tools/tns_measure.py [--grid 256] [--only matrix-free] [--out tables.md]

The tables go to stdout and, with --out, to a file of their own; profiles/tns.md quotes them next to hand-written text and is
refused as a target.

Apply times: HIP events around batches of `--reps` applies after a warm-up batch, the median of `--batches` batches.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctypes as C  # noqa: E402

import rocalution_amd as ra  # noqa: E402
from rocalution_amd import capi, solvers as S  # noqa: E402


def timed_batches(fn, reps, batches):
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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def wall(fn):
    ra.sync()
    t = time.perf_counter()
    r = fn()
    ra.sync()
    return r, time.perf_counter() - t


def measure(opname, A, args):
    n = A.GetM()
    nnz = A.GetNnz()
    rows = []
    r = ra.LocalVector(data=np.random.default_rng(1).uniform(-1, 1, n))
    x = ra.LocalVector(); x.Allocate("", n)
    ones = ra.LocalVector(); ones.Allocate("", n); ones.Ones()
    rhs = ra.LocalVector(); rhs.Allocate("", n)
    A.Apply(ones, rhs)
    spmv = timed_batches(lambda: A.Apply(r, x), args.reps, args.batches)
    cases = [("TNS matrix-free", lambda: S.TNS(form=1), 1), ("TNS stored", lambda: S.TNS(form=0), 0),
             ("Jacobi", S.Jacobi, None), ("MultiColoredSGS", S.MultiColoredSGS, None)]
    for label, mk, form in cases:
        if args.only not in label:
            continue
        if form is not None:  # Build() of the preconditioner alone
            plan, t_build = wall(lambda: S.TNSPlan(A, form=form))
            plan.Clear()
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(mk())
        _, t_all = wall(ls.Build)
        if form is None:
            t_build = t_all
        apply_ms = timed_batches(lambda: ls.PrecondApply(r, x), args.reps, args.batches)
        x.Zeros()
        _, t_solve = wall(lambda: ls.Solve(rhs, x))
        it, st = ls.GetIterationCount(), ls.GetSolverStatus()
        x.Zeros()
        _, t_solve2 = wall(lambda: ls.Solve(rhs, x))  # (the first Solve places its vectors; the second is the steady state)
        rows.append((label, apply_ms, t_build, it, st, min(t_solve, t_solve2)))
        ls.Clear()
    return dict(op=opname, n=n, nnz=nnz, spmv=spmv, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--only", default="", help="only the preconditioners whose label contains this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ra.init_rocalution()
    lines = []
    for opname in ("7-point", "27-point"):
        A = ra.LocalMatrix()
        A.GenPoisson7(args.grid) if opname == "7-point" else A.GenLaplace27(args.grid)
        m = measure("%s %d^3" % (opname, args.grid), A, args)
        lines.append("### %s (n = %d, nnz = %d, fp64)" % (m["op"], m["n"], m["nnz"]))
        lines.append("")
        lines.append("SpMV of the operator itself: %.3f ms (min %.3f, max %.3f)" % m["spmv"])
        lines.append("")
        lines.append("| preconditioner | apply ms (median; min - max) | Build() s | CG iterations (status) | CG wall s |")
        lines.append("|---|---|---|---|---|")
        for label, a, tb, it, st, ts in m["rows"]:
            lines.append("| %s | %.3f (%.3f - %.3f) | %.3f | %d (%d) | %.3f |" % (label, a[0], a[1], a[2], tb, it, st, ts))
        lines.append("")
        del A
    text = "\n".join(lines)
    print(text)
    if args.out and os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "tns.md"):
        sys.exit("--out: profiles/tns.md holds hand-written sections; write the tables elsewhere and paste them in")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
