"""Measure the MultiElimination preconditioner on the 7-point operator (default 256^3) and the 27-point operator (default 128^3),
fp64, one process:

  - Build(): MaximalIndependentSet alone (with its rounds), one elimination plan (set + blocks + Schur complement), and the whole
    CG Build() with Jacobi / MultiColoredILU(0) as the last block;
  - one elimination level's apply (down + up, the last-block solve left out) in the stepwise and in the fused form, next to
    the bytes of E, F and the vectors (algorithmic: every array read or written once) and the bandwidth that implies;
  - CG iterations and wall time for ME(Jacobi) and ME(MultiColoredILU(0)) beside plain Jacobi and MultiColoredILU.

    python tools/multielim_measure.py [--grid7 256] [--grid27 128] [--out tables.md]

Apply times: HIP events around batches of `--reps` applies after a warm-up batch, the median of `--batches` batches.
profiles/multielim.md quotes the tables next to hand-written text and is refused as a target.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    n, nnz = A.GetM(), A.GetNnz()
    out = ["### %s (n = %d, nnz = %d, fp64)" % (opname, n, nnz), ""]
    r = ra.LocalVector(data=np.random.default_rng(1).uniform(-1, 1, n))
    x = ra.LocalVector(); x.Allocate("", n)
    ones = ra.LocalVector(); ones.Allocate("", n); ones.Ones()
    rhs = ra.LocalVector(); rhs.Allocate("", n)
    A.Apply(ones, rhs)
    spmv = timed_batches(lambda: A.Apply(r, x), args.reps, args.batches)
    (size, _, info), t_mis = wall(A.MaximalIndependentSet)
    out.append("SpMV of the operator: %.3f ms.  MaximalIndependentSet: %.3f s, %d rounds on the device (host sweep: %d), size %d of %d."
               % (spmv[0], t_mis, info["rounds"], info["host_sweep"], size, n))
    out.append("")
    out.append("| form | plan Build() s | apply ms (median; min - max) | algorithmic MB | GB/s at that |")
    out.append("|---|---|---|---|---|")
    for form, label in ((0, "stepwise"), (1, "fused")):
        plan, t_plan = wall(lambda: S.MEPlan(A, form=form))
        pi = plan.Info()
        m2 = n - pi["size"]
        rhs2 = ra.LocalVector(); rhs2.Allocate("", m2)
        x2 = ra.LocalVector(data=np.random.default_rng(2).uniform(-1, 1, m2))

        def both():
            plan.Down(r, rhs2)
            plan.Up(r, x2, x)
        t = timed_batches(both, args.reps, args.batches)
        # E and F: value + column per entry, an offset per row; vectors: rhs twice, rhs2, x2, x, inv_D; q twice (fused) or
        # the permutation twice (stepwise)
        mb = (12.0 * pi["nnz_ef"] + 4.0 * (n + 2) + 8.0 * (2 * n + m2 + m2 + n + pi["size"]) + 4.0 * 2 * n) / 1e6
        out.append("| %s | %.3f | %.3f (%.3f - %.3f) | %.1f | %.0f |" % (label, t_plan, t[0], t[1], t[2], mb, mb / t[0]))
        plan.Clear()
        del rhs2, x2
    out.append("")
    out.append("| preconditioner | Build() s | apply ms (median; min - max) | CG iterations (status) | CG wall s |")
    out.append("|---|---|---|---|---|")
    cases = [("Jacobi", S.Jacobi), ("MultiColoredILU(0)", S.MultiColoredILU),
             ("ME(Jacobi, 1)", lambda: S.MultiElimination(S.Jacobi(), 1, 0.0)),
             ("ME(Jacobi, 2)", lambda: S.MultiElimination(S.Jacobi(), 2, 0.0)),
             ("ME(MultiColoredILU(0), 1)", lambda: S.MultiElimination(S.MultiColoredILU(), 1, 0.0)),
             ("ME(MultiColoredILU(0), 2, 0.4)", lambda: S.MultiElimination(S.MultiColoredILU(), 2, 0.4))]
    for label, mk in cases:
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(mk())
        _, t_build = wall(ls.Build)
        apply_ms = timed_batches(lambda: ls.PrecondApply(r, x), args.reps, args.batches)
        x.Zeros()
        _, t1 = wall(lambda: ls.Solve(rhs, x))
        it, st = ls.GetIterationCount(), ls.GetSolverStatus()
        x.Zeros()
        _, t2 = wall(lambda: ls.Solve(rhs, x))  # (the first Solve places its vectors; the second is the steady state)
        out.append("| %s | %.3f | %.3f (%.3f - %.3f) | %d (%d) | %.3f |" % (label, t_build, apply_ms[0], apply_ms[1], apply_ms[2], it, st,
                                                                          min(t1, t2)))
        ls.Clear()
        print(out[-1], flush=True)
    out.append("")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid7", type=int, default=256)
    ap.add_argument("--grid27", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out and os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "multielim.md"):
        sys.exit("--out: profiles/multielim.md holds hand-written sections; write the tables elsewhere and paste them in")
    ra.init_rocalution()
    lines = []
    for opname, grid in (("7-point", args.grid7), ("27-point", args.grid27)):
        A = ra.LocalMatrix()
        A.GenPoisson7(grid) if opname == "7-point" else A.GenLaplace27(grid)
        lines += measure("%s %d^3" % (opname, grid), A, args)
        del A
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
