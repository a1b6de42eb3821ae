#!/usr/bin/env python3
"""One Chebyshev step timed through the Python bindings (tools/, not product; profiles/chebyshev.md holds the figures).

  chebyshev_step.py --op poisson7|lap27 --n N --form unfused|fused|solver|solver-unfused [--precond jacobi|none]
                    [--steps 30] [--warmup 5] [--root TREE] [--lambda LO HI]

  unfused : the reference's call sequence from public vector / matrix entries -- PointWiseMult, ScaleAdd, AddScale, Apply,
            ScaleAdd(-1, rhs), Norm.  Uses nothing this solver added, so it also runs on a tree from before it (--root).
  fused   : ramd_fused_cheb_direction, Apply, ramd_fused_cheb_residual and the one scalar read.
  solver  : solvers.Chebyshev inside ONE Solve, timed between two iteration marks (as bench.py times CG); solver-unfused: the
            same with SetFused(False).  Prints iterations per second and the residual at the last step.
Every step ends in a blocking read (the norm of the stopping rule), so a step is timed wall-clock from the host; the median
over --steps steps after --warmup is printed as one JSON line.  Run each form in a fresh process; for kernel times run it
under a kernel trace in a run of its own.
The default bounds (0.5, 1.5 with Jacobi; 0.1 and the Gershgorin maximum without) keep the scalars of the recurrence bounded
for any number of steps; the time of a step does not depend on them.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="poisson7", choices=["poisson7", "lap27"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--form", default="fused", choices=["unfused", "fused", "solver", "solver-unfused"])
    ap.add_argument("--precond", default="jacobi", choices=["jacobi", "none"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--lambda", dest="bounds", type=float, nargs=2, default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import rocalution_amd as ra
    from rocalution_amd import capi
    ra.init_rocalution()
    lib = capi.load()

    A = ra.LocalMatrix()
    if a.op == "poisson7":
        A.GenPoisson7(a.n)
        top = 12.0
    else:
        A.GenLaplace27(a.n)
        top = 52.0
    n = A.GetM()
    jac = a.precond == "jacobi"
    lo, hi = a.bounds if a.bounds else ((0.5, 1.5) if jac else (0.1, top))
    d, c = (hi + lo) / 2.0, (hi - lo) / 2.0
    out = dict(op=a.op, n=a.n, rows=n, nnz=A.GetNnz(), ptr_bits=A.GetPtrBits() if hasattr(A, "GetPtrBits") else 32, form=a.form,
               precond=a.precond, bounds=[lo, hi], steps=a.steps, warmup=a.warmup)

    def vec():
        v = ra.LocalVector(); v.Allocate("", n)
        return v

    rhs, x = vec(), vec()
    ones = vec(); ones.Ones()
    A.Apply(ones, rhs)
    del ones

    if a.form.startswith("solver"):
        from rocalution_amd import solvers as S
        ls = S.Chebyshev(); ls.Set(lo, hi); ls.SetFused(a.form == "solver")
        if jac:
            ls.SetPreconditioner(S.Jacobi())
        total = a.warmup + a.steps
        ls.Init(0.0, 0.0, 1e300, total); ls.SetOperator(A); ls.Build()
        ls.SetTimeMark(a.warmup)
        ls.Solve(rhs, x)
        secs = ls.GetSecondsSinceTimeMark()
        hist = ls.GetResidualHistory()
        out.update(iterations=ls.GetIterationCount(), status=ls.GetSolverStatus(), ms_per_iteration=1e3 * secs / a.steps,
                   iterations_per_second=a.steps / secs, initial_residual=float(hist[0]), final_residual=float(hist[-1]))
        print(json.dumps(out))
        return

    r, p = vec(), vec()
    dinv = z = None
    if jac:
        dinv = ra.LocalVector(); A.ExtractInverseDiagonal(dinv)
    if a.form == "unfused" and jac:
        z = vec()

    def residual():
        A.Apply(x, r)
        if a.form == "unfused":
            r.ScaleAdd(-1.0, rhs)
            return r.Norm()
        capi.check(lib.ramd_fused_cheb_residual(r._h, rhs._h, 2))
        rr = C.c_double(0)
        capi.check(lib.ramd_scalars_fetch(C.byref(rr), 2, 1))
        return rr.value ** 0.5

    def direction(alpha, beta, first):
        if a.form == "unfused":
            src = r
            if jac:
                z.PointWiseMult(dinv, r)
                src = z
            if first:
                p.CopyFrom(src)
            else:
                p.ScaleAdd(beta, src)
            x.AddScale(p, alpha)
        else:
            capi.check(lib.ramd_fused_cheb_direction(x._h, p._h, r._h, dinv._h if jac else None, alpha, beta, 1 if first else 0))

    res0 = residual()
    alpha, beta, times = 2.0 / d, 0.0, []
    for k in range(a.warmup + a.steps):
        ra.sync()
        t0 = time.perf_counter()
        direction(alpha, beta, k == 0)
        res = residual()
        times.append(time.perf_counter() - t0)
        beta = (c * alpha / 2.0) ** 2
        alpha = 1.0 / (d - beta)
    t = times[a.warmup:]
    out.update(ms_per_step_median=1e3 * statistics.median(t), ms_per_step_min=1e3 * min(t), ms_per_step_max=1e3 * max(t),
               initial_residual=res0, final_residual=res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
