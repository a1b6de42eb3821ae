"""Measure the AS / RAS preconditioners on the 7-point operator (default 256^3) and the 27-point operator (default 256^3), fp64:
one preconditioner apply, the restriction and prolongation alone, and one GMRES(30) iteration, for AS and RAS with ILU(0) on
every block, nb in {2, 8, 64}, overlap in {0, 4}, in the stepwise, fused and stacked form; plain whole-matrix ILU(0) under
GMRES(30) goes beside them as the baseline.

    python tools/schwarz_measure.py [--grid7 256] [--grid27 256] [--ops 7,27] [--kinds as,ras] [--nb 2,8,64] [--overlap 0,4]
                                    [--forms 0,1,2] [--rounds 2] [--out tables.md]

Every configuration runs in a fresh process (this script with --child), one at a time, and the whole list is gone through
--rounds times in alternating order (forwards, backwards, ...): a configuration's figures are the medians over its runs, and
the spread between the runs is printed next to them.  Apply times: HIP events around batches of --reps applies after a
warm-up batch, the median of --batches batches.  An iteration's time: the wall time of the second Solve() (the first one
places its vectors) over its iteration count.  split / join: algorithmic bytes are 8 (n + S) each -- split reads n and
writes S values, join reads S and writes n.  profiles/schwarz.md quotes the tables next to hand-written text and is refused
as a target.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_batches(ra, capi, fn, reps, batches):
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


def child(args):
    import rocalution_amd as ra
    from rocalution_amd import capi, solvers as S
    ra.init_rocalution()
    A = ra.LocalMatrix()
    A.GenPoisson7(args.grid) if args.op == "7" else A.GenLaplace27(args.grid)
    n = A.GetM()
    r = ra.LocalVector(data=np.random.default_rng(1).uniform(-1, 1, n))
    x = ra.LocalVector(); x.Allocate("", n)
    ones = ra.LocalVector(); ones.Allocate("", n); ones.Ones()
    rhs = ra.LocalVector(); rhs.Allocate("", n)
    A.Apply(ones, rhs)
    res = dict(op=args.op, grid=args.grid, kind=args.kind, nb=args.nb, overlap=args.overlap, form=args.form, n=n)
    if args.kind == "ilu":
        pc = S.ILU()
    else:
        pc = (S.AS if args.kind == "as" else S.RAS)(args.nb, args.overlap, S.ILU()); pc.SetForm(args.form)
    ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.SetBasisSize(30)
    ra.sync(); t = time.perf_counter(); ls.Build(); ra.sync()
    res["build_s"] = time.perf_counter() - t
    res["apply_ms"] = timed_batches(ra, capi, lambda: ls.PrecondApply(r, x), args.reps, args.batches)
    for _ in range(2):
        x.Zeros(); ra.sync(); t = time.perf_counter(); ls.Solve(rhs, x); ra.sync()
        wall = time.perf_counter() - t
    res["iters"], res["status"] = ls.GetIterationCount(), ls.GetSolverStatus()
    res["iter_ms"] = 1e3 * wall / max(res["iters"], 1)
    if args.kind != "ilu":
        info = pc.Info()
        res["form_taken"], res["S"], res["nnz_stacked"] = info["form"], info["stacked_rows"], info["nnz_stacked"]
    ls.Clear()
    if args.kind != "ilu" and args.form == 2:  # restriction and prolongation alone, on the arena
        plan = S.ASPlan(A, args.nb, args.overlap, restricted=args.kind == "ras", form=2)
        total = plan.Info()["stacked_rows"]
        z = ra.LocalVector(); z.Allocate("", total)
        res["split_ms"] = timed_batches(ra, capi, lambda: plan.Split(r, z), args.reps, args.batches)
        res["join_ms"] = timed_batches(ra, capi, lambda: plan.Join(z, x), args.reps, args.batches)
        res["vec_mb"] = 8.0 * (n + total) / 1e6
        plan.Clear()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid7", type=int, default=256)
    ap.add_argument("--grid27", type=int, default=256)
    ap.add_argument("--ops", default="7,27")
    ap.add_argument("--kinds", default="as,ras")
    ap.add_argument("--nb", default="2,8,64")
    ap.add_argument("--overlap", default="0,4")
    ap.add_argument("--forms", default="0,1,2")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--op"); ap.add_argument("--grid", type=int); ap.add_argument("--kind")
    ap.add_argument("--form", type=int, default=-1)
    args, _ = ap.parse_known_args()
    if args.child:
        args.nb, args.overlap = int(args.nb), int(args.overlap)
        return child(args)
    if args.out and os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "schwarz.md"):
        sys.exit("--out: profiles/schwarz.md holds hand-written sections; write the tables elsewhere and paste them in")
    configs = []
    for op in args.ops.split(","):
        grid = args.grid7 if op == "7" else args.grid27
        configs.append((op, grid, "ilu", 1, 0, -1))
        for kind in args.kinds.split(","):
            for nb in args.nb.split(","):
                for ov in args.overlap.split(","):
                    for form in args.forms.split(","):
                        configs.append((op, grid, kind, int(nb), int(ov), int(form)))
    runs = {}
    for rnd in range(args.rounds):
        for cfg in (configs if rnd % 2 == 0 else configs[::-1]):
            op, grid, kind, nb, ov, form = cfg
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--op", op, "--grid", str(grid), "--kind", kind, "--nb", str(nb),
                   "--overlap", str(ov), "--form", str(form), "--reps", str(args.reps), "--batches", str(args.batches)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.child_timeout)
            text = p.stdout.decode()
            line = [l for l in text.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:  # a child that failed ends the measurement: nothing more is started on the device
                sys.exit("configuration %r failed (exit %d):\n%s" % (cfg, p.returncode, text[-2000:]))
            runs.setdefault(cfg, []).append(json.loads(line[0][7:]))
            print(cfg, line[0], flush=True)
    out = []
    for op in args.ops.split(","):
        out += ["### %s-point %d^3 (fp64, GMRES(30), ILU(0) on every block; medians of %d fresh processes, spread in brackets)"
                % (op, args.grid7 if op == "7" else args.grid27, args.rounds), "",
                "| preconditioner | nb | overlap | form | Build() s | apply ms | GMRES iteration ms | iterations (status) | split ms | join ms | "
                "vector MB each | GB/s split / join |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for cfg in configs:
            if cfg[0] != op:
                continue
            rs = runs[cfg]

            def med(key):
                v = [r[key] for r in rs if key in r]
                return ("%.3f [%.3f - %.3f]" % (float(np.median(v)), min(v), max(v))) if v else "-"
            r0 = rs[0]
            bw = "-"
            if "split_ms" in r0:
                sm, jm = np.median([r["split_ms"] for r in rs]), np.median([r["join_ms"] for r in rs])
                bw = "%.0f / %.0f" % (r0["vec_mb"] / sm, r0["vec_mb"] / jm)
            out.append("| %s | %d | %d | %s | %s | %s | %s | %d (%d) | %s | %s | %s | %s |" % (
                {"ilu": "ILU(0), whole matrix", "as": "AS", "ras": "RAS"}[cfg[2]], cfg[3], cfg[4],
                "-" if cfg[2] == "ilu" else str(r0.get("form_taken")), med("build_s"), med("apply_ms"), med("iter_ms"), r0["iters"], r0["status"],
                med("split_ms"), med("join_ms"), ("%.1f" % r0["vec_mb"]) if "vec_mb" in r0 else "-", bw))
        out.append("")
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
