"""Time the setup paths that run the row filter of csrc/csr_filter.hpp: ExtractL, ExtractSubMatrix, Compress, and Build() of
the plans that call them (MultiElimination, AS stacked, BlockPreconditioner fused, TNS stored), fp64, on the 7-point operator
(default 256^3, the default of the other measurement tools).

    python tools/csr_filter_measure.py [--grid 256] [--reps 5]

Wall clock around a drained device, one warm-up and --reps timed repetitions per path; prints one line
"RESULT {path: [seconds, ...], ...}".  One process measures one library: to compare two builds, run the tool in turns with
RAMD_LIB pointing at the other library (rocalution_amd/capi.py) and compare medians against the other's min - max.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import rocalution_amd as ra
    from rocalution_amd import solvers as S
    ra.init_rocalution()

    def wall(fn):
        ra.sync()
        t = time.perf_counter()
        r = fn()
        ra.sync()
        return r, time.perf_counter() - t

    A = ra.LocalMatrix()
    A.GenPoisson7(args.grid)
    n = A.GetM()
    sizes = [n // 16] * 15 + [n - 15 * (n // 16)]

    def tri():
        T = ra.LocalMatrix()
        A.ExtractL(T, False)
        return T

    def sub():
        T = ra.LocalMatrix()
        A.ExtractSubMatrix(n // 3, n // 3, n - n // 3, n - n // 3, T)
        return T

    cases = {
        "ExtractL": tri,
        "ExtractSubMatrix": sub,
        "MEPlan(drop 0.4, stepwise)": lambda: S.MEPlan(A, drop_off=0.4, form=0),
        "ASPlan(nb 8, overlap 4, stacked)": lambda: S.ASPlan(A, 8, 4, form=2),
        "BPPlan(nb 16, fused)": lambda: S.BPPlan(A, sizes, form=1),
        "TNSPlan(stored)": lambda: S.TNSPlan(A, form=0),
    }
    res = {"lib": os.environ.get("RAMD_LIB", "tree"), "grid": args.grid}
    ts = []  # Compress replaces its matrix: a fresh operator per repetition, generated outside the timed part
    for _ in range(args.reps + 1):
        B = ra.LocalMatrix()
        B.GenPoisson7(args.grid)
        ts.append(wall(lambda: B.Compress(1.0))[1])
        assert B.GetNnz() == n  # (the off-diagonal entries are -1: the diagonal stays)
        del B
    res["Compress(1.0)"] = ts[1:]
    for name, fn in cases.items():
        ts = []
        for _ in range(args.reps + 1):
            obj, t = wall(fn)
            ts.append(t)
            if hasattr(obj, "Clear"):
                obj.Clear()
            del obj
        res[name] = ts[1:]
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
