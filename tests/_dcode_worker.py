"""Worker of tests/test_gpu_cg_diag_codes.py: one CG + Jacobi run per process (RAMD_CG_DCODE is read once per process).

    _dcode_worker.py local  <case> <outfile>                       case a / b / c, fp64 and fp32, one device
    _dcode_worker.py global <rank> <world> <initfile> <outdir>     a rank of a Global run over the callback transport
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GLOBAL_N = 12


def case_matrix(case):
    """-> (rp, ci, va, rhs): a the 16^3 Poisson operator of tests/golden/poisson16.npz (its rhs_ones = A 1); b the same with
    a seeded subset of diagonal entries doubled and a second, disjoint one tripled (a non-negative diagonal added to an SPD
    matrix: still SPD; inverse diagonal 1/6, 1/12, 1/18); c tests/golden/rand300.npz, 300 distinct diagonal entries"""
    from rocalution_amd import generators as gen
    if case == "c":
        d = np.load(os.path.join(ROOT, "tests", "golden", "rand300.npz"))
        return d["rowptr"], d["col"], d["val"], d["rhs_ones"]
    rp, ci, va = gen.poisson7(16)
    n = len(rp) - 1
    if case == "a":
        return rp, ci, va, np.load(os.path.join(ROOT, "tests", "golden", "poisson16.npz"))["rhs_ones"]
    va = va.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    diag = np.flatnonzero(ci == rows)
    assert len(diag) == n
    pick = np.random.default_rng(16).permutation(n)
    va[diag[pick[:n // 7]]] *= 2.0
    va[diag[pick[n // 7:n // 7 + n // 11]]] *= 3.0
    import scipy.sparse as sp
    return rp, ci, va, sp.csr_matrix((va, ci, rp), shape=(n, n)) @ np.ones(n)


def dcode_info(vec):
    """(kind, count, n) of the coded form of a device vector"""
    from rocalution_amd import capi
    lib = capi.load()
    h, kind, count, n = C.c_void_p(), C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    capi.check(lib.ramd_dcode_create_from_vector(vec._h, C.byref(h)))
    capi.check(lib.ramd_dcode_info(h, C.byref(kind), C.byref(count), C.byref(n)))
    capi.check(lib.ramd_dcode_destroy(h))
    return kind.value, count.value, n.value


def local(case, outfile):
    import rocalution_amd as ra
    from rocalution_amd import solvers as S
    ra.init_rocalution()
    rp, ci, va, rhs = case_matrix(case)
    n = len(rp) - 1
    out = {}
    for dtype, tag, tol in ((np.float64, "64", 1e-8), (np.float32, "32", 1e-4)):
        A = ra.LocalMatrix(dtype)
        A.SetDataPtrCSR(rp, ci, va.astype(dtype), "A", len(ci), n, n)
        b, x, d = ra.LocalVector(dtype, data=rhs.astype(dtype)), ra.LocalVector(dtype, data=np.zeros(n, dtype)), ra.LocalVector(dtype)
        d.Allocate("d", n)
        A.ExtractInverseDiagonal(d)
        out["form" + tag] = np.array(dcode_info(d))
        ls = S.CG(dtype)
        ls.SetOperator(A)
        ls.SetPreconditioner(S.Jacobi())
        ls.Init(1e-30, tol, 1e8, 200)
        ls.Build()
        ls.Solve(b, x)
        out["x" + tag] = x.numpy()
        out["it" + tag] = np.array([ls.GetIterationCount(), ls.GetSolverStatus()])
        out["hist" + tag] = ls.GetResidualHistory()
    np.savez(outfile, **out)


def global_rank(rank, world, initfile, outdir):
    import torch.distributed as dist
    from rocalution_amd import capi, distributed as D
    import rocalution_amd as ra
    dist.init_process_group(backend="gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    ra.init_rocalution(0)
    comm = D.make_callback_comm(rank, world, dist)
    N = GLOBAL_N
    z0, z1 = (N * rank) // world, (N * (rank + 1)) // world
    g = D.DistributedSolver(comm, capi.SOLVER_CG, capi.PC_JACOBI)
    g.setup_poisson(N, z0, z1)
    g.init(1e-15, 1e-8, 1e8, 500)
    g.build()
    xs = g.solve(None, np.zeros((z1 - z0) * N * N))  # (no rhs: A 1, as the distributed tests use it)
    it, st, res = g.result()
    np.savez(os.path.join(outdir, "r%d.npz" % rank), xs=xs, it=np.array([it, st]), res=np.array([res]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if sys.argv[1] == "local":
        local(sys.argv[2], sys.argv[3])
    else:
        global_rank(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
