"""GPU parity tests of the Chebyshev iteration (include/rocalution/solvers.hpp: Chebyshev; csrc/fused.hip:
ramd_fused_cheb_direction / ramd_fused_cheb_residual) against the golden runs of the genuine library, the CPU oracle, the
narrow-offset runs and the Local runs.

No reduction feeds the recurrence (alpha and beta come from the two spectral bounds on the host), and the product, the vector
updates and the point-wise product are each bit-exact against the host arithmetic (tests/test_gpu_kernels.py), so the
solution vector is compared BIT FOR BIT everywhere; only the residual norms of the stopping rule see a different summation
order and are held to the history criterion of tests/test_gpu_solvers.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from rocalution_amd import generators as gen
from test_gpu_solvers import _check_hist, _inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the settings of the golden runs (oracle/ref_probe, tests/test_oracle_golden.py): tag -> (lambda_min, lambda_max, max_iter)
GOLDEN_RUNS = {"chebyshev_none": (0.05, 16.0, 60), "chebyshev_jacobi": (0.01, 2.0, 60)}
CASES = ["gr3030", "poisson8", "lap2d7", "poisson16", "poisson32", "lap27_6"]
WITH_X = ["gr3030", "poisson8", "lap2d7", "lap27_6"]  # the fixtures that hold <tag>_x


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


@pytest.fixture(scope="module")
def S():
    from rocalution_amd import solvers
    return solvers


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), "max abs diff %g" % np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))


def _mk(S, tag, bounds, max_iter, fused, dtype=np.float64):
    ls = S.Chebyshev(dtype)
    ls.Set(*bounds); ls.InitMaxIter(max_iter); ls.SetFused(fused)
    if tag.endswith("_jacobi"):
        ls.SetPreconditioner(S.Jacobi())
    return ls


def _run(ra, S, A, rhs_h, tag, bounds, max_iter, fused, dtype=np.float64):
    n = A.GetM()
    ls = _mk(S, tag, bounds, max_iter, fused, dtype); ls.SetOperator(A); ls.Build()
    rhs = ra.LocalVector(dtype, data=np.asarray(rhs_h).astype(dtype)); x = ra.LocalVector(dtype); x.Allocate("", n)
    ls.Solve(rhs, x)
    out = (ls.GetIterationCount(), ls.GetSolverStatus(), ls.GetResidualHistory().copy(), x.numpy())
    ls.Clear()
    return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(GOLDEN_RUNS))
@pytest.mark.parametrize("name", CASES)
def test_chebyshev_vs_golden(ra, S, name, tag, fused):
    """the runs of the genuine library: the same iteration count and status (runs that end on the iteration cap, and the
    one that ends on the divergence limit: lap27_6 without preconditioner, 22 iterations), the history within the solver
    criterion, the solution bit for bit"""
    g = load_golden(name)
    rp, ci, va, _ = _inputs(name, g)
    A = ra.LocalMatrix(); A.SetDataPtrCSR(rp, ci, va)
    lo, hi, cap = GOLDEN_RUNS[tag]
    it, st, hist, x = _run(ra, S, A, g["rhs_ones"], tag, (lo, hi), cap, fused)
    meta = g[tag + "_meta"]
    print(name, tag, fused, "iters", it, int(meta[0]), "status", st, int(meta[1]), "last residual", hist[-1], meta[2])
    assert (it, st) == (int(meta[0]), int(meta[1]))
    assert len(hist) == it + 1 and len(g[tag + "_hist"]) == it  # (the reference's history file holds the first `it` entries)
    _check_hist(hist, g[tag + "_hist"], False)
    assert (tag + "_x" in g) == (name in WITH_X)
    if tag + "_x" in g:
        eq(x, g[tag + "_x"])


def test_chebyshev_golden_set_holds_the_divergent_run():
    """(what the parametrisation above relies on) lap27_6 / chebyshev_none ends on the divergence limit after 22 iterations,
    not within the last bits of a norm of it; every other golden run ends on the iteration cap"""
    for name in CASES:
        g = load_golden(name)
        for tag in GOLDEN_RUNS:
            meta = g[tag + "_meta"]
            if (name, tag) == ("lap27_6", "chebyshev_none"):
                h = g[tag + "_hist"]  # (the residual grows 2.35-fold per step: 0.85e8 of the initial one at step 21, 1.99e8 at 22)
                assert (int(meta[0]), int(meta[1])) == (22, 3) and h[-1] / h[0] < 0.9e8 and meta[2] / h[0] > 1.9e8
            else:
                assert (int(meta[0]), int(meta[1])) == (60, 4)


# a second pair of bounds, from the spectrum of the fixture (rand300: eigenvalues of A in [1.14, 32.6] + small imaginary parts,
# of D^-1 A in [0.69, 1.30]), and another iteration cap
ORACLE_RUNS = {"chebyshev_none": (1.0, 34.0, 45), "chebyshev_jacobi": (0.3, 1.8, 45)}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(ORACLE_RUNS))
def test_chebyshev_vs_oracle_nonsymmetric(ra, S, oracle, tag, fused):
    g = load_golden("rand300")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    b = oracle.csr_apply(rp, ci, va, np.ones(n))
    lo, hi, cap = ORACLE_RUNS[tag]
    pk = oracle.PC_JACOBI if tag.endswith("_jacobi") else oracle.PC_NONE
    ref = oracle.solve(rp, ci, va, b, solver=oracle.CHEBYSHEV, precond=pk, p0=lo, p1=hi, max_iter=cap)
    A = ra.LocalMatrix(); A.SetDataPtrCSR(rp, ci, va)
    it, st, hist, x = _run(ra, S, A, b, tag, (lo, hi), cap, fused)
    print(tag, fused, "iters", it, ref["iters"], "status", st, ref["status"])
    assert it > 10 and (it, st) == (ref["iters"], ref["status"])
    _check_hist(hist, ref["history"], False)
    eq(x, ref["x"])


@pytest.mark.parametrize("tag", sorted(GOLDEN_RUNS))
@pytest.mark.parametrize("name", ["poisson8", "lap27_6"])
def test_chebyshev_fp32_fused_equals_unfused_and_oracle(ra, S, oracle, name, tag):
    """float32 operator and vectors: the fused and the unfused step leave the same x bit for bit (and not the start vector),
    and -- oracle.solve accepts float32 inputs for this solver and runs its float instantiation -- the oracle's x as well"""
    g = load_golden(name)
    rp, ci = g["rowptr"], g["col"]
    va, b = g["val"].astype(np.float32), g["rhs_ones"].astype(np.float32)
    lo, hi, cap = GOLDEN_RUNS[tag]
    A = ra.LocalMatrix(np.float32); A.SetDataPtrCSR(rp, ci, va)
    runs = [_run(ra, S, A, b, tag, (lo, hi), cap, fused, np.float32) for fused in (True, False)]
    (it0, st0, h0, x0), (it1, st1, h1, x1) = runs
    assert x0.dtype == np.float32 and it0 > 3 and (it0, st0) == (it1, st1)
    eq(x0, x1)
    assert np.any(x0 != 0.0)
    pk = oracle.PC_JACOBI if tag.endswith("_jacobi") else oracle.PC_NONE
    ref = oracle.solve(rp, ci, va, b, solver=oracle.CHEBYSHEV, precond=pk, p0=lo, p1=hi, max_iter=cap)
    assert ref["x"].dtype == np.float32
    print(name, tag, "iters", it0, ref["iters"], "status", st0, ref["status"])
    assert (it0, st0) == (ref["iters"], ref["status"])
    eq(x0, ref["x"])


def _fixture(name):
    if name == "poisson16":
        return gen.poisson7(16)
    g = load_golden(name)
    return g["rowptr"], g["col"], g["val"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(GOLDEN_RUNS))
@pytest.mark.parametrize("name", ["poisson16", "lap27_6"])
def test_wide_chebyshev_equals_the_narrow_run(ra, S, name, tag, fused):
    """an operator with 64-bit row offsets: Chebyshev needs the product and vector updates only, so history, iteration count
    and solution equal the narrow run's exactly, and the operator stays wide"""
    rp, ci, va = _fixture(name)
    lo, hi, cap = GOLDEN_RUNS[tag]
    runs = []
    for wide in (False, True):
        A = ra.LocalMatrix(); A.SetDataPtrCSR(rp, ci, va)
        if wide:
            A.ForceWide()
        assert A.GetPtrBits() == (64 if wide else 32)
        n = A.GetM()
        rhs = ra.LocalVector(); rhs.Allocate("", n)
        A.Apply(ra.LocalVector(data=np.ones(n)), rhs)
        runs.append(_run(ra, S, A, rhs.numpy(), tag, (lo, hi), cap, fused))
        assert A.GetPtrBits() == (64 if wide else 32)
    (it0, st0, h0, x0), (it1, st1, h1, x1) = runs
    assert it0 > 3 and (it1, st1) == (it0, st0)
    eq(h1, h0); eq(x1, x0)


def test_chebyshev_with_a_general_preconditioner_fused_equals_unfused(ra, S):
    """a preconditioner that is not Jacobi runs between the two kernels and hands its z to the direction update"""
    g = load_golden("poisson8")
    A = ra.LocalMatrix(); A.SetDataPtrCSR(g["rowptr"], g["col"], g["val"])
    n = A.GetM()
    xs = []
    for fused in (True, False):
        ls = S.Chebyshev(); ls.Set(0.2, 1.2); ls.InitMaxIter(25); ls.SetFused(fused); ls.SetPreconditioner(S.ILU())
        ls.SetOperator(A); ls.Build()
        x = ra.LocalVector(); x.Allocate("", n)
        ls.Solve(ra.LocalVector(data=g["rhs_ones"]), x)
        xs.append((ls.GetIterationCount(), ls.GetSolverStatus(), x.numpy()))
    assert xs[0][0] > 3 and xs[0][:2] == xs[1][:2]
    eq(xs[0][2], xs[1][2])


def test_chebyshev_misuse(ra, S):
    """Solve() before Set() is an error status, not an abort, and the library goes on working; a non-square operator is
    refused by ramd_solver_build as for every solver"""
    g = load_golden("poisson8")
    A = ra.LocalMatrix(); A.SetDataPtrCSR(g["rowptr"], g["col"], g["val"])
    n = A.GetM()
    rhs = ra.LocalVector(data=g["rhs_ones"])
    for pc in (None, S.Jacobi):
        ls = S.Chebyshev(); ls.SetOperator(A)
        if pc:
            ls.SetPreconditioner(pc())
        ls.Build()
        x = ra.LocalVector(); x.Allocate("", n)
        with pytest.raises(ra.RamdError):
            ls.Solve(rhs, x)
        assert not x.numpy().any()
    ls = S.Chebyshev(); ls.Set(0.05, 16.0); ls.InitMaxIter(60); ls.SetOperator(A); ls.Build()
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    eq(x.numpy(), g["chebyshev_none_x"])
    rp = np.array([0, 1, 2], np.int32); ci = np.array([0, 2], np.int32); va = np.array([1.0, 2.0])
    R = ra.LocalMatrix(); R.SetDataPtrCSR(rp, ci, va, nrow=2, ncol=3)
    bad = S.Chebyshev(); bad.Set(0.5, 2.0); bad.SetOperator(R)
    with pytest.raises(ra.RamdError):
        bad.Build()
    cg = S.CG(); cg.SetOperator(A); cg.SetPreconditioner(S.Jacobi()); cg.Build()
    x.Zeros(); cg.Solve(rhs, x)
    assert cg.GetSolverStatus() == 2 and np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-3


def _gxx(tmp_path, src, std="c++14"):
    exe = str(tmp_path / os.path.splitext(os.path.basename(src))[0])
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=" + std, "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-o", exe,
                           "-L" + libdir, "-lrocalution_amd", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_cpp_sample_driver_runs_chebyshev(tmp_path):
    """samples/krylov_driver.cpp: the `chebyshev` name it lists, on the generated Poisson operator with its documented default
    bounds (none, jacobi) and with bounds from the command line"""
    exe = _gxx(tmp_path, os.path.join("samples", "krylov_driver.cpp"))
    seen = {}
    for args in (["none"], ["jacobi"], ["jacobi", "csr", "0", "0.01", "2.0"]):
        r = subprocess.run([exe, "poisson:16", "chebyshev"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-2000:]
        m = re.search(r"RESULT solver=chebyshev precond=(\w+) .*iters=(\d+) status=(\d+) residual=(\S+)", out)
        assert m and m.group(1) == args[0] and int(m.group(2)) > 3 and int(m.group(3)) in (2, 3, 4), out[-2000:]
        assert ("PChebyshev" if args[0] == "jacobi" else "Chebyshev (non-precond)") in out
        seen[tuple(args)] = m.groups()
    assert seen[("jacobi",)] == seen[("jacobi", "csr", "0", "0.01", "2.0")]  # (the documented defaults)
    r = subprocess.run([exe, "poisson:16", "chebyshev", "ilu"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 2 and b"needs lambda_min lambda_max" in r.stdout


def _read_run(path):
    """a file of tests/drivers/global_chebyshev_driver.cpp: 'iters status', the history, the solution (%.17g: exact)"""
    with open(path) as f:
        it, st, nh, nx = (int(t) for t in f.readline().split())
        vals = np.array(f.read().split(), dtype=np.float64)
    assert len(vals) == nh + nx
    return it, st, vals[:nh], vals[nh:]


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_global_chebyshev_over_1_2_4_ranks(tmp_path, pc):
    """tests/drivers/global_chebyshev_driver.cpp: Chebyshev<GlobalMatrix, GlobalVector> on 1, 2 and 4 ranks of a row-block
    split, all on one device, halo and scalar sums through the callback transport, next to the LocalMatrix run.

    History: every entry within 1e-12 relative of the Local one (the bound tests/drivers/distribute_driver.cpp holds the
    Global CG residual to: the norm is the all-reduced sum of the ranks' sums of squares, a different summation order).
    One rank: no ghost part, so x equals the Local x bit for bit.  Several ranks: GlobalMatrix::Apply adds the ghost part
    of a row to the finished interior sum, (a1 + ... + a5) + (a0 + a6) instead of the left-to-right sum over the whole row,
    so a product may differ from the Local one in the last bit (tests/test_gpu_distributed.py holds it to rtol 1e-13 for
    that reason) and x is NOT bit-identical across rank counts.  Bound used here: each of the <= 40 steps adds a few
    rounding errors of relative size 1.1e-16 to x through alpha * p; 40 steps x a few ulp = ~2e-14 of max|x|, held to 1e-12."""
    exe = _gxx(tmp_path, os.path.join("tests", "drivers", "global_chebyshev_driver.cpp"), std="c++17")
    lo, hi = {"none": ("0.05", "12.0"), "jacobi": ("0.3", "1.7")}[pc]  # (the operator's spectrum lies in (0, 12), Jacobi's in (0, 2))
    runs = {}
    for world in (0, 1, 2, 4):  # 0: the LocalMatrix run
        out = str(tmp_path / ("run_%s_%d.txt" % (pc, world)))
        r = subprocess.run([exe, str(world), "12", pc, lo, hi, "40", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0 and b"global_chebyshev_driver ok" in r.stdout, r.stdout.decode()[-3000:]
        runs[world] = _read_run(out)
    it0, st0, h0, x0 = runs[0]
    assert it0 == 40 and st0 == 4 and len(h0) == 41 and len(x0) == 12 ** 3 and np.any(x0 != 0.0)
    eq(runs[1][3], x0)
    for world in (1, 2, 4):
        it, st, h, x = runs[world]
        assert (it, st) == (it0, st0)
        print(pc, world, "history max rel diff", np.max(np.abs(h / h0 - 1)), "x max abs diff", np.max(np.abs(x - x0)),
              "bit-identical" if np.array_equal(x, x0) else "differs in the last bits")
        assert np.all(np.abs(h - h0) <= 1e-12 * np.abs(h0))
        assert np.all(np.abs(x - x0) <= 1e-12 * np.max(np.abs(x0)))


# ---------------------------------------------------------------- the two kernels themselves, through the C ABI
def _np_direction(x, p, z, dinv, alpha, beta, first):
    """the unfused expressions, every operation rounded in the vectors' type: PointWiseMult, ScaleAdd (or the copy), AddScale"""
    t = x.dtype.type
    zz = dinv * z if dinv is not None else z
    pn = zz.copy() if first else t(beta) * p + zz
    return x + t(alpha) * pn, pn


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 3, 5, 49, 1023, 4099, 2 * 1024 * 4 + 7])
def test_cheb_kernels_against_numpy(ra, dtype, n):
    """ramd_fused_cheb_direction (first / later step, with and without dinv) and ramd_fused_cheb_residual called directly: sizes
    below one 16-byte packet, not a multiple of it (the scalar tail of both value types), and beyond one workgroup's share.
    Vectors bit for bit; the sum of squares against numpy's within 1e-12 relative (at most 8199 terms of one sign: the
    summation order moves it by less than n x 1.1e-16)."""
    from rocalution_amd import capi
    lib = capi.load()
    rng = np.random.default_rng(100 + n)
    mk = lambda: rng.uniform(-2.0, 2.0, n).astype(dtype)
    alpha, beta = 0.8125 / 3.0, 0.3 / 7.0
    for first in (1, 0):
        for with_dinv in (True, False):
            x0, p0, z0, d0 = mk(), mk(), mk(), mk()
            x, p, z, d = (ra.LocalVector(dtype, data=v) for v in (x0, p0, z0, d0))
            capi.check(lib.ramd_fused_cheb_direction(x._h, p._h, z._h, d._h if with_dinv else None, alpha, beta, first))
            xr, pr = _np_direction(x0, p0, z0, d0 if with_dinv else None, alpha, beta, first)
            eq(p.numpy(), pr); eq(x.numpy(), xr)
            eq(z.numpy(), z0); eq(d.numpy(), d0)
    r0, b0 = mk(), mk()
    r, b = ra.LocalVector(dtype, data=r0), ra.LocalVector(dtype, data=b0)
    capi.check(lib.ramd_scalars_set(5, -1.0))
    capi.check(lib.ramd_fused_cheb_residual(r._h, b._h, 5))
    rr = C.c_double(0)
    capi.check(lib.ramd_scalars_fetch(C.byref(rr), 5, 1))
    ref = dtype(-1) * r0 + b0
    eq(r.numpy(), ref); eq(b.numpy(), b0)
    want = float(np.sum(ref.astype(np.float64) ** 2))
    assert abs(rr.value - want) <= 1e-12 * want, (rr.value, want)


def test_cheb_kernels_refuse_bad_arguments(ra):
    from rocalution_amd import capi
    lib = capi.load()
    v = [ra.LocalVector(data=np.ones(40)) for _ in range(4)]
    short, single = ra.LocalVector(data=np.ones(39)), ra.LocalVector(np.float32, data=np.ones(40, np.float32))
    x, p, z, d = (t._h for t in v)
    bad = [(x, x, z, d), (x, p, x, d), (x, p, p, d), (x, p, z, x), (x, p, z, p), (x, short._h, z, d), (x, p, short._h, d),
           (x, p, z, short._h), (x, p, single._h, d), (x, p, z, single._h), (None, p, z, d), (x, None, z, d), (x, p, None, d)]
    for args in bad:
        assert lib.ramd_fused_cheb_direction(*args, 0.5, 0.25, 0) == capi.ERR_ARG
    for args in ((x, x, 2), (x, short._h, 2), (x, single._h, 2), (x, p, -1), (x, p, 512), (None, p, 2), (x, None, 2)):
        assert lib.ramd_fused_cheb_residual(*args) == capi.ERR_ARG
    for t in v:
        eq(t.numpy(), np.ones(40))
    e = [ra.LocalVector() for _ in range(3)]  # empty vectors: nothing to do, the slot is zero
    for t in e:
        t.Allocate("", 0)
    capi.check(lib.ramd_fused_cheb_direction(e[0]._h, e[1]._h, e[2]._h, None, 0.5, 0.25, 1))
    capi.check(lib.ramd_scalars_set(2, 3.0)); capi.check(lib.ramd_fused_cheb_residual(e[0]._h, e[1]._h, 2))
    rr = C.c_double(-1)
    capi.check(lib.ramd_scalars_fetch(C.byref(rr), 2, 1))
    assert rr.value == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tag", sorted(GOLDEN_RUNS))
def test_fused_solve_runs_the_fused_kernels(ra, S, tag, dtype):
    """fused and unfused leave the same x by construction, so which of them ran is read off the scalar record: the fused step
    leaves ||r||^2 of its last residual in slot 2 (and nothing else writes there in such a solve), the unfused sequence does
    not touch it.  lap2d7 has 49 rows: the scalar tail of both value types inside a solve."""
    from rocalution_amd import capi
    lib = capi.load()
    g = load_golden("lap2d7")
    A = ra.LocalMatrix(dtype); A.SetDataPtrCSR(g["rowptr"], g["col"], g["val"].astype(dtype))
    assert A.GetM() == 49
    lo, hi, cap = GOLDEN_RUNS[tag]
    rr = C.c_double(0)
    xs = []
    for fused in (False, True):
        capi.check(lib.ramd_scalars_set(2, -7.0))
        it, st, hist, x = _run(ra, S, A, g["rhs_ones"], tag, (lo, hi), 12, fused, dtype)
        capi.check(lib.ramd_scalars_fetch(C.byref(rr), 2, 1))
        if fused:
            assert it == 12 and float(dtype(np.sqrt(rr.value))) == hist[-1], (rr.value, hist[-1])
        else:
            assert rr.value == -7.0
        xs.append(x)
    eq(xs[0], xs[1])
