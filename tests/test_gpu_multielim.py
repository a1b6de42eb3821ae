"""MultiElimination on the device: MaximalIndependentSet, Compress and the Schur complement bit for bit against the genuine
library's arrays (tests/golden/multielim, recorded by tests/drivers/multielim_probe.cpp); the two forms of the apply against
each other, against the composition written out with the public primitives and against the library's Solve; the class
through the C table and the reference-style driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _multielim_ref as ref
from test_cpu_multielim import ROOT, SIX, SYMMETRIC, csr, load, same_bits
from test_gpu_solvers import _check_hist, _write_mtx

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


@pytest.fixture(scope="module")
def S():
    from rocalution_amd import solvers
    return solvers


def _mat(ra, rp, ci, va, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va).astype(dtype))
    return A


def _op(ra, g, dtype=np.float64):
    return _mat(ra, g["rowptr"], g["col"], g["val"], dtype)


def _vec(ra, a, dtype):
    return ra.LocalVector(dtype, data=np.asarray(a).astype(dtype))


def _zeros(ra, n, dtype):
    v = ra.LocalVector(dtype); v.Allocate("", n)
    return v


def _sfx(dtype):
    return "" if dtype == np.float64 else "_f32"


def _same_csr(M, g, key):
    rp, ci, va = M.CopyToCSR()
    assert np.array_equal(rp, g[key + "_rowptr"]) and np.array_equal(ci, g[key + "_col"]), key
    same_bits(va, g[key + "_val"])
    assert M.GetM() == g[key + "_shape"][0] and M.GetN() == g[key + "_shape"][1]


def _chain(n):
    rp, ci, va = [0], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                ci.append(j); va.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va)


# ------------------------------------------------------------------------------------------------ MaximalIndependentSet
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SIX)
def test_maximal_independent_set_equals_the_golden(ra, name, dtype):
    """size and perm of the genuine library; the four symmetric operators and the chain through the device fixed point,
    rand300u (structurally unsymmetric) through the host sweep"""
    g = load(name)
    size, perm, info = _op(ra, g, dtype).MaximalIndependentSet()
    assert size == g["size" + _sfx(dtype)][0] and np.array_equal(perm.numpy(), g["perm" + _sfx(dtype)])
    assert info["members"] == size
    if name == "rand300u":
        assert info["host_sweep"] == 1 and info["symmetric"] == 0 and info["rounds"] == 0
    else:
        assert info["host_sweep"] == 0 and info["symmetric"] == 1 and 1 <= info["rounds"] <= len(g["rowptr"]) - 1


def test_chain_whose_rounds_run_out_takes_the_host_finish(ra):
    """a chain of 4096 rows needs a round per row in the worst case: with max_rounds = 8 the host sweep finishes, with the
    default the device does; both give the closed form (the even rows)"""
    n = 4096
    A = _mat(ra, *_chain(n))
    expect = np.where(np.arange(n) % 2 == 0, np.arange(n) // 2, n // 2 + np.arange(n) // 2).astype(np.int32)
    size, perm, info = A.MaximalIndependentSet(max_rounds=8)
    assert info["host_sweep"] == 1 and info["symmetric"] == 1 and info["rounds"] == 8
    assert size == n // 2 and np.array_equal(perm.numpy(), expect)
    size, perm, info = A.MaximalIndependentSet()
    assert info["host_sweep"] == 0 and 1 <= info["rounds"] <= n
    assert size == n // 2 and np.array_equal(perm.numpy(), expect)


def test_rand300_is_refused_and_stays_usable(ra, S):
    """the reference's sweep overwrites members there (92 joined, 42 left): no permutation, RAMD_ERR_REFUSED with the reason"""
    from conftest import load_golden
    from rocalution_amd import capi
    g = load_golden("rand300")
    A = _op(ra, g)
    with pytest.raises(capi.RamdError) as ei:
        A.MaximalIndependentSet()
    assert ei.value.status == capi.ERR_REFUSED and "not structurally symmetric" in str(ei.value)
    with pytest.raises(capi.RamdError) as ei:
        S.MEPlan(A)
    assert ei.value.status == capi.ERR_REFUSED
    y = _zeros(ra, A.GetM(), np.float64)
    A.Apply(_vec(ra, g["x"], np.float64), y)
    assert np.array_equal(y.numpy(), g["spmv_csr"])


# ------------------------------------------------------------------------------------------------ Compress
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SIX)
def test_compress_equals_the_golden(ra, name, dtype):
    g = load(name)
    sfx, drop = _sfx(dtype), float(g["drop"][0])
    A = _op(ra, g, dtype)
    A.Compress(drop)
    _same_csr(A, g, "cmp" + sfx)
    AA = _mat(ra, *csr(g, "aa0" + sfx), dtype)
    AA.Compress(drop)
    _same_csr(AA, g, "aad" + sfx)
    # drop 0 keeps every non-zero entry (and the diagonal), a huge drop exactly the diagonal
    rp, ci, va = csr(g, "aa0" + sfx)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    for d, keep in ((0.0, (va != 0) | (ci == rows)), (1e300, ci == rows)):
        M = _mat(ra, rp, ci, va, dtype)
        M.Compress(d)
        r2, c2, v2 = M.CopyToCSR()
        assert np.array_equal(c2, ci[keep]) and np.array_equal(np.diff(r2), np.bincount(rows[keep], minlength=len(rp) - 1))
        same_bits(v2, va[keep])
    assert np.all(np.diff(r2) == 1)


# ------------------------------------------------------------------------------------------------ the Schur complement
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SIX)
def test_schur_complement_equals_the_golden(ra, S, name, dtype):
    g = load(name)
    for key, drop in (("aa0", 0.0), ("aad", float(g["drop"][0]))):
        plan = S.MEPlan(_op(ra, g, dtype), drop_off=drop)
        info = plan.Info()
        assert info["size"] == g["size"][0] and info["rows"] == len(g["rowptr"]) - 1
        AA = plan.Schur()
        _same_csr(AA, g, key + _sfx(dtype))
        assert info["nnz_aa"] == AA.GetNnz()


# ------------------------------------------------------------------------------------------------ the apply
def _jacobi(ra, AA, rhs2, dtype):
    """x2 = rhs2 * inv_diag(AA), as Jacobi::Solve"""
    d = ra.LocalVector(dtype)
    AA.ExtractInverseDiagonal(d)
    x2 = _zeros(ra, AA.GetM(), dtype)
    x2.CopyFrom(rhs2)
    x2.PointWiseMult(d)
    return x2


def _apply(ra, S, A, rhs, dtype, levels, form, fmt=None):
    """MultiElimination(Jacobi, levels).Solve composed from plans"""
    plan = S.MEPlan(A, form=form)
    if fmt is not None:
        plan.ConvertTo(fmt)
    info = plan.Info()
    assert info["form"] == form or form == -1
    AA = plan.Schur()
    m2 = info["rows"] - info["size"]
    rhs2 = _zeros(ra, m2, dtype)
    plan.Down(rhs, rhs2)
    if m2 == 0:
        x2 = _zeros(ra, 0, dtype)
    elif levels > 1:
        x2 = _apply(ra, S, AA, rhs2, dtype, levels - 1, form, fmt)
    else:
        x2 = _jacobi(ra, AA, rhs2, dtype)
    x = _zeros(ra, info["rows"], dtype)
    plan.Up(rhs, x2, x)
    return x


def _composed(ra, A, rhs, dtype, levels=1):
    """`levels` eliminations written out with the public primitives, step by step as the reference's Build() and Solve()"""
    n = A.GetM()
    size, perm, _ = A.MaximalIndependentSet()
    P = ra.LocalMatrix(dtype); P.CloneFrom(A)
    P.Permute(perm)
    D, F, E, Cm, AA = (ra.LocalMatrix(dtype) for _ in range(5))
    P.ExtractSubMatrix(0, 0, size, size, D)
    P.ExtractSubMatrix(0, size, size, n - size, F)
    P.ExtractSubMatrix(size, 0, n - size, size, E)
    P.ExtractSubMatrix(size, size, n - size, n - size, Cm)
    inv_d = ra.LocalVector(dtype)
    D.ExtractInverseDiagonal(inv_d)
    E.DiagonalMatrixMultR(inv_d)
    AA.MatrixMult(E, F)
    AA.MatrixAdd(Cm, -1.0, 1.0, True)
    rhs_, x_ = _zeros(ra, n, dtype), _zeros(ra, n, dtype)
    x1, rhs2 = _zeros(ra, size, dtype), _zeros(ra, n - size, dtype)
    rhs_.CopyFromPermute(rhs, perm)
    x1.CopyFrom(rhs_, 0, 0, size)
    rhs2.CopyFrom(rhs_, size, 0, n - size)
    E.ApplyAdd(x1, -1.0, rhs2)
    x2 = _composed(ra, AA, rhs2, dtype, levels - 1) if levels > 1 else _jacobi(ra, AA, rhs2, dtype)
    F.ApplyAdd(x2, -1.0, x1)
    x1.PointWiseMult(inv_d)
    x_.CopyFrom(x1, 0, 0, size)
    x_.CopyFrom(x2, 0, size, n - size)
    x = _zeros(ra, n, dtype)
    x.CopyFromPermuteBackward(x_, perm)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SIX)
def test_apply_forms_agree_with_each_other_and_the_library(ra, S, name, dtype):
    """fused == stepwise == stepwise with E and F in ELL == the composition from public primitives == the genuine library's
    Solve, bit for bit, with one and with two eliminations (path9: n - size = 4, then 2)"""
    g = load(name)
    A = _op(ra, g, dtype)
    rhs = _vec(ra, g["rhs"], dtype)
    for levels in (1, 2):
        gold = g["me%d_x%s" % (levels, _sfx(dtype))]
        same_bits(_composed(ra, A, rhs, dtype, levels).numpy(), gold)
        for form, fmt in ((1, None), (0, None), (0, ra.ELL)):
            same_bits(_apply(ra, S, A, rhs, dtype, levels, form, fmt).numpy(), gold)
    same_bits(_apply(ra, S, A, rhs, dtype, 1, -1).numpy(), g["me1_x" + _sfx(dtype)])  # auto is one of the two


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_on_a_1x1_operator_and_aliasing_refused(ra, S, dtype):
    from rocalution_amd import capi
    A = _mat(ra, [0, 1], [0], [4.0], dtype)
    rhs = _vec(ra, [3.0], dtype)
    for form in (0, 1):
        plan = S.MEPlan(A, form=form)
        assert plan.Info()["size"] == 1 and plan.Schur().GetM() == 0
        e = _zeros(ra, 0, dtype)
        plan.Down(rhs, e)
        x = _zeros(ra, 1, dtype)
        plan.Up(rhs, e, x)
        assert x.numpy()[0] == dtype(3.0) * (dtype(1) / dtype(4.0))
        with pytest.raises(capi.RamdError) as ei:
            plan.Up(rhs, e, rhs)
        assert ei.value.status == capi.ERR_ARG
    g = load("lap2d7")
    plan = S.MEPlan(_op(ra, g, dtype), form=1)  # (the fused form reads CSR: a conversion is refused)
    n, size = plan.Info()["rows"], plan.Info()["size"]
    v, x2 = _vec(ra, g["rhs"], dtype), _zeros(ra, n - size, dtype)
    for bad in (lambda: plan.Up(v, x2, v), lambda: plan.Down(v, v), lambda: plan.Up(v, _zeros(ra, n, dtype), _zeros(ra, n, dtype)),
                lambda: plan.ConvertTo(ra.ELL)):
        with pytest.raises(capi.RamdError):
            bad()


# ------------------------------------------------------------------------------------------------ solvers
def _ones_rhs(ra, A, dtype=np.float64):
    n = A.GetM()
    rhs = _zeros(ra, n, dtype)
    A.Apply(_vec(ra, np.ones(n), dtype), rhs)
    return rhs


@pytest.mark.parametrize("name", SYMMETRIC)
def test_cg_multielim_mcilu_vs_reference(ra, S, name):
    """CG + MultiElimination(MultiColoredILU(0), 2, drop): iterations within one of the genuine library's, status equal,
    the residual history to 1e-5 against the 6-digit history file and x = 1, both the bars test_gpu_rsamg holds a Krylov
    run with a nested preconditioner to"""
    g = load(name)
    A = _op(ra, g)
    n = A.GetM()
    ls = S.CG()
    ls.SetPreconditioner(S.MultiElimination(S.MultiColoredILU(), 2, float(g["drop"][0])))
    ls.SetOperator(A); ls.Build()
    x = _zeros(ra, n, np.float64)
    ls.Solve(_ones_rhs(ra, A), x)
    meta = g["cg_me_meta"]
    print(name, "iterations", ls.GetIterationCount(), "golden", int(meta[0]), "status", ls.GetSolverStatus(), int(meta[1]))
    assert abs(ls.GetIterationCount() - int(meta[0])) <= 1 and ls.GetSolverStatus() == int(meta[1])
    assert int(meta[1]) in (1, 2)
    assert np.linalg.norm(x.numpy() - 1.0) < 1e-3 and np.linalg.norm(x.numpy() - g["cg_me_x"]) < 1e-3
    hist, gold = np.asarray(ls.GetResidualHistory()), g["cg_me_hist"]
    m = min(len(hist), len(gold)) - 2
    print(name, "history: largest relative deviation %.2e" % (np.max(np.abs(hist[:m] / gold[:m] - 1)) if m > 0 else 0.0))
    _check_hist(hist, gold, False, rtol=1e-5)


def test_gmres_multielim_jacobi_on_rand300u(ra, S):
    g = load("rand300u")
    A = _op(ra, g)
    n = A.GetM()
    ls = S.GMRES(); ls.SetBasisSize(30)
    ls.SetPreconditioner(S.MultiElimination(S.Jacobi(), 1, 0.0))
    ls.SetOperator(A); ls.Build()
    rhs, x = _ones_rhs(ra, A), _zeros(ra, n, np.float64)
    ls.Solve(rhs, x)
    r = _zeros(ra, n, np.float64)
    A.Apply(x, r)
    assert ls.GetSolverStatus() in (1, 2)
    assert np.linalg.norm(r.numpy() - rhs.numpy()) < 1e-5 * np.linalg.norm(rhs.numpy())


def _table_apply(ra, S, A, rhs, dtype, levels, drop=0.0, fmt=None, last=None):
    ls = S.CG(dtype)
    pc = S.MultiElimination(last or S.Jacobi(), levels, drop)
    if fmt is not None:
        pc.SetPrecondMatrixFormat(fmt)
    ls.SetPreconditioner(pc); ls.SetOperator(A); ls.Build()
    x = _zeros(ra, A.GetM(), dtype)
    ls.PrecondApply(rhs, x)
    return ls, x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["poisson8", "path9", "rand300u"])
def test_c_table_kind_16_applies_like_the_library(ra, S, name, dtype):
    """ramd_solver_precond_apply of RAMD_PC_MULTIELIM (the C++ class behind the table): the genuine library's Solve bit for
    bit, level 1 and 2, with the default form (stepwise) and with a format request (E and F of the first level in ELL).  The
    table has no way to ask for the fused form; the class's SetForm(1) runs in the driver test"""
    g = load(name)
    A, rhs = _op(ra, g, dtype), _vec(ra, g["rhs"], dtype)
    for levels in (1, 2):
        for fmt in (None, ra.ELL):
            _, x = _table_apply(ra, S, A, rhs, dtype, levels, fmt=fmt)
            same_bits(x.numpy(), g["me%d_x%s" % (levels, _sfx(dtype))])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multielim") / "multielim_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "multielim_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    return exe


def test_driver_runs_and_the_class_applies_like_the_library(driver, tmp_path):
    """the reference-style driver on the 8^3 Poisson operator: CG + MultiElimination(MultiColoredILU(0), 2, drop) with the
    golden iteration count, and the class's own Solve (Jacobi as last block, two levels) equal to the library's bit for bit"""
    g = load("poisson8")
    mtx = str(tmp_path / "poisson8.mtx")
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    r = subprocess.run([driver, mtx, repr(float(g["drop"][0])), "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    m = re.search(r"RESULT iters=(\d+) status=(\d+) residual=(\S+) error=(\S+) size0=(-?\d+) size1=(-?\d+)", out)
    assert r.returncode == 0 and m, out[-2000:]
    assert abs(int(m.group(1)) - int(g["cg_me_meta"][0])) <= 1 and int(m.group(2)) == int(g["cg_me_meta"][1]), m.groups()
    assert float(m.group(4)) < 1e-3 and int(m.group(5)) == g["size"][0]
    assert "MultiElimination (I)LU preconditioner with 2 levels" in out
    rhs, xf = str(tmp_path / "rhs.bin"), str(tmp_path / "x.bin")
    g["rhs"].astype(np.float64).tofile(rhs)
    # SetForm reaches both levels; an ELL request takes the stepwise form at the level whose blocks it converts, whatever
    # SetForm said, and the next level keeps the form asked for
    for fmt, form, forms in (("csr", "-1", "0 0"), ("csr", "1", "1 1"), ("csr", "0", "0 0"), ("ell", "1", "0 1"), ("ell", "-1", "0 0")):
        r = subprocess.run([driver, mtx, "0", "2", fmt, form, "apply", rhs, xf], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=300)
        assert r.returncode == 0 and ("FORMS " + forms) in r.stdout.decode(), r.stdout.decode()[-2000:]
        same_bits(np.fromfile(xf), g["me2_x"])


def test_block_jacobi_multielim_on_one_rank(ra, S):
    """kind 16 through the Global table: on one rank BlockJacobi(MultiElimination) is MultiElimination of the whole operator --
    its apply equals the local class's and the library's Solve bit for bit (default parameters: Jacobi, one level; two levels
    and an ELL request sent through ramd_gsolver_set_precond_*), and CG converges as the local solver does"""
    from rocalution_amd import capi, distributed as D
    lib = capi.load()
    uid = C.create_string_buffer(128)
    capi.check(lib.ramd_comm_unique_id(uid))
    comm = C.c_void_p()
    capi.check(lib.ramd_comm_init_rccl(0, 1, uid, C.byref(comm)))
    g = load("gr3030")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    piece = dict(interior=(rp, ci, va), ghost=(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)))
    plan = dict(peers=np.zeros(0, np.int32), send_offset=np.zeros(1, np.int32), recv_offset=np.zeros(1, np.int32),
                boundary_index=np.zeros(0, np.int32))
    h = C.c_void_p()
    assert lib.ramd_gsolver_create(comm, capi.SOLVER_CG, 15, C.byref(h)) == capi.ERR_ARG
    for levels, fmt in ((None, None), (2, None), (2, ra.ELL)):
        gs = D.DistributedSolver(comm, capi.SOLVER_CG, capi.PC_MULTIELIM)
        gs.setup_csr(n, piece, plan)
        gs.init(1e-15, 1e-6, 1e8, 500)
        if levels is not None:
            gs.set_precond_params(levels, 0.0, capi.PC_JACOBI)
        if fmt is not None:
            gs.set_precond_format(fmt)
        gs.build()
        same_bits(gs.precond_apply(g["rhs"]), g["me%d_x" % (levels or 1)])
        x = gs.solve(None, np.zeros(n))
        it, st, _ = gs.result()
        ls = S.CG(); ls.SetPreconditioner(S.MultiElimination(S.Jacobi(), levels or 1, 0.0)); ls.SetOperator(_op(ra, g)); ls.Build()
        xl = _zeros(ra, n, np.float64)
        ls.Solve(_ones_rhs(ra, _op(ra, g)), xl)
        assert st == ls.GetSolverStatus() == 2 and abs(it - ls.GetIterationCount()) <= 1, (it, ls.GetIterationCount())
        assert np.linalg.norm(x - 1.0) < 1e-3
        with pytest.raises(capi.RamdError):
            gs.set_precond_params(1, 0.0, capi.PC_JACOBI)  # built
        del gs
    gs = D.DistributedSolver(comm, capi.SOLVER_CG, capi.PC_MULTIELIM)
    with pytest.raises(capi.RamdError):
        gs.set_precond_params(2, 0.0, capi.PC_SAAMG)
    del gs
    capi.check(lib.ramd_comm_destroy(comm))


def test_stepwise_up_needs_the_down_of_the_same_rhs(ra, S):
    """form 0 keeps x1 between the halves: an Up without a Down, after a Down of another vector, or a second Up is refused
    (RAMD_ERR_STATE); form 1 is a function of its arguments and takes any order"""
    from rocalution_amd import capi
    g = load("lap2d7")
    A = _op(ra, g)
    plan = S.MEPlan(A, form=0)
    n, size = plan.Info()["rows"], plan.Info()["size"]
    r1, r2 = _vec(ra, g["rhs"], np.float64), _vec(ra, g["rhs"] * 2.0, np.float64)
    rhs2, x2, x = _zeros(ra, n - size, np.float64), _zeros(ra, n - size, np.float64), _zeros(ra, n, np.float64)

    def refused(call):
        with pytest.raises(capi.RamdError) as ei:
            call()
        assert ei.value.status == capi.ERR_STATE and "ramd_me_down of the same rhs" in str(ei.value)
    refused(lambda: plan.Up(r1, x2, x))
    plan.Down(r1, rhs2)
    refused(lambda: plan.Up(r2, x2, x))
    plan.Up(r1, x2, x)
    first = x.numpy().copy()
    refused(lambda: plan.Up(r1, x2, x))
    fused = S.MEPlan(A, form=1)
    fused.Up(r1, x2, x)
    same_bits(x.numpy(), first)


def test_last_block_settings_are_not_dropped_silently(S):
    """the table takes the last-block solver by kind: an object that carries settings of its own is refused, not run with defaults"""
    ilu = S.ILU(); ilu.Set(2)
    mc = S.MultiColoredILU(); mc.SetPrecondMatrixFormat(6)
    for last in (ilu, mc, S.TNS(impl=False)):
        with pytest.raises(ValueError):
            S.MultiElimination(last, 1, 0.0)
    S.MultiElimination(S.ILU(), 1, 0.0); S.MultiElimination(S.TNS(), 2, 0.1)


# ------------------------------------------------------------------------------------------------ lifecycle and refusals
def test_clear_rebuild_and_rebuild_numeric(ra, S):
    from rocalution_amd import capi
    g = load("gr3030")
    A, rhs = _op(ra, g), _vec(ra, g["rhs"], np.float64)
    ls, x = _table_apply(ra, S, A, rhs, np.float64, 2, last=S.MultiColoredILU())
    first = x.numpy().copy()
    ls.Clear()
    capi.check(capi.load().ramd_solver_build(ls._h, A._h))
    ls.PrecondApply(rhs, x)
    same_bits(x.numpy(), first)
    A.UpdateValuesCSR(g["val"] * 2.0)
    ls.ReBuildNumeric()
    ls.PrecondApply(rhs, x)
    B = _mat(ra, g["rowptr"], g["col"], g["val"] * 2.0)
    _, fresh = _table_apply(ra, S, B, rhs, np.float64, 2, last=S.MultiColoredILU())
    same_bits(x.numpy(), fresh.numpy())
    assert not np.array_equal(x.numpy(), first)


def test_refusals(ra, S):
    from rocalution_amd import capi
    lib = capi.load()
    g = load("poisson8")
    W = _op(ra, g); W.ForceWide()
    for call in (lambda: W.MaximalIndependentSet(), lambda: W.Compress(0.1), lambda: S.MEPlan(W),
                 lambda: _table_apply(ra, S, W, _vec(ra, g["rhs"], np.float64), np.float64, 1)):
        with pytest.raises(capi.RamdError) as ei:
            call()
        assert ei.value.status == capi.ERR_UNSUPPORTED and "not provided for 64-bit row offsets" in str(ei.value)
    h = C.c_void_p()
    assert lib.ramd_solver_create_mixed(capi.SOLVER_CG, capi.PC_MULTIELIM, C.byref(h)) == capi.ERR_ARG
    assert lib.ramd_solver_create(capi.SOLVER_CG, 15, capi.F64, C.byref(h)) == capi.ERR_ARG
    assert lib.ramd_solver_create(capi.SOLVER_CG, capi.PC_MULTIELIM, capi.F64, C.byref(h)) == capi.OK
    for last in (capi.PC_MULTIELIM, capi.PC_UAAMG, capi.PC_SAAMG, capi.PC_RSAMG, capi.PC_NONE, 15):
        assert lib.ramd_solver_set_precond_params(h, 2.0, 0.0, float(last)) == capi.ERR_ARG, last
        assert b"last-block solver" in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_params(h, -1.0, 0.0, float(capi.PC_JACOBI)) == capi.ERR_ARG
    assert lib.ramd_solver_set_precond_params(h, 2.0, 0.5, float(capi.PC_MCILU)) == capi.OK
    lib.ramd_solver_destroy(h)
