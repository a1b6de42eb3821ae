"""Ruge-Stueben AMG on the device: the coarsening and interpolation primitives bit for bit against the genuine library's
arrays (tests/golden/rsamg, recorded by tests/drivers/rsamg_probe.cpp), their edges, and the class through the
reference-style driver held to the bar tests/test_gpu_solvers.py applies to the aggregation AMGs (levels equal,
iterations within one, status equal, history to 1e-5 against the 6-digit history file)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _rsamg_ref import extpi
from _tns_ref import sym_arrow
from test_cpu_rsamg import EDGE, FIVE, ROOT, load, same_bits
from test_gpu_solvers import _check_hist, _write_mtx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


@pytest.fixture(scope="module")
def S():
    from rocalution_amd import solvers
    return solvers


def _mat(ra, g, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(g["rowptr"], g["col"], g["val"].astype(dtype))
    return A


def _ivec(ra, a):
    return ra.LocalVector(np.int32, data=np.ascontiguousarray(a, dtype=np.int32))


def _check_P(P, g, key):
    rp, ci, va = P.CopyToCSR()
    assert np.array_equal(rp, g[key + "_rowptr"]) and np.array_equal(ci, g[key + "_col"])
    same_bits(va, g[key + "_val"])
    assert P.GetM() == g[key + "_shape"][0] and P.GetN() == g[key + "_shape"][1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", FIVE + EDGE)
def test_primitives_bit_exact(ra, name, dtype):
    """Greedy and PMIS maps, S, the Direct P, the extended+i P (FF1 off / on) from both maps, and the first coarse operator
    through Transpose + TripleMatrixProduct: every array equal to the probe's, in both precisions"""
    g = load(name)
    sfx = "" if dtype == np.float64 else "_f32"
    A = _mat(ra, g, dtype)
    for m in ("greedy", "pmis"):
        cf, S_ = A.RSCoarsening(0.25) if m == "greedy" else A.RSPMISCoarsening(0.25)
        assert np.array_equal(cf.numpy(), g[m + sfx + "_cf"]) and np.array_equal(S_.numpy(), g[m + sfx + "_S"])
        P = ra.LocalMatrix(dtype)
        A.RSDirectInterpolation(cf, S_, P)
        _check_P(P, g, "direct_" + m + sfx)
        for ff1 in (0, 1):
            E = ra.LocalMatrix(dtype)
            A.RSExtPIInterpolation(cf, S_, bool(ff1), E)
            _check_P(E, g, "extpi_%s%s_ff%d" % (m, sfx, ff1))
            if not ff1 and E.GetN() > 0:
                R, Ac = ra.LocalMatrix(dtype), ra.LocalMatrix(dtype)
                E.Transpose(R)
                Ac.TripleMatrixProduct(R, A, E)
                _check_P(Ac, g, "Ac_" + m + sfx)


def test_fine_row_without_a_coarse_point_in_reach(ra):
    """a hand-made map on the 1-D chain: rows 3..5 fine with only fine points at distance one and two of row 4 -- an empty
    row of P; the neighbours' sums over an empty set divide by zero exactly where the host loop does"""
    g = load("path9")
    n = 9
    cf = np.array([1, 2, 2, 2, 2, 2, 2, 2, 1], dtype=np.int32)
    S_ = (g["val"] < 0).astype(np.int32)
    for dtype in (np.float64, np.float32):
        ref = extpi(g["rowptr"], g["col"], g["val"], cf, S_, False, dtype)
        assert ref[0][5] - ref[0][4] == 0  # row 4 is empty
        E = ra.LocalMatrix(dtype)
        _mat(ra, g, dtype).RSExtPIInterpolation(_ivec(ra, cf), _ivec(ra, S_), False, E)
        rp, ci, va = E.CopyToCSR()
        assert np.array_equal(rp, ref[0]) and np.array_equal(ci, ref[1]) and E.GetN() == 2
        same_bits(va, ref[2])


@pytest.mark.parametrize("ff1", [False, True])
def test_long_row_takes_the_scratch_table(ra, ff1):
    """an arrow matrix whose row 0 strongly depends on more than 2000 points: its set of coarse points does not fit the LDS
    table, the row goes through the global scratch table (the entry's counters say so) and equals the restatement bit for bit"""
    rp, ci, va = sym_arrow(n=2700, long=2600)
    g = {"rowptr": rp, "col": ci, "val": va}
    A = _mat(ra, g)
    cf, S_ = A.RSPMISCoarsening(0.25)
    cf, S_ = cf.numpy().copy(), S_.numpy().copy()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    S_[(rows == 0) & (ci != 0)] = 1  # row 0 strongly depends on all of its 2600 neighbours
    S_[(ci == 0) & (rows != 0)] = 0  # and none of them on row 0 (keeps the restatement's loops short)
    cf[:] = 2
    cf[1::2] = 1  # every other point coarse: row 0 (fine) reaches 1300 coarse points directly and through its fine neighbours
    assert S_[rp[0]:rp[1]].sum() >= 2000
    ref = extpi(rp, ci, va, cf, S_, ff1, np.float64)
    E = ra.LocalMatrix()
    info = A.RSExtPIInterpolation(_ivec(ra, cf), _ivec(ra, S_), ff1, E)
    assert info["scratch_rows"] >= 1 and info["scratch_slots"] >= 2048 and info["max_bound"] >= 1024, info
    assert info["lds_rows"] + info["scratch_rows"] == int(np.sum(cf != 1))
    prp, pci, pva = E.CopyToCSR()
    assert prp[1] - prp[0] > 1024  # the row itself is longer than the LDS table
    assert np.array_equal(prp, ref[0]) and np.array_equal(pci, ref[1]) and E.GetN() == ref[3]
    same_bits(pva, ref[2])


def test_zero_row_operator(ra):
    A = ra.LocalMatrix()
    A.SetDataPtrCSR(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), nrow=0, ncol=0)
    E = ra.LocalMatrix()
    A.RSExtPIInterpolation(_ivec(ra, []), _ivec(ra, []), False, E)
    assert E.GetM() == 0 and E.GetN() == 0 and E.GetNnz() == 0
    cf, S_ = A.RSCoarsening(0.25)
    assert len(cf.numpy()) == 0


def test_misuse_is_refused_and_objects_stay_usable(ra):
    from rocalution_amd import capi
    lib = capi.load()
    g = load("poisson8")
    A = _mat(ra, g)
    n = A.GetM()
    cf, S_ = A.RSPMISCoarsening(0.25)
    E = ra.LocalMatrix()
    dv = ra.LocalVector(data=np.ones(n))  # a double vector where int vectors are expected
    assert lib.ramd_mat_rs_extpi_interpolation(A._h, dv._h, S_._h, 0, E._h) == capi.ERR_ARG
    assert b"RSExtPIInterpolation: int vectors of the operator's sizes, P of its value type" in lib.ramd_last_error()
    assert lib.ramd_mat_rs_coarsening(A._h, C.c_float(0.25), dv._h, S_._h) == capi.ERR_ARG
    assert b"RSCoarsening: square matrix and int vectors expected" in lib.ramd_last_error()
    assert lib.ramd_mat_rs_extpi_interpolation(A._h, cf._h, S_._h, 0, A._h) == capi.ERR_ARG  # P aliases the operator
    B = _mat(ra, g); B.ConvertTo(ra.ELL)
    assert lib.ramd_mat_rs_extpi_interpolation(B._h, cf._h, S_._h, 0, E._h) == capi.ERR_UNSUPPORTED
    assert lib.ramd_mat_rs_coarsening(B._h, C.c_float(0.25), cf._h, S_._h) == capi.ERR_UNSUPPORTED
    W = _mat(ra, g); W.ForceWide()
    for rc in (lib.ramd_mat_rs_extpi_interpolation(W._h, cf._h, S_._h, 0, E._h),
               lib.ramd_mat_rs_coarsening(W._h, C.c_float(0.25), cf._h, S_._h)):
        assert rc == capi.ERR_UNSUPPORTED and b"not provided for 64-bit row offsets" in lib.ramd_last_error()
    rect = ra.LocalMatrix(); rect.SetDataPtrCSR(g["rowptr"], g["col"], g["val"], ncol=n + 1)
    assert lib.ramd_mat_rs_extpi_interpolation(rect._h, cf._h, S_._h, 0, E._h) == capi.ERR_ARG
    # everything still works
    A.RSExtPIInterpolation(cf, S_, False, E)
    _check_P(E, g, "extpi_pmis_ff0")
    assert np.array_equal(cf.numpy(), g["pmis_cf"])


# ------------------------------------------------------------------------------------------------ the class
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rsamg") / "rsamg_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "rsamg_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    m = re.search(r"RESULT mode=\S+ levels=(\d+) iters=(\d+) status=(\d+) residual=(\S+) error=(\S+)", out)
    assert m, out[-2000:]
    sizes = [int(v) for pair in re.findall(r"LEVEL \d+ rows=(\d+) nnz=(\d+)", out) for v in pair]
    hist = np.array([float(v) for v in re.findall(r"HIST (\S+)", out)])
    x = np.array([float(v) for v in re.findall(r"^X (\S+)", out, flags=re.M)])
    return dict(levels=int(m.group(1)), iters=int(m.group(2)), status=int(m.group(3)), error=float(m.group(5)), sizes=sizes,
                hist=hist, x=x, out=out)


@pytest.mark.parametrize("name", FIVE)
def test_class_vs_reference(driver, tmp_path, name):
    """{Greedy, PMIS} x {Direct, ExtPI} x {solver, CG preconditioner}: the hierarchy (levels, rows and entries per level)
    equals the genuine library's; iterations within one and status equal, history to 1e-5, |x - 1| < 1e-3 for a converged
    run (the bar of test_cpp_uaamg_driver_vs_reference)"""
    g = load(name)
    mtx = str(tmp_path / (name + ".mtx"))
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    for mode in ("amg", "cg"):
        for strat in ("greedy", "pmis"):
            for interp in ("direct", "extpi"):
                tag = "%s_%s_%s" % (mode, strat, interp)
                r = _run(driver, mtx, mode, strat, interp)
                meta = g[tag + "_meta"]
                assert r["levels"] == int(meta[3]) and r["sizes"] == [int(v) for v in g[tag + "_sizes"]], (tag, r["sizes"])
                assert abs(r["iters"] - int(meta[0])) <= 1 and r["status"] == int(meta[1]), (tag, r["iters"], r["status"], meta)
                _check_hist(r["hist"], g[tag + "_hist"], False, rtol=1e-5)
                if int(meta[1]) in (1, 2):
                    assert r["error"] < 1e-3, (tag, r["error"])


@pytest.mark.parametrize("name", ["gr3030", "poisson8", "lap2d7"])
def test_old_rsamg_goldens_are_checked(driver, tmp_path, name):
    """rsamg_levels, rsamg_pmis_{meta,hist,x} and cg_rsamg_{meta,hist,x} of tests/golden/<name>.npz (PMIS, the library's
    default interpolation: Direct)"""
    from conftest import load_golden
    g = load_golden(name)
    mtx = str(tmp_path / (name + ".mtx"))
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    for mode, tag in (("amg", "rsamg_pmis"), ("cg", "cg_rsamg")):
        r = _run(driver, mtx, mode, "pmis", "direct")
        meta = g[tag + "_meta"]
        assert r["levels"] == int(g["rsamg_levels"][0])
        assert abs(r["iters"] - int(meta[0])) <= 1 and r["status"] == int(meta[1]), (tag, r["iters"], meta)
        _check_hist(r["hist"], g[tag + "_hist"], False, rtol=1e-5)
        if int(meta[1]) in (1, 2):  # the bar of test_cpp_uaamg_driver_vs_reference for x, against 1 and against the golden x
            assert r["error"] < 1e-3 and np.linalg.norm(r["x"] - g[tag + "_x"]) < 1e-3, tag


def test_default_settings_and_driver_iteration_counts(driver):
    """the driver with the class's defaults (Greedy, Direct) on the built-in 8^3 Poisson operator, both modes: the golden
    iteration counts"""
    g = load("poisson8")
    for mode in ("amg", "cg"):
        r = _run(driver, "poisson:8", mode)
        meta = g[mode + "_greedy_direct_meta"]
        assert "AMG Ruge-Stuben using Greedy coarsening with Direct interpolation" in r["out"]
        assert r["levels"] == int(meta[3]) and r["iters"] == int(meta[0]) and r["status"] == int(meta[1])
        assert r["sizes"] == [int(v) for v in g[mode + "_greedy_direct_sizes"]] and r["error"] < 1e-3


def test_levels_revert_when_P_has_no_columns(driver, tmp_path):
    """a diagonal operator has no strong connection: every point is fine, P has no columns, the first level cannot be built
    and Build() says so (as BaseAMG does for any AMG); below a fine level that can be coarsened once, the same revert keeps
    the hierarchy at the level reached and the solve runs"""
    g = load("diag40")
    mtx = str(tmp_path / "diag40.mtx")
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    r = subprocess.run([driver, mtx, "amg", "pmis", "extpi"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode != 0 and b"Could not build initial AMG level" in r.stdout
    # block diagonal: a 7x7 chain block coarsens, the coarse operator of a chain with every other point coarse is again a
    # chain; with the coarsest level at 1 row the hierarchy ends where a level comes out without coarse points
    n = 60
    rp, ci, va = [0], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n and (i // 2 == j // 2):  # decoupled pairs
                ci.append(j); va.append(v)
        rp.append(len(ci))
    mtx2 = str(tmp_path / "pairs.mtx")
    _write_mtx(mtx2, np.array(rp), np.array(ci), np.array(va))
    r = _run(driver, mtx2, "cg", "pmis", "extpi", "1")
    assert r["levels"] == 2 and r["sizes"][2] == n // 2 and r["sizes"][3] == n // 2  # level 1 is diagonal: reverted below it
    assert r["status"] in (1, 2) and np.linalg.norm(r["x"] - 1.0) < 1e-6


def test_c_table_kind_14(ra, S, driver, tmp_path):
    """RAMD_PC_RSAMG builds and solves through ramd_solver_*.  ramd_solver_precond_apply (one V-cycle) equals the C++ class's
    own Solve of one iteration from x = 0 (tests/drivers/rsamg_driver.cpp, mode vcycle) bit for bit, with the class's defaults
    and with PMIS + ExtPI sent through ramd_solver_set_precond_params -- the two settings give different vectors, so the
    parameters took effect.  The kind is refused inside the mixed-precision driver"""
    from rocalution_amd import capi
    lib = capi.load()
    g = load("poisson8")
    n = len(g["rowptr"]) - 1
    mtx = str(tmp_path / "poisson8.mtx")
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    A = _mat(ra, g)
    rhs = ra.LocalVector(data=A_ones(ra, A, n))
    zs = []
    for args, tag in (((), "cg_greedy_direct"), (("pmis", "extpi"), "cg_pmis_extpi")):
        pc = S.RugeStuebenAMG(); pc.SetCoarsestLevel(20)
        if args:
            pc.SetCoarseningStrategy(S.PMIS); pc.SetInterpolationType(S.ExtPI)
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.InitMaxIter(100); ls.Build()
        z = ra.LocalVector(); z.Allocate("z", n)
        ls.PrecondApply(rhs, z)
        x = ra.LocalVector(); x.Allocate("x", n)
        ls.Solve(rhs, x)
        meta = g[tag + "_meta"]
        assert abs(ls.GetIterationCount() - int(meta[0])) <= 1 and ls.GetSolverStatus() == int(meta[1]), tag
        assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-4
        ls.Clear()
        r = _run(driver, mtx, "vcycle", *args)
        assert r["iters"] == 1 and len(r["x"]) == n
        same_bits(z.numpy(), r["x"])
        zs.append(z.numpy().copy())
    assert not np.array_equal(zs[0], zs[1])
    h = C.c_void_p()
    assert lib.ramd_solver_create_mixed(capi.SOLVER_CG, capi.PC_RSAMG, C.byref(h)) == capi.ERR_ARG
    assert lib.ramd_solver_create(capi.SOLVER_CG, 15, capi.F64, C.byref(h)) == capi.ERR_ARG


def test_build_stops_on_64_bit_row_offsets(ra, S):
    from rocalution_amd import capi
    g = load("poisson8")
    A = _mat(ra, g); A.ForceWide()
    for strat in (S.Greedy, S.PMIS):
        pc = S.RugeStuebenAMG(); pc.SetCoarseningStrategy(strat)
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(pc)
        with pytest.raises(capi.RamdError) as ei:
            ls.Build()
        assert "not provided for 64-bit row offsets" in str(ei.value)
    assert A.GetPtrBits() == 64


def test_kind_14_under_blockjacobi_on_a_global_operator():
    """ramd_gsolver_create(CG, RAMD_PC_RSAMG): BlockJacobi around the local RugeStuebenAMG, one rank (a size-1 RCCL
    communicator).  BlockJacobi calls its local solver's Solve, as the reference does, so the AMG is not flagged as a
    preconditioner there and iterates to its own tolerance at every application (any AMG kind behaves so under BlockJacobi):
    CG converges to the same solution in no more iterations than CG + one V-cycle of the LocalMatrix path"""
    import sys
    body = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
import rocalution_amd as ra
from rocalution_amd import capi, solvers as S
ra.init_rocalution()
lib = capi.load()
N = 12
n = N ** 3
uid = C.create_string_buffer(128)
capi.check(lib.ramd_comm_unique_id(uid))
comm = C.c_void_p()
capi.check(lib.ramd_comm_init_rccl(0, 1, uid, C.byref(comm)))
g = C.c_void_p()
capi.check(lib.ramd_gsolver_create(comm, capi.SOLVER_CG, capi.PC_RSAMG, C.byref(g)))
capi.check(lib.ramd_gsolver_init(g, 1e-15, 1e-6, 1e8, 0, 200))
capi.check(lib.ramd_gsolver_setup_poisson(g, N, 0, N))
capi.check(lib.ramd_gsolver_build(g))
xg = np.zeros(n)
capi.check(lib.ramd_gsolver_solve(g, None, xg.ctypes.data_as(C.c_void_p)))
it, st, rs = C.c_int(0), C.c_int(0), C.c_double(0)
capi.check(lib.ramd_gsolver_result(g, C.byref(it), C.byref(st), C.byref(rs)))
capi.check(lib.ramd_gsolver_destroy(g))
A = ra.LocalMatrix(); A.GenPoisson7(N)
ones = ra.LocalVector(); ones.Allocate("", n); ones.Ones()
rhs = ra.LocalVector(); rhs.Allocate("", n); A.Apply(ones, rhs)
ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.RugeStuebenAMG()); ls.Init(1e-15, 1e-6, 1e8, 200); ls.Build()
x = ra.LocalVector(); x.Allocate("", n)
ls.Solve(rhs, x)
assert st.value == 2 and ls.GetSolverStatus() == 2, (st.value, ls.GetSolverStatus())
assert 0 < it.value <= ls.GetIterationCount() < 60, (it.value, ls.GetIterationCount())
assert np.max(np.abs(xg - 1.0)) < 1e-4 and np.max(np.abs(x.numpy() - 1.0)) < 1e-4, (np.max(np.abs(xg - 1.0)), np.max(np.abs(x.numpy() - 1.0)))
print("BLOCKJACOBI RSAMG OK", it.value)
''' % ROOT
    r = subprocess.run([sys.executable, "-c", body], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"BLOCKJACOBI RSAMG OK" in r.stdout, r.stdout.decode()[-3000:]


def A_ones(ra, A, n):
    y = ra.LocalVector(); y.Allocate("y", n)
    A.Apply(ra.LocalVector(data=np.ones(n)), y)
    return y.numpy().copy()
