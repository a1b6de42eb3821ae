"""The MCSR format on the device: CSR <-> MCSR, the diagonal-first products, the fused product + dot, the native diagonal
extraction, SetDataPtrMCSR, and solvers on a converted operator.

Yardsticks: the genuine library's recorded results (tests/golden/mcsr, tools/gen_golden_mcsr.py) and, for the generated cases
the goldens do not reach, tests/_mcsr_ref.py -- which tests/test_cpu_mcsr.py pins to those recordings byte for byte and which
accepts / refuses every generated case as this file expects.  Conversions and products are compared byte for byte: the library
is built with -ffp-contract=off and forms every row's sum in the host loop's order, the diagonal term first.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mcsr_cases as cases  # noqa: E402
import _mcsr_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
GOLDEN_MCSR = ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300", "rand300ell",  # sorted rows, a full diagonal
               "shuffled_257", "longrow", "hub", "zeros_64", "negzero_64"]  # ... and the library's word on five generated cases


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
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%d elements differ" % np.sum(a != b)


def _mat(ra, rp, ci, va, nrow=None, ncol=None, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(np.asarray(rp, np.int32), ci, np.asarray(va, dtype), nrow=nrow, ncol=ncol)
    return A


def _apply(ra, A, x, dtype):
    xv = ra.LocalVector(dtype, data=np.asarray(x, dtype))
    yv = ra.LocalVector(dtype); yv.Allocate("", A.GetM())
    A.Apply(xv, yv)
    return yv.numpy()


def _apply_add(ra, A, x, scalar, y, dtype):
    xv = ra.LocalVector(dtype, data=np.asarray(x, dtype))
    yv = ra.LocalVector(dtype, data=np.asarray(y, dtype))
    A.ApplyAdd(xv, scalar, yv)
    return yv.numpy()


# -------------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", GOLDEN_MCSR)
def test_goldens(ra, oracle, name, dtype):
    g = ref.load(name)
    sfx = "" if dtype == np.float64 else "_f32"
    rp, ci, va, x, y0 = g["rowptr"], g["col"], g["val"].astype(dtype), g["x"].astype(dtype), g["y"].astype(dtype)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToMCSR() == ra.MCSR and A.GetFormat() == ra.MCSR
    assert (A.GetM(), A.GetN(), A.GetNnz()) == (n, n, len(va))
    ro, col, val = A.mcsr_arrays()
    eq(ro, g["mcsr_rowptr"]); eq(col, g["mcsr_col"]); eq(val, g["mcsr_val" + sfx])
    eq(_apply(ra, A, x, dtype), g["spmv_mcsr" + sfx])
    eq(_apply_add(ra, A, x, -0.75, y0, dtype), g["spmv_mcsr_add" + sfx])
    assert A.ConvertTo(ra.MCSR) == ra.MCSR  # already there: nothing happens
    eq(A.mcsr_arrays()[2], g["mcsr_val" + sfx])
    assert A.ConvertToCSR() == ra.CSR and A.GetNnz() == len(va)
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, g["back_rowptr"]); eq(hci, g["back_col"]); eq(hva, g["back_val" + sfx])
    eq(_apply(ra, A, x, dtype), oracle.csr_apply(hrp, hci, hva, x))


# ------------------------------------------------------------------------------------------ shapes where the kernel can go wrong
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.ACCEPTED)
def test_generated_cases(ra, name, dtype):
    rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    n = len(rp) - 1
    ro, col, val = ref.csr_to_mcsr(rp, ci, va)  # (accepted: tests/test_cpu_mcsr.py)
    brp, bci, bva = ref.mcsr_to_csr(ro, col, val)
    x, y0 = cases.x_for(name).astype(dtype), cases.y_for(name).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToMCSR() == ra.MCSR and A.GetNnz() == len(va)
    gro, gcol, gval = A.mcsr_arrays()
    eq(gro, ro); eq(gcol, col); eq(gval, val)
    y = _apply(ra, A, x, dtype)
    eq(y, ref.apply(ro, col, val, x))
    eq(_apply_add(ra, A, x, -0.75, y0, dtype), ref.apply_add(ro, col, val, x, -0.75, y0))
    if name == "negzero_64":  # the diagonal-first start: -0.0 where a sum begun at zero gives +0.0
        assert np.all(y[:32] == 0) and np.all(np.signbit(y[:32]))
    assert A.ConvertToCSR() == ra.CSR
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva)


@pytest.mark.parametrize("name", cases.REFUSED)
def test_refused_conversion_leaves_a_working_csr_matrix(ra, oracle, name):
    rp, ci, va = cases.case(name)
    nrow, ncol = cases.shape(name)
    assert ref.csr_to_mcsr(rp, ci, va, nrow=nrow, ncol=ncol) is None
    x = cases.x_for(name)
    A = _mat(ra, rp, ci, va, nrow=nrow, ncol=ncol)
    before = _apply(ra, A, x, np.float64)
    eq(before, oracle.csr_apply(rp, ci, va, x))
    assert A.ConvertToMCSR() == ra.CSR and A.GetFormat() == ra.CSR and A.GetNnz() == len(va)
    eq(_apply(ra, A, x, np.float64), before)
    with pytest.raises(ra.RamdError) as e:
        A.mcsr_arrays()
    assert e.value.status == 6  # RAMD_ERR_STATE
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, rp); eq(hci, ci); eq(hva, va)


def test_the_library_refuses_what_the_genuine_library_refused(ra):
    g = ref.load("nodiag_row_40")
    assert int(g["format"][0]) == ra.CSR
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert A.ConvertToMCSR() == ra.CSR


def test_a_diagonal_stored_twice_is_refused(ra):
    """the deliberate departure (include/rocalution_amd.h): the reference counts the diagonal entries of the whole matrix"""
    rp, ci, va = np.array([0, 2, 3, 4], np.int32), np.array([0, 0, 1, 2], np.int32), np.array([1.0, 2.0, 3.0, 4.0])
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToMCSR() == ra.CSR
    eq(A.CopyToCSR()[2], va)


# ------------------------------------------------------------------------------------------------------------- SetDataPtrMCSR
@pytest.mark.parametrize("dtype", DTYPES)
def test_set_data_ptr_mcsr_round_trips(ra, dtype):
    rp, ci, va = cases.case("shuffled_257")
    ro, col, val = ref.csr_to_mcsr(rp, ci, va.astype(dtype))
    dirty = col.copy(); dirty[:257] = 99  # (col[0 .. n) is never read and comes back as zero)
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrMCSR(ro, dirty, val)
    assert A.GetFormat() == ra.MCSR and (A.GetM(), A.GetN(), A.GetNnz()) == (257, 257, len(val))
    gro, gcol, gval = A.mcsr_arrays()
    eq(gro, ro); eq(gcol, col); eq(gval, val)
    x = cases.x_for("shuffled_257")
    eq(_apply(ra, A, x, dtype), ref.apply(ro, col, val, x))
    assert A.ConvertToCSR() == ra.CSR
    brp, bci, bva = ref.mcsr_to_csr(ro, col, val)
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva)


def test_set_data_ptr_mcsr_checks_its_arguments(ra):
    ro, col, val = ref.csr_to_mcsr(*cases.case("tri_65"))
    A = _mat(ra, *cases.case("tri_1"))
    bad = ro.copy(); bad[0] = 64
    down = ro.copy(); down[10] = ro[9] - 1
    short = ro.copy(); short[-1] -= 1
    far = col.copy(); far[100] = 65
    for args, kw in (((bad, col, val), {}), ((ro, col, val), {"ncol": 66}), ((down, col, val), {}), ((short, col, val), {}),
                     ((ro, far, val), {})):
        with pytest.raises(ra.RamdError) as e:
            A.SetDataPtrMCSR(*args, **kw)
        assert e.value.status == 2  # RAMD_ERR_ARG
        assert A.GetFormat() == ra.CSR and A.GetM() == 1  # (the matrix is as it was)


# --------------------------------------------------------------------------------------------------------- empty, wide, clone
@pytest.mark.parametrize("n", [0, 5])
def test_a_matrix_without_entries_converts_as_it_does_to_ell(ra, n):
    """no rows, or rows and no entry: ELL gets width 0, MCSR an empty matrix; Apply gives zeros, ApplyAdd changes nothing"""
    rp = np.zeros(n + 1, np.int32)
    none_i, none_v = np.zeros(0, np.int32), np.zeros(0)
    E = _mat(ra, rp, none_i, none_v, nrow=n, ncol=n)
    assert E.ConvertToELL() == ra.ELL and E.GetNnz() == 0
    A = _mat(ra, rp, none_i, none_v, nrow=n, ncol=n)
    assert A.ConvertToMCSR() == ra.MCSR and A.GetNnz() == 0
    ro, col, val = A.mcsr_arrays()
    assert len(ro) == n + 1 and len(col) == 0 and len(val) == 0
    if n:
        x = np.arange(1.0, n + 1.0)
        eq(_apply(ra, A, x, np.float64), np.zeros(n))
        eq(_apply_add(ra, A, x, 2.0, x, np.float64), x)
    B = ra.LocalMatrix(); B.CloneFrom(A)
    assert B.GetFormat() == ra.MCSR
    assert A.ConvertToCSR() == ra.CSR and A.GetNnz() == 0 and (A.GetM(), A.GetN()) == (n, n)
    if n:
        eq(A.CopyToCSR()[0], rp)


def test_wide_source_is_unsupported(ra):
    from rocalution_amd import capi
    rp, ci, va = cases.case("tri_65")
    A = _mat(ra, rp, ci, va)
    A.ForceWide(True)
    assert capi.load().ramd_mat_convert(A._h, ra.MCSR) == 3  # RAMD_ERR_UNSUPPORTED
    with pytest.raises(ra.RamdError) as e:
        A.ConvertToMCSR()
    assert e.value.status == 3 and "not provided for 64-bit row offsets" in str(e.value)
    assert A.GetFormat() == ra.CSR and A.GetPtrBits() == 64
    A.ForceWide(False)
    assert A.ConvertToMCSR() == ra.MCSR


def test_clone_keeps_format_and_product_and_cast_answers_with_a_status(ra):
    g = ref.load("gr3030")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert A.ConvertToMCSR() == ra.MCSR
    B = ra.LocalMatrix(); B.CloneFrom(A)
    assert B.GetFormat() == ra.MCSR and (B.GetM(), B.GetN(), B.GetNnz()) == (A.GetM(), A.GetN(), A.GetNnz())
    for a, b in zip(A.mcsr_arrays(), B.mcsr_arrays()):
        eq(a, b)
    del A  # the clone owns its arrays
    eq(B.mcsr_arrays()[2], g["mcsr_val"])
    eq(_apply(ra, B, g["x"], np.float64), g["spmv_mcsr"])
    F = ra.LocalMatrix(np.float32)
    with pytest.raises(ra.RamdError) as e:
        F.CastFrom(B)
    assert e.value.status == 6  # RAMD_ERR_STATE, as from a DIA source: the value cast is defined on CSR
    B.Clear()
    assert B.GetFormat() == ra.CSR and B.GetNnz() == 0


# -------------------------------------------------------------------------------------------------- the fused product + dot
def _fused(ra, A, x, w, dtype):
    """-> (y, <x, y>, <w, y>) through ramd_fused_apply_dot / _dotv, what CG and BiCGStab call"""
    from rocalution_amd import capi
    lib = capi.load()
    n = A.GetM()
    xv, wv = ra.LocalVector(dtype, data=x), ra.LocalVector(dtype, data=w)
    yv = ra.LocalVector(dtype); yv.Allocate("", n)
    out = C.c_double(0.0)
    res = []
    for call in (lambda: lib.ramd_fused_apply_dot(A._h, xv._h, yv._h, 7), lambda: lib.ramd_fused_apply_dotv(A._h, xv._h, yv._h, wv._h, 7)):
        capi.check(lib.ramd_scalars_set(7, -1.0))
        yv.Zeros()
        capi.check(call())
        capi.check(lib.ramd_scalars_fetch(C.byref(out), 7, 1))
        res.append((yv.numpy(), out.value))
    eq(res[0][0], res[1][0])
    return res[0][0], res[0][1], res[1][1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["tri_1", "tri_65", "tri_1000", "diag_only_130", "shuffled_257", "longrow", "hub"])
def test_fused_product_and_dot_equals_apply_then_dot(ra, name, dtype):
    """Operands that are multiples of 1/8: every product and every partial sum of the dot is exact in double (the kernels
    multiply and add the dot in double), so the fused kernel's per-wave partials and LocalVector::Dot's grid-stride partials,
    two different orders of the same additions, must give the same bits"""
    rp, ci, va = cases.case(name)
    n = len(rp) - 1
    x, w = cases.dyadic(n, 21).astype(dtype), cases.dyadic(n, 22, -8, 8).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToMCSR() == ra.MCSR
    y_ref = _apply(ra, A, x, dtype)
    eq(y_ref, ref.apply(*ref.csr_to_mcsr(rp, ci, va.astype(dtype)), x))
    yv = ra.LocalVector(dtype, data=y_ref)
    dot_x, dot_w = yv.Dot(ra.LocalVector(dtype, data=x)), yv.Dot(ra.LocalVector(dtype, data=w))
    assert dot_x == math.fsum(float(a) * float(b) for a, b in zip(x, y_ref))  # (exact indeed)
    y, fx, fw = _fused(ra, A, x, w, dtype)
    eq(y, y_ref)
    assert (fx, fw) == (dot_x, dot_w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["gr3030", "lap27_6"])
def test_fused_product_and_dot_on_inexact_operands(ra, name, dtype):
    """the goldens' x and values round in every operation: y is still the recorded product bit for bit; the two dots differ from
    the exactly rounded sum (math.fsum) by at most n 2^-52 sum |w_i y_i|, the bound of n double additions in any order"""
    g = ref.load(name)
    rp, ci, va, x = g["rowptr"], g["col"], g["val"].astype(dtype), g["x"].astype(dtype)
    n = len(rp) - 1
    w = np.random.default_rng(9).uniform(-1.0, 1.0, size=n).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToMCSR() == ra.MCSR
    y_ref = g["spmv_mcsr" + ("" if dtype == np.float64 else "_f32")]
    y, fx, fw = _fused(ra, A, x, w, dtype)
    eq(y, y_ref)
    for got, against in ((fx, x), (fw, w)):
        terms = [float(a) * float(b) for a, b in zip(against, y_ref)]
        exact, bound = math.fsum(terms), n * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
        unfused = ra.LocalVector(dtype, data=y_ref).Dot(ra.LocalVector(dtype, data=against))
        print("%s %s: fused %.17g unfused %.17g exact %.17g bound %.3g" % (name, np.dtype(dtype).name, got, unfused, exact, bound))
        assert abs(got - exact) <= bound


# ------------------------------------------------------------------------------------------------------------------- diagonal
def test_diagonal_extraction_is_native_and_equals_the_csr_path(ra):
    """val[0 .. n) copied, or inverted by the CSR kernel's rule; the operator keeps its format"""
    g = load_golden("poisson8")
    n = len(g["rowptr"]) - 1
    runs = {}
    for fmt in ("CSR", "MCSR"):
        A = _mat(ra, g["rowptr"], g["col"], g["val"])
        assert A.ConvertTo(getattr(ra, fmt)) == getattr(ra, fmt)
        d, dinv = ra.LocalVector(), ra.LocalVector()
        d.Allocate("", n); dinv.Allocate("", n)
        A.ExtractDiagonal(d)
        A.ExtractInverseDiagonal(dinv)
        runs[fmt] = (d.numpy(), dinv.numpy())
        assert A.GetFormat() == getattr(ra, fmt)
    eq(runs["CSR"][0], runs["MCSR"][0]); eq(runs["CSR"][1], runs["MCSR"][1])
    eq(runs["MCSR"][1], g["inv_diag"])
    eq(runs["MCSR"][0], ref.load("poisson8")["mcsr_val"][:n])


@pytest.mark.parametrize("dtype", DTYPES)
def test_inverse_diagonal_of_a_zero_is_one_as_in_csr(ra, dtype):
    rp, ci, va = cases.case("zeros_64")  # rows 20 and 30 store 0.0 and -0.0 on the diagonal
    runs = []
    for fmt in (ra.CSR, ra.MCSR):
        A = _mat(ra, rp, ci, va, dtype=dtype)
        assert A.ConvertTo(fmt) == fmt
        d = ra.LocalVector(dtype); d.Allocate("", 64)
        A.ExtractInverseDiagonal(d)
        runs.append(d.numpy())
    eq(runs[0], runs[1])
    assert runs[1][20] == 1 and runs[1][30] == 1


# --------------------------------------------------------------------------------------------------------------------- solvers
def _check_hist(hist, ref_hist, rtol=2e-6):
    """the bar of tests/test_gpu_solvers.py for a CG history against the reference's: relative 2e-6 per recorded iteration
    up to the last two, with its absolute floor at round-off level"""
    m = min(len(hist), len(ref_hist)) - 2
    assert m > 0
    h, r = np.asarray(hist[:m]), np.asarray(ref_hist[:m])
    assert np.all(np.abs(h - r) <= rtol * np.abs(r) + 1e-12 * h[0]), np.max(np.abs(h / r - 1))


@pytest.mark.parametrize("name", ["gr3030", "poisson8"])
def test_cg_jacobi_history(ra, S, name):
    g = ref.load(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToMCSR() == ra.MCSR
    rhs = ra.LocalVector(data=g["rhs"])
    ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Build()
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    assert A.GetFormat() == ra.MCSR
    meta = g["cg_jacobi_mcsr_meta"]
    assert abs(ls.GetIterationCount() - int(meta[0])) <= 1 and ls.GetSolverStatus() == int(meta[1])
    _check_hist(ls.GetResidualHistory(), g["cg_jacobi_mcsr_hist"])
    want = g["cg_jacobi_mcsr_x"]
    assert np.linalg.norm(x.numpy() - want) / np.linalg.norm(want) < 1e-8
    ls.Clear()


@pytest.mark.parametrize("when", ["before_build", "after_build"])
def test_cg_jacobi_poisson16(ra, S, when):
    """tests/test_gpu_solvers.py::test_convert_after_build's bar, with the operator converted before Build() as well"""
    from rocalution_amd import generators as gen
    g = load_golden("poisson16")
    rp, ci, va = gen.poisson7(16)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = ra.LocalVector(data=g["rhs_ones"])
    if when == "before_build":
        assert A.ConvertToMCSR() == ra.MCSR
    ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Build()
    if when == "after_build":
        assert A.ConvertToMCSR() == ra.MCSR
    assert A.GetFormat() == ra.MCSR
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    meta = g["cg_jacobi_meta"]  # (the reference's CG + Jacobi on this operator; its count does not depend on the format)
    assert abs(ls.GetIterationCount() - int(meta[0])) <= 2
    assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-3
    ls.Clear()


def test_multicolored_sgs_with_mcsr_blocks(ra, S):
    """SetPrecondMatrixFormat(MCSR): the square diagonal blocks convert, the rectangular ones are refused and stay CSR (a
    warning, as in the reference); CG converges in the iteration count of CSR blocks, +-1"""
    g = load_golden("poisson8")
    n = len(g["rowptr"]) - 1
    iters = {}
    for fmt in (None, ra.MCSR):
        A = _mat(ra, g["rowptr"], g["col"], g["val"])
        pc = S.MultiColoredSGS()
        if fmt is not None:
            pc.SetPrecondMatrixFormat(fmt)
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
        x = ra.LocalVector(); x.Allocate("", n)
        ls.Solve(ra.LocalVector(data=g["rhs_ones"]), x)
        assert ls.GetSolverStatus() in (1, 2)  # converged (absolute or relative tolerance)
        assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-3
        iters[fmt] = ls.GetIterationCount()
        ls.Clear()
    assert abs(iters[ra.MCSR] - iters[None]) <= 1
