"""The DIA format on the device: CSR <-> DIA, the diagonal-wise products, the fused product + dot, and CG + Jacobi on a
converted operator.

Yardstick: the CPU oracle (oracle/oracle.py: csr_to_dia, dia_apply, dia_apply_add, dia_to_csr, pinned bit-exact to the
reference's host backend) and the committed goldens.  Conversions and products are compared byte for byte: the library is
built with -ffp-contract=off and forms every row's sum in the host loop's order.  tests/test_cpu_dia.py checks without a GPU
that the oracle accepts every generated matrix, so nothing here depends on a refusal except where it says so.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dia_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
GOLDEN_DIA = ["gr3030", "poisson8", "lap2d7", "lap27_6"]  # 9, 7, 5 and 27 diagonals


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
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "max abs diff %g" % np.max(np.abs(a - b))


def eq_nan(a, b):
    """byte for byte except that a NaN matches a NaN: the sign and payload of a NaN that an invalid operation creates
    (0 * inf) are the processor's choice, not the algorithm's"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (np.nonzero(na)[0], np.nonzero(nb)[0])
    eq(np.where(na, 0, a), np.where(nb, 0, b))


def _mat(ra, rp, ci, va, nrow=None, ncol=None, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(np.asarray(rp, np.int32), ci, np.asarray(va, dtype), nrow=nrow, ncol=ncol)
    return A


def _apply(ra, A, x, dtype):
    xv = ra.LocalVector(dtype, data=x)
    yv = ra.LocalVector(dtype); yv.Allocate("", A.GetM())
    A.Apply(xv, yv)
    return yv.numpy()


def _apply_add(ra, A, x, scalar, y, dtype):
    xv = ra.LocalVector(dtype, data=x)
    yv = ra.LocalVector(dtype, data=y)
    A.ApplyAdd(xv, scalar, yv)
    return yv.numpy()


# -------------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", GOLDEN_DIA)
def test_goldens(ra, oracle, name, dtype):
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"].astype(dtype)
    n = len(rp) - 1
    x, y0 = g["x"].astype(dtype), g["y"].astype(dtype)
    off, dv = oracle.csr_to_dia(rp, ci, va)
    y_ref, ya_ref = oracle.dia_apply(n, off, dv, x), oracle.dia_apply_add(n, off, dv, x, -0.75, y0)
    brp, bci, bva = oracle.dia_to_csr(n, off, dv)
    if dtype == np.float64:  # the oracle is the goldens' restatement: here the committed fields themselves
        eq(off, g["dia_offset"]); eq(dv, g["dia_val"])
        eq(y_ref, g["spmv_dia"]); eq(ya_ref, g["spmv_dia_add"])
        eq(brp, g["dia_back_rowptr"]); eq(bci, g["dia_back_col"]); eq(bva, g["dia_back_val"])
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToDIA() == ra.DIA and A.GetFormat() == ra.DIA
    assert (A.GetM(), A.GetN(), A.GetNnz()) == (n, n, n * len(off))
    goff, gval = A.dia_arrays()
    eq(goff, off); eq(gval, dv)
    eq(_apply(ra, A, x, dtype), y_ref)
    eq(_apply_add(ra, A, x, -0.75, y0, dtype), ya_ref)
    assert A.ConvertTo(ra.DIA) == ra.DIA  # already there: nothing happens
    eq(A.dia_arrays()[1], dv)
    assert A.ConvertToCSR() == ra.CSR and A.GetNnz() == len(bva)
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva)
    eq(_apply(ra, A, x, dtype), oracle.csr_apply(brp, bci, bva, x))


@pytest.mark.parametrize("name", ["rand300", "rand300ell"])
def test_refused_conversion_leaves_a_working_csr_matrix(ra, oracle, name):
    g = load_golden(name)
    assert oracle.csr_to_dia(g["rowptr"], g["col"], g["val"]) is None
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert A.ConvertToDIA() == ra.CSR and A.GetFormat() == ra.CSR and A.GetNnz() == len(g["val"])
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])
    with pytest.raises(ra.RamdError) as e:
        A.dia_arrays()
    assert e.value.status == 6  # RAMD_ERR_STATE
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, g["rowptr"].astype(np.int32)); eq(hci, g["col"].astype(np.int32)); eq(hva, g["val"])


# ------------------------------------------------------------------------------------------ shapes where the kernel can go wrong
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_generated_cases(ra, oracle, name, dtype):
    rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    n = len(rp) - 1
    off, dv = oracle.csr_to_dia(rp, ci, va)  # (accepted: tests/test_cpu_dia.py)
    brp, bci, bva = oracle.dia_to_csr(n, off, dv)
    x = (cases.special_x(n) if name == "holes_64" else cases.dyadic(n, 5)).astype(dtype)
    y0 = cases.dyadic(n, 6, -16, 16).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToDIA() == ra.DIA
    assert A.GetNnz() == n * len(off)
    goff, gval = A.dia_arrays()
    eq(goff, off); eq(gval, dv)
    cmp = eq_nan if name == "holes_64" else eq
    cmp(_apply(ra, A, x, dtype), oracle.dia_apply(n, off, dv, x))
    cmp(_apply_add(ra, A, x, -0.75, y0, dtype), oracle.dia_apply_add(n, off, dv, x, -0.75, y0))
    if name == "holes_64":  # a padded zero inside the range is multiplied; what lies outside the range is never read
        assert np.nonzero(np.isnan(_apply(ra, A, x, dtype)))[0].tolist() == [0, 1, 20, 30]
    assert A.ConvertToCSR() == ra.CSR
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva)


def test_nan_values_survive_the_round_trip(ra, oracle):
    rp, ci, va = cases.case("tri_65")
    va[7] = np.nan
    off, dv = oracle.csr_to_dia(rp, ci, va)
    brp, bci, bva = oracle.dia_to_csr(65, off, dv)
    assert len(bva) == len(va) and np.isnan(bva[7])
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToDIA() == ra.DIA
    eq(A.dia_arrays()[1], dv)
    assert A.ConvertToCSR() == ra.CSR
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva)


def test_non_square_is_refused(ra):
    rp, ci, va = cases.banded(12, (-1, 0, 1), 3)
    for nrow, ncol in ((12, 30), (12, 13)):
        A = _mat(ra, rp, ci, va, nrow=nrow, ncol=ncol)
        assert A.ConvertToDIA() == ra.CSR and A.GetFormat() == ra.CSR
        hrp, hci, hva = A.CopyToCSR()
        eq(hrp, rp); eq(hci, ci); eq(hva, va)
    # nrow > ncol: two empty rows under the 12 x 12 band
    tall = np.concatenate([rp, rp[-1:], rp[-1:]])
    A = _mat(ra, tall, ci, va, nrow=14, ncol=12)
    assert A.ConvertToDIA() == ra.CSR and A.GetFormat() == ra.CSR
    eq(A.CopyToCSR()[0], tall)


def test_wide_source_is_unsupported(ra):
    from rocalution_amd import capi
    rp, ci, va = cases.case("tri_65")
    A = _mat(ra, rp, ci, va)
    A.ForceWide(True)
    assert capi.load().ramd_mat_convert(A._h, ra.DIA) == 3  # RAMD_ERR_UNSUPPORTED
    with pytest.raises(ra.RamdError) as e:
        A.ConvertToDIA()
    assert e.value.status == 3 and "not provided for 64-bit row offsets" in str(e.value)
    assert A.GetFormat() == ra.CSR and A.GetPtrBits() == 64
    A.ForceWide(False)
    assert A.ConvertToDIA() == ra.DIA


@pytest.mark.parametrize("n", [0, 5])
def test_a_matrix_without_entries_converts_as_it_does_to_ell(ra, n):
    """no rows, or rows and no entry: ELL gets width 0, DIA gets no diagonal; Apply gives zeros, ApplyAdd changes nothing"""
    rp = np.zeros(n + 1, np.int32)
    none_i, none_v = np.zeros(0, np.int32), np.zeros(0)
    E = _mat(ra, rp, none_i, none_v, nrow=n, ncol=n)
    assert E.ConvertToELL() == ra.ELL and E.GetNnz() == 0
    A = _mat(ra, rp, none_i, none_v, nrow=n, ncol=n)
    assert A.ConvertToDIA() == ra.DIA and A.GetNnz() == 0
    off, val = A.dia_arrays()
    assert len(off) == 0 and len(val) == 0
    if n:
        x = np.arange(1.0, n + 1.0)
        eq(_apply(ra, A, x, np.float64), np.zeros(n))
        eq(_apply_add(ra, A, x, 2.0, x, np.float64), x)
    B = ra.LocalMatrix(); B.CloneFrom(A)
    assert B.GetFormat() == ra.DIA
    assert A.ConvertToCSR() == ra.CSR and A.GetNnz() == 0 and (A.GetM(), A.GetN()) == (n, n)
    if n:
        eq(A.CopyToCSR()[0], rp)


# ----------------------------------------------------------------------------------------------------------------- clone, cast
def test_clone_keeps_format_and_product_and_cast_answers_with_a_status(ra, oracle):
    g = load_golden("gr3030")
    rp, ci, va, x = g["rowptr"], g["col"], g["val"], g["x"]
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToDIA() == ra.DIA
    B = ra.LocalMatrix(); B.CloneFrom(A)
    assert B.GetFormat() == ra.DIA and (B.GetM(), B.GetN(), B.GetNnz()) == (A.GetM(), A.GetN(), A.GetNnz())
    for a, b in zip(A.dia_arrays(), B.dia_arrays()):
        eq(a, b)
    del A  # the clone owns its arrays
    eq(B.dia_arrays()[0], g["dia_offset"]); eq(B.dia_arrays()[1], g["dia_val"])
    eq(_apply(ra, B, x, np.float64), g["spmv_dia"])
    F = ra.LocalMatrix(np.float32)
    with pytest.raises(ra.RamdError) as e:
        F.CastFrom(B)
    assert e.value.status == 6  # RAMD_ERR_STATE: the value cast is defined on CSR
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
@pytest.mark.parametrize("name", ["tri_1", "tri_65", "tri_1000", "band40_130", "far300_1000", "corners_200", "off3_only"])
def test_fused_product_and_dot_equals_apply_then_dot(ra, name, dtype):
    """Operands that are multiples of 1/8: every product and every partial sum of the dot is exact in double (the kernels
    multiply and add the dot in double), so the fused kernel's per-wave partials and LocalVector::Dot's grid-stride partials,
    two different orders of the same additions, must give the same bits"""
    rp, ci, va = cases.case(name)
    n = len(rp) - 1
    x, w = cases.dyadic(n, 21).astype(dtype), cases.dyadic(n, 22, -8, 8).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToDIA() == ra.DIA
    y_ref = _apply(ra, A, x, dtype)
    yv = ra.LocalVector(dtype, data=y_ref)
    dot_x, dot_w = yv.Dot(ra.LocalVector(dtype, data=x)), yv.Dot(ra.LocalVector(dtype, data=w))
    assert dot_x == math.fsum(float(a) * float(b) for a, b in zip(x, y_ref))  # (exact indeed)
    y, fx, fw = _fused(ra, A, x, w, dtype)
    eq(y, y_ref)
    assert (fx, fw) == (dot_x, dot_w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["gr3030", "lap27_6"])
def test_fused_product_and_dot_on_inexact_operands(ra, name, dtype):
    """the goldens' x and values round in every operation: y is still the product bit for bit; the two dots differ from the
    exactly rounded sum (math.fsum) by at most n 2^-52 sum |w_i y_i|, the bound of n double additions in any order"""
    g = load_golden(name)
    rp, ci, va, x = g["rowptr"], g["col"], g["val"].astype(dtype), g["x"].astype(dtype)
    n = len(rp) - 1
    w = np.random.default_rng(9).uniform(-1.0, 1.0, size=n).astype(dtype)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToDIA() == ra.DIA
    y_ref = _apply(ra, A, x, dtype)
    y, fx, fw = _fused(ra, A, x, w, dtype)
    eq(y, y_ref)
    for got, against in ((fx, x), (fw, w)):
        terms = [float(a) * float(b) for a, b in zip(against, y_ref)]
        exact, bound = math.fsum(terms), n * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
        unfused = ra.LocalVector(dtype, data=y_ref).Dot(ra.LocalVector(dtype, data=against))
        print("%s %s: fused %.17g unfused %.17g exact %.17g bound %.3g" % (name, np.dtype(dtype).name, got, unfused, exact, bound))
        assert abs(got - exact) <= bound


# --------------------------------------------------------------------------------------------------------------------- solvers
def _check_hist(hist, ref_hist, rtol=2e-6):
    """the bar of tests/test_gpu_solvers.py for a CG history against the reference's: relative 2e-6 per recorded iteration
    up to the last two, with its absolute floor at round-off level"""
    m = min(len(hist), len(ref_hist)) - 2
    assert m > 0
    h, r = np.asarray(hist[:m]), np.asarray(ref_hist[:m])
    assert np.all(np.abs(h - r) <= rtol * np.abs(r) + 1e-12 * h[0]), np.max(np.abs(h / r - 1))


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
        assert A.ConvertToDIA() == ra.DIA
    ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Build()
    if when == "after_build":
        assert A.ConvertToDIA() == ra.DIA
    assert A.GetFormat() == ra.DIA
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    meta = g["cg_jacobi_dia_meta"]
    assert abs(ls.GetIterationCount() - int(meta[0])) <= 2
    assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-3
    ls.Clear()


@pytest.mark.parametrize("name", ["gr3030", "poisson8"])
def test_cg_jacobi_history(ra, S, name):
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToDIA() == ra.DIA
    rhs = ra.LocalVector(data=g["rhs_ones"])
    ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Build()
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    meta = g["cg_jacobi_dia_meta"]
    assert abs(ls.GetIterationCount() - int(meta[0])) <= 1 and ls.GetSolverStatus() == int(meta[1])
    _check_hist(ls.GetResidualHistory(), g["cg_jacobi_dia_hist"])
    ref = g["cg_jacobi_dia_x"]
    assert np.linalg.norm(x.numpy() - ref) / np.linalg.norm(ref) < 1e-8
    ls.Clear()


def test_inverse_diagonal_goes_through_a_csr_copy(ra):
    """what Jacobi's Build() asks of the operator: the reference's front end converts to CSR first; here a copy is converted
    and the operator keeps its format"""
    g = load_golden("poisson8")
    n = len(g["rowptr"]) - 1
    runs = []
    for fmt in ("CSR", "DIA"):
        A = _mat(ra, g["rowptr"], g["col"], g["val"])
        assert A.ConvertTo(getattr(ra, fmt)) == getattr(ra, fmt)
        d = ra.LocalVector(); d.Allocate("", n)
        A.ExtractInverseDiagonal(d)
        runs.append(d.numpy())
        assert A.GetFormat() == getattr(ra, fmt)
    eq(runs[0], runs[1]); eq(runs[1], g["inv_diag"])
