"""ELL, HYB and COO on the device at the shapes the goldens and poisson7 do not reach: ragged rows, empty rows, row counts off
a wave, rectangular operands, the 5x limit of ELL, HYB without a tail / with one long tail row / with tails in 500 rows,
unsorted rows.  The conversions (k_csr2ell, k_csr2hyb, k_expand_rows, build_coo_groups, k_x2csr_*), the products (k_ell, k_ell2,
k_coo_grouped), the fused product + dot (k_coo_grouped_dot on top) -- and what a change of format leaves of the row-pattern
analysis of the format before it.

Yardsticks: the layout rules of the reference restated in tests/_ellhyb_cases.py and the CPU oracle's products;
tests/test_cpu_ellhyb.py pins the former to the oracle and the goldens, checks without a GPU that the oracle accepts every case
used as ELL here, and that the dyadic data makes every sum exact.  So every comparison in this file is bit for bit, in fp64
and fp32, and there is no tolerance in it."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ellhyb_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [np.float64, np.float32]
FORMATS = ["ELL", "HYB", "COO"]
FMT_CASES = [(f, n) for f in FORMATS for n in (cases.ELL_NAMES if f == "ELL" else cases.NAMES)]
SCALAR = -0.75


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "differs in %d places" % np.sum(a != b)


def _mat(ra, name, dtype):
    nrow, ncol, rp, ci, va = cases.case(name)
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(rp, ci, va.astype(dtype), nrow=nrow, ncol=ncol)
    assert (A.GetM(), A.GetN(), A.GetNnz(), A.GetFormat()) == (nrow, ncol, len(va), ra.CSR)
    return A


def _apply(ra, A, x, dtype):
    xv = ra.LocalVector(dtype, data=x)
    yv = ra.LocalVector(dtype); yv.Allocate("", A.GetM())
    A.Apply(xv, yv)
    return yv.numpy()


def _apply_add(ra, A, x, y0, dtype):
    xv, yv = ra.LocalVector(dtype, data=x), ra.LocalVector(dtype, data=y0)
    A.ApplyAdd(xv, SCALAR, yv)
    return yv.numpy()


def _layout(fmt, nrow, rp, ci, va):
    """the restated layout of `fmt` -> (ell part or None, coo part or None, GetNnz())"""
    if fmt == "ELL":
        w, ec, ev = cases.csr_to_ell(nrow, rp, ci, va)
        return (w, ec, ev), None, w * nrow
    if fmt == "HYB":
        w, ec, ev, cr, cc, cv = cases.csr_to_hyb(nrow, rp, ci, va)
        return (w, ec, ev), (cr, cc, cv), w * nrow + len(cv)
    return None, cases.csr_to_coo(nrow, rp, ci, va), len(va)


def _back(fmt, nrow, ncol, ell, coo):
    if fmt == "ELL":
        return cases.ell_to_csr(nrow, ncol, *ell)
    if fmt == "HYB":
        return cases.hyb_to_csr(nrow, ncol, *ell, *coo)
    return cases.coo_to_csr(nrow, *coo)


def _products(oracle, fmt, nrow, ncol, ell, coo, x, y0):
    if fmt == "ELL":
        return oracle.ell_apply(nrow, *ell, x), oracle.ell_apply_add(nrow, *ell, x, SCALAR, y0)
    if fmt == "HYB":
        return oracle.hyb_apply(nrow, ncol, *ell, *coo, x), oracle.hyb_apply_add(nrow, ncol, *ell, *coo, x, SCALAR, y0)
    return oracle.coo_apply(nrow, *coo, x), oracle.coo_apply_add(*coo, x, SCALAR, y0)


def _check_layout(A, ell, coo, nnz):
    assert A.GetNnz() == nnz
    if ell is not None:
        w, ec, ev = A.ell_arrays()
        assert w == ell[0]
        eq(ec, ell[1]); eq(ev, ell[2])
    if coo is not None:
        for a, b in zip(A.coo_arrays(), coo):
            eq(a, b)


def _check_products(ra, oracle, A, fmt, name, ell, coo, dtype):
    nrow, ncol = cases.case(name)[:2]
    y0 = cases.y0_of(name).astype(dtype)
    for x in (cases.x_of(name).astype(dtype), cases.poisoned_x(name).astype(dtype)):
        y, ya = _products(oracle, fmt, nrow, ncol, ell, coo, x, y0)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(ya))  # (no padded slot multiplies an element of x)
        eq(_apply(ra, A, x, dtype), y)
        eq(_apply_add(ra, A, x, y0, dtype), ya)


# ---------------------------------------------------------------------------------- layouts, products and the ways back to CSR
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt,name", FMT_CASES)
def test_layout_products_and_the_way_back(ra, oracle, fmt, name, dtype):
    nrow, ncol, rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    ell, coo, nnz = _layout(fmt, nrow, rp, ci, va)
    A = _mat(ra, name, dtype)
    F = getattr(ra, fmt)
    assert A.ConvertTo(F) == F and A.GetFormat() == F and (A.GetM(), A.GetN()) == (nrow, ncol)
    _check_layout(A, ell, coo, nnz)
    _check_products(ra, oracle, A, fmt, name, ell, coo, dtype)
    # X -> CSR: storage order for ELL and HYB, columns sorted (stably) inside every row for COO
    brp, bci, bva = _back(fmt, nrow, ncol, ell, coo)
    assert A.ConvertTo(ra.CSR) == ra.CSR and A.GetFormat() == ra.CSR and A.GetNnz() == len(bva) == len(va)
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, brp); eq(hci, bci); eq(hva, bva.astype(dtype))
    if fmt != "COO" or name not in cases.UNSORTED:
        eq(hrp, rp); eq(hci, ci); eq(hva, va)
    else:
        assert cases.rows_sorted(hrp, hci) and not np.array_equal(hci, ci)
    x = cases.poisoned_x(name).astype(dtype)
    eq(_apply(ra, A, x, dtype), oracle.csr_apply(brp, bci, bva.astype(dtype), x))


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_ell_conversion_leaves_a_working_csr_matrix(ra, oracle, dtype):
    """one entry over the reference's limit max row nnz <= 5 * (nnz / nrow); with exactly the limit the conversion is taken
    (ell_at_limit, among the cases above)"""
    name = "ell_over_limit"
    nrow, ncol, rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    A = _mat(ra, name, dtype)
    assert A.ConvertTo(ra.ELL) == ra.CSR and A.GetFormat() == ra.CSR and A.GetNnz() == len(va)
    hrp, hci, hva = A.CopyToCSR()
    eq(hrp, rp); eq(hci, ci); eq(hva, va)
    x, y0 = cases.poisoned_x(name).astype(dtype), cases.y0_of(name).astype(dtype)
    eq(_apply(ra, A, x, dtype), oracle.csr_apply(rp, ci, va, x))
    eq(_apply_add(ra, A, x, y0, dtype), oracle.csr_apply_add(rp, ci, va, x, SCALAR, y0))
    with pytest.raises(ra.RamdError) as e:
        A.ell_arrays()
    assert e.value.status == 6  # RAMD_ERR_STATE
    B = _mat(ra, "ell_at_limit", dtype)
    assert B.ConvertTo(ra.ELL) == ra.ELL and B.ell_arrays()[0] == 10


@pytest.mark.parametrize("name", ["wide_300x1000", "tall_1000x300"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_vector_of_the_wrong_size_is_refused(ra, fmt, name):
    nrow, ncol = cases.case(name)[:2]
    A = _mat(ra, name, np.float64)
    assert A.ConvertTo(getattr(ra, fmt)) == getattr(ra, fmt)
    good_x, good_y = ra.LocalVector(data=np.zeros(ncol)), ra.LocalVector(data=np.zeros(nrow))
    A.Apply(good_x, good_y)
    for x, y in ((good_y, good_x), (good_x, ra.LocalVector(data=np.zeros(ncol))), (ra.LocalVector(data=np.zeros(nrow)), good_y)):
        with pytest.raises(ra.RamdError):
            A.Apply(x, y)
        with pytest.raises(ra.RamdError):
            A.ApplyAdd(x, SCALAR, y)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged_257", "wide_300x1000", "unsorted_257"])
@pytest.mark.parametrize("src,dst", [(a, b) for a in FORMATS for b in FORMATS if a != b])
def test_from_one_format_to_another_through_csr(ra, oracle, src, dst, name, dtype):
    """LocalMatrix::ConvertTo goes X -> CSR -> Y: the layout of Y is that of the CSR matrix X gives back (for COO: with its
    rows sorted)"""
    nrow, ncol, rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    ell, coo, _ = _layout(src, nrow, rp, ci, va)
    mrp, mci, mva = _back(src, nrow, ncol, ell, coo)
    ell, coo, nnz = _layout(dst, nrow, mrp, mci, mva)
    A = _mat(ra, name, dtype)
    assert A.ConvertTo(getattr(ra, src)) == getattr(ra, src)
    assert A.ConvertTo(getattr(ra, dst)) == getattr(ra, dst) and A.GetFormat() == getattr(ra, dst)
    _check_layout(A, ell, coo, nnz)
    _check_products(ra, oracle, A, dst, name, ell, coo, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged_257", "tall_1000x300", "hyb_one_long_65"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_clone_in_every_format(ra, oracle, fmt, name, dtype):
    if fmt == "ELL" and name not in cases.ELL_NAMES:
        name = "hyb_many_tails_1000"  # (the one long row is refused as ELL)
    nrow, ncol, rp, ci, va = cases.case(name)
    ell, coo, nnz = _layout(fmt, nrow, rp, ci, va.astype(dtype))
    A = _mat(ra, name, dtype)
    assert A.ConvertTo(getattr(ra, fmt)) == getattr(ra, fmt)
    B = ra.LocalMatrix(dtype); B.CloneFrom(A)
    assert B.GetFormat() == getattr(ra, fmt) and (B.GetM(), B.GetN()) == (nrow, ncol)
    del A  # the clone owns its arrays
    _check_layout(B, ell, coo, nnz)
    _check_products(ra, oracle, B, fmt, name, ell, coo, dtype)
    assert B.ConvertTo(ra.CSR) == ra.CSR
    for a, b in zip(B.CopyToCSR(), _back(fmt, nrow, ncol, ell, coo)):
        eq(a, b)


# ------------------------------------------------------------------------------------------------- the fused product and dot
def _exact_dot(a, b):
    return math.fsum(float(p) * float(q) for p, q in zip(a, b))


FUSED = [(f, n) for f in FORMATS for n in cases.RAGGED + ["hyb_many_tails_1000", "hyb_one_long_65"]
         if f != "ELL" or n in cases.ELL_NAMES]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt,name", FUSED)
def test_fused_product_and_dot(ra, fmt, name, dtype):
    """ramd_fused_apply_dot / _dotv (CG, BiCGStab): y is Apply's, the scalar <x, y> / <w, y>; ramd_fused_apply_add_dot: y is
    ApplyAdd's and a slot that held <p, y_old> holds <p, y_new>.  Multiples of 1/8: every product and partial sum of the dots
    is exact in double, whatever their order, so the scalars are compared with =="""
    from rocalution_amd import capi
    lib = capi.load()
    n = cases.case(name)[0]
    x, y0 = cases.x_of(name).astype(dtype), cases.y0_of(name).astype(dtype)
    w = cases.dyadic(n, 23, -8, 8).astype(dtype)
    A = _mat(ra, name, dtype)
    assert A.ConvertTo(getattr(ra, fmt)) == getattr(ra, fmt)
    y_ref, ya_ref = _apply(ra, A, x, dtype), _apply_add(ra, A, x, y0, dtype)
    xv, wv = ra.LocalVector(dtype, data=x), ra.LocalVector(dtype, data=w)
    out = C.c_double(0.0)
    for against, call in ((x, lambda yv: lib.ramd_fused_apply_dot(A._h, xv._h, yv._h, 7)),
                          (w, lambda yv: lib.ramd_fused_apply_dotv(A._h, xv._h, yv._h, wv._h, 7))):
        yv = ra.LocalVector(dtype, data=y0)  # (what it held before plays no role)
        capi.check(lib.ramd_scalars_set(7, -1.0))
        capi.check(call(yv))
        capi.check(lib.ramd_scalars_fetch(C.byref(out), 7, 1))
        eq(yv.numpy(), y_ref)
        assert out.value == _exact_dot(against, y_ref)
    yv = ra.LocalVector(dtype, data=y0)
    capi.check(lib.ramd_scalars_set(7, _exact_dot(w, y0)))
    capi.check(lib.ramd_fused_apply_add_dot(A._h, xv._h, SCALAR, yv._h, wv._h, 7))
    capi.check(lib.ramd_scalars_fetch(C.byref(out), 7, 1))
    eq(yv.numpy(), ya_ref)
    assert out.value == _exact_dot(w, ya_ref)


# ------------------------------------------------------------------------ what a conversion leaves of the row-pattern analysis
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_analysis_survives_a_format_change_in_a_fresh_process(dtype):
    """multiply, convert, multiply again, with the row-pattern analysis forced on (RAMD_CSR_PAT=1; by default it runs from 2^20
    entries or slots on): tests/_ellhyb_carry.py.  A dictionary of CSR rows read as ELL slot tuples multiplies the padded zeros
    by x[row]; a dictionary of slot tuples read as CSR rows gives the rows that share a tuple the same columns whatever their
    COO tails held.  ramd_mat_convert drops it, and everything derived from it, in both directions; the pattern state is
    checked before every product, so an analysis that survived fails the test before a kernel reads it."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_ellhyb_carry.py"), np.dtype(dtype).name],
                       env=dict(os.environ, RAMD_CSR_PAT="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stdout.decode()[-3000:]


# ----------------------------------------------------------------------------------------------------------- forced kernel forms
FORCED = ["RAMD_CSR_PAT=1", "RAMD_ELL2=1,RAMD_CSR_PAT=1", "RAMD_ELL2=1,RAMD_CSR_PAT=0"]


def _family():
    jobs = {}
    for variant in FORCED:
        env = dict(os.environ)
        for kv in variant.split(","):
            env[kv.split("=")[0]] = kv.split("=")[1]
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k",
               "not fresh_process"]
        jobs[variant] = (cmd, env, 900)
    return jobs


@pytest.mark.parametrize("variant", FORCED)
def test_forced_forms_in_a_fresh_process(variant):
    """every test above once more with the slot tuples of ELL / HYB taken from a row-pattern dictionary whatever the size
    (k_ell<PAT>; the CSR products before and after a conversion from theirs), and with two rows per thread wherever the row
    count is even (k_ell2, with patterns and with the columns read; an odd count keeps k_ell): not a bit may change.  The three
    processes run side by side (conftest.forced_run)"""
    from conftest import forced_run
    rc, out = forced_run("ellhyb", variant, _family())
    assert rc == 0, out[-3000:]
