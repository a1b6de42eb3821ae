"""Worker of tests/test_gpu_ellhyb.py::test_no_analysis_survives_a_format_change_in_a_fresh_process (RAMD_CSR_PAT=1 is read
once per process): a matrix is multiplied in a format whose row-pattern analysis has run, converted, and multiplied again.
The pattern state (ramd_mat_pattern_info) is checked at every step -- 0 right after every change between CSR and ELL / HYB,
so that no kernel ever runs with the dictionary of the format the matrix has left -- and every product against the oracle.

    python tests/_ellhyb_carry.py float64|float32
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import rocalution_amd as ra  # noqa: E402
from rocalution_amd import capi, generators as gen  # noqa: E402
from oracle import oracle  # noqa: E402
import _ellhyb_cases as cases  # noqa: E402

assert os.environ.get("RAMD_CSR_PAT") == "1"
oracle.build(); oracle.set_threads(1); lib = capi.load(); ra.init_rocalution()
dtype = getattr(np, sys.argv[1])


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "differs in %d places" % np.sum(a != b)


def state(A):
    s = C.c_int(9)
    capi.check(lib.ramd_mat_pattern_info(A._h, C.byref(s), None, None))
    return s.value


def mat(rp, ci, va, nrow=None, ncol=None):
    A = ra.LocalMatrix(dtype); A.SetDataPtrCSR(rp, ci, np.asarray(va, dtype), nrow=nrow, ncol=ncol)
    return A


def apply(A, x):
    y = ra.LocalVector(dtype); y.Allocate("", A.GetM())
    A.Apply(ra.LocalVector(dtype, data=np.asarray(x, dtype)), y)
    return y.numpy()


def apply_add(A, x, y0):
    y = ra.LocalVector(dtype, data=np.asarray(y0, dtype))
    A.ApplyAdd(ra.LocalVector(dtype, data=np.asarray(x, dtype)), -0.75, y)
    return y.numpy()


def inputs(name):
    nrow, ncol, rp, ci, va = cases.case(name)
    va, y0 = va.astype(dtype), cases.y0_of(name).astype(dtype)
    ref = {}
    for key, x in (("x", cases.x_of(name).astype(dtype)), ("px", cases.poisoned_x(name).astype(dtype))):
        ref[key] = (x, oracle.csr_apply(rp, ci, va, x), oracle.csr_apply_add(rp, ci, va, x, -0.75, y0))
        assert np.all(np.isfinite(ref[key][1])) and np.all(np.isfinite(ref[key][2]))
    return rp, ci, va, y0, ref


def check(A, y0, r):
    x, y, ya = r
    eq(apply(A, x), y)
    eq(apply_add(A, x, y0), ya)


# ---- odd_columns_512: CSR analysed -> ELL / HYB.  A CSR dictionary holds offset 0 in the slots past a row's length: read as
# an ELL dictionary it sends every padded slot to x[row], NaN in the poisoned x for every even row
rp, ci, va, y0, ref = inputs("odd_columns_512")
for fmt in (ra.ELL, ra.HYB):
    A = mat(rp, ci, va)
    assert state(A) == 0
    check(A, y0, ref["x"])
    assert state(A) == 1, state(A)
    assert A.ConvertTo(fmt) == fmt
    assert state(A) == 0, "the CSR dictionary is still there after ConvertTo(%d)" % fmt
    check(A, y0, ref["px"])
    assert state(A) == 1, state(A)  # (the slot tuples of the ELL block, analysed on that product)
    B = ra.LocalMatrix(dtype); B.CloneFrom(A)  # a clone is a matrix of its own: not analysed yet, the same products
    assert B.GetFormat() == fmt and state(B) == 0
    check(B, y0, ref["px"])
    # ... and back: an ELL dictionary counts its slots, a CSR row its rp
    assert A.ConvertTo(ra.CSR) == ra.CSR
    assert state(A) == 0, "the ELL dictionary is still there after ConvertTo(CSR)"
    for a, b in zip(A.CopyToCSR(), (rp, ci, va)):
        eq(a, b)
    check(A, y0, ref["px"])
    assert state(A) == 1, state(A)

# ---- stencil_tails_512: HYB analysed -> CSR.  Five rows share one slot tuple and differ in their COO tails; as CSR rows they
# are 33 entries long
rp, ci, va, y0, ref = inputs("stencil_tails_512")
A = mat(rp, ci, va)
assert A.ConvertTo(ra.HYB) == ra.HYB and state(A) == 0
check(A, y0, ref["x"])
assert state(A) == 1, state(A)
assert A.ConvertTo(ra.CSR) == ra.CSR
assert state(A) == 0, "the ELL dictionary is still there after ConvertTo(CSR)"
for a, b in zip(A.CopyToCSR(), (rp, ci, va)):
    eq(a, b)
check(A, y0, ref["x"])
assert state(A) == -1, state(A)  # analysed again, for the CSR rows: 33 entries are more than a pattern holds

# ---- width29_64: the ELL analysis gives up (29 slots), and that verdict does not outlive the format either
rp, ci, va, y0, ref = inputs("width29_64")
A = mat(rp, ci, va)
assert A.ConvertTo(ra.ELL) == ra.ELL and state(A) == 0
check(A, y0, ref["px"])
assert state(A) == -1, state(A)
assert A.ConvertTo(ra.CSR) == ra.CSR
assert state(A) == 0
check(A, y0, ref["px"])
assert state(A) == -1, state(A)

# ---- UseRowPatterns(False), the user's setting, holds across conversions.  Seen through the value patterns of a constant
# stencil: they are analysed only for a matrix whose products use its row patterns
rp, ci, va = gen.poisson7(8, np.float64)
n = len(rp) - 1
x = cases.dyadic(n, 9).astype(dtype)
y = oracle.csr_apply(rp, ci, va.astype(dtype), x)
for fmt in (ra.ELL, ra.HYB):
    for use in (True, False):
        A = mat(rp, ci, va)
        A.UseRowPatterns(use)
        assert A.ConvertTo(fmt) == fmt
        eq(apply(A, x), y)
        assert state(A) == 1
        assert A.ConvertTo(ra.CSR) == ra.CSR and state(A) == 0 and A.ValuePatternState() == 0
        eq(apply(A, x), y)
        assert state(A) == 1 and A.ValuePatternState() == (1 if use else 0), (use, state(A), A.ValuePatternState())
print("OK")
