"""Value patterns of the CSR product (spmv.hip: csr_analyse_values, k_csr_patv): a matrix whose values are a function of its
row pattern -- a constant-coefficient stencil -- has them taken from the dictionary; any other matrix keeps the columns-only
path.  Everything is compared BIT FOR BIT with the CPU oracle (or the committed goldens); the fused dot to rel 1e-13 (fp64) of
<x, y> of the bit-exact y, as the other reduction tests do.

RAMD_CSR_PAT / RAMD_CSR_PATV are read once per process, so every case runs in a fresh interpreter with both set to 1 (the
matrices here are far below the size threshold of the analysis).  Shapes: poisson7 N = 8 (512 rows: two full row blocks, all
27 boundary patterns) and N = 9 (729 rows: a partial last block); the 27-point operator of lap27_6.npz for the long-row
dispatch (on by default; RAMD_CSR_PATV_LONG=0 switches it off)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PRELUDE = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rocalution_amd as ra
from rocalution_amd import capi, generators as gen, solvers as S
from oracle import oracle
oracle.build(); oracle.set_threads(1); lib = capi.load(); ra.init_rocalution()
dtype = np.%s
def eq(a, b):
    a = np.asarray(a); b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "max |diff| = %%r" %% float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
def vec(a):
    return ra.LocalVector(dtype, data=np.ascontiguousarray(a, dtype=dtype))
def mat(rp, ci, va, wide=False):
    A = ra.LocalMatrix(dtype); A.SetDataPtrCSR(rp, ci, np.ascontiguousarray(va, dtype=dtype))
    if wide:
        A.ForceWide(True)
    return A
def apply(A, xh):
    y = ra.LocalVector(dtype); y.Allocate("", A.GetM()); A.Apply(vec(xh), y); return y.numpy()
def col_state(A):
    s = C.c_int(9); capi.check(lib.ramd_mat_pattern_info(A._h, C.byref(s), None, None)); return s.value
def rnd(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
def products(rp, ci, va, A, nrow, tol, strict=True):
    # Apply, ApplyAdd (scalar != 1), product + <x, y>, damped-Jacobi sweep: the four instantiations of the kernel.
    # <x, y>: relative `tol` for the operators whose values are patterns (x^T A x of a definite stencil: no cancellation); for
    # the arbitrary values of the fallback cases the bound of a double-precision sum of nrow terms, nrow * 2^-53 * sum |terms|
    va = np.ascontiguousarray(va, dtype=dtype)
    xh, y0, rhs = rnd(5, nrow), rnd(6, nrow), rnd(7, nrow)
    ref = oracle.csr_apply(rp, ci, va, xh)
    eq(apply(A, xh), ref)
    ya = vec(y0); A.ApplyAdd(vec(xh), 0.375, ya)
    eq(ya.numpy(), oracle.csr_apply_add(rp, ci, va, xh, dtype(0.375), y0))
    w = ra.LocalVector(dtype); w.Allocate("", nrow)
    xv = vec(xh)
    capi.check(lib.ramd_fused_apply_dot(A._h, xv._h, w._h, 11))
    eq(w.numpy(), ref)
    out = (C.c_double * 1)(); capi.check(lib.ramd_scalars_fetch(out, 11, 1))
    want = float(np.dot(xh.astype(np.float64), ref.astype(np.float64)))
    bound = tol * abs(want) if strict else nrow * 2.0 ** -53 * float(np.sum(np.abs(xh.astype(np.float64) * ref.astype(np.float64))))
    assert abs(out[0] - want) <= bound, (out[0], want, bound)
    dinv = rnd(8, nrow); omega = dtype(0.8)
    xn = ra.LocalVector(dtype); xn.Allocate("", nrow)
    dv, rv = vec(dinv), vec(rhs)
    capi.check(lib.ramd_fused_jacobi_sweep(A._h, dv._h, rv._h, xv._h, xn._h, float(omega)))
    t = dtype(-1) * ref + rhs; t = dinv * t
    eq(xn.numpy(), xh + omega * t)
"""


def _run(body, dtype, env=None, timeout=300):
    code = PRELUDE % (ROOT, HERE, np.dtype(dtype).name) + body + "\nprint('OK')\n"
    e = dict(os.environ, RAMD_CSR_PAT="1", RAMD_CSR_PATV="1")
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stdout.decode()[-3000:]
    return r.stdout.decode()


TOL = {np.float64: 1e-13, np.float32: 1e-6}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", [8, 9])
def test_value_patterns_products(dtype, N):
    """the 7-point operator: values analysed on the first product (state 0 -> 1), then every form of the product runs k_csr_patv"""
    _run(r"""
rp, ci, va = gen.poisson7(%d, np.float64)
n = len(rp) - 1
A = mat(rp, ci, va)
assert A.ValuePatternState() == 0
apply(A, rnd(1, n))
assert col_state(A) == 1 and A.ValuePatternState() == 1, (col_state(A), A.ValuePatternState())
products(rp, ci, va, A, n, %r)
assert A.ValuePatternState() == 1
# the device generator's operator is the same one
B = ra.LocalMatrix(dtype); B.GenPoisson7(%d)
eq(apply(B, rnd(2, n)), oracle.csr_apply(rp, ci, va.astype(dtype), rnd(2, n)))
assert B.ValuePatternState() == 1
""" % (N, TOL[dtype], N), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_value_patterns_wide_offsets(dtype):
    """the N = 8 operator stored with 64-bit row offsets: the analysis through PatCsr64, then every form of the product, bit
    for bit.  What this case does NOT assert is which kernel ran: the info entry reads int32 matrices only, as every entry
    outside the wide-aware list, so the value state of W cannot be read back (the state of the narrow twin A says nothing
    about W).  A wide matrix that fell back to the columns-only kernel would pass here too, with the same correct result."""
    _run(r"""
rp, ci, va = gen.poisson7(8, np.float64)
n = len(rp) - 1
A = mat(rp, ci, va); apply(A, rnd(1, n)); assert A.ValuePatternState() == 1
W = mat(rp, ci, va, wide=True); assert W.GetPtrBits() == 64
products(rp, ci, va, W, n, %r)
assert col_state(W) == 1
# ... and a wide matrix with one other value still gives the oracle's result
vb = va.copy(); vb[rp[300] + 1] = -1.5
products(rp, ci, vb, mat(rp, ci, vb, wide=True), n, %r, strict=False)
""" % (TOL[dtype], TOL[dtype]), dtype)


@pytest.mark.parametrize("long_rows", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_value_patterns_long_rows_27_point(dtype, long_rows):
    """27-entry rows (beyond k_csr_pat2's reach) take the new kernel as well (the default, RAMD_CSR_PATV_LONG=1); with
    RAMD_CSR_PATV_LONG=0 they keep the columns-only kernels they had, and the values are never analysed"""
    _run(r"""
LONG = %d""" % int(long_rows) + r"""
from conftest import load_golden
g = load_golden("lap27_6")
rp, ci, va = g["rowptr"], g["col"], g["val"]
n = len(rp) - 1
A = mat(rp, ci, va)
y = apply(A, g["x"])
if dtype == np.float64:
    eq(y, g["spmv_csr"])
assert col_state(A) == 1 and A.ValuePatternState() == LONG, (col_state(A), A.ValuePatternState())
products(rp, ci, va, A, n, %r)
assert A.ValuePatternState() == LONG
""" % TOL[dtype], dtype, env={"RAMD_CSR_PATV_LONG": long_rows})


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_value_patterns_fallback(dtype):
    """the Poisson structure with values that are NOT a function of the pattern: state -1, the columns-only path, oracle's bits"""
    _run(r"""
rp, ci, va = gen.poisson7(8, np.float64)
n = len(rp) - 1
interior = 3 * 64 + 3 * 8 + 3
assert rp[interior + 1] - rp[interior] == 7
variants = []
v1 = va.copy(); v1[rp[interior] + 1] = -1.25; variants.append(v1)          # one off-diagonal value of one interior row
diag = np.array([rp[r] + int(np.nonzero(ci[rp[r]:rp[r + 1]] == r)[0][0]) for r in range(n)])
v2 = va.copy(); v2[diag] = 0.0; v2[diag[interior]] = -0.0; variants.append(v2)   # one diagonal -0.0 against 0.0 elsewhere
variants.append(np.random.default_rng(3).uniform(-1, 1, len(va)))           # random values
for vb in variants:
    A = mat(rp, ci, vb)
    apply(A, rnd(1, n))
    assert col_state(A) == 1 and A.ValuePatternState() == -1, (col_state(A), A.ValuePatternState())
    products(rp, ci, vb, A, n, %r, strict=False)
    assert A.ValuePatternState() == -1
# -0.0 everywhere on the diagonal IS a function of the pattern, and the sign of zero reaches the result
v3 = va.copy(); v3[diag] = -0.0
A = mat(rp, ci, v3); apply(A, rnd(1, n)); assert A.ValuePatternState() == 1
products(rp, ci, v3, A, n, %r, strict=False)
""" % (TOL[dtype], TOL[dtype]), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_value_patterns_invalidation(dtype):
    """every in-place writer of the values: a matrix in state 1 is mutated, the next Apply equals the oracle on the NEW values"""
    _run(r"""
rp, ci, va0 = gen.poisson7(8, np.float64)
va0 = va0.astype(dtype)
n = len(rp) - 1
xh = rnd(1, n)
isdiag = np.repeat(np.arange(n), np.diff(rp)) == ci
def fresh():
    A = mat(rp, ci, va0); apply(A, xh); assert A.ValuePatternState() == 1; return A
def check(A, va, want=None):
    va = np.ascontiguousarray(va, dtype=dtype)
    assert A.ValuePatternState() == 0, A.ValuePatternState()
    eq(apply(A, xh), oracle.csr_apply(rp, ci, va, xh))
    rp2, ci2, va2 = A.CopyToCSR()
    eq(va2, va)
    if want is not None:
        assert A.ValuePatternState() == want, (A.ValuePatternState(), want)
a = dtype(0.75)
A = fresh(); A.Scale(0.75); check(A, va0 * a, 1)
A = fresh(); A.ScaleDiagonal(0.75); check(A, np.where(isdiag, va0 * a, va0), 1)
A = fresh(); A.ScaleOffDiagonal(0.75); check(A, np.where(isdiag, va0, va0 * a), 1)
A = fresh(); A.AddScalar(0.75); check(A, va0 + a, 1)
A = fresh(); A.AddScalarDiagonal(0.75); check(A, np.where(isdiag, va0 + a, va0), 1)
A = fresh(); vr = rnd(9, len(va0)); A.UpdateValuesCSR(vr); check(A, vr, -1)
A.UpdateValuesCSR(va0 * dtype(2)); check(A, va0 * dtype(2), 1)                      # ... and pattern values again
A = fresh(); d = rnd(10, n); dv = vec(d); capi.check(lib.ramd_mat_diag_mult(A._h, dv._h, 1))   # DiagonalMatrixMultL, non-constant
check(A, va0 * np.repeat(d, np.diff(rp)), -1)
A = fresh(); A.ILU0Factorize(); assert A.ValuePatternState() == 0
lu = A.CopyToCSR()[2]; assert not np.array_equal(lu, va0)       # the factors in place of the operator's values
check(A, lu)
# Sort: the same rows stored with their columns descending; sorted they are the operator again
rev = np.concatenate([np.arange(rp[r], rp[r + 1])[::-1] for r in range(n)])
B = mat(rp, ci[rev], va0[rev]); eq(apply(B, xh), oracle.csr_apply(rp, ci[rev], va0[rev], xh)); assert B.ValuePatternState() == 1
B.Sort(); assert B.ValuePatternState() == 0
eq(apply(B, xh), oracle.csr_apply(rp, ci, va0, xh)); eq(B.CopyToCSR()[2], va0)
# clone, then mutate the clone: the original keeps its dictionary and its values
A = fresh(); Cl = ra.LocalMatrix(dtype); Cl.CloneFrom(A); assert Cl.ValuePatternState() == 0
Cl.ScaleDiagonal(3.0)
eq(apply(Cl, xh), oracle.csr_apply(rp, ci, np.where(isdiag, va0 * dtype(3), va0).astype(dtype), xh))
assert A.ValuePatternState() == 1
eq(apply(A, xh), oracle.csr_apply(rp, ci, va0, xh))
# MatrixAdd on the same structure (in place)
A = fresh(); O = mat(rp, ci, rnd(11, len(va0))); A.MatrixAdd(O, 1.0, 0.5, False)
assert A.ValuePatternState() == 0
eq(apply(A, xh), oracle.csr_apply(rp, ci, A.CopyToCSR()[2], xh)); assert A.ValuePatternState() == -1
""", dtype)


def test_value_patterns_cast_copy():
    """the fp32 copy MixedPrecisionDC makes of its operator (CastFrom): analysed on its own, in its own dtype; a value that is
    exact in neither precision keeps the two dictionaries apart"""
    _run(r"""
rp, ci, va = gen.poisson7(8, np.float64)
va = va * 0.1                                            # 0.6 / -0.1: not representable, fp32 and fp64 differ
n = len(rp) - 1
A = mat(rp, ci, va); xh = rnd(1, n)
eq(apply(A, xh), oracle.csr_apply(rp, ci, va, xh)); assert A.ValuePatternState() == 1
F = ra.LocalMatrix(np.float32); F.CastFrom(A); assert F.ValuePatternState() == 0
x32 = xh.astype(np.float32); y = ra.LocalVector(np.float32); y.Allocate("", n); F.Apply(ra.LocalVector(np.float32, data=x32), y)
eq(y.numpy(), oracle.csr_apply(rp, ci, va.astype(np.float32), x32))
assert F.ValuePatternState() == 1 and A.ValuePatternState() == 1
A.Scale(2.0)                                             # the original changes, the copy does not
F.Apply(ra.LocalVector(np.float32, data=x32), y); eq(y.numpy(), oracle.csr_apply(rp, ci, va.astype(np.float32), x32))
eq(apply(A, xh), oracle.csr_apply(rp, ci, va * 2.0, xh))
""", np.float64)


@pytest.mark.parametrize("how", ["UseRowPatterns", "RAMD_CSR_PATV=0"])
def test_value_patterns_switched_off(how):
    """ramd_mat_pattern_use(m, 0) switches the values off together with the columns; RAMD_CSR_PATV=0 never analyses them"""
    _run(r"""
rp, ci, va = gen.poisson7(9, np.float64)
n = len(rp) - 1
A = mat(rp, ci, va)
off = %r
if off:
    A.UseRowPatterns(False)
products(rp, ci, va, A, n, 1e-13)
assert col_state(A) == 1 and A.ValuePatternState() == 0, (col_state(A), A.ValuePatternState())   # never analysed: never used
if off:
    A.UseRowPatterns(True); products(rp, ci, va, A, n, 1e-13); assert A.ValuePatternState() == 1
""" % (how == "UseRowPatterns"), np.float64, env=({} if how == "UseRowPatterns" else {"RAMD_CSR_PATV": "0"}))


def test_value_patterns_cg_history_identical(tmp_path):
    """CG + Jacobi on poisson7 N = 16, 40 iterations: residual history and x bit-identical between RAMD_CSR_PATV=0 and =1"""
    outs = []
    for v in ("0", "1"):
        f = str(tmp_path / ("cg_%s.npz" % v))
        _run(r"""
A = ra.LocalMatrix(dtype); A.GenPoisson7(16); n = A.GetM()
ones = ra.LocalVector(dtype); ones.Allocate("", n); ones.Ones()
rhs = ra.LocalVector(dtype); rhs.Allocate("", n); A.Apply(ones, rhs)
x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Init(0.0, 0.0, 1e300, 40); ls.Build()
ls.Solve(rhs, x)
assert ls.GetIterationCount() == 40
assert A.ValuePatternState() == %d, A.ValuePatternState()
np.savez(%r, hist=ls.GetResidualHistory(), x=x.numpy(), res=np.array([ls.GetCurrentResidual()]))
""" % (int(v), f), np.float64, env={"RAMD_CSR_PATV": v})
        outs.append(dict(np.load(f)))
    assert len(outs[0]["hist"]) >= 40
    for k in ("hist", "x", "res"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
