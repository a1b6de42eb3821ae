"""The BCSR format on the device: CSR <-> BCSR, the block-row products, and a solver run on a converted operator.

Yardstick: tests/_bcsr_ref.py, the NumPy restatement of the reference's csr_to_bcsr / bcsr_to_csr / Apply / ApplyAdd
(checked without a GPU by tests/test_cpu_bcsr.py).  Conversions and products are compared bit for bit: the library is built
with -ffp-contract=off and forms every row's sum in the reference's order, one rounded multiply and one rounded add per
stored value.
"""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bcsr_ref as ref  # noqa: E402

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


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "max abs diff %g" % np.max(np.abs(a - b))


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


def _shuffled(rp, ci, va, seed):
    rng = np.random.default_rng(seed)
    ci, va = ci.copy(), va.copy()
    for r in range(len(rp) - 1):
        p = rng.permutation(int(rp[r + 1] - rp[r])) + int(rp[r])
        ci[rp[r]:rp[r + 1]] = ci[p]
        va[rp[r]:rp[r + 1]] = va[p]
    return ci, va


# ---------------------------------------------------------------------------------------------------------------- conversion
CONV = [("poisson8", 2), ("poisson8", 4), ("poisson8", 8), ("rand300", 2), ("rand300", 3), ("rand300", 5), ("rand300", 6)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name,d", CONV)
def test_conversion_equals_the_restatement(ra, name, d, dtype):
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"].astype(dtype)
    n = len(rp) - 1
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, n, n, d)
    crp, cci, cva = ref.bcsr_to_csr(brp, bci, bval, d)
    for k, (ci_k, va_k) in enumerate([(ci, va), _shuffled(rp, ci, va, 7)]):
        A = _mat(ra, rp, ci_k, va_k, dtype=dtype)
        assert A.ConvertTo(ra.BCSR, d) == ra.BCSR and A.GetFormat() == ra.BCSR
        assert (A.GetM(), A.GetN(), A.GetNnz()) == (n, n, len(bci) * d * d)
        gd, grp, gci, gval = A.bcsr_arrays()
        assert gd == d
        eq(grp, brp); eq(gci, bci); eq(gval, bval)
        assert A.ConvertTo(ra.BCSR, d + 1) == ra.BCSR and A.bcsr_arrays()[0] == d  # already BCSR: a no-op, whatever d
        assert A.ConvertToCSR() == ra.CSR
        hrp, hci, hva = A.CopyToCSR()
        eq(hrp, crp); eq(hci, cci); eq(hva, cva)


def test_refusal_leaves_a_working_csr_matrix(ra):
    g = load_golden("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert A.ConvertTo(ra.BCSR, 3) == ra.CSR and A.GetFormat() == ra.CSR  # 512 % 3
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])
    for bad in (1, 0):
        with pytest.raises(ra.RamdError) as e:
            A.ConvertTo(ra.BCSR, bad)
        assert e.value.status == 2  # RAMD_ERR_ARG
        assert A.GetFormat() == ra.CSR
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])


# ------------------------------------------------------------------------------------------ shapes where the kernel can go wrong
def _csr_from_dense(D):
    nrow, ncol = D.shape
    rp = np.zeros(nrow + 1, np.int32)
    ci, va = [], []
    for r in range(nrow):
        nz = np.nonzero(D[r])[0]
        ci.extend(nz.tolist()); va.extend(D[r, nz].tolist())
        rp[r + 1] = len(ci)
    return rp, np.array(ci, np.int32), np.array(va, np.float64)


def _shape(name):
    """-> (rp, ci, va, nrow, ncol, d)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    rv = lambda *s: rng.integers(1, 64, size=s).astype(np.float64) / 8.0 * rng.choice([-1.0, 1.0], size=s)  # noqa: E731
    if name == "one_block_per_block_row":  # a block diagonal of 3 x 3 blocks with holes inside the blocks
        n, d = 30, 3
        D = np.zeros((n, n))
        for b in range(n // d):
            D[b * d:(b + 1) * d, b * d:(b + 1) * d] = rv(d, d) * (rng.random((d, d)) < 0.7)
            D[b * d, b * d] = 1.5
    elif name == "empty_block_rows":  # block rows 1, 2, 5 and the last hold nothing
        n, d = 40, 4
        D = rv(n, n) * (rng.random((n, n)) < 0.15)
        for b in (1, 2, 5, 9):
            D[b * d:(b + 1) * d] = 0.0
    elif name == "blockdim_is_nrow":  # one block row, one block: the run-time kernel
        n, d = 24, 24
        D = rv(n, n) * (rng.random((n, n)) < 0.5)
    elif name == "rectangular_12x30":
        D = rv(12, 30) * (rng.random((12, 30)) < 0.3)
        d = 3
    elif name == "rectangular_12x30_d6":  # the run-time kernel on a rectangle
        D = rv(12, 30) * (rng.random((12, 30)) < 0.3)
        d = 6
    elif name == "full_first_block_row_140":  # 70 blocks in block row 0, the rest tridiagonal
        n, d = 140, 2
        D = np.zeros((n, n))
        D[0:2] = rv(2, n)
        for r in range(2, n):
            for c in (r - 1, r, r + 1):
                if c < n:
                    D[r, c] = rv(1)[0]
    elif name == "long_block_rows_d5":  # block rows of 40 blocks: a wave's 12 block rows take 15 steps of 32 blocks
        n, d = 200, 5
        D = rv(n, n) * (rng.random((n, n)) < 0.6)
    elif name == "compile_time_5":
        n, d = 65, 5
        D = rv(n, n) * (rng.random((n, n)) < 0.1)
    elif name == "compile_time_4_several_workgroups":  # 300 block rows: 19 waves, 5 workgroups, the last wave partly filled
        n, d = 1200, 4
        D = np.zeros((n, n))
        for r in range(n):
            for c in rng.choice(n, size=3, replace=False):
                D[r, c] = rv(1)[0]
    elif name == "run_time_7":
        n, d = 70 * 7, 7  # 490 rows: two workgroups of the run-time kernel
        D = np.zeros((n, n))
        for r in range(n):
            for c in rng.choice(n, size=4, replace=False):
                D[r, c] = rv(1)[0]
    else:
        raise KeyError(name)
    rp, ci, va = _csr_from_dense(D)
    return rp, ci, va, D.shape[0], D.shape[1], d


SHAPES = ["one_block_per_block_row", "empty_block_rows", "blockdim_is_nrow", "rectangular_12x30", "rectangular_12x30_d6",
          "full_first_block_row_140", "long_block_rows_d5", "compile_time_5", "compile_time_4_several_workgroups", "run_time_7"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", SHAPES)
def test_products_equal_the_restatement(ra, name, dtype):
    rp, ci, va, nrow, ncol, d = _shape(name)
    va = va.astype(dtype)
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, nrow, ncol, d)
    rng = np.random.default_rng(5)
    x = rng.uniform(-4.0, 6.0, size=ncol).astype(dtype)
    y0 = rng.uniform(-2.0, 2.0, size=nrow).astype(dtype)
    A = _mat(ra, rp, ci, va, nrow=nrow, ncol=ncol, dtype=dtype)
    assert A.ConvertToBCSR(d) == ra.BCSR
    gd, grp, gci, gval = A.bcsr_arrays()
    eq(grp, brp); eq(gci, bci); eq(gval, bval)
    eq(_apply(ra, A, x, dtype), ref.apply(brp, bci, bval, d, x))
    eq(_apply_add(ra, A, x, -0.75, y0, dtype), ref.apply_add(brp, bci, bval, d, x, -0.75, y0))


# ---------------------------------------------------------------------------------------------------------------------- shell
@pytest.mark.parametrize("nx", [2, 8])  # 2: the smallest surrogate with a mesh edge (20 rows); 8: 320 rows, two workgroups
def test_shell_blocks_are_dense_and_the_product_is_the_csr_product(ra, nx):
    from rocalution_amd import generators as gen
    rp, ci, va = gen.shell_surrogate(nx, nx)
    n = len(rp) - 1
    x = np.random.default_rng(11).uniform(-4.0, 6.0, size=n)
    A = _mat(ra, rp, ci, va)
    y_csr = _apply(ra, A, x, np.float64)
    assert A.ConvertToBCSR(5) == ra.BCSR
    assert A.GetNnz() == len(ci)  # dense 5 x 5 blocks: no fill
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, n, n, 5)
    y = _apply(ra, A, x, np.float64)
    eq(y, y_csr)
    eq(y, ref.apply(brp, bci, bval, 5, x))


# --------------------------------------------------------------------------------------------------------------------- solvers
def _check_hist(hist, ref_hist, rtol=1e-6):
    """the bar of tests/test_gpu_solvers.py for CG: relative 1e-6 per recorded iteration up to the last two, with its
    absolute floor at round-off level"""
    m = min(len(hist), len(ref_hist)) - 2
    assert m > 0
    h, r = np.asarray(hist[:m]), np.asarray(ref_hist[:m])
    assert np.all(np.abs(h - r) <= rtol * np.abs(r) + 1e-12 * h[0]), np.max(np.abs(h / r - 1))


def test_cg_jacobi_on_a_converted_operator(ra, S):
    g = load_golden("poisson8")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    runs = []
    for fmt in ("csr", "bcsr"):
        A = _mat(ra, rp, ci, va)
        rhs = ra.LocalVector(data=g["rhs_ones"])
        ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Build()
        if fmt == "bcsr":
            assert A.ConvertTo(ra.BCSR, 4) == ra.BCSR
        x = ra.LocalVector(); x.Allocate("", n)
        ls.Solve(rhs, x)
        runs.append((ls.GetIterationCount(), ls.GetSolverStatus(), np.array(ls.GetResidualHistory()), x.numpy()))
        ls.Clear()
    (it_c, st_c, h_c, x_c), (it_b, st_b, h_b, x_b) = runs
    assert it_b == it_c and st_b == st_c
    _check_hist(h_b, h_c)
    _check_hist(h_b, g["cg_jacobi_hist"])
    assert np.linalg.norm(x_b - 1.0) / np.sqrt(n) < 1e-3


def test_bicgstab_mcsgs_on_a_converted_operator(ra, S):
    g = load_golden("poisson8")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = ra.LocalVector(data=g["rhs_ones"])
    ls = S.BiCGStab(); ls.SetOperator(A); ls.SetPreconditioner(S.MultiColoredSGS()); ls.Build()
    assert A.ConvertTo(ra.BCSR, 4) == ra.BCSR
    x = ra.LocalVector(); x.Allocate("", n)
    ls.Solve(rhs, x)
    assert ls.GetSolverStatus() in (1, 2)
    assert abs(ls.GetIterationCount() - int(g["bicgstab_mcsgs_meta"][0])) <= 2
    assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-3
    ls.Clear()


# ------------------------------------------------------------------------------------------------------------ CSR-only operations
def test_csr_only_operations_stop_with_a_status(ra, tmp_path):
    """what needs CSR answers a BCSR matrix as it answers an ELL matrix: a status (or, the file writers, a converted copy),
    never a fault; the library goes on working"""
    g = load_golden("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert A.ConvertToBCSR(4) == ra.BCSR
    E = _mat(ra, g["rowptr"], g["col"], g["val"])
    assert E.ConvertToELL() == ra.ELL

    def outcome(M, f):
        try:
            f(M)
        except ra.RamdError as e:
            return e.status
        return 0

    with pytest.raises(ra.RamdError):
        A.ILU0Factorize()
    perm = ra.LocalVector(np.int32, data=np.arange(A.GetM(), dtype=np.int32))
    out = ra.LocalMatrix()
    path = str(tmp_path / "m.csr")
    ops = [lambda M: M.ILU0Factorize(), lambda M: M.ILUpFactorize(1), lambda M: M.Permute(perm), lambda M: out.MatrixMult(M, M),
           lambda M: M.Sort(), lambda M: M.AMGPMISAggregate(0.01), lambda M: M.RSPMISCoarsening(0.25),
           lambda M: M.WriteFileCSR(path), lambda M: M.WriteFileMTX(path)]
    got = [outcome(A, f) for f in ops]
    assert got == [outcome(E, f) for f in ops], got  # what an ELL matrix gets there
    assert all(s != 0 for s in got[:7]), got
    assert A.GetFormat() == ra.BCSR
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])  # poisson8 has sorted rows: the BCSR product is the CSR product
    B = _mat(ra, g["rowptr"], g["col"], g["val"])
    eq(_apply(ra, B, g["x"], np.float64), g["spmv_csr"])


# ------------------------------------------------------------------------------------------------------------------ clone, cast
def test_clone_keeps_format_and_arrays_and_cast_round_trips(ra):
    g = load_golden("rand300")
    rp, ci = g["rowptr"], g["col"]
    va = np.round(g["val"] * 64.0) / 64.0  # exactly representable in fp32
    assert np.array_equal(va.astype(np.float32).astype(np.float64), va)
    A = _mat(ra, rp, ci, va)
    assert A.ConvertToBCSR(5) == ra.BCSR
    arrays = A.bcsr_arrays()
    C = ra.LocalMatrix(); C.CloneFrom(A)
    assert C.GetFormat() == ra.BCSR and (C.GetM(), C.GetN(), C.GetNnz()) == (A.GetM(), A.GetN(), A.GetNnz())
    for a, b in zip(arrays[1:], C.bcsr_arrays()[1:]):
        eq(a, b)
    assert C.bcsr_arrays()[0] == 5
    del A  # the clone owns its arrays
    x = g["x"]
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, 300, 300, 5)
    eq(_apply(ra, C, x, np.float64), ref.apply(brp, bci, bval, 5, x))
    F = ra.LocalMatrix(np.float32); F.CastFrom(C)
    assert F.GetFormat() == ra.BCSR and F.dtype == np.float32
    fd, frp, fci, fval = F.bcsr_arrays()
    assert fd == 5 and fval.dtype == np.float32
    eq(frp, brp); eq(fci, bci); eq(fval, bval.astype(np.float32))
    x32 = x.astype(np.float32)
    eq(_apply(ra, F, x32, np.float32), ref.apply(brp, bci, bval.astype(np.float32), 5, x32))
    B = ra.LocalMatrix(); B.CastFrom(F)
    assert B.GetFormat() == ra.BCSR and B.dtype == np.float64
    for a, b in zip(arrays[1:], B.bcsr_arrays()[1:]):
        eq(a, b)


# -------------------------------------------------------------------------------------------------- the fused product + dot
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["full_first_block_row_140", "one_block_per_block_row", "compile_time_4_several_workgroups",
                                  "compile_time_5", "long_block_rows_d5", "run_time_7"])
def test_fused_product_and_dot(ra, name, dtype):
    """ramd_fused_apply_dot / _dotv on a BCSR operator (what CG and BiCGStab call): y is the product bit for bit; the slot
    holds <x, y> / <w, y>.  The kernel multiplies in double (exact for fp32 operands, one rounding for fp64) and adds in
    double in a fixed tree, so the error against the exactly rounded sum (math.fsum) is at most n 2^-52 sum |w_i y_i|"""
    import ctypes as C
    import math
    from rocalution_amd import capi
    lib = capi.load()
    rp, ci, va, nrow, ncol, d = _shape(name)
    assert nrow == ncol
    va = va.astype(dtype)
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, nrow, ncol, d)
    rng = np.random.default_rng(9)
    x = rng.uniform(-4.0, 6.0, size=ncol).astype(dtype)
    w = rng.uniform(-1.0, 1.0, size=nrow).astype(dtype)
    y_ref = ref.apply(brp, bci, bval, d, x)
    A = _mat(ra, rp, ci, va, dtype=dtype)
    assert A.ConvertToBCSR(d) == ra.BCSR
    xv, wv = ra.LocalVector(dtype, data=x), ra.LocalVector(dtype, data=w)
    yv = ra.LocalVector(dtype); yv.Allocate("", nrow)
    out = C.c_double(0.0)
    for against, call in ((x, lambda: lib.ramd_fused_apply_dot(A._h, xv._h, yv._h, 7)),
                          (w, lambda: lib.ramd_fused_apply_dotv(A._h, xv._h, yv._h, wv._h, 7))):
        capi.check(lib.ramd_scalars_set(7, -1.0))
        yv.Zeros()
        capi.check(call())
        capi.check(lib.ramd_scalars_fetch(C.byref(out), 7, 1))
        eq(yv.numpy(), y_ref)
        terms = [float(a) * float(b) for a, b in zip(against, y_ref)]
        exact = math.fsum(terms)
        bound = nrow * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
        print("%s %s: slot %.17g exact %.17g diff %.3g bound %.3g" % (name, np.dtype(dtype).name, out.value, exact,
                                                                    abs(out.value - exact), bound))
        assert abs(out.value - exact) <= bound
