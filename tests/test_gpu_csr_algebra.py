"""GPU parity tests of the CSR matrix algebra (matrix_algebra.hip; transpose_into in trisolve.hip; the scans and the radix
sort of scan.hip) on rectangular operands, rows without entries and rows with many products, in fp64 and fp32: Transpose,
MatrixMult, MatrixAdd, Sort, DiagonalMatrixMultL/R through ra.LocalMatrix against the CPU oracle on the operands of
tests/_csr_algebra_cases.py (test_cpu_csr_algebra.py holds the oracle to scipy on the same operands).

Bar (as in test_gpu_kernels.py): row offsets, columns and values BIT-EXACT, in both value types; no tolerance
anywhere in this file.  Every test first checks on the host that its operands have the property that puts them on the code
path they are meant for (cs.check_*), so that an edit of the generators cannot quietly move a case elsewhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _csr_algebra_cases as cs
from _csr_algebra_cases import arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(a, b), "%d of %d entries differ" % (int((a != b).sum()), a.size)


def dev(ra, M):
    D = ra.LocalMatrix(M.va.dtype)
    D.SetDataPtrCSR(M.rp, M.ci, M.va, nrow=M.shape[0], ncol=M.shape[1])
    return D


def check(D, shape, expected):
    """shape, entry count and the three arrays of a device matrix"""
    erp, eci, eva = expected
    assert (D.GetM(), D.GetN()) == tuple(shape)
    assert D.GetNnz() == len(eci)
    rp, ci, va = D.CopyToCSR()
    eq(rp, np.asarray(erp, dtype=np.int32)); eq(ci, np.asarray(eci, dtype=np.int32)); eq(va, eva)


# ------------------------------------------------------------------------------------------------ MatrixMult
@pytest.mark.parametrize("dtype", cs.DTYPES)
@pytest.mark.parametrize("name", cs.MM_CASES)
def test_matmult(ra, oracle, name, dtype):
    """C = A.B.  short: per-thread insertion (at most 64 products in every row, 64 included); medium: every row through
    k_mm_row_lds, sort sizes 128 ... 2048 and 2048 exactly full; long: rows of 2049 and 2080 products send their chunk
    through the two global sorts; over_chunk: (under RAMD_MM_CHUNK=2500) a row larger than the chunk; row_vector: one row,
    the row sort sees only the key 0; column: B has one column (every product on column 0; with RAMD_MM_LDS=0 the column
    sort has max_key 0); narrow16/17: one and two 4-bit passes of the column sort; cancel*: sums that come out as exact
    zeros stay in the pattern, as in the reference; empty_*: HostMatrixCSR::MatMatMult (host_matrix_csr.cpp:2805-2938) has no
    special case for nnz == 0 -- it computes the n x m result with an all-zero row offset array, and so must the device."""
    A, B = cs.mm_case(name, dtype)
    cs.check_mm_case(name, A, B)
    exp = oracle.csr_matmult(arrays(A), arrays(B), ncol_b=B.shape[1])
    dA, dB = dev(ra, A), dev(ra, B)
    C = ra.LocalMatrix(dtype)
    C.MatrixMult(dA, dB)
    check(C, (A.shape[0], B.shape[1]), exp)
    if name in cs.EMPTY_CASES:
        rp, ci, va = C.CopyToCSR()
        assert C.GetNnz() == 0 and len(rp) == A.shape[0] + 1 and not rp.any()
    if name.startswith("cancel"):
        assert int((C.CopyToCSR()[2] == 0).sum()) == int((exp[2] == 0).sum()) > 0
    # the operands are untouched, and a result matrix that held something else before is replaced as a whole
    check(dA, A.shape, arrays(A)); check(dB, B.shape, arrays(B))
    C.MatrixMult(dA, dB)
    check(C, (A.shape[0], B.shape[1]), exp)


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_matmult_galerkin(ra, oracle, dtype):
    """R = P^T, AP = A.P, RAP = R.AP with a 700 x 90 prolongation with empty rows and uneven aggregates: the shape of every
    AMG Build(); every step against the oracle"""
    A, P = cs.galerkin_case(dtype)
    cs.check_galerkin_case(A, P)
    n, nc = P.shape
    eR = oracle.csr_transpose(*arrays(P), ncol=nc)
    eAP = oracle.csr_matmult(arrays(A), arrays(P), ncol_b=nc)
    eRAP = oracle.csr_matmult(eR, eAP, ncol_b=nc)
    dA, dP = dev(ra, A), dev(ra, P)
    R = ra.LocalMatrix(dtype); dP.Transpose(R)
    check(R, (nc, n), eR)
    AP = ra.LocalMatrix(dtype); AP.MatrixMult(dA, dP)
    check(AP, (n, nc), eAP)
    RAP = ra.LocalMatrix(dtype); RAP.MatrixMult(R, AP)
    check(RAP, (nc, nc), eRAP)
    T = ra.LocalMatrix(dtype); T.TripleMatrixProduct(R, dA, dP)  # (R.A).P: the other association, its own oracle chain
    eRA = oracle.csr_matmult(eR, arrays(A), ncol_b=n)
    check(T, (nc, nc), oracle.csr_matmult(eRA, arrays(P), ncol_b=nc))


FRESH_RUNS = {"chunk2500": {"RAMD_MM_CHUNK": str(cs.SMALL_CHUNK)},
              # a second run, without the LDS kernel: every row above 64 products goes through the two global sorts, so
              # `column` (column key 0 only), `cancel_lds` and the medium rows reach them as well
              "lds0": {"RAMD_MM_LDS": "0"}}


@pytest.mark.parametrize("run", list(FRESH_RUNS))
def test_mm_switches_in_a_fresh_process(run):
    """the MatrixMult tests of this file again with RAMD_MM_CHUNK=2500 (read once per process; RAMD_MM_LDS at its default):
    `long` then splits into chunks served by the LDS kernel alone, a chunk with a 2049-product row that falls back to the
    global sort together with its neighbour, and a chunk that is the 2080-product row alone; `over_chunk` has a row larger
    than the chunk (the "at least one row" branch of the chunk search; no row of `long` can be, 2080 < 2500); the pieces of
    both paths are concatenated into one result.  The split itself is asserted on the host in cs.check_mm_case('long')."""
    A, B = cs.mm_case("long", np.float64)
    pc = cs.check_mm_case("long", A, B)
    assert len(cs.chunk_rows(pc, cs.SMALL_CHUNK)) >= 3
    pc = cs.check_mm_case("over_chunk", *cs.mm_case("over_chunk", np.float64))
    assert any(b - a == 1 and pc[a] > cs.SMALL_CHUNK for a, b in cs.chunk_rows(pc, cs.SMALL_CHUNK))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **FRESH_RUNS[run])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_matmult"],
                       env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    expected = len(cs.MM_CASES) * len(cs.DTYPES) + len(cs.DTYPES)  # test_matmult and test_matmult_galerkin
    assert r.returncode == 0 and ("%d passed" % expected) in out, out[-3000:]


def test_argument_checks(ra):
    """MatrixMult with A.ncol != B.nrow, with mixed value types and with C is A, MatrixAdd with unequal shapes: RamdError
    (the reference asserts), and the operands are unchanged afterwards"""
    A = cs.random_csr((30, 40), [3] * 30, 1, np.float64)
    B = cs.random_csr((41, 20), [2] * 41, 3, np.float64)
    B32 = cs.random_csr((40, 20), [2] * 40, 5, np.float32)
    A2 = cs.random_csr((30, 41), [3] * 30, 7, np.float64)
    S = cs.random_csr((40, 40), [3] * 40, 9, np.float64)
    dA, dB, dB32, dA2, dS = (dev(ra, M) for M in (A, B, B32, A2, S))
    C = ra.LocalMatrix(np.float64)
    with pytest.raises(ra.RamdError):
        C.MatrixMult(dA, dB)        # 30 x 40 times 41 x 20
    with pytest.raises(ra.RamdError):
        C.MatrixMult(dA, dB32)      # fp64 times fp32
    with pytest.raises(ra.RamdError):
        ra.LocalMatrix(np.float32).MatrixMult(dA, dS)  # an fp32 result of fp64 operands
    with pytest.raises(ra.RamdError):
        dS.MatrixMult(dS, dS)       # C is A (and B)
    with pytest.raises(ra.RamdError):
        dA.MatrixMult(dA, dS)       # C is A
    for structure in (False, True):
        with pytest.raises(ra.RamdError):
            dA.MatrixAdd(dA2, 1.5, -0.3, structure)  # 30 x 40 plus 30 x 41
        with pytest.raises(ra.RamdError):
            dA.MatrixAdd(dA, 1.5, -0.3, structure)
    assert C.GetNnz() == 0
    for D, M in ((dA, A), (dB, B), (dB32, B32), (dA2, A2), (dS, S)):
        check(D, M.shape, arrays(M))


# ------------------------------------------------------------------------------------------------ Transpose
@pytest.mark.parametrize("dtype", cs.DTYPES)
@pytest.mark.parametrize("variant", cs.TRANSPOSE_VARIANTS)
@pytest.mark.parametrize("shape", cs.TRANSPOSE_SHAPES)
def test_transpose(ra, oracle, shape, variant, dtype):
    """rectangular, with empty rows, a column in every non-empty row (a transposed row of about as many entries as the matrix
    has rows, sorted by a single thread) and -- holes: empty columns, the last among them, i.e. empty rows of the result;
    full: one full row.  Out of place, in place, and twice (= the input, bit for bit)"""
    M = cs.transpose_case(shape, variant, dtype)
    cs.check_transpose_case(M, variant)
    nrow, ncol = M.shape
    exp = oracle.csr_transpose(*arrays(M), ncol=ncol)
    assert len(exp[0]) == ncol + 1
    dM = dev(ra, M)
    T = ra.LocalMatrix(dtype); dM.Transpose(T)
    check(T, (ncol, nrow), exp)
    check(dM, M.shape, arrays(M))
    I = ra.LocalMatrix(dtype); I.CloneFrom(dM); I.Transpose()
    check(I, (ncol, nrow), exp)
    assert (I.GetM(), I.GetN()) == (dM.GetN(), dM.GetM())
    I.Transpose()
    check(I, M.shape, arrays(M))
    TT = ra.LocalMatrix(dtype); T.Transpose(TT)
    check(TT, M.shape, arrays(M))


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_transpose_keeps_repeated_columns_in_storage_order(ra, oracle, dtype):
    """two entries of one row on the same column, different values: the reference keeps both, in storage order"""
    M = cs.repeated_column_matrix(dtype)
    exp = oracle.csr_transpose(*arrays(M), ncol=M.shape[1])
    T = ra.LocalMatrix(dtype); dev(ra, M).Transpose(T)
    check(T, (M.shape[1], M.shape[0]), exp)


# ------------------------------------------------------------------------------------------------ MatrixAdd
@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_matrix_add_union(ra, oracle, dtype):
    """this = 1.5 this - 0.3 B on the union pattern, 300 x 450; rows where only A, only B or neither has entries, identical,
    disjoint and interleaved patterns, both reaching the last column; B or A without entries.  Precondition of the
    reference (and of the oracle): sorted rows, unique columns"""
    A, B = cs.add_union_case(dtype)
    cs.check_add_union_case(A, B)
    E = cs.empty_csr(cs.ADD_SHAPE, dtype)
    for X, Y in ((A, B), (A, E), (E, B)):
        exp = oracle.csr_matrix_add(arrays(X), arrays(Y), cs.ADD_ALPHA, cs.ADD_BETA, True)
        dX, dY = dev(ra, X), dev(ra, Y)
        dX.MatrixAdd(dY, cs.ADD_ALPHA, cs.ADD_BETA, True)
        check(dX, cs.ADD_SHAPE, exp)
        check(dY, cs.ADD_SHAPE, arrays(Y))


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_matrix_add_subset(ra, oracle, dtype):
    """structure=False, the pattern of B a strict subset of this one's (sorted rows, unique columns: the reference's
    precondition), B empty in some rows: the matched entries become 1.5 a - 0.3 b, the entries of A WITHOUT a partner keep
    their value -- the reference does not scale them by alpha, and neither does the oracle.  B without entries: no change"""
    A, B = cs.add_subset_case(dtype)
    mask = cs.subset_partner_mask(A, B)
    exp = oracle.csr_matrix_add(arrays(A), arrays(B), cs.ADD_ALPHA, cs.ADD_BETA, False)
    eq(exp[2][~mask], A.va[~mask])
    assert np.all(exp[2][mask] != A.va[mask])
    dA, dB = dev(ra, A), dev(ra, B)
    dA.MatrixAdd(dB, cs.ADD_ALPHA, cs.ADD_BETA, False)
    check(dA, cs.ADD_SHAPE, exp)
    check(dB, cs.ADD_SHAPE, arrays(B))
    dA = dev(ra, A)
    dA.MatrixAdd(dev(ra, cs.empty_csr(cs.ADD_SHAPE, dtype)), cs.ADD_ALPHA, cs.ADD_BETA, False)
    check(dA, cs.ADD_SHAPE, arrays(A))


# ------------------------------------------------------------------------------------------------ Sort, DiagonalMatrixMult
@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_sort(ra, dtype):
    """40 x 500, rows of 0, 1, 2, 64 and 300 entries scrambled on the host, one with a repeated column: stable by column,
    values follow their columns, ties in storage order (numpy's stable argsort per row)"""
    M, eci, eva = cs.sort_case(dtype)
    D = dev(ra, M)
    D.Sort()
    check(D, M.shape, (M.rp, eci, eva))


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_diagonal_matrix_mult(ra, dtype):
    """300 x 450: L takes a vector of 300 (val * d[row]), R one of 450 (val * d[col]); one multiplication per entry in the
    matrix' type, so bit-exact.  The vector of the other length is refused"""
    M, dl, dr = cs.diag_case(dtype)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.rp))
    vl, vr = ra.LocalVector(dtype, data=dl), ra.LocalVector(dtype, data=dr)
    L = dev(ra, M); L.DiagonalMatrixMultL(vl)
    check(L, M.shape, (M.rp, M.ci, M.va * dl[rows]))
    R = dev(ra, M); R.DiagonalMatrixMultR(vr)
    check(R, M.shape, (M.rp, M.ci, M.va * dr[M.ci]))
    with pytest.raises(ra.RamdError):
        L.DiagonalMatrixMultL(vr)
    with pytest.raises(ra.RamdError):
        R.DiagonalMatrixMultR(vl)
    check(L, M.shape, (M.rp, M.ci, M.va * dl[rows]))
    check(R, M.shape, (M.rp, M.ci, M.va * dr[M.ci]))
