"""The shared row filter (csrc/csr_filter.hpp) through its API users ExtractL/U, ExtractSubMatrix and Compress, in the corners
the other files leave out: fp32 windows, rows that lose everything, empty rows and matrices, unsorted rows, and more rows than
one grid covers.  Every expectation is the reference's host loop (host_matrix_csr.cpp:848-1160, :3679-3740) as a numpy mask
over the input arrays in storage order; offsets and columns must be equal, values equal by bits."""
import numpy as np
import pytest

from rocalution_amd import generators as gen

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


def _mat(ra, csr, dtype, nrow=None, ncol=None):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(csr[0], csr[1], csr[2].astype(dtype), nrow=nrow, ncol=ncol)
    return A


def _rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _expect(csr, keep, r0=0, rs=None, c0=0):
    """rows [r0, r0 + rs) of the entries under the mask `keep`, in storage order, columns moved by -c0"""
    rp, ci, va = csr
    rs = len(rp) - 1 - r0 if rs is None else rs
    rows = _rows(rp)
    keep = keep & (rows >= r0) & (rows < r0 + rs)
    orp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep] - r0, minlength=rs))]).astype(np.int32)
    return orp, (ci[keep] - c0).astype(np.int32), va[keep]


def _same(M, exp, shape):
    rp, ci, va = M.CopyToCSR()
    assert (M.GetM(), M.GetN(), M.GetNnz()) == (shape[0], shape[1], len(exp[1]))
    assert rp.dtype == np.int32 and np.array_equal(rp, exp[0])
    assert np.array_equal(ci, exp[1])
    bits = np.uint64 if va.dtype == np.float64 else np.uint32
    assert va.dtype == exp[2].dtype and np.array_equal(va.view(bits), exp[2].view(bits))
    return rp, ci, va


TRI = {  # name -> (upper, diag, mask of (col, row))
    "L": (0, 0, lambda c, r: c < r), "L+diag": (0, 1, lambda c, r: c <= r),
    "U": (1, 0, lambda c, r: c > r), "U+diag": (1, 1, lambda c, r: c >= r),
}


def _tri(ra, A, csr, kind, dtype):
    upper, diag, mask = TRI[kind]
    T = ra.LocalMatrix(dtype)
    (A.ExtractU if upper else A.ExtractL)(T, diag)
    return _same(T, _expect(csr, mask(csr[1], _rows(csr[0]))), (A.GetM(), A.GetN()))


def _sub(ra, A, csr, r0, c0, rs, cs, dtype):
    S = ra.LocalMatrix(dtype)
    A.ExtractSubMatrix(r0, c0, rs, cs, S)
    ci = csr[1]
    return _same(S, _expect(csr, (ci >= c0) & (ci < c0 + cs), r0, rs, c0), (rs, cs))


def _compress(ra, csr, drop, dtype):
    """(the comparison is made in double on the stored value, host_matrix_csr.cpp:3696)"""
    A = _mat(ra, csr, dtype)
    A.Compress(drop)
    keep = (np.abs(csr[2].astype(np.float64)) > drop) | (csr[1] == _rows(csr[0]))
    n = len(csr[0]) - 1
    return _same(A, _expect(csr, keep), (n, n))


@pytest.fixture(scope="module")
def rand500():
    return gen.random_sparse(500, 7, seed=29)


@pytest.mark.parametrize("window", [(100, 50, 233, 301), (10, 20, 0, 30), (10, 20, 40, 0), (17, 0, 1, 500), (0, 0, 500, 500)],
                         ids=["interior", "no_rows", "no_columns", "one_row", "whole"])
def test_extract_submatrix_fp32_windows(ra, rand500, window):
    csr = (rand500[0], rand500[1], rand500[2].astype(np.float32))
    _sub(ra, _mat(ra, csr, np.float32), csr, *window, np.float32)


def _forty():
    """40 rows: r % 4 == 0 empty; 1: columns in front of the diagonal only, small values; 2: the diagonal and columns behind it,
    large values; 3: one small entry in front, a small diagonal, one large entry behind"""
    rng = np.random.default_rng(5)
    rp, ci, va = [0], [], []
    for r in range(40):
        if r % 4 == 1:
            cols = list(range(max(0, r - 3), r))
            vals = [0.01 * s for s in rng.choice([-1.0, 1.0], len(cols))]
        elif r % 4 == 2:
            cols = list(range(r, min(40, r + 3)))
            vals = [2.0 * s for s in rng.choice([-1.0, 1.0], len(cols))]
        elif r % 4 == 3:
            cols, vals = [r - 2, r, (r + 1) % 40], [0.01, -0.01, 3.0]  # (row 39: the large entry in column 0, unsorted)
        else:
            cols, vals = [], []
        ci += cols
        va += vals
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_that_lose_everything_and_empty_rows(ra, dtype):
    rp, ci, va = _forty()
    csr = (rp, ci, va.astype(dtype))
    A = _mat(ra, csr, dtype)
    per_row = lambda orp: np.diff(orp)
    src = np.diff(rp)
    # every case sees empty source rows, rows that keep nothing and rows that keep all of their entries
    for got in (per_row(_tri(ra, A, csr, "L", dtype)[0]), per_row(_tri(ra, A, csr, "U+diag", dtype)[0]),
                per_row(_compress(ra, csr, 0.1, dtype)[0])):
        assert np.any(src == 0) and np.any((src > 0) & (got == 0)) and np.any((src > 0) & (got == src))
    got = per_row(_sub(ra, A, csr, 5, 10, 30, 20, dtype)[0])
    assert np.any(src[5:35] == 0) and np.any((src[5:35] > 0) & (got == 0)) and np.any((src[5:35] > 0) & (got == src[5:35]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_diagonal_matrix_has_no_strict_lower_part(ra, dtype):
    n = 40
    csr = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(1, 2, n).astype(dtype))
    rp, ci, va = _tri(ra, _mat(ra, csr, dtype), csr, "L", dtype)
    assert len(rp) == n + 1 and not rp.any() and len(ci) == 0 and len(va) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_unsorted_rows_keep_their_storage_order(ra, dtype):
    """what the direct sum of the AS blocks and the BlockPreconditioner's references rely on"""
    rp, ci, va = gen.random_sparse(300, 7, seed=31)
    rng = np.random.default_rng(31)
    ci, va = ci.copy(), va.astype(dtype)
    for r in range(len(rp) - 1):
        p = rng.permutation(rp[r + 1] - rp[r]) + rp[r]
        ci[rp[r]:rp[r + 1]], va[rp[r]:rp[r + 1]] = ci[p], va[p]
    csr = (rp, ci, va)
    A = _mat(ra, csr, dtype)
    for orp, oci, _ in [_tri(ra, A, csr, k, dtype) for k in TRI] + [_sub(ra, A, csr, 40, 25, 200, 230, dtype)]:
        inside = np.diff(_rows(orp)) == 0  # neighbours that belong to one row
        assert np.any(np.diff(oci)[inside] < 0)  # (the results do hold rows that are not ascending)


@pytest.fixture(scope="module")
def poisson104():
    return gen.poisson7(104)


# The kernels' grid is capped at num_cu * 16 workgroups of 256 lanes, one lane a row (ew_grid, csrc/common.hpp): 1 048 576 rows
# on the 256 compute units of this device.  Only a matrix with more rows makes the grid-stride loop of a lane turn a second
# time; 104^3 = 1 124 864.  On a device with more compute units, or under RAMD_EW_GRID_MULT, the cap is higher and these cases
# pass without the second turn; the assertion below only states the figure for this device.  (Compress(0.5) keeps every entry of this operator, whose off-diagonal entries are -1; 1.0 is the
# threshold that leaves the diagonal alone.)
@pytest.mark.parametrize("case", ["L+diag", "U", "sub", "compress_0.5", "compress_1.0"])
def test_more_rows_than_one_grid_covers(ra, poisson104, case):
    csr = poisson104
    n = len(csr[0]) - 1
    assert n > 256 * 16 * 256
    if case.startswith("compress"):
        orp = _compress(ra, csr, float(case.split("_")[1]), np.float64)[0]
        assert orp[-1] == (n if case == "compress_1.0" else csr[0][-1])
        return
    A = _mat(ra, csr, np.float64)
    if case == "sub":
        _sub(ra, A, csr, n // 3, n // 3, n - n // 3, n - n // 3, np.float64)
    else:
        _tri(ra, A, csr, case, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_source_without_entries(ra, dtype):
    n = 5
    csr = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    A = _mat(ra, csr, dtype, nrow=n, ncol=n)
    for kind in ("L", "U+diag"):
        assert not _tri(ra, A, csr, kind, dtype)[0].any()
    assert not _sub(ra, A, csr, 1, 0, 3, 4, dtype)[0].any()
    A.Compress(0.5)
    _same(A, csr, (n, n))
