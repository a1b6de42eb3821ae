"""The CPU oracle's CSR algebra (csr_transpose, csr_matmult, csr_matrix_add) at the rectangular, long-row and empty-row
operands of tests/_csr_algebra_cases.py, against scipy on float64 copies of the same operands.  test_gpu_csr_algebra.py holds
the device to these oracle results bit for bit, so this file guards the guard (test_oracle_golden.py pins the oracle on the
square golden matrices only).

Patterns must be equal.  Transposed values must be equal.  Products and sums are compared per entry with the standard forward
bound of a sum of k products,  |c_oracle - c_scipy| <= k . u . sum |a| |b|,  k = number of products of the entry, u = unit
round-off of the oracle's value type (2^-24, 2^-53), the sum taken from |A| . |B|.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import _csr_algebra_cases as cs
from _csr_algebra_cases import arrays


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(a, b)


def _sp64(M, data=None):
    va = M.va.astype(np.float64) if data is None else data
    return sp.csr_matrix((va, M.ci.copy(), M.rp.copy()), shape=M.shape)


def _ones(M):
    return _sp64(M, np.ones(len(M.ci)))


def _sorted(S):
    S = S.tocsr()
    S.sort_indices()
    return S


def _on_pattern(C, K):
    """the values of C at the entries of K (scipy drops the entries of a product or sum that come out as exact zeros)"""
    if K.nnz == 0:
        return np.zeros(0)
    rows = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
    return np.asarray(C.tocsr()[rows, K.indices]).ravel()


def _unit_roundoff(dtype):
    return np.finfo(dtype).eps / 2


def _check_product(got, A, B):
    """got = oracle (rp, ci, va) of A.B"""
    rp, ci, va = got
    K = _sorted(_ones(A) @ _ones(B))                      # structural product: products per entry, nothing cancels
    eq(rp, K.indptr); eq(ci, K.indices)
    assert va.dtype == A.va.dtype
    C = _on_pattern(_sp64(A) @ _sp64(B), K)
    S = _sorted(_sp64(A, np.abs(A.va.astype(np.float64))) @ _sp64(B, np.abs(B.va.astype(np.float64))))
    eq(S.indices, K.indices)
    bound = K.data * _unit_roundoff(va.dtype) * S.data
    err = np.abs(va.astype(np.float64) - C)
    assert np.all(err <= bound), "worst err/bound %g" % np.max(err / np.maximum(bound, 1e-300))
    return K, C


@pytest.mark.parametrize("dtype", cs.DTYPES)
@pytest.mark.parametrize("name", cs.MM_CASES)
def test_oracle_matmult_vs_scipy(oracle, name, dtype):
    A, B = cs.mm_case(name, dtype)
    cs.check_mm_case(name, A, B)
    got = oracle.csr_matmult(arrays(A), arrays(B), ncol_b=B.shape[1])
    K, C = _check_product(got, A, B)
    if name in cs.EMPTY_CASES:
        assert len(got[1]) == 0 and not got[0].any() and len(got[0]) == A.shape[0] + 1
    if name.startswith("cancel"):
        zeros = int((got[2] == 0).sum())
        assert zeros > 0 and zeros == int((C == 0).sum())   # sums that cancel exactly stay in the pattern


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_oracle_galerkin_vs_scipy(oracle, dtype):
    A, P = cs.galerkin_case(dtype)
    cs.check_galerkin_case(A, P)
    R = cs.Csr((P.shape[1], P.shape[0]), *oracle.csr_transpose(*arrays(P), ncol=P.shape[1]))
    Rs = _sorted(_sp64(P).T)
    eq(R.rp, Rs.indptr); eq(R.ci, Rs.indices); eq(R.va.astype(np.float64), Rs.data)
    AP = cs.Csr((A.shape[0], P.shape[1]), *oracle.csr_matmult(arrays(A), arrays(P), ncol_b=P.shape[1]))
    _check_product(arrays(AP), A, P)
    RAP = oracle.csr_matmult(arrays(R), arrays(AP), ncol_b=AP.shape[1])
    _check_product(RAP, R, AP)
    assert len(RAP[0]) == P.shape[1] + 1


@pytest.mark.parametrize("dtype", cs.DTYPES)
@pytest.mark.parametrize("variant", cs.TRANSPOSE_VARIANTS)
@pytest.mark.parametrize("shape", cs.TRANSPOSE_SHAPES)
def test_oracle_transpose_vs_scipy(oracle, shape, variant, dtype):
    M = cs.transpose_case(shape, variant, dtype)
    cs.check_transpose_case(M, variant)
    trp, tci, tva = oracle.csr_transpose(*arrays(M), ncol=M.shape[1])
    T = _sorted(_sp64(M).T)
    eq(trp, T.indptr); eq(tci, T.indices)
    assert tva.dtype == M.va.dtype
    eq(tva.astype(np.float64), T.data)
    back = oracle.csr_transpose(trp, tci, tva, ncol=M.shape[0])
    for g, e in zip(back, arrays(M)):
        eq(g, e)


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_oracle_transpose_keeps_repeated_columns_in_storage_order(oracle, dtype):
    M = cs.repeated_column_matrix(dtype)
    trp, tci, tva = oracle.csr_transpose(*arrays(M), ncol=M.shape[1])
    # stable counting sort by column, written out: entries of a transposed row in the order they are stored
    order = np.argsort(M.ci, kind="stable")
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.rp))
    eq(tci, rows[order]); eq(tva, M.va[order])
    eq(trp, np.concatenate([[0], np.cumsum(np.bincount(M.ci, minlength=M.shape[1]))]))
    assert list(tci[trp[3]:trp[4]]) == [1, 1, 3, 3, 4]


def _check_union(oracle, A, B, dtype):
    alpha, beta = cs.ADD_ALPHA, cs.ADD_BETA
    rp, ci, va = oracle.csr_matrix_add(arrays(A), arrays(B), alpha, beta, True)
    K = _sorted(_ones(A) + _ones(B))
    eq(rp, K.indptr); eq(ci, K.indices)
    # the scalars are operands too: the oracle holds them in its value type
    a64, b64 = float(dtype(alpha)), float(dtype(beta))
    C = _on_pattern(a64 * _sp64(A) + b64 * _sp64(B), K)
    Sa, Sb = _sp64(A, np.abs(A.va.astype(np.float64))), _sp64(B, np.abs(B.va.astype(np.float64)))
    S = _sorted(abs(a64) * Sa + abs(b64) * Sb)
    eq(S.indices, K.indices)
    bound = K.data * _unit_roundoff(dtype) * S.data
    err = np.abs(va.astype(np.float64) - C)
    assert va.dtype == np.dtype(dtype) and np.all(err <= bound)


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_oracle_matrix_add_union_vs_scipy(oracle, dtype):
    A, B = cs.add_union_case(dtype)
    cs.check_add_union_case(A, B)
    _check_union(oracle, A, B, dtype)
    E = cs.empty_csr(cs.ADD_SHAPE, dtype)
    _check_union(oracle, A, E, dtype)
    _check_union(oracle, E, B, dtype)


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_oracle_matrix_add_subset_vs_numpy_loop(oracle, dtype):
    """the reference's behaviour: entries of A without a partner in B keep their value, NOT scaled by alpha"""
    A, B = cs.add_subset_case(dtype)
    mask = cs.subset_partner_mask(A, B)
    alpha, beta = dtype(cs.ADD_ALPHA), dtype(cs.ADD_BETA)
    exp = A.va.copy()
    for i in range(A.shape[0]):
        bcol = {int(c): j for j, c in enumerate(B.ci[B.rp[i]:B.rp[i + 1]], start=B.rp[i])}
        for j in range(A.rp[i], A.rp[i + 1]):
            if int(A.ci[j]) in bcol:
                exp[j] = dtype(alpha * A.va[j]) + dtype(beta * B.va[bcol[int(A.ci[j])]])
    rp, ci, va = oracle.csr_matrix_add(arrays(A), arrays(B), cs.ADD_ALPHA, cs.ADD_BETA, False)
    eq(rp, A.rp); eq(ci, A.ci); eq(va, exp)
    eq(va[~mask], A.va[~mask])
    assert np.all(va[mask] != A.va[mask])
    rp, ci, va = oracle.csr_matrix_add(arrays(A), arrays(cs.empty_csr(cs.ADD_SHAPE, dtype)), cs.ADD_ALPHA, cs.ADD_BETA, False)
    eq(va, A.va)
