"""ELL / HYB / COO without a GPU: the numpy layout rules of tests/_ellhyb_cases.py against the oracle (pinned bit-exact to the
reference's host backend) and against the committed goldens (output of the genuine reference), the oracle's products in the
three layouts against its CSR product, and -- so that no case of tests/test_gpu_ellhyb.py can pass by skipping or by a refusal
-- what every generated matrix is there for."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ellhyb_cases as cases  # noqa: E402

DTYPES = [np.float64, np.float32]


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_layout_rules_equal_the_oracle(oracle, name, dtype):
    nrow, ncol, rp, ci, va = cases.case(name)
    assert np.array_equal(va.astype(np.float32).astype(np.float64), va) and np.max(np.abs(va)) <= 8  # exact in fp32
    assert np.array_equal(va * 8, np.round(va * 8))
    va = va.astype(dtype)
    ell, ref = cases.csr_to_ell(nrow, rp, ci, va), oracle.csr_to_ell(rp, ci, va)
    assert (ell is None) == (ref is None) == (name in cases.ELL_REFUSED)  # the oracle accepts every ELL case
    if ell is not None:
        assert ell[0] == ref[0]
        eq(ell[1], ref[1]); eq(ell[2], ref[2])
    hyb, ref = cases.csr_to_hyb(nrow, rp, ci, va), oracle.csr_to_hyb(rp, ci, va)
    assert hyb[0] == ref[0]
    for a, b in zip(hyb[1:], ref[1:]):
        eq(a, b)
    row, col, val = cases.csr_to_coo(nrow, rp, ci, va)
    eq(row, np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))); eq(col, ci); eq(val, va)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_products_agree_in_every_layout(oracle, name, dtype):
    """the dyadic data makes every sum exact, so ELL, HYB and COO -- three orders of the same additions -- give the bits of
    the CSR product; with the poisoned x as well: no layout's product reads a padded slot's column"""
    nrow, ncol, rp, ci, va = cases.case(name)
    va = va.astype(dtype)
    y0, s = cases.y0_of(name).astype(dtype), -0.75
    for x in (cases.x_of(name).astype(dtype), cases.poisoned_x(name).astype(dtype)):
        y, ya = oracle.csr_apply(rp, ci, va, x), oracle.csr_apply_add(rp, ci, va, x, s, y0)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(ya))
        # exact indeed: the sums in double, of the same operands, are the same numbers
        eq(y.astype(np.float64), oracle.csr_apply(rp, ci, va.astype(np.float64), x.astype(np.float64)))
        eq(ya.astype(np.float64), oracle.csr_apply_add(rp, ci, va.astype(np.float64), x.astype(np.float64), s, y0.astype(np.float64)))
        if name in cases.ELL_NAMES:
            w, ec, ev = cases.csr_to_ell(nrow, rp, ci, va)
            eq(oracle.ell_apply(nrow, w, ec, ev, x), y)
            eq(oracle.ell_apply_add(nrow, w, ec, ev, x, s, y0), ya)
        w, ec, ev, cr, cc, cv = cases.csr_to_hyb(nrow, rp, ci, va)
        eq(oracle.hyb_apply(nrow, ncol, w, ec, ev, cr, cc, cv, x), y)
        eq(oracle.hyb_apply_add(nrow, ncol, w, ec, ev, cr, cc, cv, x, s, y0), ya)
        row, col, val = cases.csr_to_coo(nrow, rp, ci, va)
        eq(oracle.coo_apply(nrow, row, col, val, x), y)
        eq(oracle.coo_apply_add(row, col, val, x, s, y0), ya)


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_ways_back(name):
    """ELL -> CSR and HYB -> CSR give the input back, entry for entry, sorted or not; COO -> CSR gives it back for sorted rows
    and sorts the others stably"""
    nrow, ncol, rp, ci, va = cases.case(name)
    assert cases.rows_sorted(rp, ci) == (name not in cases.UNSORTED)
    if name in cases.ELL_NAMES:
        for a, b in zip(cases.ell_to_csr(nrow, ncol, *cases.csr_to_ell(nrow, rp, ci, va)), (rp, ci, va)):
            eq(a, b)
    for a, b in zip(cases.hyb_to_csr(nrow, ncol, *cases.csr_to_hyb(nrow, rp, ci, va)), (rp, ci, va)):
        eq(a, b)
    brp, bci, bva = cases.coo_to_csr(nrow, *cases.csr_to_coo(nrow, rp, ci, va))
    eq(brp, rp)
    if name not in cases.UNSORTED:
        eq(bci, ci); eq(bva, va)
    else:
        assert not np.array_equal(bci, ci) and cases.rows_sorted(brp, bci)
    for r in range(nrow):  # the bubble sort of the reference, row by row
        c, v = ci[rp[r]:rp[r + 1]].tolist(), va[rp[r]:rp[r + 1]].tolist()
        for _ in c:
            for j in range(len(c) - 1):
                if c[j] > c[j + 1]:
                    c[j], c[j + 1], v[j], v[j + 1] = c[j + 1], c[j], v[j + 1], v[j]
        assert bci[rp[r]:rp[r + 1]].tolist() == c and bva[rp[r]:rp[r + 1]].tolist() == v


@pytest.mark.parametrize("name", ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300", "rand300ell"])
def test_layout_rules_reproduce_the_goldens(name):
    g = load_golden(name)
    rp, ci, va = g["rowptr"].astype(np.int32), g["col"].astype(np.int32), g["val"]
    n = len(rp) - 1
    ell = cases.csr_to_ell(n, rp, ci, va)
    if name == "rand300":  # refused by the reference
        assert ell is None and "ell_col" not in g
        return
    assert ell[0] == int(g["ell_width"][0])
    eq(ell[1], g["ell_col"].astype(np.int32)); eq(ell[2], g["ell_val"])
    for a, b in zip(cases.ell_to_csr(n, n, *ell), (rp, ci, va)):
        eq(a, b)


def test_what_the_cases_are_there_for():
    lens = {name: np.diff(cases.case(name)[2]) for name in cases.NAMES}
    hyb = {name: cases.csr_to_hyb(*cases.case(name)[:1], *cases.case(name)[2:]) for name in cases.NAMES}
    for n in cases.RAGGED_SIZES:
        L = lens["ragged_%d" % n]
        assert len(L) == n and L.max() <= 9
        if n > 1:
            assert L[0] == 0 and L[-1] == 0 and len(set(L.tolist())) >= 8
        if n >= 255:
            assert np.all(L[100:170] == 0)  # more than a wave of empty rows
    for k in (1, 8, 9, 17):
        assert set(lens["len%d_130" % k].tolist()) == {k}
    assert set(lens["lenmix_130"].tolist()) == {1, 8, 9, 17}
    nrow, ncol, rp, ci, va = cases.case("wide_300x1000")
    assert (nrow, ncol) == (300, 1000) and ci.max() == 999
    nrow, ncol, rp, ci, va = cases.case("tall_1000x300")
    assert (nrow, ncol) == (1000, 300) and ci.max() < 300 and lens["tall_1000x300"][301:].sum() > 0
    assert cases.case("row_1x500")[:2] == (1, 500)
    for name, over in (("ell_at_limit", 0), ("ell_over_limit", 1)):
        nrow, ncol, rp, ci, va = cases.case(name)
        assert lens[name].max() == 5 * (208 // nrow) + over and len(va) == 208 + over
    assert len(hyb["hyb_no_tail"][3]) == 0
    w, ec, ev, cr, cc, cv = hyb["hyb_one_long_65"]
    assert w == 13 and len(cr) == 587 and set(cr.tolist()) == {20}
    w, ec, ev, cr, cc, cv = hyb["hyb_many_tails_1000"]
    assert w == 5 and len(set(cr.tolist())) == 500 > 256 and len(cr) == 2000
    assert set(lens["width29_64"].tolist()) == {29}
    # stencil_tails_512: at most 64 slot tuples (offsets, -1 as it is), and rows that share a tuple with different tails
    nrow, ncol, rp, ci, va = cases.case("stencil_tails_512")
    w, ec, ev, cr, cc, cv = hyb["stencil_tails_512"]
    assert w == 4 and len(cr) == 5 * 29
    slots = ec.reshape(w, nrow).T
    tuples = [tuple(int(c) - r if c >= 0 else None for c in slots[r]) for r in range(nrow)]
    assert len(set(tuples)) <= 64
    assert len({tuples[r] for r in (40, 41, 200, 333, 480)}) == 1
    assert len({tuple((cc[cr == r] - r).tolist()) for r in (40, 41, 200, 333, 480)}) == 5
    # odd_columns_512: CSR rows in at most 64 patterns; every even element of x is poisoned, which is x[row] of every even
    # row -- the element a padded slot's offset 0 of a CSR dictionary would point at
    nrow, ncol, rp, ci, va = cases.case("odd_columns_512")
    assert np.all(ci % 2 == 1) and lens["odd_columns_512"].tolist() == [1, 3] * 256
    assert len({tuple((ci[rp[r]:rp[r + 1]] - r).tolist()) for r in range(nrow)}) <= 64
    px = cases.poisoned_x("odd_columns_512")
    assert np.all(np.isnan(px[0::2])) and np.all(np.isfinite(px[1::2]))
    assert cases.csr_to_ell(nrow, rp, ci, va)[0] == 3 and hyb["odd_columns_512"][0] == 2 and len(hyb["odd_columns_512"][3]) == 256
    for name in cases.NAMES:  # a poisoned x poisons something wherever a column is free
        nrow, ncol, rp, ci, va = cases.case(name)
        assert np.isnan(cases.poisoned_x(name)).sum() == ncol - len(set(ci.tolist()))
