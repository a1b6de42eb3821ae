"""Generated matrices for the ELL / HYB / COO tests -- ragged, rectangular, at the limits of the layouts -- and numpy
restatements of the reference's layout rules (host_conversion.cpp: csr_to_ell, csr_to_hyb, csr_to_coo, ell_to_csr, hyb_to_csr,
coo_to_csr).  Shared by tests/test_cpu_ellhyb.py, which pins the restatements to the oracle and the committed goldens and checks
what every case is there for, and tests/test_gpu_ellhyb.py.

Values and x are multiples of 1/8 (values of magnitude up to 8, x within [-4, 4)): exact in fp32 and fp64, and so is every
product, every product with the ApplyAdd scalar -0.75 and every row sum in any order -- the longest row has 600 entries, its
sum stays below 2^15 in multiples of 2^-8: 23 bits.  A comparison with `==` is therefore a comparison of the algorithm, not
of a summation order."""
import functools

import numpy as np


def _vals(rng, k):
    return rng.integers(1, 65, size=k).astype(np.float64) / 8.0 * rng.choice([-1.0, 1.0], size=k)


def dyadic(n, seed, lo=-32, hi=32):
    return np.random.default_rng(seed).integers(lo, hi, size=n).astype(np.float64) / 8.0


def from_rows(nrow, ncol, rows, seed):
    """rows: one sequence of column indices per row, stored as given -> (nrow, ncol, rp, ci, va)"""
    assert len(rows) == nrow
    rp = np.zeros(nrow + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], np.int32)
    assert ci.size == 0 or (ci.min() >= 0 and ci.max() < ncol)
    return nrow, ncol, rp, ci, _vals(np.random.default_rng(seed), len(ci))


def _pick(rng, ncol, k):
    return np.sort(rng.choice(ncol, size=k, replace=False)).tolist()


def ragged(nrow, ncol, seed, shuffle=False):
    """row lengths 0..9 at random (never more than ncol), sorted unique columns.  From two rows on the first and the last row
    are empty; from 255 rows on rows 100..169 are empty too: a whole wave of rows, and more, without an entry.  (One row: a row
    of the one length a 1 x 1 matrix can have.)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, size=nrow).clip(max=ncol)
    if nrow == 1:
        lens[:] = min(ncol, 7)
    else:
        lens[0] = lens[-1] = 0
    if nrow >= 255:
        lens[100:170] = 0
    rows = [_pick(rng, ncol, int(k)) for k in lens]
    if shuffle:
        rows = [rng.permutation(r).tolist() for r in rows]
    if nrow > 1 and ncol > nrow:  # the last column is referenced
        rows[1] = sorted(set(rows[1][:8] + [ncol - 1]))
    return from_rows(nrow, ncol, rows, seed + 1)


def lengths(nrow, ncol, lens, seed):
    rng = np.random.default_rng(seed)
    return from_rows(nrow, ncol, [_pick(rng, ncol, int(k)) for k in lens], seed + 1)


RAGGED_SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 1001]
RAGGED = ["ragged_%d" % n for n in RAGGED_SIZES]
WIDTHS = ["len1_130", "len8_130", "len9_130", "len17_130", "lenmix_130"]
RECT = ["wide_300x1000", "tall_1000x300", "row_1x500"]
# every one of these is accepted by csr_to_ell (max row nnz <= 5 * (nnz / nrow)): tests/test_cpu_ellhyb.py
ELL_NAMES = (RAGGED + WIDTHS + RECT + ["ell_at_limit", "hyb_no_tail", "hyb_many_tails_1000", "unsorted_257", "width29_64",
                                       "odd_columns_512"])
# ... and these three are refused
ELL_REFUSED = ["ell_over_limit", "hyb_one_long_65", "stencil_tails_512"]
NAMES = ELL_NAMES + ELL_REFUSED  # HYB and COO take every one of them
UNSORTED = ["unsorted_257", "stencil_tails_512"]  # (the five long rows of the stencil store their extra entries last)


def _limit(extra):
    # 99 rows of 2 entries and one of 10 (+ extra): nnz = 208 (209), nnz / nrow = 2, the limit is 10
    rng = np.random.default_rng(31)
    rows = [_pick(rng, 100, 2) for _ in range(100)]
    rows[37] = _pick(rng, 100, 10 + extra)
    return from_rows(100, 100, rows, 32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (nrow, ncol, rp, ci, va); the arrays are shared between the tests and must not be written"""
    out = _case(name)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def _case(name):
    if name.startswith("ragged_"):
        n = int(name[7:])
        return ragged(n, n, 100 + n)
    if name.startswith("len") and name.endswith("_130"):  # around the gather batch of the product kernels, kGatherW = 8
        k = name[3:-4]
        lens = np.random.default_rng(40).choice([1, 8, 9, 17], size=130) if k == "mix" else [int(k)] * 130
        return lengths(130, 130, lens, 41)
    if name == "wide_300x1000":
        return ragged(300, 1000, 50)
    if name == "tall_1000x300":
        return ragged(1000, 300, 51)
    if name == "row_1x500":
        return ragged(1, 500, 52)
    if name == "ell_at_limit":
        return _limit(0)
    if name == "ell_over_limit":
        return _limit(1)
    if name == "hyb_no_tail":  # every row as long as the HYB width: coo_nnz == 0
        return lengths(200, 200, [5] * 200, 60)
    if name == "hyb_one_long_65":
        # 64 rows of 3 entries and one of 600: the HYB width is 13, the tail is ONE group of 587 entries.  A square matrix (the
        # fused product + dot wants one) of 65 columns holds 600 entries in a row only with columns stored more than once: the
        # long row's columns are 600 draws, in non-decreasing order -- entries like any other in all three layouts
        rng = np.random.default_rng(61)
        rows = [_pick(rng, 65, 3) for _ in range(65)]
        rows[20] = np.sort(rng.integers(0, 65, size=600)).tolist()
        return from_rows(65, 65, rows, 62)
    if name == "hyb_many_tails_1000":  # lengths 1, 9, 1, 9, ...: width 5, a tail of 4 in 500 rows -- two workgroups of groups
        return lengths(1000, 1000, [1, 9] * 500, 63)
    if name == "unsorted_257":
        return ragged(257, 257, 64, shuffle=True)
    if name == "width29_64":  # one entry more than a row pattern holds (kPatMaxW = 28)
        return lengths(64, 64, [29] * 64, 65)
    if name == "stencil_tails_512":
        # the 1-D 3-point stencil, and in five rows 30 more entries stored after the row's own: the first of them at column
        # row + 2 (the fourth ELL slot, HYB width 4: the five rows share ONE slot tuple), the other 29 -- the COO tail -- at
        # columns that differ from row to row
        rng = np.random.default_rng(66)
        rows = [[c for c in (r - 1, r, r + 1) if 0 <= c < 512] for r in range(512)]
        for r in (40, 41, 200, 333, 480):
            far = [c for c in rng.permutation(512).tolist() if abs(c - r) > 2][:29]
            rows[r] = rows[r] + [r + 2] + far
        return from_rows(512, 512, rows, 67)
    if name == "odd_columns_512":
        # only odd columns are referenced; even rows hold 1 entry, odd rows 3: ELL width 3; HYB width 2, a padded slot
        # in every even row and a tail of one entry in every odd row
        rows = []
        for r in range(512):
            if r % 2 == 0:
                rows.append([r + 1])
            else:
                rows.append(sorted(c if 0 < c < 512 else (r + 4 if c < 0 else r - 4) for c in (r - 2, r, r + 2)))
        return from_rows(512, 512, rows, 68)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def x_of(name):
    x = dyadic(case(name)[1], 7)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def y0_of(name):
    y = dyadic(case(name)[0], 8, -16, 16)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def poisoned_x(name):
    """x_of(name) with NaN at every column that no entry of the case references: the reference never reads x for a padded
    slot, so the product stays finite and the same"""
    nrow, ncol, rp, ci, va = case(name)
    x = x_of(name).copy()
    free = np.ones(ncol, bool)
    free[ci] = False
    x[free] = np.nan
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------- the reference's layout rules
def _slots(nrow, rp):
    """per entry: its row and its position inside the row"""
    lens = np.diff(rp).astype(np.int64)
    row = np.repeat(np.arange(nrow, dtype=np.int64), lens)
    return row, np.arange(int(rp[-1]), dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lens)


def _ell_fill(nrow, width, row, k, ci, va):
    ec = np.full(width * nrow, -1, np.int32)  # ELL_IND(row, el) = el * nrow + row; padding: column -1, value 0
    ev = np.zeros(width * nrow, va.dtype)
    ec[k * nrow + row] = ci
    ev[k * nrow + row] = va
    return ec, ev


def csr_to_ell(nrow, rp, ci, va):
    """host_conversion.cpp:621-687 -> (width, ell_col, ell_val), or None: refused, max row nnz > 5 * (nnz / nrow)"""
    nnz = int(rp[-1])
    width = int(np.max(np.diff(rp))) if nrow else 0
    if nrow and width > 5 * (nnz // nrow):
        return None
    row, k = _slots(nrow, rp)
    return (width,) + _ell_fill(nrow, width, row, k, ci, va)


def csr_to_hyb(nrow, rp, ci, va):
    """host_conversion.cpp:1117-1243 -> (width, ell_col, ell_val, coo_row, coo_col, coo_val), or None: no entry.  The ELL
    width is the mean row length rounded up; the first `width` entries of a row are its ELL slots, the rest the COO tail in
    storage order"""
    nnz = int(rp[-1])
    if nrow == 0 or nnz <= 0:
        return None
    width = (nnz - 1) // nrow + 1
    row, k = _slots(nrow, rp)
    e = k < width
    ec, ev = _ell_fill(nrow, width, row[e], k[e], ci[e], va[e])
    return width, ec, ev, row[~e].astype(np.int32), ci[~e].copy(), va[~e].copy()


def csr_to_coo(nrow, rp, ci, va):
    """host_conversion.cpp:582-618 -> (row, col, val): the row of every entry; columns and values as they are"""
    return _slots(nrow, rp)[0].astype(np.int32), ci.copy(), va.copy()


def _rows_to_csr(nrow, row, col, val):
    rp = np.zeros(nrow + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(row, minlength=nrow)[:nrow])
    return rp, col.astype(np.int32), val


def ell_to_csr(nrow, ncol, width, ec, ev):
    """host_conversion.cpp:690-762: a row keeps its slots with 0 <= col < ncol, in slot order"""
    c = ec.reshape(width, nrow).T  # [row, slot]
    v = ev.reshape(width, nrow).T
    ok = (c >= 0) & (c < ncol)
    row = np.repeat(np.arange(nrow), ok.sum(axis=1))
    return _rows_to_csr(nrow, row, c[ok], v[ok])


def hyb_to_csr(nrow, ncol, width, ec, ev, cr, cc, cv):
    """host_conversion.cpp:765-881: the ELL slots of a row as ell_to_csr keeps them, then its COO entries in storage order;
    nothing is sorted"""
    rp, ci, va = ell_to_csr(nrow, ncol, width, ec, ev)
    row = np.concatenate([np.repeat(np.arange(nrow), np.diff(rp)), cr.astype(np.int64)])
    order = np.argsort(row, kind="stable")
    return _rows_to_csr(nrow, row[order], np.concatenate([ci, cc])[order], np.concatenate([va, cv])[order])


def coo_to_csr(nrow, row, col, val):
    """host_conversion.cpp:884-955: rows are sorted already; inside a row the columns are bubble-sorted, which is stable"""
    order = np.lexsort((col, row))  # (a stable sort by row, then column)
    return _rows_to_csr(nrow, row[order].astype(np.int64), col[order], val[order])


def rows_sorted(rp, ci):
    return all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) >= 0) for r in range(len(rp) - 1))
