"""Generated matrices for the MCSR tests: shapes the goldens do not reach.  Shared by tests/test_cpu_mcsr.py (tests/_mcsr_ref.py
accepts every one meant to be accepted and refuses the two meant to be refused, so no GPU case rests on an unchecked refusal),
tests/test_gpu_mcsr.py and tools/gen_golden_mcsr.py.

Values are multiples of 1/8 of magnitude up to 8, so they are exact in fp32 as well."""
import numpy as np

CAP = 1024  # kMcsrCap of csrc/mcsr.hip: entries of a wave's 64 rows that one staging pass holds


def _vals(rng, k):
    return rng.integers(1, 64, size=k).astype(np.float64) / 8.0 * rng.choice([-1.0, 1.0], size=k)


def from_rows(rows, seed):
    """rows[r] = columns of row r in storage order -> (rp, ci, va) with seeded dyadic values"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.array([c for r in rows for c in r], np.int32)
    return rp, ci, _vals(np.random.default_rng(seed), len(ci))


def banded(n, offsets, seed, ncol=None):
    ncol = n if ncol is None else ncol
    return from_rows([[r + o for o in sorted(offsets) if 0 <= r + o < ncol] for r in range(n)], seed)


def shuffled(rp, ci, va, seed):
    """the same matrix with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    ci, va = ci.copy(), va.copy()
    for r in range(len(rp) - 1):
        p = rng.permutation(int(rp[r + 1] - rp[r])) + int(rp[r])
        ci[rp[r]:rp[r + 1]] = ci[p]
        va[rp[r]:rp[r + 1]] = va[p]
    return ci, va


SIZES = [1, 63, 64, 65, 257, 1000]  # one lane; under, at and over a wave; a workgroup and one row; several workgroups
ACCEPTED = ["tri_%d" % n for n in SIZES] + ["diag_only_130", "shuffled_257", "longrow", "hub", "zeros_64", "negzero_64"]
REFUSED = ["nodiag_row_40", "rect_5x7"]
NAMES = ACCEPTED + REFUSED


def shape(name):
    return (5, 7) if name == "rect_5x7" else (len(case(name)[0]) - 1,) * 2


def case(name):
    """-> (rp, ci, va); square except rect_5x7 (see shape)"""
    if name.startswith("tri_"):
        return banded(int(name[4:]), (-1, 0, 1), 3)
    if name == "diag_only_130":  # every off-diagonal range is empty: no wave stages anything
        return banded(130, (0,), 4)
    if name == "shuffled_257":  # rows in random storage order: the diagonal first, last and in the middle of a row
        rp, ci, va = banded(257, (-17, -2, -1, 0, 1, 2, 17), 8)
        ci, va = shuffled(rp, ci, va, 9)
        return rp, ci, va
    if name == "longrow":
        # CAP = 1024 entries per staging pass.  Row 70 is dense: 1299 off-diagonal entries, one row across two passes (and the
        # rows of its wave behind it begin in the second).  Rows 128 .. 191 hold 20 off-diagonal entries each: 1280 in the wave,
        # no row longer than a pass, rows cut by the pass boundary.  The other rows are tridiagonal.
        n = 1300
        rows = [[r + o for o in (-1, 0, 1) if 0 <= r + o < n] for r in range(n)]
        rows[70] = list(range(n))
        for r in range(128, 192):
            rows[r] = [r + o for o in range(-10, 11)]
        return from_rows(rows, 14)
    if name == "hub":
        # the construction of tools/gen_golden_amg.py's `hub` with dyadic values: row 0 coupled to every fourth row of a chain of
        # 2049 rows behind it -- a 514-entry row 0 and two- to four-entry rows beside it in the same wave
        n, e = 2049, {(0, 0): 8.0}
        for i in range(1, n + 1):
            e[(i, i)] = 2.0
            if i > 1:
                e[(i, i - 1)] = e[(i - 1, i)] = -1.0
        for k in range(1, n + 1, 4):
            e[(0, k)] = e[(k, 0)] = -(4 + k % 7) / 8.0
        rows = [[] for _ in range(n + 1)]
        for (i, j) in sorted(e):
            rows[i].append(j)
        rp, ci, _ = from_rows(rows, 0)
        va = np.array([e[(i, int(ci[j]))] for i in range(n + 1) for j in range(rp[i], rp[i + 1])])
        return rp, ci, va
    if name == "zeros_64":  # stored 0.0 and -0.0 on and off the diagonal: both conversions keep them, with their sign
        rp, ci, va = banded(64, (-1, 0, 1), 11)
        va[[4, 100]] = 0.0    # (row 1, column 2) and (row 33, column 34)
        va[[50, 121]] = -0.0  # (row 17, column 16) and (row 40, column 41)
        va[rp[20] + 1] = 0.0  # the diagonal of row 20
        va[rp[30] + 1] = -0.0  # the diagonal of row 30
        return rp, ci, va
    if name == "negzero_64":  # rows 0 .. 31 store the diagonal alone (see x_for): the only term is val[i] * x[i]
        n = 64
        return from_rows([[r] if r < 32 else [r + o for o in (-1, 0, 1) if 0 <= r + o < n] for r in range(n)], 12)
    if name == "nodiag_row_40":  # row 17 stores no diagonal entry: refused
        n = 40
        return from_rows([[r + o for o in (-1, 0, 1) if 0 <= r + o < n and not (r == 17 and o == 0)] for r in range(n)], 13)
    if name == "rect_5x7":  # refused
        return banded(5, (-1, 0, 1, 2), 15, ncol=7)
    raise KeyError(name)


def dyadic(n, seed, lo=-32, hi=48):
    return np.random.default_rng(seed).integers(lo, hi, size=n).astype(np.float64) / 8.0


def x_for(name):
    """the x of the products: dyadic; negzero_64: in elements 0 .. 47 zeros of the sign that makes val[i] * x[i] == -0.0, so
    the MCSR sum of rows 0 .. 31 is -0.0 where the CSR loop's 0 + ... gives +0.0 (rows 32 .. 46 add zeros of either sign to it)"""
    rp, ci, va = case(name)
    x = dyadic(shape(name)[1], 5)
    if name == "negzero_64":
        for r in range(48):
            d = [va[j] for j in range(rp[r], rp[r + 1]) if ci[j] == r][0]
            x[r] = -0.0 if d > 0 else 0.0
    return x


def y_for(name):
    return dyadic(shape(name)[0], 6, -16, 16)
