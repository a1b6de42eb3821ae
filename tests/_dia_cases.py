"""Generated matrices for the DIA tests: shapes the goldens do not reach.  Shared by tests/test_cpu_dia.py (the oracle accepts
every one of them under the reference's 5x rule, so no GPU case depends on a refusal) and tests/test_gpu_dia.py.

Values are multiples of 1/8 of magnitude up to 8, so they are exact in fp32 as well."""
import numpy as np


def _vals(rng, k):
    return rng.integers(1, 64, size=k).astype(np.float64) / 8.0 * rng.choice([-1.0, 1.0], size=k)


def banded(n, offsets, seed, keep=None):
    """CSR with sorted rows and one entry on every diagonal of `offsets` where the column exists (keep(row, off) -> bool
    thins it out)"""
    rng = np.random.default_rng(seed)
    rp, ci = [0], []
    for r in range(n):
        for o in sorted(offsets):
            if 0 <= r + o < n and (keep is None or keep(r, o)):
                ci.append(r + o)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), _vals(rng, len(ci))


def shuffled(rp, ci, va, seed):
    """the same matrix with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    ci, va = ci.copy(), va.copy()
    for r in range(len(rp) - 1):
        p = rng.permutation(int(rp[r + 1] - rp[r])) + int(rp[r])
        ci[rp[r]:rp[r + 1]] = ci[p]
        va[rp[r]:rp[r + 1]] = va[p]
    return ci, va


def _with_extra(rp, ci, va, extra):
    """append to row r the entries extra[r] = [(col, val), ...] (stored after the row's own)"""
    nrp, nci, nva = [0], [], []
    for r in range(len(rp) - 1):
        nci.extend(ci[rp[r]:rp[r + 1]].tolist()); nva.extend(va[rp[r]:rp[r + 1]].tolist())
        for c, v in extra.get(r, []):
            nci.append(c); nva.append(v)
        nrp.append(len(nci))
    return np.array(nrp, np.int32), np.array(nci, np.int32), np.array(nva, np.float64)


SIZES = [1, 63, 64, 65, 257, 1000]  # one lane; under, at and over a wave; a workgroup and one row; four workgroups, two interior
NAMES = ["tri_%d" % n for n in SIZES] + ["band40_130", "far300_1000", "corners_200", "off3_only", "shuffled_257",
                                          "duplicate_65", "zeros_64", "holes_64"]


def case(name):
    """-> (rp, ci, va) of a square matrix"""
    if name.startswith("tri_"):
        return banded(int(name[4:]), (-1, 0, 1), 3)
    if name == "band40_130":  # a full band of 40 diagonals: five chunks of eight in the product
        return banded(130, range(-20, 20), 4)
    if name == "far300_1000":  # offsets beyond a workgroup's 256 rows: no workgroup is interior
        return banded(1000, (-300, 0, 300), 5)
    if name == "corners_200":  # the two one-entry diagonals +-(n - 1)
        return banded(200, (-199, 0, 199), 6)
    if name == "off3_only":
        # one diagonal, +3, and no main diagonal.  Its n - 3 entries alone give nnz / n = 0 and the reference refuses; the
        # first ten rows store their entry twice (the later value is the one that stays), which lifts nnz to n + 7
        rp, ci, va = banded(100, (3,), 7)
        return _with_extra(rp, ci, va, {r: [(r + 3, 0.125 * (r + 1))] for r in range(10)})
    if name == "shuffled_257":
        rp, ci, va = banded(257, (-17, -2, -1, 0, 1, 2, 17), 8)
        ci, va = shuffled(rp, ci, va, 9)
        return rp, ci, va
    if name == "duplicate_65":  # row 5 stores column 5 a second time, row 40 column 41: the entry stored later stays
        rp, ci, va = banded(65, (-1, 0, 1), 10)
        return _with_extra(rp, ci, va, {5: [(5, -2.5)], 40: [(41, 3.25)]})
    if name == "zeros_64":  # stored zeros and a stored -0.0: kept (with their sign) in DIA, dropped on the way back
        rp, ci, va = banded(64, (-1, 0, 1), 11)
        va[[4, 17, 100]] = 0.0
        va[50] = -0.0
        return rp, ci, va
    if name == "holes_64":  # diagonal +5 is stored in rows 0..9 only: padded zeros inside its range in rows 10..58
        return banded(64, (-1, 0, 5), 12, keep=lambda r, o: o != 5 or r < 10)
    raise KeyError(name)


def special_x(n):
    """x for holes_64: +-inf where only PADDED zeros of diagonal +5 multiply it, NaN at element 0 -- the element the product
    reads in place of a column outside [0, n)"""
    x = np.random.default_rng(13).integers(-32, 48, size=n).astype(np.float64) / 8.0
    x[25] = np.inf   # row 20, diagonal +5: a padded zero inside the range -> 0 * inf = NaN, as the host loop gives
    x[35] = -np.inf  # row 30
    x[0] = np.nan    # rows 0 (main diagonal) and 1 (diagonal -1) take it; rows 59..63 (diagonal +5 out of range) must not
    return x


def dyadic(n, seed, lo=-32, hi=48):
    return np.random.default_rng(seed).integers(lo, hi, size=n).astype(np.float64) / 8.0
