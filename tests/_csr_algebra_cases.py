"""Operands of the CSR algebra tests (Transpose, MatrixMult, MatrixAdd, Sort, DiagonalMatrixMult), shared by
test_cpu_csr_algebra.py (the oracle against scipy) and test_gpu_csr_algebra.py (the device against the oracle).

Everything is generated from seeds.  Columns are sorted and unique within a row unless a builder says otherwise; values are
standard_normal cast to the value type, so they are not dyadic and the order of a sum shows in its last bit.

The MatrixMult cases are laid out by the number of products per row of C = A.B, which is what selects the code path
(matrix_algebra.hip, mat_mult_t): up to INSERT_LIMIT products in every row -> per-thread insertion; else row chunks, each
through one workgroup per row in LDS, or -- when a row of the chunk has more than LDS_CAP products -- through two global
stable sorts.  The standard B is 400 x 700 with rows of 32 entries, except row 0 (1 entry), row 1 (31) and row 2 (none), so a
row of A with any wanted product count is a choice of rows of B.
"""
import collections
import functools

import numpy as np

INSERT_LIMIT = 64   # mat_mult_t: `limit`
LDS_CAP = 2048      # kMmCap
SMALL_CHUNK = 2500  # RAMD_MM_CHUNK of the fresh-process test

Csr = collections.namedtuple("Csr", "shape rp ci va")

DTYPES = [np.float64, np.float32]


def arrays(M):
    return M.rp, M.ci, M.va


def csr_from_columns(shape, rows, seed, dtype, values="normal"):
    """rows: one sequence of column indices per row, stored as given"""
    nrow, ncol = shape
    assert len(rows) == nrow
    rp = np.zeros(nrow + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], dtype=np.int32)
    assert ci.size == 0 or (ci.min() >= 0 and ci.max() < ncol)
    rng = np.random.default_rng(seed)
    if values == "normal":
        va = rng.standard_normal(ci.size).astype(dtype)
    else:  # "pm1"
        va = rng.choice(np.array([-1.0, 1.0]), size=ci.size).astype(dtype)
    return Csr((nrow, ncol), rp, ci, va)


def random_csr(shape, row_lengths, seed, dtype, values="normal"):
    """the helper of the tests: a shape, a list of row lengths and a seed"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(shape[1], size=k, replace=False)).tolist() for k in row_lengths]
    return csr_from_columns(shape, rows, seed + 1, dtype, values)


def empty_csr(shape, dtype):
    return csr_from_columns(shape, [[]] * shape[0], 0, dtype)


def row_lengths(M):
    return np.diff(M.rp)


def is_sorted_unique(M):
    return all(np.all(np.diff(M.ci[M.rp[i]:M.rp[i + 1]]) > 0) for i in range(M.shape[0]))


def product_counts(A, B):
    """products per row of A.B (k_mm_bound)"""
    lb = row_lengths(B).astype(np.int64)
    return np.array([lb[A.ci[A.rp[i]:A.rp[i + 1]]].sum() for i in range(A.shape[0])], dtype=np.int64)


def chunk_rows(counts, chunk):
    """the row chunks of mat_mult_chunked_t: the largest r1 with at most `chunk` products in [r0, r1), at least one row"""
    out, r0, n = [], 0, len(counts)
    while r0 < n:
        r1, p = r0 + 1, int(counts[r0])
        while r1 < n and p + int(counts[r1]) <= chunk:
            p += int(counts[r1])
            r1 += 1
        out.append((r0, r1))
        r0 = r1
    return out


# ------------------------------------------------------------------------------------------------ MatrixMult
def std_b(dtype):
    lens = [32] * 400
    lens[0], lens[1], lens[2] = 1, 31, 0
    return random_csr((400, 700), lens, 11, dtype)


def _a_for_counts(spec, seed, dtype):
    """spec: (product count, also hit the empty row 2 of B) per row of A; B = std_b"""
    rng = np.random.default_rng(seed)
    rows = []
    for count, hit_empty in spec:
        q, r = divmod(count, 32)
        cols = {0: [], 1: [0], 31: [1]}[r] + ([2] if hit_empty else [])
        cols += np.sort(rng.choice(np.arange(3, 400), size=q, replace=False)).tolist()
        rows.append(cols)
    return csr_from_columns((len(spec), 400), rows, seed + 1, dtype)


_SHORT = [(0, False), (0, True), (1, False), (31, False), (32, False), (63, True), (64, False)]
_MEDIUM = [(0, False), (1, False), (64, False), (65, False), (96, True), (256, False), (257, False), (1024, False),
           (1025, False), (2047, False), (2048, True)]
# the two rows beyond the LDS capacity sit in the middle: rows before and after them share their chunk
_LONG = _MEDIUM[:6] + [(2049, False)] + _MEDIUM[6:8] + [(2080, True)] + _MEDIUM[8:]
# (not in the issue's list) one row with more products than SMALL_CHUNK: the "at least one row" branch of the chunk search
_OVER_CHUNK = [(96, False), (2528, False), (257, False)]


def _narrow(ncol, dtype):
    # rows of B: 8 of the 16 (17) columns; a row of A with 300 entries has 2400 products: the global sort, whose column key
    # needs one 4-bit pass for 16 columns (max_key 15) and two for 17 (max_key 16)
    B = random_csr((400, ncol), [8] * 400, 21 + ncol, dtype)
    A = random_csr((20, 400), [0, 3, 300, 40, 1, 9, 260, 8] + [5] * 12, 23 + ncol, dtype)
    return A, B


def _column(dtype):
    lens = [1] * 400
    for r in (2, 50, 51, 399):
        lens[r] = 0
    B = random_csr((400, 1), lens, 31, dtype)
    A = random_csr((50, 400), [0, 1, 5, 80] * 12 + [0, 80], 33, dtype)
    return A, B


def _cancel(dtype, long_row):
    B = random_csr((40, 12), [5] * 40, 41, dtype, values="pm1")
    lens = [6] * 30
    lens[4] = 0
    if long_row:
        lens[17] = 20  # 100 products: the whole product leaves the insertion path
    A = random_csr((30, 40), lens, 43, dtype, values="pm1")
    return A, B


def _hit_only_empty_rows(dtype):
    B = std_b(dtype)
    Bh = csr_from_columns((400, 700), [[] if r in (2, 7, 9) else B.ci[B.rp[r]:B.rp[r + 1]].tolist() for r in range(400)],
                          53, dtype)
    A = csr_from_columns((6, 400), [[2], [2, 7], [], [7, 9], [9], [2, 7, 9]], 55, dtype)
    return A, Bh


_MM = {
    "short": lambda dt: (_a_for_counts(_SHORT, 101, dt), std_b(dt)),
    "medium": lambda dt: (_a_for_counts(_MEDIUM, 103, dt), std_b(dt)),
    "long": lambda dt: (_a_for_counts(_LONG, 105, dt), std_b(dt)),
    "over_chunk": lambda dt: (_a_for_counts(_OVER_CHUNK, 107, dt), std_b(dt)),
    "row_vector": lambda dt: (_a_for_counts([(2240, False)], 109, dt), std_b(dt)),
    "column": _column,
    "narrow16": lambda dt: _narrow(16, dt),
    "narrow17": lambda dt: _narrow(17, dt),
    "cancel": lambda dt: _cancel(dt, False),
    "cancel_lds": lambda dt: _cancel(dt, True),
    "empty_a": lambda dt: (empty_csr((5, 400), dt), std_b(dt)),
    "empty_b": lambda dt: (_a_for_counts(_SHORT, 101, dt), empty_csr((400, 700), dt)),
    "empty_both": lambda dt: (empty_csr((5, 400), dt), empty_csr((400, 700), dt)),
    "empty_hit": _hit_only_empty_rows,
}
MM_CASES = list(_MM)
EMPTY_CASES = [c for c in MM_CASES if c.startswith("empty")]


@functools.lru_cache(maxsize=None)
def _mm_case(name, dtype_name):
    return _MM[name](np.dtype(dtype_name).type)


def mm_case(name, dtype):
    """-> (A, B); built once per (case, type), never modified"""
    return _mm_case(name, np.dtype(dtype).name)


def check_mm_case(name, A, B):
    """the property that puts the case on its code path, checked on the host"""
    pc = product_counts(A, B)
    assert A.shape[1] == B.shape[0] and is_sorted_unique(A) and is_sorted_unique(B)
    if name == "short":
        assert sorted(pc.tolist()) == [0, 0, 1, 31, 32, 63, 64] and pc.max() == INSERT_LIMIT
        assert any(row_lengths(A)[i] > 0 and pc[i] == 0 for i in range(A.shape[0]))  # a row holding only column 2
    elif name == "medium":
        assert sorted(pc.tolist()) == [0, 1, 64, 65, 96, 256, 257, 1024, 1025, 2047, 2048]
        assert pc.max() == LDS_CAP and (pc > INSERT_LIMIT).any()
    elif name == "long":
        assert sorted(pc.tolist()) == [0, 1, 64, 65, 96, 256, 257, 1024, 1025, 2047, 2048, 2049, 2080]
        assert pc.max() > LDS_CAP
        for big in (2049, 2080):  # rows before and after in the same (only) chunk
            i = pc.tolist().index(big)
            assert 0 < i < len(pc) - 1
        ch = chunk_rows(pc, SMALL_CHUNK)
        assert len(ch) >= 3
        assert any(pc[a:b].max() <= LDS_CAP and pc[a:b].sum() > 0 for a, b in ch)      # served by the LDS kernel alone
        assert any(pc[a:b].max() > LDS_CAP and b - a > 1 for a, b in ch)               # redone by the global sort, with neighbours
        assert any(b - a == 1 and pc[a] > LDS_CAP for a, b in ch)                      # a one-row chunk: row key 0 only
    elif name == "over_chunk":
        assert pc.max() > SMALL_CHUNK and 0 < int(np.argmax(pc)) < len(pc) - 1
    elif name == "row_vector":
        assert A.shape[0] == 1 and pc[0] == 2240 > LDS_CAP and row_lengths(A)[0] == 70  # max_key of the row sort: nrow - 1 == 0
    elif name == "column":
        assert B.shape[1] - 1 == 0                                                      # max_key of the column sort
        assert sorted(set(row_lengths(A).tolist())) == [0, 1, 5, 80]
        assert pc.max() > INSERT_LIMIT and (row_lengths(B) == 0).any()
    elif name in ("narrow16", "narrow17"):
        bits = int(B.shape[1] - 1).bit_length()
        assert (bits + 3) // 4 == (1 if name == "narrow16" else 2)                      # 4-bit passes of the column sort
        assert B.ci.max() == B.shape[1] - 1 and pc.max() > LDS_CAP and pc.min() == 0
    elif name in ("cancel", "cancel_lds"):
        assert set(np.unique(A.va)) == {-1.0, 1.0} and set(np.unique(B.va)) == {-1.0, 1.0}
        assert (pc.max() <= INSERT_LIMIT) == (name == "cancel")
    elif name == "empty_a":
        assert A.shape[0] == 5 and len(A.va) == 0 and len(B.va) > 0
    elif name == "empty_b":
        assert len(A.va) > 0 and len(B.va) == 0
    elif name == "empty_both":
        assert A.shape[0] == 5 and len(A.va) == 0 and len(B.va) == 0
    elif name == "empty_hit":
        assert len(A.va) > 0 and len(B.va) > 0 and pc.max() == 0
    else:
        raise KeyError(name)
    return pc


@functools.lru_cache(maxsize=None)
def _galerkin(dtype_name):
    from rocalution_amd import generators
    dtype = np.dtype(dtype_name).type
    n, nc = 700, 90
    rp, ci, va = generators.random_sparse(n, 7, 61)
    A = Csr((n, n), rp, ci, va.astype(dtype))
    rng = np.random.default_rng(63)
    agg = np.minimum((nc * rng.random(n) ** 2.2).astype(np.int64), nc - 1)  # uneven aggregate sizes
    keep = rng.random(n) >= 0.05
    P = csr_from_columns((n, nc), [[int(agg[i])] if keep[i] else [] for i in range(n)], 65, dtype)
    return A, P


def galerkin_case(dtype):
    """-> (A 700 x 700, P 700 x 90): the operands of every AMG Build()"""
    return _galerkin(np.dtype(dtype).name)


def check_galerkin_case(A, P):
    lp = row_lengths(P)
    assert A.shape == (700, 700) and P.shape == (700, 90) and lp.max() == 1
    assert 0.02 < (lp == 0).mean() < 0.09
    sizes = np.bincount(P.ci, minlength=90)
    assert sizes.max() >= 4 * max(1, np.median(sizes))


# ------------------------------------------------------------------------------------------------ Transpose
TRANSPOSE_SHAPES = [(600, 90), (90, 600), (257, 1), (1, 257)]
TRANSPOSE_VARIANTS = ["holes", "full"]


@functools.lru_cache(maxsize=None)
def _transpose_case(shape, variant, dtype_name):
    nrow, ncol = shape
    rng = np.random.default_rng(71 + nrow + 3 * ncol)
    empty_cols = set()
    if variant == "holes" and ncol >= 3:
        empty_cols = {ncol - 1} | set(rng.choice(np.arange(1, ncol - 1), size=max(1, ncol // 10), replace=False).tolist())
    allowed = np.array([c for c in range(1, ncol) if c not in empty_cols], dtype=np.int64)
    kmax = min(6 if nrow > 1 else 60, len(allowed))
    rows = []
    for i in range(nrow):
        if nrow >= 2 and i % 11 == 3:
            rows.append([])
            continue
        k = int(rng.integers(0, kmax + 1))
        rows.append([0] + np.sort(rng.choice(allowed, size=k, replace=False)).tolist())  # column 0: in every non-empty row
    if variant == "full":
        rows[nrow // 2] = list(range(ncol))
    return csr_from_columns(shape, rows, 73 + nrow, np.dtype(dtype_name).type)


def transpose_case(shape, variant, dtype):
    return _transpose_case(tuple(shape), variant, np.dtype(dtype).name)


def check_transpose_case(M, variant):
    """what the shape allows of: empty rows; empty columns, the last among them (holes); one column in every non-empty row;
    one full row (full).  A full row and an empty column exclude each other, hence the two variants."""
    nrow, ncol = M.shape
    lens = row_lengths(M)
    assert len(M.va) > 0 and is_sorted_unique(M)
    if nrow >= 2:
        assert (lens == 0).any()
    assert all(M.ci[M.rp[i]] == 0 for i in range(nrow) if lens[i] > 0)
    colcount = np.bincount(M.ci, minlength=ncol)
    assert colcount[0] == (lens > 0).sum()
    if variant == "holes" and ncol >= 3:
        assert colcount[ncol - 1] == 0 and (colcount[:ncol - 1] == 0).any()
    if variant == "full":
        assert lens.max() == ncol


def repeated_column_matrix(dtype):
    """a repeated column inside a row, two entries with different values (rows 1 and 3)"""
    M = csr_from_columns((5, 7), [[0, 2], [1, 3, 3, 6], [], [3, 3], [0, 3, 6]], 79, dtype)
    assert M.va[3] != M.va[4]
    return M


# ------------------------------------------------------------------------------------------------ MatrixAdd
ADD_SHAPE = (300, 450)
ADD_ALPHA, ADD_BETA = 1.5, -0.3
ADD_KINDS = ["only_a", "only_b", "neither", "identical", "disjoint", "interleaved", "both_last"]


@functools.lru_cache(maxsize=None)
def _add_union_case(dtype_name):
    nrow, ncol = ADD_SHAPE
    rng = np.random.default_rng(81)
    ra_, rb_ = [], []
    for i in range(nrow):
        kind = ADD_KINDS[i % len(ADD_KINDS)]
        k = int(rng.integers(1, 12))
        pick = lambda m, hi=ncol - 1: np.sort(rng.choice(hi, size=m, replace=False)).tolist()  # (never the last column)
        if kind == "only_a":
            a, b = pick(k), []
        elif kind == "only_b":
            a, b = [], pick(k)
        elif kind == "neither":
            a, b = [], []
        elif kind == "identical":
            a = pick(k)
            b = list(a)
        elif kind == "disjoint":  # all of A left of all of B
            c = pick(2 * k)
            a, b = c[:k], c[k:]
        elif kind == "interleaved":  # alternating, and a few shared columns
            c = pick(2 * k + 2)
            a, b = sorted(c[0::2] + c[-1:]), sorted(c[1::2] + c[:1])
        else:  # both_last
            a, b = pick(k) + [ncol - 1], pick(k) + [ncol - 1]
        ra_.append(a)
        rb_.append(b)
    dtype = np.dtype(dtype_name).type
    return csr_from_columns(ADD_SHAPE, ra_, 83, dtype), csr_from_columns(ADD_SHAPE, rb_, 85, dtype)


def add_union_case(dtype):
    return _add_union_case(np.dtype(dtype).name)


def check_add_union_case(A, B):
    assert A.shape == B.shape == ADD_SHAPE and is_sorted_unique(A) and is_sorted_unique(B)
    seen = set()
    for i in range(ADD_SHAPE[0]):
        a = A.ci[A.rp[i]:A.rp[i + 1]].tolist()
        b = B.ci[B.rp[i]:B.rp[i + 1]].tolist()
        sa, sb = set(a), set(b)
        if a and not b:
            seen.add("only_a")
        elif b and not a:
            seen.add("only_b")
        elif not a and not b:
            seen.add("neither")
        elif a == b:
            seen.add("identical")
        elif not (sa & sb) and (a[-1] < b[0] or b[-1] < a[0]):
            seen.add("disjoint")
        elif a[-1] == b[-1] == ADD_SHAPE[1] - 1:
            seen.add("both_last")
        elif (sa & sb) and (sa - sb) and (sb - sa):
            seen.add("interleaved")
    assert seen == set(ADD_KINDS), seen


@functools.lru_cache(maxsize=None)
def _add_subset_case(dtype_name):
    """-> (A, B): the pattern of B a strict subset of A's row by row, B empty in some rows, A empty in a few"""
    nrow, ncol = ADD_SHAPE
    rng = np.random.default_rng(87)
    ra_, rb_ = [], []
    for i in range(nrow):
        k = 0 if i % 13 == 6 else int(rng.integers(2, 14))
        a = np.sort(rng.choice(ncol, size=k, replace=False)).tolist()
        if i % 5 == 2 or not a:
            b = []
        else:
            m = int(rng.integers(1, len(a)))
            b = sorted(rng.choice(a, size=m, replace=False).tolist())
        ra_.append(a)
        rb_.append(b)
    dtype = np.dtype(dtype_name).type
    return csr_from_columns(ADD_SHAPE, ra_, 89, dtype), csr_from_columns(ADD_SHAPE, rb_, 91, dtype)


def add_subset_case(dtype):
    return _add_subset_case(np.dtype(dtype).name)


def subset_partner_mask(A, B):
    """per entry of A: does B hold that (row, column)?  Also checks the strict-subset property."""
    mask = np.zeros(len(A.ci), dtype=bool)
    empty_b = False
    for i in range(A.shape[0]):
        a = A.ci[A.rp[i]:A.rp[i + 1]]
        b = B.ci[B.rp[i]:B.rp[i + 1]]
        assert set(b.tolist()) <= set(a.tolist()) and (len(a) == 0 or len(b) < len(a))
        empty_b = empty_b or (len(a) > 0 and len(b) == 0)
        mask[A.rp[i]:A.rp[i + 1]] = np.isin(a, b)
    assert empty_b and mask.any() and not mask.all()
    return mask


# ------------------------------------------------------------------------------------------------ Sort
def sort_case(dtype):
    """-> (scrambled matrix, expected ci, expected va): 40 x 500, rows of 0, 1, 2, 64 and 300 entries permuted on the host,
    row 3 with a repeated column carrying two different values; expected = numpy's stable argsort per row"""
    lens = [0, 1, 2, 64, 300] * 8
    M = random_csr((40, 500), lens, 93, dtype)
    rng = np.random.default_rng(95)
    ci, va = M.ci.copy(), M.va.copy()
    ci[M.rp[3] + 10] = ci[M.rp[3] + 40]  # the repeat, 30 positions apart in storage
    assert va[M.rp[3] + 10] != va[M.rp[3] + 40]
    for i in range(40):
        p = rng.permutation(lens[i]) + M.rp[i]
        ci[M.rp[i]:M.rp[i + 1]] = ci[p]
        va[M.rp[i]:M.rp[i + 1]] = va[p]
    eci, eva = ci.copy(), va.copy()
    for i in range(40):
        s = slice(M.rp[i], M.rp[i + 1])
        o = np.argsort(ci[s], kind="stable")
        eci[s], eva[s] = ci[s][o], va[s][o]
    assert sorted(set(lens)) == [0, 1, 2, 64, 300] and not np.array_equal(ci, eci)
    r3 = eci[M.rp[3]:M.rp[4]]
    assert (np.diff(r3) == 0).sum() == 1
    return Csr(M.shape, M.rp, ci, va), eci, eva


# ------------------------------------------------------------------------------------------------ DiagonalMatrixMult
def diag_case(dtype):
    """-> (M 300 x 450 with empty rows, d_left[300], d_right[450])"""
    rng = np.random.default_rng(97)
    lens = rng.integers(0, 15, size=300).tolist()
    lens[0], lens[299] = 0, 450
    M = random_csr((300, 450), lens, 99, dtype)
    return M, rng.standard_normal(300).astype(dtype), rng.standard_normal(450).astype(dtype)
