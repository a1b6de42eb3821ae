"""Plain restatement of the aggregation-AMG setup (the local case: no ghost part), for the tests of
ramd_mat_amg_{pmis,greedy}_aggregate and ramd_mat_amg_{unsmoothed,smoothed}_prolong.  Scalar arithmetic in the operator's
value type, loops in the reference's order.  What it follows (the reference's host backend, src/base/host/host_matrix_csr.cpp):
    ExtractDiagonal :772-800                     AMGComputeStrongConnections :5098-5160
    AMGGreedyAggregate :4841-4938                AMGUnsmoothedAggregationProlongNnz / Fill :6331-6516
    AMGSmoothedAggregationProlongNnz / Fill :5936-6328
and the drivers src/base/local_matrix.cpp:6409-6511 (Greedy: the vectors come zero-filled from Allocate).  PMIS is not
restated here: oracle/pmis_pway.pmis_single is the restatement of it.  tests/test_cpu_amg_aggregation.py checks this module
against the goldens recorded from the genuine library (tests/golden/amg, tools/gen_golden_amg.py).

`greedy` is the SEQUENTIAL sweep, with its removed / undefined states, on purpose: the device computes the same arrays from
three order-free rules (seeds, largest neighbouring seed, smallest seed two hops away), and the tests hold that form
against the sweep."""
import numpy as np

UNDEFINED, REMOVED = -1, -2


def diagonal(rp, ci, va, dtype=np.float64):
    """:772-800 -- the first stored entry of the row's own column; zero where the row stores none"""
    n = len(rp) - 1
    d = np.zeros(n, dtype=dtype)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                d[i] = va[j]
                break
    return d


def connections(rp, ci, va, eps, dtype=np.float64):
    """:5098-5160 -- conn[j] = (c != i) and v*v > ((eps*eps) * d_i) * d_c, every product rounded to dtype -> int32 per entry"""
    T = np.dtype(dtype).type
    rp, ci = np.asarray(rp), np.asarray(ci)
    va = np.asarray(va, dtype=dtype)
    n = len(rp) - 1
    d = diagonal(rp, ci, va, dtype)
    eps2 = T(T(eps) * T(eps))
    rows = np.repeat(np.arange(n), np.diff(rp))
    with np.errstate(all="ignore"):
        eps_dia = (eps2 * d).astype(dtype)  # eps_dia_i, per row
        conn = (ci != rows) & ((va * va).astype(dtype) > (eps_dia[rows] * d[ci]).astype(dtype))
    return conn.astype(np.int32)


def greedy(rp, ci, conn, stats=None):
    """:4841-4938 -- the sweep in index order -> (aggregates, root nodes) int32.  stats (a dict) receives: removed (rows
    without a strong connection), seeds, tentative_owned (rows whose final owner claimed them tentatively),
    overwrites (direct claims on a row an earlier seed had claimed: of a tentative claim / of a direct one)"""
    n = len(rp) - 1
    rp, ci, conn = [int(v) for v in rp], [int(v) for v in ci], [bool(v) for v in conn]
    agg, roots = [0] * n, [0] * n  # (Allocate: zeros; a removed row's root entry is never written)
    how = [0] * n  # 0 unclaimed, 1 seed, 2 direct, 3 tentative
    over_t = over_d = 0
    for i in range(n):
        state = REMOVED
        for j in range(rp[i], rp[i + 1]):
            if conn[j]:
                state = UNDEFINED
                break
        agg[i] = state
    last_g = -1
    for i in range(n):
        if agg[i] != UNDEFINED:
            continue
        last_g += 1
        agg[i], roots[i], how[i] = last_g, i, 1
        neib = []
        for j in range(rp[i], rp[i + 1]):
            c = ci[j]
            if conn[j] and agg[c] != REMOVED:
                if how[c] == 3:
                    over_t += 1
                elif how[c] == 2 and roots[c] != i:
                    over_d += 1
                agg[c], roots[c], how[c] = last_g, i, 2
                neib.append(c)
        for nb in neib:
            for j in range(rp[nb], rp[nb + 1]):
                c = ci[j]
                if conn[j] and agg[c] == UNDEFINED:
                    agg[c], roots[c], how[c] = last_g, i, 3
    if stats is not None:
        stats.update(removed=sum(1 for a in agg if a == REMOVED), seeds=last_g + 1,
                     tentative_owned=sum(1 for h in how if h == 3), overwrites_of_tentative=over_t,
                     overwrites_of_direct=over_d, overwrites=over_t + over_d)
    return np.array(agg, dtype=np.int32), np.array(roots, dtype=np.int32)


def _f2c(n, agg, roots, marked):
    f2c = np.zeros(n + 1, dtype=np.int64)
    f2c[list(marked)] = 1
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(f2c)[:-1]  # ExclusiveSum
    return out


def ua_prolong(agg, roots, dtype=np.float64):
    """:6331-6516 -- one entry 1 per aggregated row, at the rank of the aggregate's root node among the root nodes in use
    -> (rowptr int32, col int32, val dtype, ncol)"""
    n = len(agg)
    live = [i for i in range(n) if agg[i] >= 0]
    f2c = _f2c(n, agg, roots, {int(roots[i]) for i in live})
    rp = np.zeros(n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.asarray(agg) >= 0)
    ci = np.array([f2c[roots[i]] for i in live], dtype=np.int32)
    return rp, ci, np.ones(len(live), dtype=dtype), int(f2c[n])


def sa_prolong(rp, ci, va, conn, agg, roots, relax, lumping, dtype=np.float64, stats=None, stable=True):
    """:5936-6328 -- row i of (I - relax D_f^-1 A_f) P_tent -> (rowptr int32, col int32, val dtype, ncol).  The lumped
    diagonal: the stored diagonal entries plus (lumping 0) or minus (1) the weak off-diagonal ones, in row order; the row's
    contributions (1 - relax from the diagonal entry, ((-relax) * (1/dia)) * a_ij from a strong one) are keyed by the root node
    of the neighbour's aggregate, equal keys add in row order (std::map: the first one assigns), keys leave ascending;
    neighbours outside every aggregate are left out.  stats receives max_same_key (the most entries of one row under one
    key) and nonfinite (values that are no finite number).  stable=False adds equal keys in REVERSE row order -- what a sort
    that is not stable may do; only for checking that a test tells the two apart."""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    va = np.asarray(va, dtype=dtype)
    relax, one, zero = T(relax), T(1), T(0)
    tables, marked, most = [], set(), 0
    with np.errstate(all="ignore"):
        for i in range(n):
            dia = zero
            for j in range(rp[i], rp[i + 1]):
                if ci[j] == i:
                    dia = T(dia + va[j])
                elif not conn[j]:
                    dia = T(dia + va[j]) if lumping == 0 else T(dia - va[j])
            dia = T(one / dia)
            parts = {}
            for j in range(rp[i], rp[i + 1]):
                c = int(ci[j])
                if c != i and not conn[j]:
                    continue
                if agg[c] < 0:
                    continue
                v = T(one - relax) if c == i else T(T(T(-relax) * dia) * va[j])
                parts.setdefault(int(roots[c]), []).append(v)
            table = {}
            for key, vs in parts.items():
                most = max(most, len(vs))
                acc = None
                for v in (vs if stable else vs[::-1]):
                    acc = v if acc is None else T(acc + v)
                table[key] = acc
            marked.update(table)
            tables.append(table)
    f2c = _f2c(n, agg, roots, marked)
    prp, pci, pval = [0], [], []
    for table in tables:
        for key in sorted(table):
            pci.append(f2c[key]); pval.append(table[key])
        prp.append(len(pci))
    pval = np.array(pval, dtype=dtype)
    if stats is not None:
        stats.update(max_same_key=most, nonfinite=int(np.sum(~np.isfinite(pval))))
    return np.array(prp, dtype=np.int32), np.array(pci, dtype=np.int32), pval, int(f2c[n])


def chain(n, dtype=np.float64):
    """the 1-D chain of n rows: (-1, 2, -1)"""
    rp = np.zeros(n + 1, dtype=np.int32)
    cnt = np.full(n, 3, dtype=np.int64)
    if n:
        cnt[0] -= 1; cnt[-1] -= 1
    rp[1:] = np.cumsum(cnt)
    ci = np.empty(rp[-1], dtype=np.int32)
    va = np.empty(rp[-1], dtype=dtype)
    i = np.arange(n)
    ci[rp[:-1] + (i > 0)], va[rp[:-1] + (i > 0)] = i, 2.0
    ci[rp[1:][i < n - 1] - 1], va[rp[1:][i < n - 1] - 1] = i[i < n - 1] + 1, -1.0
    ci[rp[:-1][i > 0]], va[rp[:-1][i > 0]] = i[i > 0] - 1, -1.0
    return rp, ci, va


def chain_greedy(n):
    """the sweep's result on the chain in closed form: seeds at 0, 3, 6, ...; agg[i] = (i + 1) // 3, the seed next to row i
    (seed 3k takes row 3k - 1 back from seed 3k - 3, which held it tentatively); when n % 3 == 0 the last row lies two hops
    past the last seed and stays with it, claimed tentatively; n = 1 has no strong connection at all
    -> (aggregates, root nodes) int32"""
    i = np.arange(n, dtype=np.int64)
    if n == 1:
        return np.array([REMOVED], dtype=np.int32), np.array([0], dtype=np.int32)
    agg = (i + 1) // 3
    nseeds = (n + 2) // 3  # seeds 0, 3, ..., 3 (nseeds - 1) <= n - 1
    agg = np.minimum(agg, nseeds - 1)  # the last row when n % 3 == 0: no seed at n, it stays with seed n - 3
    return agg.astype(np.int32), (3 * agg).astype(np.int32)


# ---- which branches the operators of tests/golden/amg take (tools/gen_golden_amg.py prints these; the CPU test recomputes them)
def conn_symmetric(rp, ci, conn):
    strong = {(i, int(ci[j])) for i in range(len(rp) - 1) for j in range(rp[i], rp[i + 1]) if conn[j]}
    return all((j, i) in strong for (i, j) in strong)


def branch_counts(d):
    """the counts that show which branches an operator of tests/golden/amg takes, from its recorded arrays alone"""
    rp, ci, va, conn = d["rowptr"], d["col"], d["val"], d["conn"]
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    st, sa = {}, {}
    greedy(rp, ci, conn, st)
    sa_prolong(rp, ci, va, conn, d["greedy_agg"], d["greedy_roots"], 2.0 / 3.0, 0, np.float64, sa)
    diag_rows = set(rows[ci == rows].tolist())
    return dict(rows=n, max_row=int(np.diff(rp).max()), min_row=int(np.diff(rp).min()), strong=int(conn.sum()),
                removed=st["removed"], seeds=st["seeds"], tentative_owned=st["tentative_owned"],
                overwrites=st["overwrites"], unsorted_rows=int(sum(1 for i in range(n) if np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0))),
                no_diagonal=n - len(diag_rows), max_same_key=sa["max_same_key"], nonfinite=sa["nonfinite"],
                conn_symmetric=int(conn_symmetric(rp, ci, conn)),
                strong_to_unaggregated=int(np.sum((conn == 1) & (d["pmis_agg"][ci] < 0))))


NEEDS = {"path9": ["tentative_owned", "overwrites"], "diag40": ["removed"], "irr_sym": ["tentative_owned", "overwrites"],
         "irr_sym_rev": ["unsorted_rows", "tentative_owned", "overwrites"], "weakmix": ["removed", "no_diagonal", "nonfinite", "seeds"],
         "hub": ["overwrites"], "unsym": ["strong_to_unaggregated"], "level2": ["seeds"]}


def check_counts(name, c):
    for k in NEEDS[name]:
        assert c[k] > 0, (name, k, c)
    assert c["conn_symmetric"] == (0 if name == "unsym" else 1), (name, c)
    if name == "diag40":
        assert c["removed"] == c["rows"] and c["strong"] == 0
    if name in ("irr_sym", "irr_sym_rev", "hub", "level2"):
        assert c["max_same_key"] >= 3, (name, c)  # (two equal keys add to the same sum in either order)
    if name == "hub":
        assert c["max_row"] >= 500 and c["max_same_key"] >= 100, c
    if name == "weakmix":
        assert c["removed"] < c["rows"]
    if name == "level2":
        assert c["max_row"] >= 40


def irregular_sym(n, seed):
    """a seeded irregular operator, symmetric in values and pattern: rows of very different length (row 0 is a hub once
    n >= 64), strong couplings of both signs and weak ones (1e-3 of a strong one, far from the threshold in either value
    type), ascending columns"""
    rng = np.random.default_rng(seed)
    e = {(i, i): float(rng.uniform(3.0, 5.0)) for i in range(n)}
    for i in range(n):
        for j in rng.integers(0, n, size=int(rng.integers(0, 7))):
            j = int(j)
            if j != i and (i, j) not in e:
                v = float(rng.uniform(0.5, 1.5)) * (1.0 if rng.random() < 0.3 else -1.0) * (1e-3 if rng.random() < 0.25 else 1.0)
                e[(i, j)] = e[(j, i)] = v
    if n >= 64:
        for j in range(3, n, 5):
            e[(0, j)] = e[(j, 0)] = -float(rng.uniform(0.5, 1.5))
    rows = [[] for _ in range(n)]
    for (i, j), v in e.items():
        rows[i].append((j, v))
    rp, ci, va = [0], [], []
    for r in rows:
        for j, v in sorted(r):
            ci.append(j); va.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)
