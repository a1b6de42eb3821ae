"""The aggregation-AMG setup on the device -- AMGPMISAggregate, AMGGreedyAggregate, AMGUnsmoothedAggregation,
AMGSmoothedAggregation through the Python wrappers -- against the genuine library's arrays (tests/golden/amg, recorded by
tools/gen_golden_amg.py) and, where no golden exists, against the plain restatement that tests/test_cpu_amg_aggregation.py
pins to those goldens (tests/_amg_ref.py; oracle/pmis_pway.pmis_single for PMIS).  Every comparison is exact: integer
arrays equal, values bit for bit (a NaN equal to a NaN: its sign and payload are not results -- weakmix has some, where
infinities of both signs meet under one key)."""
import functools
import time

import numpy as np
import pytest

import _amg_ref as ref
from conftest import load_golden
from oracle.pmis_pway import pmis_single

pytestmark = pytest.mark.gpu

NAMES = ["path9", "diag40", "irr_sym", "irr_sym_rev", "weakmix", "hub", "unsym", "level2"]
EPS = 0.01
SA = (("sa0", 2.0 / 3.0, 0), ("sa1", 0.5, 1))
EDGE_N = [1, 2, 255, 256, 257, 511, 513]


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


def load(name):
    return load_golden("amg/" + name)


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a, b), "%d of %d differ, first at %d" % (np.sum(a != b), a.size, np.flatnonzero(a != b)[0])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert a[~nan].tobytes() == b[~nan].tobytes(), "%d of %d values differ" % (np.sum(a[~nan] != b[~nan]), a.size)


def _mat(ra, rp, ci, va, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(rp, ci, np.asarray(va).astype(dtype))
    return A


def _same_P(P, want):
    """want: (rowptr, col, val, ncol)"""
    rp, ci, va = P.CopyToCSR()
    eq(rp, want[0]); eq(ci, want[1]); same_bits(va, want[2])
    assert (P.GetM(), P.GetN(), P.GetNnz()) == (len(want[0]) - 1, want[3], len(want[1]))


def _golden_P(g, key, val_key=None):
    return g[key + "_rowptr"], g[key + "_col"], g[val_key or key + "_val"], int(g[key + "_shape"][1])


def _prolongators(ra, A, conn, agg, roots, want_ua, want_sa):
    P = ra.LocalMatrix(A.dtype)
    A.AMGUnsmoothedAggregation(agg, roots, P)
    _same_P(P, want_ua)
    for (key, relax, lump), want in zip(SA, want_sa):
        Ps = ra.LocalMatrix(A.dtype)
        A.AMGSmoothedAggregation(relax, conn, agg, roots, Ps, lump)
        _same_P(Ps, want)


def _refused(ra, A):
    """Greedy on an unsymmetric strong graph: refused with the agreed status and text, nothing else happens"""
    from rocalution_amd import capi
    with pytest.raises(capi.RamdError, match="not symmetric") as err:
        A.AMGGreedyAggregate(EPS)
    assert err.value.status == capi.ERR_UNSUPPORTED


# ---------------------------------------------------------------- more workgroups than the device holds at once
def test_greedy_beyond_residency(ra):
    """the sync-free seed sweep with 2344 workgroups of 256 rows -- the device holds 2048 of them at once, so the last ones
    start only when earlier ones have left, and the ticket order is what keeps every awaited row resident or done: the
    1-D chain of 600001 rows, about n/3 hand-offs in sequence, against the closed form that test_cpu_amg_aggregation pins
    to the sequential sweep; then the unsmoothed prolongator of it"""
    n = 600001
    rp, ci, va = ref.chain(n)
    A = _mat(ra, rp, ci, va)
    t0 = time.perf_counter()
    conn, agg, roots = A.AMGGreedyAggregate(EPS)
    got = agg.numpy()
    print("AMGGreedyAggregate, chain of %d rows (%d workgroups): %.3f s" % (n, (n + 255) // 256, time.perf_counter() - t0))
    want_agg, want_roots = ref.chain_greedy(n)
    eq(conn.numpy(), (ci != np.repeat(np.arange(n), np.diff(rp))).astype(np.int32))
    eq(got, want_agg); eq(roots.numpy(), want_roots)
    P = ra.LocalMatrix()
    A.AMGUnsmoothedAggregation(agg, roots, P)
    _same_P(P, ref.ua_prolong(want_agg, want_roots))
    assert P.GetN() == (n + 2) // 3


# ---------------------------------------------------------------- the library's arrays
@pytest.mark.parametrize("name", NAMES)
def test_all_four_entries_vs_golden(ra, name):
    g = load(name)
    for dt, sfx in ((np.float64, ""), (np.float32, "_f32")):
        A = _mat(ra, g["rowptr"], g["col"], g["val"], dt)
        for m in ("pmis", "greedy"):
            if m == "greedy" and name == "unsym":
                _refused(ra, A)
                continue
            conn, agg, roots = A.AMGPMISAggregate(EPS) if m == "pmis" else A.AMGGreedyAggregate(EPS)
            eq(conn.numpy(), g["conn"]); eq(agg.numpy(), g[m + "_agg"]); eq(roots.numpy(), g[m + "_roots"])
            ua = _golden_P(g, "ua_" + m)
            _prolongators(ra, A, conn, agg, roots, ua[:2] + (ua[2].astype(dt),) + ua[3:],
                          [_golden_P(g, "%s_%s" % (key, m), "%s_%s%s_val" % (key, m, sfx)) for key, _, _ in SA])


def test_unsymmetric_strong_graph_refuse_and_go_on(ra):
    g = load("unsym")
    assert not ref.conn_symmetric(g["rowptr"], g["col"], g["conn"])
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    _refused(ra, A)
    conn, agg, roots = A.AMGPMISAggregate(EPS)  # the same matrix, the next call: exact
    eq(conn.numpy(), g["conn"]); eq(agg.numpy(), g["pmis_agg"]); eq(roots.numpy(), g["pmis_roots"])
    _refused(ra, A)  # ... and it refuses again: no state left behind
    s = load("irr_sym")  # Greedy on another matrix afterwards
    conn, agg, roots = _mat(ra, s["rowptr"], s["col"], s["val"]).AMGGreedyAggregate(EPS)
    eq(conn.numpy(), s["conn"]); eq(agg.numpy(), s["greedy_agg"]); eq(roots.numpy(), s["greedy_roots"])


def test_no_strong_connection_gives_an_empty_prolongator(ra):
    g = load("diag40")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    for call in (A.AMGGreedyAggregate, A.AMGPMISAggregate):
        conn, agg, roots = call(EPS)
        eq(conn.numpy(), np.zeros(40, np.int32)); eq(agg.numpy(), np.full(40, -2, np.int32))
        for build in (lambda P: A.AMGUnsmoothedAggregation(agg, roots, P),
                      lambda P: A.AMGSmoothedAggregation(2.0 / 3.0, conn, agg, roots, P, 0)):
            P = ra.LocalMatrix()
            build(P)
            assert (P.GetM(), P.GetNnz(), P.GetN()) == (40, 0, int(g["ua_greedy_shape"][1])) and P.GetN() == 0
            rp, ci, va = P.CopyToCSR()
            eq(rp, np.zeros(41, np.int32))
            assert len(ci) == 0 and len(va) == 0
    p = load("path9")  # a following aggregation on another matrix is unaffected
    B = _mat(ra, p["rowptr"], p["col"], p["val"])
    conn, agg, roots = B.AMGGreedyAggregate(EPS)
    eq(agg.numpy(), p["greedy_agg"]); eq(roots.numpy(), p["greedy_roots"])
    _prolongators(ra, B, conn, agg, roots, _golden_P(p, "ua_greedy"), [_golden_P(p, k + "_greedy") for k, _, _ in SA])


# ---------------------------------------------------------------- block edges: n around the multiples of 256
@functools.lru_cache(maxsize=None)
def _edge_case(kind, n):
    """the operator and everything the restatement says about it, computed once"""
    rp, ci, va = ref.chain(n) if kind == "chain" else ref.irregular_sym(n, n)
    out = {"A": (rp, ci, va)}
    for dt in (np.float64, np.float32):
        conn = ref.connections(rp, ci, va, EPS, dt)
        assert ref.conn_symmetric(rp, ci, conn)
        pconn, pagg, proots = pmis_single(rp, ci, va.astype(dt).astype(np.float64), EPS)
        eq(pconn, conn)  # (far from the threshold: the same graph in either value type)
        res = {"conn": conn}
        for m, (agg, roots) in (("greedy", ref.greedy(rp, ci, conn)), ("pmis", (pagg, proots))):
            res[m] = (agg, roots, ref.ua_prolong(agg, roots, dt),
                      [ref.sa_prolong(rp, ci, va, conn, agg, roots, relax, lump, dt) for _, relax, lump in SA])
        out[np.dtype(dt).name] = res
    return out


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("kind", ["chain", "irregular"])
def test_block_edges_vs_restatement(ra, kind, n):
    case = _edge_case(kind, n)
    rp, ci, va = case["A"]
    for dt in (np.float64, np.float32):
        want = case[np.dtype(dt).name]
        A = _mat(ra, rp, ci, va, dt)
        for m in ("greedy", "pmis"):
            conn, agg, roots = A.AMGGreedyAggregate(EPS) if m == "greedy" else A.AMGPMISAggregate(EPS)
            wagg, wroots, wua, wsa = want[m]
            eq(conn.numpy(), want["conn"]); eq(agg.numpy(), wagg); eq(roots.numpy(), wroots)
            _prolongators(ra, A, conn, agg, roots, wua, wsa)
    if kind == "chain":
        eq(case["float64"]["greedy"][0], ref.chain_greedy(n)[0])


# ---------------------------------------------------------------- every level of a hierarchy, each on its own operator
def _start(ra, which):
    if which == "poisson16":
        from rocalution_amd import generators as gen
        return gen.poisson7(16, np.float64)
    g = load_golden("lap27_6")
    return g["rowptr"], g["col"], g["val"]


@pytest.mark.parametrize("strategy", ["greedy", "pmis"])
@pytest.mark.parametrize("which", ["poisson16", "lap27_6"])
def test_hierarchy_walk_level_by_level(ra, which, strategy):
    """aggregate, smoothed prolongator, A1 = P^T A P with the device's Transpose / MatrixMult, again, down to 20 rows; at
    every level the device's arrays against the restatement applied to the device's OWN operator of that level, copied
    back: errors do not compound, and every level below the first is an irregular, dense Galerkin operator"""
    rp, ci, va = _start(ra, which)
    A = _mat(ra, rp, ci, va)
    level, switched = 0, []
    while A.GetM() > 20 and level < 12:
        rp, ci, va = A.CopyToCSR()
        n = len(rp) - 1
        wconn = ref.connections(rp, ci, va, EPS)
        use = strategy
        if use == "greedy" and not ref.conn_symmetric(rp, ci, wconn):
            # a Galerkin operator symmetric only up to rounding: the strong graph may lose one direction of a pair
            _refused(ra, A)
            switched.append(level)
            print("%s: level %d (%d rows): strong graph not symmetric, Greedy refused -- this level goes on with PMIS"
                  % (which, level, n))
            use = "pmis"
        if use == "greedy":
            conn, agg, roots = A.AMGGreedyAggregate(EPS)
            wagg, wroots = ref.greedy(rp, ci, wconn)
        else:
            conn, agg, roots = A.AMGPMISAggregate(EPS)
            pconn, wagg, wroots = pmis_single(rp, ci, va, EPS)
            eq(pconn, wconn)
        eq(conn.numpy(), wconn); eq(agg.numpy(), wagg); eq(roots.numpy(), wroots)
        P = ra.LocalMatrix()
        A.AMGSmoothedAggregation(2.0 / 3.0, conn, agg, roots, P, 0)
        want = ref.sa_prolong(rp, ci, va, wconn, wagg, wroots, 2.0 / 3.0, 0)
        _same_P(P, want)
        print("%s/%s level %d: %d rows, %d entries (longest row %d) -> %d aggregates" % (
            which, strategy, level, n, len(ci), int(np.diff(rp).max()), want[3]))
        if want[3] == 0 or want[3] >= n:
            break
        R, A1 = ra.LocalMatrix(), ra.LocalMatrix()
        P.Transpose(R)
        A1.TripleMatrixProduct(R, A, P)
        assert (A1.GetM(), A1.GetN()) == (want[3], want[3])
        A, level = A1, level + 1
    assert level >= 1 and A.GetM() <= 20, (level, A.GetM())  # (poisson16: three levels, two of them Galerkin operators)
    if switched:
        print("%s/%s: Greedy refused at level(s) %s" % (which, strategy, switched))
