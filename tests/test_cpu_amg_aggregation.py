"""Aggregation-AMG setup, the part that needs no GPU: the plain restatement (tests/_amg_ref.py, and oracle/pmis_pway.py for
PMIS) reproduces every array the genuine library returned -- tests/golden/amg/*.npz (tools/gen_golden_amg.py) and the amg_*
arrays of tests/golden/{gr3030,poisson8,lap2d7}.npz -- with no mismatch: integers equal, values byte for byte.  The GPU
tests then use the restatement where no golden exists."""
import os

import numpy as np
import pytest

import _amg_ref as ref
from conftest import load_golden
from oracle.pmis_pway import pmis_single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["path9", "diag40", "irr_sym", "irr_sym_rev", "weakmix", "hub", "unsym", "level2"]
EPS = 0.01
SA = (("sa0", 2.0 / 3.0, 0), ("sa1", 0.5, 1))


def load(name):
    return load_golden(os.path.join("amg", name))


def same_ints(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), "%d mismatches" % np.sum(a != b) if a.shape == b.shape else (a.shape, b.shape)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%d of %d values differ" % (np.sum(a.view(np.uint8) != b.view(np.uint8)), a.size)


def same_csr(got, g, key, val_key=None):
    rp, ci, va, ncol = got
    same_ints(rp, g[key + "_rowptr"]); same_ints(ci, g[key + "_col"]); same_bytes(va, g[val_key or key + "_val"])
    assert list(g[key + "_shape"]) == [len(rp) - 1, ncol, len(ci)]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_library(name):
    g = load(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    for dt in (np.float64, np.float32):  # (the generator checked: the fp32 run gives the same integers)
        same_ints(ref.connections(rp, ci, va, EPS, dt), g["conn"])
    conn = g["conn"]
    agg, roots = ref.greedy(rp, ci, conn)
    same_ints(agg, g["greedy_agg"]); same_ints(roots, g["greedy_roots"])
    pconn, pagg, proots = pmis_single(rp, ci, va, EPS)
    same_ints(pconn, conn); same_ints(pagg, g["pmis_agg"]); same_ints(proots, g["pmis_roots"])
    for m in ("greedy", "pmis"):
        a, r = g[m + "_agg"], g[m + "_roots"]
        same_csr(ref.ua_prolong(a, r), g, "ua_" + m)
        for key, relax, lump in SA:
            same_csr(ref.sa_prolong(rp, ci, va, conn, a, r, relax, lump, np.float64), g, "%s_%s" % (key, m))
            same_csr(ref.sa_prolong(rp, ci, va, conn, a, r, relax, lump, np.float32), g, "%s_%s" % (key, m),
                     "%s_%s_f32_val" % (key, m))


@pytest.mark.parametrize("name", ["gr3030", "poisson8", "lap2d7"])
def test_restatement_reproduces_the_first_goldens(name):
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    conn = ref.connections(rp, ci, va, EPS)
    same_ints(conn, g["amg_conn"])
    agg, roots = ref.greedy(rp, ci, conn)
    same_ints(agg, g["amg_gagg"]); same_ints(roots, g["amg_groots"])
    _, pagg, proots = pmis_single(rp, ci, va, EPS)
    same_ints(pagg, g["amg_agg"]); same_ints(proots, g["amg_roots"])
    urp, uci, uva, ncol = ref.ua_prolong(pagg, proots)
    same_ints(urp, g["amg_P_rowptr"]); same_ints(uci, g["amg_P_col"]); same_bytes(uva, g["amg_P_val"])
    assert ncol == int(g["amg_P_col"].max()) + 1
    for key, relax, lump in (("amg_Ps", 2.0 / 3.0, 0), ("amg_Ps1", 0.5, 1)):
        srp, sci, sva, _ = ref.sa_prolong(rp, ci, va, conn, pagg, proots, relax, lump)
        same_ints(srp, g[key + "_rowptr"]); same_ints(sci, g[key + "_col"]); same_bytes(sva, g[key + "_val"])


@pytest.mark.parametrize("name", NAMES)
def test_every_operator_takes_its_branch(name):
    """removed rows, rows owned through a tentative claim, overwriting direct claims, unsorted rows, rows without a
    diagonal, many terms under one key, values that are not finite, an unsymmetric strong graph: recomputed here"""
    g = load(name)
    c = ref.branch_counts(g)
    print(name, c)
    ref.check_counts(name, c)
    if name == "diag40":
        assert np.all(g["greedy_agg"] == -2) and np.all(g["pmis_agg"] == -2)
        for p in ("ua_greedy", "ua_pmis", "sa0_greedy", "sa1_pmis"):
            assert list(g[p + "_shape"]) == [40, 0, 0] and len(g[p + "_col"]) == 0
    if name == "irr_sym_rev":  # same operator, other storage order: same aggregates; the sums of the smoothed P differ
        s = load("irr_sym")
        same_ints(g["greedy_agg"], s["greedy_agg"]); same_ints(g["sa0_greedy_col"], s["sa0_greedy_col"])
        assert g["sa0_greedy_val"].tobytes() != s["sa0_greedy_val"].tobytes()
    if name in ("irr_sym", "hub"):  # equal keys added in another order give other bits: the goldens can tell
        got = ref.sa_prolong(g["rowptr"], g["col"], g["val"], g["conn"], g["greedy_agg"], g["greedy_roots"], 2.0 / 3.0, 0,
                             stable=False)
        assert got[2].tobytes() != g["sa0_greedy_val"].tobytes()


@pytest.mark.parametrize("n", list(range(1, 41)) + [255, 256, 257, 3001])
def test_greedy_on_the_chain_in_closed_form(n):
    rp, ci, va = ref.chain(n)
    assert len(rp) == n + 1 and rp[-1] == len(ci) == max(3 * n - 2, 1)
    agg, roots = ref.greedy(rp, ci, ref.connections(rp, ci, va, EPS))
    cagg, croots = ref.chain_greedy(n)
    same_ints(agg, cagg); same_ints(roots, croots)
    if n > 1:
        i = np.arange(n)
        seeds = np.flatnonzero(roots == i)
        assert list(seeds) == list(range(0, n, 3))
        want = (i + 1) // 3
        if n % 3 == 0:
            want[-1] -= 1  # the last row, two hops past the last seed: a tentative claim nobody takes back
        same_ints(agg, want)
