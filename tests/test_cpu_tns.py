"""TNS without a GPU: the class compiles in a reference-style driver, and the numpy reference that the GPU tests are held
against (tests/_tns_ref.py) is itself checked against a dense M^-1."""
import os
import subprocess

import numpy as np

import _tns_ref as T
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tns_driver_compiles_and_links_with_plain_gxx(tmp_path):
    """TNS<LocalMatrix<T>, LocalVector<T>, T> for double and float inside CG, the way a driver written for the reference says
    it: compiled with plain g++ and linked against the library, so every ramd_tns_* symbol the class uses has to be exported
    (running it needs the accelerator)"""
    from rocalution_amd import capi
    capi.load()  # builds the library if it is not there yet
    exe = str(tmp_path / "tns_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "tns_driver.cpp"), "-o", exe, capi.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(capi.LIB_PATH)])
    assert os.path.exists(exe)


def test_numpy_reference_against_a_dense_inverse_operator():
    g = load_golden("poisson8")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    A = T.csr_to_dense(rp, ci, va)
    Minv = T.dense_inverse_operator(A)
    assert np.array_equal(Minv, Minv.T) or np.allclose(Minv, Minv.T, rtol=0, atol=1e-15)  # the operator is symmetric
    rng = np.random.default_rng(7)
    for _ in range(3):
        r = rng.uniform(-1.0, 1.0, n)
        x = T.tns_apply(rp, ci, va, r)
        ref = Minv @ r
        # the dense evaluation is a float64 product of rows of 512: its own error bounds the difference
        assert np.max(np.abs(x.astype(np.float64) - ref)) <= 512 * 2.0 ** -53 * np.max(np.abs(Minv) @ np.abs(r))
        # ... and the bound's x-bar dominates |x|
        assert np.all(T.tns_apply(rp, ci, va, r, absolute=True) >= np.abs(x))
    assert T.longest_triangle_row(rp, ci) == 3
    assert T.is_bitwise_symmetric(rp, ci, va) == (True, True)


def test_numpy_reference_inverse_diagonal_rules_and_synthetic_fixtures():
    rp, ci, va = T.sym_diagonal_holes()
    n = len(rp) - 1
    d = T.inverse_diagonal(rp, ci, va, np.float64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    stored = np.zeros(n, dtype=bool)
    stored[rows[ci == rows]] = True
    assert np.all(d[~stored] == 0.0) and (~stored).sum() > 0  # no stored diagonal: 0
    zero = stored.copy()
    zero[rows[ci == rows]] = va[ci == rows] == 0.0
    assert np.all(d[zero] == 1.0) and zero.sum() > 0  # stored as zero: 1
    assert T.is_bitwise_symmetric(rp, ci, va) == (True, True)
    assert T.is_bitwise_symmetric(*T.structurally_symmetric_only()) == (True, False)
    rp, ci, va = T.sym_arrow()
    assert T.is_bitwise_symmetric(rp, ci, va) == (True, True) and T.longest_triangle_row(rp, ci) >= 2600
    assert rp[1] - rp[0] >= 2601 and rp[-1] - rp[-2] >= 2601


def test_numpy_krylov_runs_converge_with_tns():
    """the fixtures' choice of tests/test_gpu_tns.py: every numpy run converges by the relative tolerance"""
    from rocalution_amd import generators as gen
    g27, gr = load_golden("lap27_6"), load_golden("rand300")
    cases = [(T.cg, gen.poisson7(16), {}), (T.cg, (g27["rowptr"], g27["col"], g27["val"]), {}),
             (T.gmres, (gr["rowptr"], gr["col"], gr["val"]), dict(basis=30)), (T.bicgstab, (gr["rowptr"], gr["col"], gr["val"]), {})]
    for solver, (rp, ci, va), kw in cases:
        A = lambda v: T.csr_matvec(rp, ci, va, v)
        M = lambda v: T.tns_apply(rp, ci, va, v).astype(np.float64)
        n = len(rp) - 1
        it, st, x, hist = solver(A, M, A(np.ones(n)), **kw)
        assert st == 2 and it < 60 and np.linalg.norm(x - 1.0) / np.sqrt(n) < 1e-5
