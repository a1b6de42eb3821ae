"""BlockPreconditioner / VariablePreconditioner, the parts that need no GPU: the ABI tables, the Python argument checks, the
reference-style driver and a Global instantiation compiling against the headers, and the plain restatement
(tests/_blockprec_ref.py) against a dense computation."""
import os
import re
import subprocess

import numpy as np
import pytest

import _blockprec_ref as ref
from _schwarz_ref import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BP_ENTRIES = ["ramd_bp_build", "ramd_bp_local", "ramd_bp_step", "ramd_bp_join", "ramd_bp_info", "ramd_bp_piece_cap", "ramd_bp_destroy",
              "ramd_solver_set_precond_blocks", "ramd_solver_set_precond_perm", "ramd_solver_set_precond_params",
              "ramd_solver_set_precond_form", "ramd_solver_set_precond_local_params", "ramd_solver_precond_info"]


def test_bp_entries_are_in_the_header_the_table_and_the_library():
    from rocalution_amd import build, capi
    lib = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    exported = set(re.findall(r" T (ramd_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "rocalution_amd.h")).read()
    for name in BP_ENTRIES:
        assert name in exported and name in capi.SIGNATURES and name not in capi.OPTIONAL and re.search(r"\b%s\(" % name, hdr), name
    assert capi.PC_BLOCK == 20 and "RAMD_PC_BLOCK = 20" in hdr and "15 and 19 are not assigned" in hdr
    kinds = {k: v for k, v in vars(capi).items() if k.startswith("PC_")}
    assert 15 not in kinds.values() and 19 not in kinds.values() and len(set(kinds.values())) == len(kinds)


def test_python_objects_check_their_arguments():
    from rocalution_amd import solvers as S
    p = S.BlockPreconditioner([3, 4, 5], S.ILU())
    assert p.kind == S.PC_BLOCK and p.params == (0.0, 0.0, float(S.PC_ILU0)) and p.local_params is None and p.form == -1
    assert S.BlockPreconditioner([7], diagonal=True).params == (1.0, 0.0, float(S.PC_JACOBI))
    p.SetDiagonalSolver()
    assert p.params[0] == 1.0
    p.SetLSolver()
    assert p.params[0] == 0.0
    ilu1 = S.ILU(); ilu1.Set(1)
    assert S.BlockPreconditioner([2, 2], ilu1).local_params == (1.0, 1.0, 0.0)
    mc = S.MultiColoredILU(); mc.SetPrecondMatrixFormat(6)
    d = S.SGS(); d.SetSolverDescriptor(S.SolverDescr())
    for local in (mc, d, S.TNS(impl=False), S.SAAMG(), S.RugeStuebenAMG(), S.MultiElimination(), S.AS(), p):
        with pytest.raises(ValueError):
            S.BlockPreconditioner([3, 3], local)
    for bad in ([], [3, 0], [-1, 4]):
        with pytest.raises(ValueError):
            S.BlockPreconditioner(bad)
    for form in (2, -2):
        with pytest.raises(ValueError):
            p.SetForm(form)
    perm = np.random.default_rng(3).permutation(12)
    assert np.array_equal(S.BlockPreconditioner([3, 4, 5], perm=perm).perm, perm)
    for bad in (np.arange(11), np.zeros(12, int), np.arange(12) + 1, np.arange(12.0), np.arange(12).reshape(3, 4)):
        with pytest.raises(ValueError):
            S.BlockPreconditioner([3, 4, 5], perm=bad)


def _compile(src, exe):
    from rocalution_amd import build
    build.build()
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])


def test_blockprec_driver_compiles_with_a_plain_host_compiler(tmp_path):
    exe = str(tmp_path / "blockprec_driver")
    path = os.path.join(ROOT, "tests", "drivers", "blockprec_driver.cpp")
    _compile(path, exe)
    assert os.path.exists(exe)
    src = open(path).read()
    assert "BlockPreconditioner<Mat, Vec, double>" in src and "bp.Set(3, sz, list)" in src
    assert "VariablePreconditioner<Mat, Vec, double>" in src and "vp.SetPreconditioner(3, list)" in src


GLOBAL_PROGRAM = r"""
#include <rocalution/rocalution.hpp>
using namespace rocalution;
typedef GlobalMatrix<double> GM;
typedef GlobalVector<double> GV;
int main()
{
    BlockPreconditioner<GM, GV, double> bp; // compiles: the classes exist for Global types
    VariablePreconditioner<GM, GV, double> vp;
    Jacobi<GM, GV, double> j;
    Solver<GM, GV, double>* list[1] = {&j};
    GM A;
    const int sz[1] = {4};
    bp.Set(1, sz, list);
    vp.SetPreconditioner(1, list);
    bp.SetOperator(A);
    bp.Build(); // ... and stops here
    return 0;
}
"""


def test_global_objects_compile_and_stop_in_build(tmp_path):
    src, exe = str(tmp_path / "g.cpp"), str(tmp_path / "g")
    open(src, "w").write(GLOBAL_PROGRAM)
    _compile(src, exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode != 0 and b"BlockPreconditioner: not provided on Global objects" in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------------------------------------ restatement against dense
def _unsorted40(dtype):
    """40 rows, columns in random order inside a row, a few rows without entries left of the diagonal; the values and the
    vectors used with it are small dyadic rationals: every product and sum is exact, so no order of summation changes a bit"""
    rng = np.random.default_rng(40)
    rp, ci, va = [0], [], []
    for i in range(40):
        cols = np.unique(np.concatenate([[i], rng.integers(0, 40, 7)]))
        if i % 9 == 4:
            cols = cols[cols >= i]
        cols = rng.permutation(cols)
        ci.extend(cols.tolist())
        va.extend(np.where(cols == i, 4.0, rng.integers(-4, 5, len(cols)) / 2.0).tolist())
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, dtype)


def _dense_apply(A, off, rhs, dinv, diag_only):
    """the same apply on the dense matrix: per block row, the columns in front of the block in ascending order, structural
    zeros left out; then the diagonal scaling that stands for the block solver"""
    t = rhs.dtype.type
    n = len(rhs)
    z = np.zeros(n, rhs.dtype)
    for b in range(len(off) - 1):
        for i in range(off[b], off[b + 1]):
            acc = rhs[i]
            if not diag_only:
                for c in range(off[b]):
                    if A[i, c] != 0:
                        acc = t(acc + t(t(t(-1) * A[i, c]) * z[c]))
            z[i] = t(acc * dinv[i])
    return z


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["gr3030", "unsorted40"])
def test_restatement_blocks_and_apply_agree_with_dense(name, dtype):
    dtype = np.dtype(dtype).type
    if name == "gr3030":
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "gr3030.npz")))
        rp, ci, va = g["rowptr"], g["col"], g["val"].astype(dtype)
        assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(len(rp) - 1))  # sorted rows: dense order = storage order
        sizes = [300, 300, 300]
        rhs = np.random.default_rng(7).uniform(-1, 1, 900).astype(dtype)
    else:
        rp, ci, va = _unsorted40(dtype)
        assert any(np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0) for i in range(40))
        sizes = [13, 1, 17, 9]
        rhs = (np.random.default_rng(8).integers(-8, 9, 40) / 2.0).astype(dtype)
    n = len(rp) - 1
    off = ref.offsets(sizes)
    A = dense(rp, ci, va)
    blocks = ref.build(rp, ci, va, sizes)
    for i in range(len(sizes)):
        assert len(blocks[i]) == i + 1
        for j in range(i + 1):
            assert np.array_equal(dense_rect(blocks[i][j], sizes[j]), A[off[i]:off[i + 1], off[j]:off[j + 1]])
    # the block solver of this check: a scaling by a power of two per row (exact in both computations)
    dinv = np.ldexp(1.0, -(np.arange(n) % 2)).astype(dtype)
    for diag_only in (False, True):
        got = ref.solve(blocks, sizes, rhs, lambda b, r: (r * dinv[off[b]:off[b + 1]]).astype(dtype), diag_only=diag_only)
        want = _dense_apply(A, off, rhs, dinv, diag_only)
        assert got.dtype == want.dtype == dtype and got.tobytes() == want.tobytes()
    assert not np.array_equal(ref.solve(blocks, sizes, rhs, lambda b, r: r), ref.solve(blocks, sizes, rhs, lambda b, r: r, diag_only=True))


def dense_rect(block, ncol):
    rp, ci, va = block
    out = np.zeros((len(rp) - 1, ncol), va.dtype)
    for i in range(len(rp) - 1):
        for k in range(rp[i], rp[i + 1]):
            out[i, ci[k]] += va[k]
    return out


def test_restatement_permutation_is_permute_and_the_two_vector_copies():
    """with a permutation the apply is the one without on Permute(A), between CopyFromPermute and CopyFromPermuteBackward"""
    rp, ci, va = _unsorted40(np.float64)
    perm = np.random.default_rng(41).permutation(40)
    sizes = [10, 20, 10]
    rhs = (np.random.default_rng(9).integers(-8, 9, 40) / 4.0)
    prp, pci, pva = ref.permute(rp, ci, va, perm)
    A, P = dense(rp, ci, va), dense(prp, pci, pva)
    assert np.array_equal(P[np.ix_(perm, perm)], A)  # P[perm[i], perm[j]] = A[i, j]
    assert all(np.all(np.diff(pci[prp[i]:prp[i + 1]]) > 0) for i in range(40))
    local = lambda b, r: r * 0.5
    got = ref.solve(ref.build(rp, ci, va, sizes, perm), sizes, rhs, local, perm=perm)
    mid = ref.solve(ref.build(prp, pci, pva, sizes), sizes, ref.permuted_rhs(rhs, perm), local)
    assert np.array_equal(got, mid[perm])
    ident = np.arange(40)
    assert np.array_equal(ref.solve(ref.build(rp, ci, va, sizes, ident), sizes, rhs, local, perm=ident),
                          ref.solve(ref.build(rp, ci, va, sizes), sizes, rhs, local))
