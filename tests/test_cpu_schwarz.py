"""AS / RAS, the parts that need no GPU: ramd_as_layout (host code) against the plain restatement (tests/_schwarz_ref.py)
and its refusals, the weight rule of the reference's loop, the restatement's own AS / RAS apply on lap2d7 with exact block
inverses, the ABI tables, and the reference-style driver compiling against the headers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _schwarz_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIPLES = [(7, 3, 1), (49, 3, 4), (512, 3, 4), (900, 3, 4), (10, 2, 5), (10, 2, 0), (12, 1, 0), (4099, 8, 3), (64, 4, 16)]
AS_ENTRIES = ["ramd_as_layout", "ramd_as_build", "ramd_as_local", "ramd_as_split", "ramd_as_split_v", "ramd_as_join", "ramd_as_join_v",
              "ramd_as_weights", "ramd_as_info", "ramd_as_piece_cap", "ramd_as_destroy", "ramd_solver_set_precond_form",
              "ramd_solver_set_precond_local_params", "ramd_solver_precond_info"]


def _layout(n, nb, ov):
    from rocalution_amd import capi
    lib = capi.load()
    k = max(nb, 1)
    pos, sizes = (C.c_int * k)(), (C.c_int * k)()
    st = lib.ramd_as_layout(n, nb, ov, pos, sizes)
    return st, list(pos), list(sizes), (lib.ramd_last_error() or b"").decode()


@pytest.mark.parametrize("n,nb,ov", TRIPLES)
def test_layout_is_the_restatement(n, nb, ov):
    from rocalution_amd import capi
    st, pos, sizes, _ = _layout(n, nb, ov)
    size, rpos, rsizes = ref.layout(n, nb, ov)
    assert st == capi.OK and pos == list(rpos) and sizes == list(rsizes)
    # the plan's arithmetic: offsets of the pieces, every block inside the matrix, rows of no block
    assert all(p >= 0 and p + s <= n for p, s in zip(pos, sizes)) and n - nb * size == n % nb
    from rocalution_amd import solvers as S
    p2, s2 = S.as_layout(n, nb, ov)
    assert list(p2) == pos and list(s2) == sizes


@pytest.mark.parametrize("n,nb,ov,text", [
    (10, 0, 0, "number of blocks must be at least 1"), (10, -2, 1, "number of blocks must be at least 1"),
    (10, 2, -1, "overlap must not be negative"), (3, 4, 0, "fewer rows than blocks"), (0, 1, 0, "fewer rows than blocks"),
    (12, 1, 1, "one block with an overlap would overrun the matrix"), (10, 2, 6, "larger than a block"),
    (64, 4, 17, "larger than a block")])
def test_layout_refusals_have_text(n, nb, ov, text):
    from rocalution_amd import capi
    st, _, _, msg = _layout(n, nb, ov)
    assert st == capi.ERR_ARG and "AS: " in msg and text in msg, msg
    with pytest.raises(ValueError):
        ref.layout(n, nb, ov)
    from rocalution_amd import solvers as S
    with pytest.raises(capi.RamdError) as ei:
        S.as_layout(n, nb, ov)
    assert ei.value.status == capi.ERR_ARG and text in str(ei.value)


def test_weights_are_what_the_loop_writes():
    """(900, 3, 4): size 300, blocks [0, 304), [296, 604), [596, 900).  The loop's second store is w[pos_i + size + j]: for
    block 0 (pos_0 was set to 0 before) that is [300, 304), the far half of the first overlap; for block 1 it is
    [296 + 300, 600) = [596, 600) AGAIN and not [600, 604), so these four rows keep 1 although blocks 1 and 2 cover them"""
    w = ref.weights(900, 3, 4, np.float64)
    assert np.all(w[296:300] == 0.5) and np.all(w[596:600] == 0.5)
    assert np.all(w[600:604] == 1.0)  # covered twice, weight one: the reference's quirk
    assert np.all(w[300:304] == 0.5)  # (block 0's second store)
    half = np.zeros(900, bool); half[296:304] = True; half[596:600] = True
    assert np.array_equal(w == 0.5, half) and np.all(w[~half] == 1.0)
    # an overlap as large as a block, rows covered three times: (64, 4, 16)
    w = ref.weights(64, 4, 16, np.float32)
    assert w.dtype == np.float32 and np.all(w[0:16] == 0.5) and np.all(w[16:48] == 0.5) and np.all(w[48:64] == 1.0)
    assert np.all(ref.weights(10, 2, 0, np.float64) == 1.0) and np.all(ref.weights(12, 1, 0, np.float64) == 1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_apply_on_lap2d7(dtype):
    """n = 49, 3 blocks of 16 with overlap 4: row 48 belongs to no block.  Local solves: exact dense inverses of the blocks"""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lap2d7.npz")))
    rp, ci, va = g["rowptr"], g["col"], g["val"].astype(dtype)
    n = len(rp) - 1
    size, pos, sizes = ref.layout(n, 3, 4)
    assert (n, size, list(pos), list(sizes)) == (49, 16, [0, 12, 28], [20, 24, 20])
    rhs = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    parts = ref.blocks(rp, ci, va, 3, 4)
    A = ref.dense(rp, ci, va)
    r = ref.split(rhs, 3, 4)
    z = []
    for i, (p, s) in enumerate(zip(pos, sizes)):
        Ai = ref.dense(*parts[i])
        assert np.array_equal(Ai, A[p:p + s, p:p + s]) and np.array_equal(r[i], rhs[p:p + s])
        z.append(np.linalg.solve(Ai.astype(np.float64), r[i].astype(np.float64)).astype(dtype))
    x = ref.join_as(z, n, 3, 4)
    assert x.dtype == dtype and x[48] == 0 and not np.signbit(x[48])
    want = np.zeros(n)
    for i, (p, s) in enumerate(zip(pos, sizes)):
        want[p:p + s] += z[i]
    want *= ref.weights(n, 3, 4, np.float64)
    eps = np.finfo(dtype).eps
    assert np.allclose(x, want, rtol=4 * eps, atol=0)
    sentinel = dtype(-77.25)
    y = ref.join_ras(z, np.full(n, sentinel, dtype), 3, 4)
    assert y[48] == sentinel and not np.any(y[:48] == sentinel)
    assert np.array_equal(y[0:16], z[0][0:16]) and np.array_equal(y[16:32], z[1][4:20]) and np.array_equal(y[32:48], z[2][4:20])
    # the direct sum of the blocks is block diagonal with the blocks on its diagonal
    srp, sci, sva = ref.direct_sum(parts)
    Sd = ref.dense(srp, sci, sva)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for i in range(3):
        assert np.array_equal(Sd[off[i]:off[i + 1], off[i]:off[i + 1]], ref.dense(*parts[i]))
    assert np.count_nonzero(Sd) == sum(np.count_nonzero(ref.dense(*p)) for p in parts)


def test_as_entries_are_in_the_header_the_table_and_the_library():
    from rocalution_amd import build, capi
    lib = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    exported = set(re.findall(r" T (ramd_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "rocalution_amd.h")).read()
    for name in AS_ENTRIES:
        assert name in exported and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, hdr), name
    assert capi.PC_AS == 17 and capi.PC_RAS == 18 and "RAMD_PC_AS = 17, RAMD_PC_RAS = 18" in hdr


def test_python_objects_take_the_local_solver_by_kind():
    from rocalution_amd import solvers as S
    p = S.AS(3, 4, S.ILU())
    assert p.params == (3.0, 4.0, float(S.PC_ILU0)) and p.local_params is None and S.RAS(2, 0).kind == S.PC_RAS
    ilu1 = S.ILU(); ilu1.Set(1)
    assert S.AS(3, 4, ilu1).local_params == (1.0, 1.0, 0.0)  # ILU.Set is the one setting that reaches the blocks
    mc = S.MultiColoredILU(); mc.SetPrecondMatrixFormat(6)
    d = S.SGS(); d.SetSolverDescriptor(S.SolverDescr())
    for local in (mc, d, S.TNS(impl=False), S.SAAMG(), S.RugeStuebenAMG(), S.MultiElimination(), S.AS()):
        with pytest.raises(ValueError):
            S.AS(3, 4, local)
    for bad in ((0, 0), (2, -1)):
        with pytest.raises(ValueError):
            S.AS(*bad)
    with pytest.raises(ValueError):
        p.SetForm(3)


def test_schwarz_driver_compiles_with_a_plain_host_compiler(tmp_path):
    from rocalution_amd import build
    build.build()
    libdir = os.path.join(ROOT, "rocalution_amd")
    exe = str(tmp_path / "schwarz_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "schwarz_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "drivers", "schwarz_driver.cpp")).read()
    assert "AS<LocalMatrix<double>, LocalVector<double>, double>" in src and "p.Set(3, 4, list)" in src
