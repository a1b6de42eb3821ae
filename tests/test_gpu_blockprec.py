"""BlockPreconditioner / VariablePreconditioner on the device: GMRES + BlockPreconditioner (3 blocks n/3, n/3, rest, ILU(0)),
block forward substitution and SetDiagonalSolver, against the genuine library's runs (the gmres_block / gmres_blockdiag records
of tests/golden) in both forms; one block row (step) and the join bit for bit against the plain restatement
(tests/_blockprec_ref.py) on the shapes where the kernels can go wrong; the two forms against each other; the permutation
property from the public primitives; refusals, lifecycle and the reference-style driver (external last matrix, SetLSolver,
FGMRES + VariablePreconditioner)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _blockprec_ref as ref
from conftest import load_golden
from test_cpu_blockprec import ROOT
from test_cpu_multielim import same_bits
from test_gpu_schwarz import _check_hist
from test_gpu_solvers import _inputs, _write_mtx

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
CASES = ["gr3030", "poisson8", "lap2d7", "lap27_6", "poisson16", "poisson32"]  # every fixture with gmres_block_* records
_GOLD = {}


def gold(name):
    if name not in _GOLD:
        _GOLD[name] = load_golden(name)
    return _GOLD[name]


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


@pytest.fixture(scope="module")
def S():
    from rocalution_amd import solvers
    return solvers


def _mat(ra, rp, ci, va, dtype=np.float64):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va).astype(dtype))
    return A


def _vec(ra, a, dtype):
    return ra.LocalVector(dtype, data=np.asarray(a).astype(dtype))


def _zeros(ra, n, dtype):
    v = ra.LocalVector(dtype); v.Allocate("", n)
    return v


def _thirds(n):
    return [n // 3, n // 3, n - 2 * (n // 3)]


# ------------------------------------------------------------------------------------------------ solver parity
def test_every_fixture_with_block_records_is_in_the_list():
    import glob
    have = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))
                  if "gmres_block_meta" in np.load(f).files)
    assert have == sorted(CASES)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("tag", ["gmres_block", "gmres_blockdiag"])
@pytest.mark.parametrize("name", CASES)
def test_gmres_blockprec_vs_golden(ra, S, name, tag, form):
    """the iteration count of the genuine library, its status, the history by the bar of the Schwarz tests (_check_hist,
    rtol 2e-6), the final residual, x where the golden has one"""
    g = gold(name)
    rp, ci, va, _ = _inputs(name, g)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = _vec(ra, g["rhs_ones"], np.float64)
    pc = S.BlockPreconditioner(_thirds(n), S.ILU(), diagonal=tag == "gmres_blockdiag"); pc.SetForm(form)
    ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.SetBasisSize(int(g["basis"][0])); ls.Build()
    info = pc.Info()
    assert (info["form"], info["nb"], info["n"], info["diagonal"], info["permuted"]) == (form, 3, n, int(tag == "gmres_blockdiag"), 0)
    assert (info["largest"], info["smallest"]) == (n - 2 * (n // 3), n // 3) and (info["nnz_lower"] > 0) == (form == 1 and not info["diagonal"])
    x = _zeros(ra, n, np.float64)
    ls.Solve(rhs, x)
    meta, ref_hist, hist = g[tag + "_meta"], g[tag + "_hist"], ls.GetResidualHistory()
    iters, status = ls.GetIterationCount(), ls.GetSolverStatus()
    print(name, tag, form, "iters", iters, int(meta[0]), "status", status, int(meta[1]), "res", ls.GetCurrentResidual(), meta[2])
    assert iters == int(meta[0]), (iters, int(meta[0]))
    assert status == int(meta[1]), (status, int(meta[1]))
    _check_hist(hist, ref_hist)
    assert abs(ls.GetCurrentResidual() - meta[2]) <= 1e-6 * meta[2] + 1e-12 * ref_hist[0]
    if tag + "_x" in g:
        xr = g[tag + "_x"]
        assert np.linalg.norm(x.numpy() - xr) / np.linalg.norm(xr) < 1e-8
    ls.Clear()


# ------------------------------------------------------------------------------------------------ kernel edges
def _pass_length():
    """entries of a wave's LDS image per pass of the wave-private walk (wave_rows.hpp's CAP as csrc/blockprec.hip sets it)"""
    src = open(os.path.join(ROOT, "rocalution_amd", "csrc", "blockprec.hip")).read()
    return int(re.search(r"constexpr int kBpCap\s*=\s*(\d+);", src).group(1))


def _signed(rng, n, dtype):
    """mixed signs, some -0.0 / +0.0"""
    a = rng.uniform(-2.0, 2.0, n).astype(dtype)
    k = rng.integers(0, 8, n)
    a[k == 0] = dtype(-0.0)
    a[k == 1] = dtype(0.0)
    return a


def _operator(n, sizes, seed, per_row=5, lower=None, rows=None):
    """n rows with a diagonal, `per_row` random columns anywhere and a few near the diagonal, in random order inside a row.
    lower(b, l) -> False: row l of block b gets no entry in front of its block.  rows: {row: columns} replaces rows"""
    rng = np.random.default_rng(seed)
    off = ref.offsets(sizes)
    blk = np.repeat(np.arange(len(sizes)), sizes)
    rp, ci, va = [0], [], []
    for i in range(n):
        if rows is not None and i in rows:
            cols = np.unique(np.concatenate([[i], np.asarray(rows[i])]))
        else:
            cols = np.unique(np.concatenate([[i], rng.integers(0, n, per_row), rng.integers(max(0, i - 6), min(n, i + 7), 3)]))
        b = blk[i]
        if lower is not None and not lower(b, i - off[b]):
            cols = cols[cols >= off[b]]
        cols = rng.permutation(cols)
        ci.extend(cols.tolist())
        va.extend(np.where(cols == i, 8.0, rng.uniform(-1, 1, len(cols))).tolist())
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va)


def _shapes():
    cap = 64  # (ramd_bp_piece_cap(), asserted in the test)
    rng = np.random.default_rng(99)
    small = lambda k: [int(s) for s in rng.integers(1, 4, k)]
    long_len = _pass_length() + 300
    out = {
        "one_block": dict(sizes=[130]),
        "first_is_one_row": dict(sizes=[1, 129]),
        "last_is_one_row": dict(sizes=[129, 1]),
        "around_the_wave": dict(sizes=[63, 64, 65]),
        # block row 1: no row has a lower part; block row 2: every third row has none; block row 3: all have one
        "empty_lower_parts": dict(sizes=[70, 50, 90, 40], lower=lambda b, l: b == 3 or (b == 2 and l % 3 != 0)),
        # rows 400 .. 403 (the last block) hold entries in every earlier block; 24 columns a row: the wave-private walk
        "every_earlier_block": dict(sizes=[80, 90, 70, 60, 100, 40], per_row=24,
                                    rows={r: np.concatenate([np.arange(3, 400, 11), np.arange(400, 440, 7)]) for r in (400, 401, 402, 403)}),
        # one row of the second block with more entries in front of its block than one pass stages, its neighbours with 24
        "longer_than_a_pass": dict(sizes=[long_len + 200, 300], per_row=24, rows={long_len + 200 + 77: np.arange(0, long_len)}),
        "piece_cap": dict(sizes=small(cap)),
        "piece_cap_plus_one": dict(sizes=small(cap + 1)),
    }
    return out


SHAPES = _shapes()


def _perm(kind, n, seed):
    if kind == "none":
        return None
    return np.arange(n, dtype=np.int32) if kind == "identity" else np.random.default_rng(seed).permutation(n).astype(np.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("perm_kind", ["none", "identity", "random"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_and_join_bit_for_bit(ra, S, shape, perm_kind, dtype):
    """every block row and the join against the restatement, stepwise and fused; the pieces handed to a step are given
    vectors (no block solver in between), so a wrong bit in one block row cannot hide behind another"""
    from rocalution_amd import capi
    cap = capi.load().ramd_bp_piece_cap()
    assert cap == 64
    spec = dict(SHAPES[shape])
    sizes = spec.pop("sizes")
    n, nb = int(sum(sizes)), len(sizes)
    dtype = np.dtype(dtype).type
    seed = sum(map(ord, shape))
    rp, ci, va = _operator(n, sizes, seed, **spec)
    va = va.astype(dtype)
    assert any(np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0) for i in range(n))  # unsorted columns inside rows
    perm = _perm(perm_kind, n, seed + 1)
    rng = np.random.default_rng(seed + 2)
    rhs_h = _signed(rng, n, dtype)
    z_h = [_signed(rng, s, dtype) for s in sizes]
    blocks = ref.build(rp, ci, va, sizes, perm)
    want_r = [ref.step(blocks, sizes, b, rhs_h, z_h, perm) for b in range(nb)]
    want_rd = [ref.step(blocks, sizes, b, rhs_h, z_h, perm, diag_only=True) for b in range(nb)]
    want_x = ref.join(z_h, perm)
    off = ref.offsets(sizes)
    if shape == "longer_than_a_pass" and perm_kind != "random":
        assert len(blocks[1][0][1]) >= 16 * sizes[1] and np.max(np.diff(blocks[1][0][0])) > _pass_length()
    if shape == "every_earlier_block" and perm_kind != "random":
        assert all(blocks[5][j][0][1] > blocks[5][j][0][0] for j in range(5))  # row 400 = row 0 of block 5
    if shape == "empty_lower_parts" and perm_kind != "random":
        assert len(blocks[1][0][1]) == 0 and all(len(blocks[3][j][1]) > 0 for j in range(3))
    A = _mat(ra, rp, ci, va, dtype)
    pv = ra.LocalVector(np.int32, data=perm) if perm is not None else None
    rhs = _vec(ra, rhs_h, dtype)
    z = [_vec(ra, a, dtype) for a in z_h]
    sentinel = dtype(-1234.5)
    for form in (1, 0):
        for diag_only in (False, True):
            plan = S.BPPlan(A, sizes, perm=pv, diagonal=diag_only, form=form)
            info = plan.Info()
            taken = 0 if nb > cap else form
            assert (info["form"], info["nb"], info["n"], info["diagonal"], info["permuted"], info["largest"], info["smallest"]) == (
                taken, nb, n, int(diag_only), int(perm is not None), max(sizes), min(sizes))
            if taken == 1 and not diag_only:
                assert info["nnz_lower"] == sum(len(blocks[i][j][1]) for i in range(nb) for j in range(i))
            else:
                assert info["nnz_lower"] == 0
            for b in range(nb):
                r = _vec(ra, np.full(sizes[b], sentinel, dtype), dtype)
                plan.Step(b, rhs, z[:b], r)
                same_bits(r.numpy(), (want_rd if diag_only else want_r)[b])
            x = _vec(ra, np.full(n, sentinel, dtype), dtype)
            plan.Join(z, x)
            same_bits(x.numpy(), want_x)
            if form == 1 and not diag_only:  # the diagonal blocks are the ExtractSubMatrix results themselves
                for b in sorted({0, nb - 1}):
                    got, exp = plan.Local(b).CopyToCSR(), blocks[b][b]
                    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
                    same_bits(got[2], exp[2])
                with pytest.raises(capi.RamdError) as ei:
                    plan.Local(0)
                assert ei.value.status == capi.ERR_STATE
            plan.Clear()


# ------------------------------------------------------------------------------------------------ forms agree
@pytest.mark.parametrize("which", ["Jacobi", "ILU", "SGS", "IC", "TNS"])
@pytest.mark.parametrize("name", ["gr3030", "poisson16", "lap27_6"])
def test_forms_give_identical_bits(ra, S, name, which):
    g = gold(name)
    rp, ci, va, _ = _inputs(name, g)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = _vec(ra, np.random.default_rng(11).uniform(-1, 1, n), np.float64)
    out = []
    for form in (0, 1):
        pc = S.BlockPreconditioner(_thirds(n), getattr(S, which)()); pc.SetForm(form)
        ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
        assert pc.Info()["form"] == form
        x = _zeros(ra, n, np.float64)
        pc.PrecondApply(rhs, x)
        out.append(x.numpy())
        ls.Clear()
    assert np.all(np.isfinite(out[0])) and np.any(out[0] != 0)
    same_bits(out[1], out[0])


def test_auto_form_is_the_fused_one_up_to_the_piece_cap(ra, S):
    g = gold("gr3030")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    for sizes, form in ((_thirds(900), 1), ([14] * 64 + [4], 0)):
        pc = S.BlockPreconditioner(sizes, S.Jacobi())
        ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
        assert pc.Info()["form"] == form
        ls.Clear()


# ------------------------------------------------------------------------------------------------ permutation property
@pytest.mark.parametrize("form", [0, 1])
def test_permutation_is_permute_between_the_two_vector_copies(ra, S, form):
    """BlockPreconditioner with the permutation p on A = the one without on Permute(A, p), applied to CopyFromPermute(rhs)
    and followed by CopyFromPermuteBackward; from the public primitives only"""
    g = gold("gr3030")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    p_h = np.random.default_rng(5).permutation(n).astype(np.int32)
    pv = ra.LocalVector(np.int32, data=p_h)
    rhs = _vec(ra, np.random.default_rng(6).uniform(-1, 1, n), np.float64)
    sizes = [250, 350, 300]

    def apply(op, perm, r):
        pc = S.BlockPreconditioner(sizes, S.ILU(), perm=perm); pc.SetForm(form)
        ls = S.GMRES(); ls.SetOperator(op); ls.SetPreconditioner(pc); ls.Build()
        assert pc.Info()["permuted"] == int(perm is not None)
        x = _zeros(ra, n, np.float64)
        pc.PrecondApply(r, x)
        ls.Clear()
        return x

    A = _mat(ra, rp, ci, va)
    got = apply(A, p_h, rhs).numpy()
    same_bits(apply(A, pv, rhs).numpy(), got)  # (the permutation as a device vector)
    P = _mat(ra, rp, ci, va); P.Permute(pv)
    r2 = _zeros(ra, n, np.float64); r2.CopyFromPermute(rhs, pv)
    mid = apply(P, None, r2)
    x = _zeros(ra, n, np.float64); x.CopyFromPermuteBackward(mid, pv)
    assert np.any(got != apply(A, None, rhs).numpy())
    same_bits(got, x.numpy())


# ------------------------------------------------------------------------------------------------ refusals and lifecycle
def test_refusals(ra, S):
    from rocalution_amd import capi
    lib = capi.load()
    g = gold("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    n = A.GetM()

    def build(pc, op=A):
        ls = S.GMRES(); ls.SetOperator(op); ls.SetPreconditioner(pc); ls.Build()
        return ls

    W = _mat(ra, g["rowptr"], g["col"], g["val"]); W.ForceWide()
    with pytest.raises(capi.RamdError) as ei:
        build(S.BlockPreconditioner(_thirds(n), S.ILU()), W)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "not provided for 64-bit row offsets" in str(ei.value)
    with pytest.raises(capi.RamdError) as ei:
        S.BPPlan(W, _thirds(n))
    assert ei.value.status == capi.ERR_UNSUPPORTED and "not provided for 64-bit row offsets" in str(ei.value)
    short = ra.LocalVector(np.int32, data=np.arange(n - 1, dtype=np.int32))
    twice = ra.LocalVector(np.int32, data=np.zeros(n, np.int32))
    beyond = ra.LocalVector(np.int32, data=np.arange(1, n + 1, dtype=np.int32))
    for sizes, perm, text in (([200, 200, 111], None, "sum to 511"), ([200, 0, 312], None, "has size 0"), ([], None, "at least 1"),
                              (_thirds(n), short, "length %d" % n), (_thirds(n), twice, "not a permutation"),
                              (_thirds(n), beyond, "not a permutation")):
        with pytest.raises(capi.RamdError) as ei:
            S.BPPlan(A, sizes, perm=perm)
        assert ei.value.status == capi.ERR_ARG and "BlockPreconditioner: " in str(ei.value) and text in str(ei.value), str(ei.value)
    for sizes, perm, text in (([200, 200, 111], None, "sum to 511"), (_thirds(n), short, "length %d" % n)):
        with pytest.raises(capi.RamdError) as ei:
            build(S.BlockPreconditioner(sizes, S.Jacobi(), perm=perm))
        assert ei.value.status == capi.ERR_ARG and "BlockPreconditioner: " in str(ei.value) and text in str(ei.value), str(ei.value)
    R = ra.LocalMatrix(); R.SetDataPtrCSR(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2), ncol=3)
    with pytest.raises(capi.RamdError) as ei:
        S.BPPlan(R, [2])
    assert "not square" in str(ei.value)
    h = C.c_void_p()
    assert lib.ramd_solver_create(capi.SOLVER_GMRES, capi.PC_BLOCK, capi.F64, C.byref(h)) == capi.OK
    three = (C.c_int * 3)(*_thirds(n))
    assert lib.ramd_solver_build(h, A._h) == capi.ERR_ARG and b"no block sizes" in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_blocks(h, three, 0) == capi.ERR_ARG and b"at least 1" in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_blocks(h, (C.c_int * 3)(5, 0, 5), 3) == capi.ERR_ARG and b"at least one row" in lib.ramd_last_error()
    for p2, text in ((capi.PC_SAAMG, b"block solvers"), (capi.PC_BLOCK, b"block solvers"), (capi.PC_AS, b"block solvers")):
        assert lib.ramd_solver_set_precond_params(h, 0.0, 0.0, float(p2)) == capi.ERR_ARG and text in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_form(h, 2) == capi.ERR_ARG and b"BlockPreconditioner: form" in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_perm(h, rhs_f64(ra, n)._h) == capi.ERR_ARG and b"int32" in lib.ramd_last_error()
    assert lib.ramd_solver_precond_info(h, (C.c_int64 * 8)()) == capi.ERR_STATE
    assert lib.ramd_solver_set_precond_blocks(h, three, 3) == capi.OK and lib.ramd_solver_build(h, A._h) == capi.OK
    assert lib.ramd_solver_set_precond_blocks(h, three, 3) == capi.ERR_ARG  # (built)
    lib.ramd_solver_destroy(h)
    assert lib.ramd_solver_create(capi.SOLVER_CG, capi.PC_JACOBI, capi.F64, C.byref(h)) == capi.OK
    assert lib.ramd_solver_set_precond_blocks(h, three, 3) == capi.ERR_ARG and lib.ramd_solver_set_precond_perm(h, None) == capi.ERR_ARG
    lib.ramd_solver_destroy(h)
    assert lib.ramd_solver_create_mixed(capi.SOLVER_CG, capi.PC_BLOCK, C.byref(h)) == capi.ERR_ARG
    assert b"mixed-precision" in lib.ramd_last_error()
    assert lib.ramd_gsolver_create(None, capi.SOLVER_CG, capi.PC_BLOCK, C.byref(h)) == capi.ERR_ARG
    assert b"not provided on Global objects" in lib.ramd_last_error()
    # the plan's own argument checks
    plan = S.BPPlan(A, _thirds(n), form=1)
    z = [_zeros(ra, s, np.float64) for s in _thirds(n)]
    full = _zeros(ra, n, np.float64)
    for call in (lambda: plan.Step(3, full, z, z[0]), lambda: plan.Step(1, full, [z[1]], z[1]), lambda: plan.Step(1, full, [z[0]], z[0]),
                 lambda: plan.Step(1, z[0], [z[0]], z[1]), lambda: plan.Join(z[:2], full), lambda: plan.Join(z, z[0]),
                 lambda: plan.Step(0, full, [], _zeros(ra, _thirds(n)[0], np.float32))):
        with pytest.raises(capi.RamdError) as ei:
            call()
        assert ei.value.status == capi.ERR_ARG
    plan.Clear()
    plan.Clear()
    assert lib.ramd_bp_destroy(None) == capi.OK


def rhs_f64(ra, n):
    return _zeros(ra, n, np.float64)


@pytest.mark.parametrize("form", [0, 1])
def test_lifecycle(ra, S, form):
    """settings handed to a built solver wait for the next Build(); Clear() then Build() and ReBuildNumeric() rebuild"""
    from rocalution_amd import capi
    lib = capi.load()
    g = gold("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    n = A.GetM()
    rhs = _vec(ra, g["rhs_ones"], np.float64)
    pc = S.BlockPreconditioner(_thirds(n), S.ILU()); pc.SetForm(form)
    ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()

    def apply():
        x = _zeros(ra, n, np.float64)
        pc.PrecondApply(rhs, x)
        return x.numpy()

    x3 = apply()
    capi.check(lib.ramd_solver_set_precond_params(ls._h, 1.0, 0.0, float(capi.PC_ILU0)))  # the diagonal solve, from the next Build()
    same_bits(apply(), x3)
    assert pc.Info()["diagonal"] == 0
    ls.Clear()
    capi.check(lib.ramd_solver_set_precond_blocks(ls._h, (C.c_int * 2)(200, 312), 2))
    capi.check(lib.ramd_solver_build(ls._h, A._h))
    info = pc.Info()
    assert (info["nb"], info["diagonal"], info["form"], info["largest"]) == (2, 1, form, 312)
    x2 = apply()
    assert not np.array_equal(x2, x3)
    A.UpdateValuesCSR(g["val"] * 2.0)
    ls.ReBuildNumeric()
    assert pc.Info()["nb"] == 2
    same_bits(apply(), x2 * 0.5)  # (every value doubled: the factors scale by powers of two, the apply halves exactly)
    ls.Clear()
    ls.Clear()


# ------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("blockprec_driver")
    exe = str(d / "blockprec_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "blockprec_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    g = gold("gr3030")
    mtx = str(d / "gr3030.mtx")
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    return exe, mtx, g


def _run(driver, mode, form=-1):
    exe, mtx, g = driver
    r = subprocess.run([exe, mtx, str(int(g["basis"][0])), mode, str(form)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return r.returncode, r.stdout.decode()


@pytest.mark.parametrize("mode,tag", [("block", "gmres_block"), ("blockdiag", "gmres_blockdiag"), ("variable", "fgmres_variable")])
def test_driver_runs_with_the_golden_iteration_count(driver, mode, tag):
    g = driver[2]
    rc, out = _run(driver, mode)
    m = re.search(r"RESULT iters=(\d+) status=(\d+) residual=(\S+) error=(\S+) form=(-?\d+)", out)
    assert rc == 0 and m, out[-2000:]
    meta, ref_hist = g[tag + "_meta"], g[tag + "_hist"]
    assert abs(int(m.group(1)) - int(meta[0])) <= 2 and int(m.group(2)) == int(meta[1]), (m.groups(), meta)
    assert abs(float(m.group(3)) - meta[2]) <= 1e-6 * meta[2] + 1e-12 * ref_hist[0] or int(m.group(1)) != int(meta[0])
    assert float(m.group(4)) < 1e-3
    hist = np.array([float(v) for v in re.findall(r"^HIST (\S+)", out, re.M)])
    assert len(hist) > 2
    _check_hist(hist, ref_hist)
    if mode == "variable":
        assert int(m.group(5)) == -1 and "VariablePreconditioner with 3 preconditioners:" in out
        assert "Jacobi preconditioner" in out and "ILU(0) preconditioner" in out
    else:
        assert int(m.group(5)) == 1 and "BlockPreconditioner with 3 blocks:" in out and out.count("ILU(0) preconditioner") >= 3


@pytest.mark.parametrize("form", [0, 1])
def test_driver_external_last_matrix_and_lsolver(driver, form):
    rc, out = _run(driver, "extlast", form)
    assert rc == 0 and "CHECK extlast same=1" in out and "CHECK lsolver same=1" in out, out[-2000:]
    assert float(re.search(r"CHECK norm2=(\S+)", out).group(1)) > 0
    rc, out = _run(driver, "extbad", form)
    assert rc != 0 and "BlockPreconditioner: the external last matrix has not the dimensions of the last diagonal block" in out
    assert "CHECK extbad built" not in out
