"""AS / RAS on the device: GMRES + AS / RAS (3 blocks, overlap 4, ILU(0)) against the genuine library's runs (the gmres_as /
gmres_ras records of tests/golden) in every form; restriction and prolongation bit for bit against the plain restatement
(tests/_schwarz_ref.py); the direct sum against the block-diagonal assembly of ExtractSubMatrix; the three forms against each
other; refusals, lifecycle and the reference-style driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _schwarz_ref as ref
from conftest import load_golden
from test_cpu_multielim import same_bits
from test_cpu_schwarz import ROOT, TRIPLES
from test_gpu_solvers import _inputs, _write_mtx

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
CASES = ["gr3030", "poisson8", "lap2d7", "poisson16", "poisson32", "lap27_6"]
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


# ------------------------------------------------------------------------------------------------ solver parity
def _check_hist(hist, ref_hist, rtol=2e-6):
    """the bar of test_gpu_solvers._check_hist for GMRES: 2e-6 relative per iteration plus the floor 1e-12 x initial residual,
    over all but the last two entries of the shorter history"""
    m = min(len(hist), len(ref_hist)) - 2
    if m <= 0:
        return
    h, r = np.asarray(hist[:m]), np.asarray(ref_hist[:m])
    floor = 1e-12 * h[0]
    assert np.all(np.abs(h - r) <= rtol * np.abs(r) + floor), np.max(np.abs(h / r - 1))


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("kind", ["as", "ras"])
@pytest.mark.parametrize("name", CASES)
def test_gmres_schwarz_vs_golden(ra, S, name, kind, form):
    """the bars of test_solvers_vs_golden: iteration count within 2, the same status (or both within round-off of
    convergence), history, final residual where the counts agree, x where the golden has one"""
    g = gold(name)
    tag = "gmres_" + kind
    rp, ci, va, _ = _inputs(name, g)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = _vec(ra, g["rhs_ones"], np.float64)
    pc = (S.AS if kind == "as" else S.RAS)(3, 4, S.ILU()); pc.SetForm(form)
    ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.SetBasisSize(int(g["basis"][0])); ls.Build()
    info = pc.Info()
    assert (info["form"], info["nb"], info["overlap"], info["size"], info["uncovered"]) == (form, 3, 4, n // 3, n % 3)
    assert info["restricted"] == (kind == "ras") and info["stacked_rows"] == 3 * (n // 3) + 16
    x = _zeros(ra, n, np.float64)
    ls.Solve(rhs, x)
    meta, ref_hist, hist = g[tag + "_meta"], g[tag + "_hist"], ls.GetResidualHistory()
    iters, status = ls.GetIterationCount(), ls.GetSolverStatus()
    print(name, tag, form, "iters", iters, int(meta[0]), "status", status, int(meta[1]), "res", ls.GetCurrentResidual(), meta[2])
    assert abs(iters - int(meta[0])) <= 2, (iters, int(meta[0]))
    roundoff = min(hist[-1], ref_hist[-1]) <= 1e-12 * ref_hist[0] and {status, int(meta[1])} <= {1, 2}
    assert status == int(meta[1]) or roundoff, (status, int(meta[1]))
    _check_hist(hist, ref_hist)
    if iters == int(meta[0]):
        assert abs(ls.GetCurrentResidual() - meta[2]) <= 1e-6 * meta[2] + 1e-12 * ref_hist[0]
    if tag + "_x" in g:
        xr = g[tag + "_x"]
        assert np.linalg.norm(x.numpy() - xr) / np.linalg.norm(xr) < 1e-8
    ls.Clear()


# ------------------------------------------------------------------------------------------------ kernel edges
def _awkward(rng, n, dtype):
    """mixed signs, some -0.0 / +0.0, some denormals"""
    a = rng.uniform(-2.0, 2.0, n).astype(dtype)
    tiny = np.finfo(dtype).tiny
    k = rng.integers(0, 8, n)
    a[k == 0] = dtype(-0.0)
    a[k == 1] = (rng.uniform(-1, 1, int(np.sum(k == 1))) * tiny).astype(dtype)
    a[k == 2] = dtype(0.0)
    return a


def _identity(ra, n, dtype):
    return _mat(ra, np.arange(n + 1), np.arange(n), np.ones(n), dtype)


def _cap():
    from rocalution_amd import capi
    return capi.load().ramd_as_piece_cap()


def _edge_triples():
    cap = 64
    return TRIPLES + [(65537, 5, 64), (36, 3, 12), (cap * 5 + 3, cap, 2), ((cap + 1) * 5 + 3, cap + 1, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nb,ov", _edge_triples())
def test_split_and_join_bit_for_bit(ra, S, n, nb, ov, dtype):
    """split / join on the arena and split_v / join_v on piece vectors (fused: one launch up to the cap, the reference's
    calls beyond it; stepwise: the calls), AS and RAS, against the restatement; +0.0 / a kept sentinel on rows of no block"""
    assert _cap() == 64
    rng = np.random.default_rng(n * 131 + nb * 7 + ov)
    dtype = np.dtype(dtype).type
    A = _identity(ra, n, dtype)
    size, pos, sizes = ref.layout(n, nb, ov)
    total = int(sizes.sum())
    rhs_h = _awkward(rng, n, dtype)
    z_h = [_awkward(rng, int(s), dtype) for s in sizes]
    pieces_ref = ref.split(rhs_h, nb, ov)
    want_as = ref.join_as(z_h, n, nb, ov)
    sentinel = dtype(-1234.5)
    want_ras = ref.join_ras(z_h, np.full(n, sentinel, dtype), nb, ov)
    assert np.all(want_as[nb * size:] == 0) and not np.any(np.signbit(want_as[nb * size:]))
    assert np.all(want_ras[nb * size:] == sentinel)
    rhs = _vec(ra, rhs_h, dtype)
    for restricted in (False, True):
        want = want_ras if restricted else want_as
        for form in (2, 1, 0):
            plan = S.ASPlan(A, nb, ov, restricted=restricted, form=form)
            info = plan.Info()
            assert (info["form"], info["nb"], info["overlap"], info["size"], info["stacked_rows"], info["uncovered"]) == (
                form, nb, ov, size, total, n - nb * size)
            if form == 2:  # the arena
                r = _zeros(ra, total, dtype)
                plan.Split(rhs, r)
                same_bits(r.numpy(), np.concatenate(pieces_ref))
                x = _vec(ra, np.full(n, sentinel, dtype), dtype)
                plan.Join(_vec(ra, np.concatenate(z_h), dtype), x)
                same_bits(x.numpy(), want)
                if not restricted:
                    w = ra.LocalVector(dtype)
                    plan.Weights(w)
                    same_bits(w.numpy(), ref.weights(n, nb, ov, dtype))
            rs = [_zeros(ra, int(s), dtype) for s in sizes]
            plan.SplitV(rhs, rs)
            for got, exp in zip(rs, pieces_ref):
                same_bits(got.numpy(), exp)
            x = _vec(ra, np.full(n, sentinel, dtype), dtype)
            plan.JoinV([_vec(ra, z, dtype) for z in z_h], x)
            same_bits(x.numpy(), want)
            plan.Clear()


# ------------------------------------------------------------------------------------------------ direct sum
def _rand_sparse(n, seed):
    rng = np.random.default_rng(seed)
    rp, ci, va = [0], [], []
    for i in range(n):
        cols = np.unique(np.concatenate([[i], rng.integers(0, n, 6), rng.integers(max(0, i - 9), min(n, i + 10), 4)]))
        cols = rng.permutation(cols)  # (unsorted rows: the order within a row must survive)
        ci.extend(cols.tolist())
        va.extend(np.where(cols == i, 8.0, rng.uniform(-1, 1, len(cols))).tolist())
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,nb,ov", [("gr3030", 3, 4), ("rand300", 4, 7), ("lap27_6", 3, 4)])
def test_direct_sum_is_the_block_diagonal_of_the_submatrices(ra, S, name, nb, ov, dtype):
    if name == "rand300":
        rp, ci, va = _rand_sparse(300, 300)
    else:
        g = gold(name)
        rp, ci, va = g["rowptr"], g["col"], g["val"]
    A = _mat(ra, rp, ci, va, dtype)
    n = len(rp) - 1
    _, pos, sizes = ref.layout(n, nb, ov)
    parts = []
    for p, s in zip(pos, sizes):
        B = ra.LocalMatrix(dtype)
        A.ExtractSubMatrix(int(p), int(p), int(s), int(s), B)
        parts.append(B.CopyToCSR())
    for got, exp in zip(parts, ref.blocks(rp, ci, np.asarray(va).astype(dtype), nb, ov)):
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
        same_bits(got[2], exp[2])
    plan = S.ASPlan(A, nb, ov, form=2)
    D = plan.Local(0)
    assert D.GetM() == D.GetN() == int(sizes.sum()) and plan.Info()["nnz_stacked"] == D.GetNnz() == sum(len(p[1]) for p in parts)
    srp, sci, sva = ref.direct_sum(parts)
    grp, gci, gva = D.CopyToCSR()
    assert grp.dtype == np.int32 and np.array_equal(grp, srp) and np.array_equal(gci, sci)
    same_bits(gva, sva)
    from rocalution_amd import capi
    with pytest.raises(capi.RamdError) as ei:
        plan.Local(0)
    assert ei.value.status == capi.ERR_STATE
    # the blocks of the other forms are the ExtractSubMatrix results themselves
    plan = S.ASPlan(A, nb, ov, form=1)
    for i, exp in enumerate(parts):
        got = plan.Local(i).CopyToCSR()
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
        same_bits(got[2], exp[2])


# ------------------------------------------------------------------------------------------------ forms agree
def _local(S, which):
    if which == "ILU1":
        p = S.ILU(); p.Set(1)
        return p
    return {"Jacobi": S.Jacobi, "ILU": S.ILU, "SGS": S.SGS, "IC": S.IC, "TNS": S.TNS}[which]()


@pytest.mark.parametrize("which", ["Jacobi", "ILU", "ILU1", "SGS", "IC", "TNS"])
@pytest.mark.parametrize("name", ["gr3030", "poisson16", "lap27_6"])
def test_forms_give_identical_bits(ra, S, name, which):
    g = gold(name)
    rp, ci, va, _ = _inputs(name, g)
    n = len(rp) - 1
    A = _mat(ra, rp, ci, va)
    rhs = _vec(ra, np.random.default_rng(11).uniform(-1, 1, n), np.float64)
    for cls in (S.AS, S.RAS):
        out = []
        for form in (0, 1, 2):
            pc = cls(3, 4, _local(S, which)); pc.SetForm(form)
            ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
            assert pc.Info()["form"] == form
            x = _zeros(ra, n, np.float64)
            pc.PrecondApply(rhs, x)
            out.append(x.numpy())
            ls.Clear()
        assert np.all(np.isfinite(out[0])) and np.any(out[0] != 0)
        same_bits(out[1], out[0])
        same_bits(out[2], out[0])


def test_auto_form_is_stacked_where_the_local_solvers_allow_it(ra, S):
    g = gold("gr3030")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    for local, form in ((S.ILU(), 2), (S.Jacobi(), 2), (S.MultiColoredSGS(), 1)):
        pc = S.AS(3, 4, local)
        ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()
        assert pc.Info()["form"] == form
        ls.Clear()


# ------------------------------------------------------------------------------------------------ refusals and lifecycle
def test_refusals_through_the_solver_api(ra, S):
    from rocalution_amd import capi
    lib = capi.load()
    g = gold("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])

    def build(pc, op=A):
        ls = S.GMRES(); ls.SetOperator(op); ls.SetPreconditioner(pc); ls.Build()
        return ls

    pc = S.AS(3, 4, S.MultiColoredSGS()); pc.SetForm(2)
    with pytest.raises(capi.RamdError) as ei:
        build(pc)
    assert "AS: the stacked form" in str(ei.value)
    W = _mat(ra, g["rowptr"], g["col"], g["val"]); W.ForceWide()
    with pytest.raises(capi.RamdError) as ei:
        build(S.AS(3, 4, S.ILU()), W)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "not provided for 64-bit row offsets" in str(ei.value)
    with pytest.raises(capi.RamdError) as ei:
        S.ASPlan(W, 3, 4)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "not provided for 64-bit row offsets" in str(ei.value)
    for nb, ov, text in ((1000, 0, "fewer rows than blocks"), (3, 171, "larger than a block"), (1, 2, "one block with an overlap")):
        with pytest.raises(capi.RamdError) as ei:
            build(S.RAS(nb, ov, S.Jacobi()))
        assert "AS: " in str(ei.value) and text in str(ei.value)
        with pytest.raises(capi.RamdError) as ei:
            S.ASPlan(A, nb, ov)
        assert ei.value.status == capi.ERR_ARG and text in str(ei.value)
    R = ra.LocalMatrix(); R.SetDataPtrCSR(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2), ncol=3)
    with pytest.raises(capi.RamdError) as ei:
        S.ASPlan(R, 1, 0)
    assert "not square" in str(ei.value)
    h = C.c_void_p()
    assert lib.ramd_solver_create(capi.SOLVER_GMRES, capi.PC_RAS, capi.F64, C.byref(h)) == capi.OK
    for p0, p1, p2, text in ((0.0, 0.0, capi.PC_JACOBI, b"number of blocks"), (2.0, -1.0, capi.PC_JACOBI, b"overlap"),
                             (2.0, 1.0, capi.PC_SAAMG, b"local solvers"), (2.0, 1.0, capi.PC_AS, b"local solvers"),
                             (2.5, 1.0, capi.PC_JACOBI, b"integers")):
        assert lib.ramd_solver_set_precond_params(h, p0, p1, float(p2)) == capi.ERR_ARG
        assert text in lib.ramd_last_error()
    assert lib.ramd_solver_set_precond_form(h, 3) == capi.ERR_ARG
    assert lib.ramd_solver_precond_info(h, (C.c_int64 * 8)()) == capi.ERR_STATE
    lib.ramd_solver_destroy(h)
    assert lib.ramd_solver_create(capi.SOLVER_CG, capi.PC_JACOBI, capi.F64, C.byref(h)) == capi.OK
    assert lib.ramd_solver_set_precond_form(h, 1) == capi.ERR_ARG
    lib.ramd_solver_destroy(h)
    assert lib.ramd_solver_create_mixed(capi.SOLVER_CG, capi.PC_AS, C.byref(h)) == capi.ERR_ARG
    assert lib.ramd_solver_create(capi.SOLVER_CG, 19, capi.F64, C.byref(h)) == capi.ERR_ARG


@pytest.mark.parametrize("form", [0, 1, 2])
def test_lifecycle(ra, S, form):
    """settings handed to a built solver wait for the next Build(); Clear() then Build() and ReBuildNumeric() rebuild"""
    from rocalution_amd import capi
    lib = capi.load()
    g = gold("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"])
    n = A.GetM()
    rhs = _vec(ra, g["rhs_ones"], np.float64)
    pc = S.AS(3, 4, S.ILU()); pc.SetForm(form)
    ls = S.GMRES(); ls.SetOperator(A); ls.SetPreconditioner(pc); ls.Build()

    def apply():
        x = _zeros(ra, n, np.float64)
        pc.PrecondApply(rhs, x)
        return x.numpy()

    x3 = apply()
    capi.check(lib.ramd_solver_set_precond_params(ls._h, 2.0, 1.0, float(capi.PC_ILU0)))
    same_bits(apply(), x3)
    assert pc.Info()["nb"] == 3
    ls.Clear()
    capi.check(lib.ramd_solver_build(ls._h, A._h))
    info = pc.Info()
    assert (info["nb"], info["overlap"], info["form"]) == (2, 1, form)
    x2 = apply()
    assert not np.array_equal(x2, x3)
    A.UpdateValuesCSR(g["val"] * 2.0)
    ls.ReBuildNumeric()
    assert pc.Info()["nb"] == 2
    scaled = apply()
    same_bits(scaled, x2 * 0.5)  # (every value doubled: the factors scale by powers of two, the apply halves exactly)
    ls.Clear()


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_runs_with_the_golden_iteration_count(tmp_path):
    g = gold("gr3030")
    exe = str(tmp_path / "schwarz_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "schwarz_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    mtx = str(tmp_path / "gr3030.mtx")
    _write_mtx(mtx, g["rowptr"], g["col"], g["val"])
    for kind, banner in (("as", "Additive Schwarz preconditioner number of blocks = 3; overlap = 4; block preconditioner:"),
                         ("ras", "Restricted Additive Schwarz preconditioner number of blocks = 3; overlap = 4")):
        r = subprocess.run([exe, mtx, str(int(g["basis"][0])), kind], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        out = r.stdout.decode()
        m = re.search(r"RESULT iters=(\d+) status=(\d+) residual=(\S+) error=(\S+) form=(-?\d+)", out)
        assert r.returncode == 0 and m, out[-2000:]
        meta = g["gmres_%s_meta" % kind]
        assert abs(int(m.group(1)) - int(meta[0])) <= 2 and int(m.group(2)) == int(meta[1]), (m.groups(), meta)
        assert abs(float(m.group(3)) - meta[2]) <= 1e-6 * meta[2] + 1e-12 * g["gmres_%s_hist" % kind][0] or int(m.group(1)) != int(meta[0])
        assert float(m.group(4)) < 1e-3 and int(m.group(5)) == 2 and banner in out and "ILU(0) preconditioner" in out
