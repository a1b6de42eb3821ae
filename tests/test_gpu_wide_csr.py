"""CSR matrices with 64-bit row offsets ("wide" storage: more than 2^31 - 1 entries, the reference's BUILD_PTRTYPE_64 flavour).

Small fixtures reach the wide kernels through LocalMatrix.ForceWide(): everything a wide matrix provides must equal the narrow
path bit for bit (same products, same order of additions, same partials of the fused dots), everything it does not provide must
be refused before a kernel sees the null int32 offsets.  One test builds an operator that really needs the 64-bit offsets (the
27-point Laplacian at 432^3: 2 166 720 184 entries).
"""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import load_golden
from rocalution_amd import generators as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["gr3030", "poisson8", "lap2d7", "rand300", "rand300ell", "lap27_6"]  # every fixture with spmv_* / pc_jacobi goldens


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


@pytest.fixture(scope="module")
def S():
    from rocalution_amd import solvers
    return solvers


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=True), "max abs diff %g" % np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))


def _mat(ra, rp, ci, va, dtype=np.float64, wide=False):
    A = ra.LocalMatrix(dtype)
    A.SetDataPtrCSR(rp, ci, np.asarray(va).astype(dtype))
    if wide:
        A.ForceWide()
        assert A.GetPtrBits() == 64
    return A


def _apply(ra, A, x, dtype):
    y = ra.LocalVector(dtype); y.Allocate("", A.GetM())
    A.Apply(ra.LocalVector(dtype, data=np.asarray(x).astype(dtype)), y)
    return y.numpy()


def _apply_add(ra, A, x, scalar, y0, dtype):
    y = ra.LocalVector(dtype, data=np.asarray(y0).astype(dtype))
    A.ApplyAdd(ra.LocalVector(dtype, data=np.asarray(x).astype(dtype)), scalar, y)
    return y.numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_wide_products_and_jacobi_equal_the_goldens(ra, S, name, dtype):
    """Apply, ApplyAdd, inverse diagonal and the Jacobi apply of the forced-wide matrix: bit for bit the reference's host results
    (fp64: tests/golden) and the narrow kernels' (both value types)."""
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    N, W = _mat(ra, rp, ci, va, dtype), _mat(ra, rp, ci, va, dtype, wide=True)
    assert N.GetPtrBits() == 32 and W.GetNnz() == N.GetNnz()
    n = N.GetM()
    yn, yw = _apply(ra, N, g["x"], dtype), _apply(ra, W, g["x"], dtype)
    an, aw = _apply_add(ra, N, g["x"], -0.75, g["y"], dtype), _apply_add(ra, W, g["x"], -0.75, g["y"], dtype)
    eq(yw, yn); eq(aw, an)
    dn, dw = ra.LocalVector(dtype), ra.LocalVector(dtype)
    N.ExtractInverseDiagonal(dn); W.ExtractInverseDiagonal(dw)
    eq(dw.numpy(), dn.numpy())
    d2 = ra.LocalVector(dtype); d2.Allocate("", n); W.ExtractDiagonal(d2)
    d1 = ra.LocalVector(dtype); d1.Allocate("", n); N.ExtractDiagonal(d1)
    eq(d2.numpy(), d1.numpy())
    zs = []
    for A in (N, W):
        ls = S.CG(dtype); ls.SetPreconditioner(S.Jacobi()); ls.SetOperator(A); ls.Build()
        z = ra.LocalVector(dtype); z.Allocate("", n)
        ls.PrecondApply(ra.LocalVector(dtype, data=g["x"].astype(dtype)), z)
        zs.append(z.numpy())
    eq(zs[1], zs[0])
    if dtype == np.float64:
        eq(yw, g["spmv_csr"]); eq(aw, g["spmv_csr_add"]); eq(dw.numpy(), g["inv_diag"]); eq(zs[1], g["pc_jacobi"])


def _ragged():
    """rows of length 0, 1, 63, 64, 65, 700 (they straddle the 1024 / 2048-entry passes of a wave) and 2600 (longer than a whole
    pass: a row with a first, a middle and a last pass), repeated so that they fall on different lanes and waves of several
    256-row blocks"""
    rng = np.random.default_rng(7)
    lens = np.array([0, 1, 63, 64, 65, 700, 0, 0, 1, 700, 2600, 64] * 45 + [2600, 0, 5000])
    ncol = 5200
    rp = np.zeros(len(lens) + 1, np.int32); np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(ncol, l, replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    va = rng.uniform(-2, 2, len(ci))
    return rp, ci, va, ncol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_rows_of_any_length(ra, dtype):
    """empty rows, single entries, rows around the wave size and rows far longer than a wave, and a 1-row matrix: wide == narrow"""
    rp, ci, va, ncol = _ragged()
    rng = np.random.default_rng(8)
    x, y0 = rng.uniform(-3, 3, ncol), rng.uniform(-1, 1, len(rp) - 1)
    N = ra.LocalMatrix(dtype); N.SetDataPtrCSR(rp, ci, va.astype(dtype), nrow=len(rp) - 1, ncol=ncol)
    W = ra.LocalMatrix(dtype); W.SetDataPtrCSR(rp, ci, va.astype(dtype), nrow=len(rp) - 1, ncol=ncol); W.ForceWide()
    eq(_apply(ra, W, x, dtype), _apply(ra, N, x, dtype))
    eq(_apply_add(ra, W, x, 0.375, y0, dtype), _apply_add(ra, N, x, 0.375, y0, dtype))
    one = (np.array([0, 3], np.int32), np.array([0, 2, 4], np.int32), np.array([1.5, -2.0, 0.25]))
    N = ra.LocalMatrix(dtype); N.SetDataPtrCSR(one[0], one[1], one[2].astype(dtype), nrow=1, ncol=5)
    W = ra.LocalMatrix(dtype); W.SetDataPtrCSR(one[0], one[1], one[2].astype(dtype), nrow=1, ncol=5); W.ForceWide()
    eq(_apply(ra, W, np.arange(5.0), dtype), _apply(ra, N, np.arange(5.0), dtype))
    assert _apply(ra, W, np.arange(5.0), dtype)[0] == dtype(1.5 * 0 - 2.0 * 2 + 0.25 * 4)
    # an empty first and last block row and an all-empty matrix of several blocks
    rp0 = np.zeros(600, np.int32)
    E = ra.LocalMatrix(dtype); E.SetDataPtrCSR(rp0, np.zeros(0, np.int32), np.zeros(0, dtype), nrow=599, ncol=599)
    E.ForceWide()
    assert not _apply(ra, E, np.ones(599), dtype).any()
    # no rows at all: ForceWide and the products are no-ops
    Z = ra.LocalMatrix(dtype); Z.SetDataPtrCSR(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype), nrow=0, ncol=0)
    Z.ForceWide()
    assert Z.GetPtrBits() == 64 and Z.GetM() == 0 and Z.GetNnz() == 0
    y = ra.LocalVector(dtype); y.Allocate("", 0); xz = ra.LocalVector(dtype); xz.Allocate("", 0)
    Z.Apply(xz, y); Z.ApplyAdd(xz, 2.0, y)
    assert len(Z.CopyToCSR()[0]) == 1
    Z.ForceWide(False)
    assert Z.GetPtrBits() == 32


@pytest.fixture(scope="module")
def ragged_by_the_oracle(oracle):
    """{dtype: (x, y0, A x, y0 + 0.375 A x)} of the _ragged() matrix by the CPU oracle, computed once"""
    rp, ci, va, ncol = _ragged()
    rng = np.random.default_rng(8)
    x, y0 = rng.uniform(-3, 3, ncol), rng.uniform(-1, 1, len(rp) - 1)
    out = {}
    for dtype in (np.float64, np.float32):
        v, xd, yd = va.astype(dtype), x.astype(dtype), y0.astype(dtype)
        out[dtype] = (xd, yd, oracle.csr_apply(rp, ci, v, xd), oracle.csr_apply_add(rp, ci, v, xd, 0.375, yd))
    return out


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ragged_products_equal_the_cpu_oracle(ra, ragged_by_the_oracle, dtype, wide):
    """k_csr_wr and k_csr_wide share one row walk (csrc/wave_rows.hpp), so wide == narrow alone would compare that code with
    itself: Apply and ApplyAdd of the ragged matrix (rows that straddle passes, rows with a first, a middle and a last pass)
    against the host arithmetic of the CPU oracle, bit for bit.  (By default rows like these take k_csr_wp / k_csr_w4 in the
    narrow matrix; test_row_walk_kernels_forced_in_a_fresh_process runs this test with k_csr_wr.)"""
    rp, ci, va, ncol = _ragged()
    x, y0, y, ya = ragged_by_the_oracle[dtype]
    A = ra.LocalMatrix(dtype); A.SetDataPtrCSR(rp, ci, va.astype(dtype), nrow=len(rp) - 1, ncol=ncol)
    if wide:
        A.ForceWide()
    assert A.GetPtrBits() == (64 if wide else 32)
    eq(_apply(ra, A, x, dtype), y)
    eq(_apply_add(ra, A, x, 0.375, y0, dtype), ya)


@pytest.mark.parametrize("setting", ["RAMD_CSR_W4=0", "RAMD_CSR_PAT=1 RAMD_CSR_PATV=0"])
def test_row_walk_kernels_forced_in_a_fresh_process(setting):
    """the settings are read once per process.  RAMD_CSR_W4=0: the narrow ragged matrix and lap27_6 in k_csr_wr with the stored
    columns.  RAMD_CSR_PAT=1 RAMD_CSR_PATV=0: lap27_6 with the columns from the dictionary and the values read -- k_csr_wr<PAT>
    and, forced wide, k_csr_wide<PAT> -- against the golden arrays (with RAMD_CSR_PAT=1 alone k_csr_patv takes this operator)."""
    env = dict(os.environ); env.update(s.split("=") for s in setting.split())
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k",
           "ragged_products or (goldens and lap27_6)"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "6 passed" in p.stdout, p.stdout[-3000:]


def _fixture(name):
    if name == "poisson16":
        return gen.poisson7(16)
    g = load_golden(name)
    return g["rowptr"], g["col"], g["val"]


@pytest.mark.parametrize("tag", ["cg_jacobi", "bicgstab_jacobi", "gmres_jacobi"])
@pytest.mark.parametrize("name", ["poisson16", "lap27_6"])
def test_wide_krylov_histories_equal_the_narrow_ones(ra, S, name, tag):
    """CG, BiCGStab and GMRES(30) with Jacobi on a forced-wide operator: the fused products hand the same per-wave partials to
    the same fixed-order reduction, so iteration count and the whole residual history equal the narrow run's exactly"""
    rp, ci, va = _fixture(name)
    runs = []
    for wide in (False, True):
        A = _mat(ra, rp, ci, va, wide=wide)
        n = A.GetM()
        ones = ra.LocalVector(data=np.ones(n)); rhs = ra.LocalVector(); rhs.Allocate("", n)
        A.Apply(ones, rhs)
        ls = {"cg": S.CG, "bicgstab": S.BiCGStab, "gmres": S.GMRES}[tag.split("_")[0]]()
        if tag.startswith("gmres"):
            ls.SetBasisSize(30)
        ls.SetPreconditioner(S.Jacobi()); ls.SetOperator(A); ls.Build()
        x = ra.LocalVector(); x.Allocate("", n)
        ls.Solve(rhs, x)
        assert A.GetPtrBits() == (64 if wide else 32)
        runs.append((ls.GetIterationCount(), ls.GetSolverStatus(), ls.GetResidualHistory().copy(), x.numpy(), rhs.numpy()))
    (it0, st0, h0, x0, b0), (it1, st1, h1, x1, b1) = runs
    assert it0 > 3 and (it1, st1) == (it0, st0)
    eq(b1, b0); eq(h1, h0); eq(x1, x0)


def test_wide_fixedpoint_jacobi_and_mixed_precision(ra, S):
    """the fused Jacobi sweep (FixedPoint + Jacobi), clone, the fp64 -> fp32 cast of a wide operator and a MixedPrecisionDC solve on
    it: histories and solutions equal the narrow runs"""
    rp, ci, va = gen.poisson7(12)
    xs = []
    for wide in (False, True):
        A = _mat(ra, rp, ci, va, wide=wide)
        n = A.GetM()
        rhs = ra.LocalVector(); rhs.Allocate("", n); A.Apply(ra.LocalVector(data=np.ones(n)), rhs)
        fp = S.FixedPoint(); fp.SetRelaxation(0.8); fp.InitMaxIter(40); fp.SetPreconditioner(S.Jacobi()); fp.SetOperator(A); fp.Build()
        x = ra.LocalVector(); x.Allocate("", n); fp.Solve(rhs, x)
        F = ra.LocalMatrix(np.float32); F.CastFrom(A)
        assert F.GetPtrBits() == A.GetPtrBits() and F.GetNnz() == A.GetNnz()
        xs.append((x.numpy(), fp.GetResidualHistory().copy(), _apply(ra, F, np.ones(n), np.float32)))
        B = ra.LocalMatrix(); B.CloneFrom(A)
        assert B.GetPtrBits() == A.GetPtrBits()
        eq(_apply(ra, B, np.arange(n) % 5 - 2.0, np.float64), _apply(ra, A, np.arange(n) % 5 - 2.0, np.float64))
        # MixedPrecisionDC: fp64 defect correction around an fp32 CG + Jacobi on the value-cast (wide) operator
        inner = S.CG(np.float32); inner.SetPreconditioner(S.Jacobi()); inner.Init(1e-5, 1e-2, 1e20, 100000)
        mp = S.MixedPrecisionDC(); mp.SetOperator(A); mp.Set(inner); mp.Build()
        xm = ra.LocalVector(); xm.Allocate("", n); mp.Solve(rhs, xm)
        assert np.linalg.norm(xm.numpy() - 1.0) / np.sqrt(n) < 1e-4  # (test_mixed_precision's bound)
        xs[-1] = xs[-1] + (xm.numpy(), mp.GetIterationCount(), mp.GetSolverStatus(), mp.GetResidualHistory().copy())
    for k in range(7):
        eq(xs[1][k], xs[0][k])


def test_wide_round_trip_and_ptr_bits(ra):
    """int64 offsets in -> the same arrays out; a matrix that fits 32 bits is stored narrow whichever entry set it"""
    g = load_golden("rand300")
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    A = ra.LocalMatrix(); A.SetDataPtrCSR(rp.astype(np.int64), ci, va)
    assert A.GetPtrBits() == 32
    r2, c2, v2 = A.CopyToCSR()
    assert r2.dtype == np.int32
    eq(r2, rp.astype(np.int32)); eq(c2, ci.astype(np.int32)); eq(v2, va)
    y0 = _apply(ra, A, g["x"], np.float64)
    eq(y0, g["spmv_csr"])
    A.ForceWide()
    assert A.GetPtrBits() == 64
    r3, c3, v3 = A.CopyToCSR()
    assert r3.dtype == np.int64
    eq(r3, rp.astype(np.int64)); eq(c3, ci.astype(np.int32)); eq(v3, va)
    # the int32 entry names the 64-bit one instead of truncating
    from rocalution_amd import capi
    buf = np.empty(len(rp), np.int32)
    st = capi.load().ramd_mat_copy_csr_to_host(A._h, buf.ctypes.data_as(C.c_void_p), None, None)
    assert st == capi.ERR_STATE and b"csr64" in capi.load().ramd_last_error()
    eq(_apply(ra, A, g["x"], np.float64), y0)
    A.ForceWide(False)
    assert A.GetPtrBits() == 32
    eq(_apply(ra, A, g["x"], np.float64), y0)
    r4, _, _ = A.CopyToCSR()
    eq(r4, rp.astype(np.int32))
    # ExtractSubMatrix from a wide source gives a narrow matrix with the rows of the narrow extraction
    W = _mat(ra, rp, ci, va, wide=True); Nn = _mat(ra, rp, ci, va)
    for (r0, c0, rs, cs) in ((0, 0, 300, 300), (17, 40, 200, 211), (299, 0, 1, 300)):
        o1, o2 = ra.LocalMatrix(), ra.LocalMatrix()
        W.ExtractSubMatrix(r0, c0, rs, cs, o1); Nn.ExtractSubMatrix(r0, c0, rs, cs, o2)
        assert o1.GetPtrBits() == 32
        for a, b in zip(o1.CopyToCSR(), o2.CopyToCSR()):
            eq(a, b)


def _refusals(ra, S):
    v = lambda n, dt=np.float64: ra.LocalVector(dt, data=np.ones(n, dt))
    other = lambda: ra.LocalMatrix()
    perm = lambda n: ra.LocalVector(np.int32, data=np.arange(n, dtype=np.int32))
    return {
        "convert_ell": lambda A, n: A.ConvertTo(ra.ELL), "convert_hyb": lambda A, n: A.ConvertTo(ra.HYB),
        "convert_coo": lambda A, n: A.ConvertTo(ra.COO),
        "ilu0": lambda A, n: A.ILU0Factorize(), "ilup": lambda A, n: A.ILUpFactorize(1),
        "lu_analyse": lambda A, n: A.LUAnalyse(), "l_analyse": lambda A, n: A.LAnalyse(), "u_analyse": lambda A, n: A.UAnalyse(),
        "lu_solve": lambda A, n: A.LUSolve(v(n), v(n)), "l_solve": lambda A, n: A.LSolve(v(n), v(n)),
        "u_solve": lambda A, n: A.USolve(v(n), v(n)),
        "multicoloring": lambda A, n: A.MultiColoring(), "permute": lambda A, n: A.Permute(perm(n)),
        "transpose": lambda A, n: A.Transpose(other()), "mat_mult": lambda A, n: other().MatrixMult(A, A),
        "mat_mult_right": lambda A, n: (lambda B: other().MatrixMult(B, A))(_narrow_like(ra, n)),
        "matrix_add": lambda A, n: A.MatrixAdd(_narrow_like(ra, n)), "sort": lambda A, n: A.Sort(),
        "amg_pmis": lambda A, n: A.AMGPMISAggregate(0.01), "amg_greedy": lambda A, n: A.AMGGreedyAggregate(0.01),
        "scale": lambda A, n: A.Scale(2.0), "scale_diag": lambda A, n: A.ScaleDiagonal(2.0), "add_scalar": lambda A, n: A.AddScalar(1.0),
        "update_values": lambda A, n: A.UpdateValuesCSR(np.ones(A.GetNnz())),
        "extract_l": lambda A, n: A.ExtractL(other(), True), "extract_u": lambda A, n: A.ExtractU(other(), True),
        "write_mtx": lambda A, n: A.WriteFileMTX("/dev/null"), "write_csr": lambda A, n: A.WriteFileCSR("/dev/null"),
        "build_ilu": lambda A, n: _build(S, S.ILU(), A), "build_mcsgs": lambda A, n: _build(S, S.MultiColoredSGS(), A),
        "build_saamg": lambda A, n: _build(S, S.SAAMG(), A) if hasattr(S, "SAAMG") else A.AMGPMISAggregate(0.01),
    }


def _narrow_like(ra, n):
    B = ra.LocalMatrix()
    B.SetDataPtrCSR(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    return B


def _build(S, pc, A):
    ls = S.CG(); ls.SetPreconditioner(pc); ls.SetOperator(A); ls.Build()


REFUSED = ["convert_ell", "convert_hyb", "convert_coo", "ilu0", "ilup", "lu_analyse", "l_analyse", "u_analyse", "lu_solve", "l_solve",
           "u_solve", "multicoloring", "permute", "transpose", "mat_mult", "mat_mult_right", "matrix_add", "sort", "amg_pmis",
           "amg_greedy", "scale", "scale_diag", "add_scalar", "update_values", "extract_l", "extract_u",
           "write_mtx", "write_csr", "build_ilu", "build_mcsgs", "build_saamg"]


@pytest.mark.parametrize("what", REFUSED)
def test_wide_matrix_refuses_what_it_does_not_provide(ra, S, what):
    """every operation that would read the int32 row offsets stops with RAMD_ERR_UNSUPPORTED ("not provided for 64-bit row offsets")
    in front of its kernels; the library goes on working afterwards"""
    from rocalution_amd import capi
    g = load_golden("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"], wide=True)
    n = A.GetM()
    with pytest.raises(capi.RamdError) as ei:
        _refusals(ra, S)[what](A, n)
    assert ei.value.status == capi.ERR_UNSUPPORTED, str(ei.value)
    assert "not provided for 64-bit row offsets" in str(ei.value)
    assert A.GetPtrBits() == 64 and A.GetNnz() == len(g["val"])
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])  # the wide matrix is intact ...
    eq(_apply(ra, _mat(ra, g["rowptr"], g["col"], g["val"]), g["x"], np.float64), g["spmv_csr"])  # ... and so is the narrow path


# ---- every entry of the ABI that takes a matrix, from the header itself: it either serves wide matrices (WIDE_AWARE, each covered
# by a test above) or refuses them with its first statement.  One case per entry and per matrix it reads, so a guard that goes
# missing names itself here instead of handing a null row-offset array to a kernel.
WIDE_AWARE = set("""ramd_mat_destroy ramd_mat_clear ramd_mat_info ramd_mat_set_csr_from_host ramd_mat_copy_csr_to_host
ramd_mat_set_csr64_from_host ramd_mat_copy_csr64_to_host ramd_mat_ptr_bits ramd_mat_force_wide ramd_mat_clone ramd_mat_cast
ramd_mat_apply ramd_mat_apply_add ramd_mat_pattern_info ramd_mat_pattern_use ramd_mat_extract_diag ramd_mat_extract_inv_diag
ramd_mat_extract_submatrix ramd_fused_apply_dot ramd_fused_apply_dotv ramd_fused_jacobi_sweep ramd_fused_apply_add_dot
ramd_solver_build""".split())
# entries that replace the matrix they are given (whatever it held) or never look at CSR row offsets
REPLACES_OR_NO_OFFSETS = set("""ramd_mat_gen_poisson7 ramd_mat_gen_laplace27 ramd_mat_gen_laplace27_slab ramd_mat_gen_poisson7_slab
ramd_mat_ell_info ramd_mat_copy_ell_to_host ramd_mat_copy_coo_to_host
ramd_mat_ll_analyse_clear ramd_mat_it_lu_analyse_clear ramd_mat_it_ll_analyse_clear ramd_mat_it_l_analyse_clear
ramd_mat_it_u_analyse_clear ramd_mat_lu_analyse_clear ramd_mat_l_analyse_clear ramd_mat_u_analyse_clear""".split())
RESULT_PARAMS = {"out", "prolong", "c"}  # matrices an entry only writes


def _abi_matrix_entries():
    """[(entry, [(type, name), ...])] of include/rocalution_amd.h for every entry with a ramd_mat_t parameter"""
    h = open(os.path.join(ROOT, "include", "rocalution_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    out = []
    for name, args in re.findall(r"\bint\s+(ramd_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.S):
        params = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("", "void"):
                continue
            m = re.match(r"(.*?)(\w+)(?:\[\d*\])?$", a)
            params.append((m.group(1).strip(), m.group(2)))
        if any(t == "ramd_mat_t" for t, _ in params):
            out.append((name, params))
    return out


def _abi_refusal_cases():
    cases = []
    for name, params in _abi_matrix_entries():
        if name in WIDE_AWARE or name in REPLACES_OR_NO_OFFSETS:
            continue
        for i, (t, pn) in enumerate(params):
            if t == "ramd_mat_t" and pn not in RESULT_PARAMS:
                cases.append(pytest.param(name, i, id="%s-%s" % (name, pn)))
    return cases


def test_abi_refusal_list_covers_the_header():
    """the three lists partition the header's matrix entries, and the entries the issue names are among the refused ones"""
    names = [n for n, _ in _abi_matrix_entries()]
    assert len(names) == len(set(names)) and WIDE_AWARE <= set(names) and REPLACES_OR_NO_OFFSETS <= set(names)
    refused = {c.values[0] for c in _abi_refusal_cases()}
    assert refused == set(names) - WIDE_AWARE - REPLACES_OR_NO_OFFSETS
    for n in ("ramd_mat_convert", "ramd_mat_ilu0_factorize", "ramd_mat_ilup_factorize", "ramd_mat_ic_factorize", "ramd_mat_lu_analyse",
              "ramd_mat_lu_solve", "ramd_mat_ll_solve", "ramd_mat_it_lu_solve", "ramd_mat_it_ll_solve", "ramd_mat_it_l_solve",
              "ramd_mat_it_u_solve", "ramd_mat_it_l_analyse", "ramd_mat_it_u_analyse", "ramd_mat_multicoloring", "ramd_mcsgs_build",
              "ramd_mat_permute", "ramd_mat_transpose", "ramd_mat_mat_mult", "ramd_mat_matrix_add", "ramd_mat_amg_pmis_aggregate",
              "ramd_mat_amg_greedy_aggregate", "ramd_mat_amg_unsmoothed_prolong", "ramd_mat_amg_smoothed_prolong",
              "ramd_mat_rs_pmis_coarsening", "ramd_mat_rs_direct_interpolation", "ramd_mat_fsai", "ramd_mat_fsai_pattern", "ramd_mat_spai",
              "ramd_mat_scale_values", "ramd_mat_add_scalar_values", "ramd_mat_update_values", "ramd_mat_write_file",
              "ramd_mat_merge_columns", "ramd_mat_amg_pmis_aggregate_global", "ramd_mat_amg_prolong_global", "ramd_mat_extract_tri",
              "ramd_mat_sort", "ramd_mat_diag_mult", "ramd_mat_gershgorin"):
        assert n in refused, n
    assert sum(1 for c in _abi_refusal_cases() if c.values[0] == "ramd_mat_merge_columns") == 2  # wide interior; wide ghost


@pytest.mark.parametrize("entry,position", _abi_refusal_cases())
def test_wide_abi_entry_refuses(ra, entry, position):
    """`entry` called with a wide matrix at `position` (every other matrix it reads narrow and valid, results empty, dummy scalars,
    null arrays: the refusal is the first statement) returns RAMD_ERR_UNSUPPORTED with the agreed text; then both paths still work"""
    from rocalution_amd import capi
    lib = capi.load()
    if not capi.has(entry):
        # outside the default build (-DRAMD_WITH_OFFSCOPE): the binary has no such symbol, so there is no kernel behind it to guard
        assert entry in capi.OPTIONAL and not hasattr(lib, entry)
        return
    params = dict(_abi_matrix_entries())[entry]
    g = load_golden("poisson8")
    A = _mat(ra, g["rowptr"], g["col"], g["val"], wide=True)
    B = _mat(ra, g["rowptr"], g["col"], g["val"])
    O = ra.LocalMatrix()
    n = A.GetM()
    v = ra.LocalVector(data=np.ones(n))
    args = []
    for i, (t, pn) in enumerate(params):
        if t == "ramd_mat_t":
            args.append(O._h if pn in RESULT_PARAMS else (A._h if i == position else B._h))
        elif t == "ramd_vec_t":
            args.append(v._h)
        elif "*" in t or t == "ramd_comm_t":
            args.append(None)
        elif t in ("double", "float"):
            args.append(0.0)
        else:
            assert t in ("int", "int64_t"), (entry, t)
            args.append(0)
    assert getattr(lib, entry)(*args) == capi.ERR_UNSUPPORTED, entry
    assert b"not provided for 64-bit row offsets" in lib.ramd_last_error(), entry
    assert A.GetPtrBits() == 64 and B.GetPtrBits() == 32
    eq(_apply(ra, A, g["x"], np.float64), g["spmv_csr"])
    eq(_apply(ra, B, g["x"], np.float64), g["spmv_csr"])


def test_wide_patterns_analysed_and_switched(ra):
    """ramd_mat_pattern_info / ramd_mat_pattern_use on a wide matrix: the 27-point operator falls into the dictionary, and the
    product is the same with the dictionary and with the stored columns"""
    A = ra.LocalMatrix(); A.GenLaplace27(40)  # 1.6 M entries: analysed on the first product
    N = ra.LocalMatrix(); N.GenLaplace27(40)
    A.ForceWide()
    n = A.GetM()
    x = (np.arange(n) % 7 - 3.0)
    y_n = _apply(ra, N, x, np.float64)
    from rocalution_amd import capi
    y_w = _apply(ra, A, x, np.float64)
    st, ne, w = C.c_int(0), C.c_int(0), C.c_int(0)
    capi.check(capi.load().ramd_mat_pattern_info(A._h, C.byref(st), C.byref(ne), C.byref(w)))
    if os.environ.get("RAMD_CSR_PAT") != "0":
        assert st.value == 1 and ne.value == 27 and w.value == 28
    A.UseRowPatterns(False)
    y_c = _apply(ra, A, x, np.float64)
    eq(y_w, y_n); eq(y_c, y_n)
    eq(y_n, _lap27_apply(x.reshape(40, 40, 40)).ravel())


@pytest.mark.parametrize("setting", ["RAMD_CSR_PAT=0", "RAMD_CSR_PAT=1"])
def test_wide_with_row_patterns_forced_in_a_fresh_process(setting):
    """the setting is read once per process: the bit-exact tests of this file with the dictionary forced off / forced on for every
    matrix, however small"""
    env = dict(os.environ); env[setting.split("=")[0]] = setting.split("=")[1]
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k",
           "goldens or any_length or histories or fixedpoint or round_trip or patterns_analysed"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]


def test_ptr64_cpp_driver_end_to_end(tmp_path):
    """tests/drivers/ptr64_driver.cpp, compiled with -DRAMD_PTR64: int64_t offsets in and out, CG + Jacobi on the 32^3 Poisson
    operator with the reference's known answer (66 iterations; the int32 driver of test_gpu_solvers holds the same bar)"""
    import json
    exe = str(tmp_path / "ptr64_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-DRAMD_PTR64", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "ptr64_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    m = re.search(r"RESULT ptr_bytes=8 iters=(\d+) status=(\d+) residual=(\S+) error=(\S+)", out)
    assert r.returncode == 0 and m, out[-2000:]
    ka = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))["poisson32"]["cg_jacobi"]
    print("ptr64 driver:", m.groups())
    assert int(m.group(1)) == ka["iters"] and int(m.group(2)) == 2, m.groups()
    # (the bound of test_oracle_golden for a run whose reductions are ordered differently from the recorded one)
    assert abs(float(m.group(3)) / ka["final_res"] - 1) < 1e-6, m.groups()
    assert float(m.group(4)) < 1e-3


def _lap27_apply(x):
    """y = A x of the 27-point operator on the lattice x[z, y, x]: 26 x - sum of the existing neighbours of the 3 x 3 x 3 box"""
    p = np.pad(x, 1)
    s = np.zeros_like(x)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                s += p[dz:dz + x.shape[0], dy:dy + x.shape[1], dx:dx + x.shape[2]]
    return 27.0 * x - s


def _lap27_rows(N, r0, r1):
    """rows [r0, r1) of generators.laplace27(N), built without the whole matrix: (row offsets from 0, columns, values)"""
    r = np.arange(r0, r1, dtype=np.int64)
    x, y, z = r % N, (r // N) % N, r // (N * N)
    cols, ok = [], []
    for sz in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sx in (-1, 0, 1):
                ok.append((z + sz >= 0) & (z + sz < N) & (y + sy >= 0) & (y + sy < N) & (x + sx >= 0) & (x + sx < N))
                cols.append(r + (sz * N + sy) * N + sx)
    ok, cols = np.stack(ok, 1), np.stack(cols, 1)
    rp = np.zeros(len(r) + 1, np.int64); np.cumsum(ok.sum(1), out=rp[1:])
    ci = cols[ok]
    va = np.where(ci == np.repeat(r, ok.sum(1)), 26.0, -1.0)
    return rp, ci.astype(np.int32), va


def test_lap27_rows_helper_is_the_generator():
    rp, ci, va = gen.laplace27(7)
    for (r0, r1) in ((0, 343), (100, 200)):
        a, b, c = _lap27_rows(7, r0, r1)
        eq(a, (rp[r0:r1 + 1] - rp[r0]).astype(np.int64)); eq(b, ci[rp[r0]:rp[r1]].astype(np.int32)); eq(c, va[rp[r0]:rp[r1]].astype(np.float64))


def _cg_jacobi_error(ra, S, A):
    n = A.GetM()
    ones = ra.LocalVector(); ones.Allocate("", n); ones.Ones()
    rhs = ra.LocalVector(); rhs.Allocate("", n); A.Apply(ones, rhs)
    x = ra.LocalVector(); x.Allocate("", n); x.Zeros()
    ls = S.CG(); ls.SetPreconditioner(S.Jacobi()); ls.SetOperator(A); ls.Build()
    ls.Solve(rhs, x)
    err = float(np.abs(x.numpy() - 1.0).max())
    out = (ls.GetIterationCount(), ls.GetSolverStatus(), err)
    ls.Clear()
    return out


def test_laplace27_432_needs_and_gets_64_bit_offsets(ra, S):
    """The 27-point operator at 432^3: 80 621 568 rows, 2 166 720 184 entries (24.8 GiB in fp64) -- beyond INT32_MAX.
    Measured on an MI355X (this test's own printout): generated and checked in 7.6 s; product 4.89 ms with row patterns, 6.07 ms
    with the columns read; CG + Jacobi 462 iterations, max|x - 1| = 3.57e-05 against 2.60e-05 (282 iterations) at 256^3."""
    from rocalution_amd import capi
    free, total = C.c_uint64(0), C.c_uint64(0)
    capi.check(capi.load().ramd_mem_info(C.byref(free), C.byref(total)))
    if free.value < 40 * 2**30:
        pytest.skip("needs 40 GiB of free device memory, %.1f GiB are free (shared machine)" % (free.value / 2**30))
    t0 = time.time()
    N = 432
    n = N ** 3
    A = ra.LocalMatrix(); A.GenLaplace27(N)
    print("generated in %.1f s" % (time.time() - t0))
    assert A.GetM() == n and A.GetNnz() == (3 * N - 2) ** 3 == 2166720184 and A.GetPtrBits() == 64
    # rows: the first and last 3 planes and 2 000 rows around the one whose offset crosses 2^31
    # (the offset of a plane's first row from the entries per plane: plane 0 is a face plane, planes 1 .. N - 2 are alike)
    per_plane = np.diff(_lap27_rows(N, 0, N * N)[0]).sum(), np.diff(_lap27_rows(N, N * N, 2 * N * N)[0]).sum()
    z_cross = int((2**31 - per_plane[0]) // per_plane[1]) + 1  # plane that holds the crossing (first plane is a face plane)
    base = per_plane[0] + (z_cross - 1) * per_plane[1]
    rp_plane = _lap27_rows(N, z_cross * N * N, (z_cross + 1) * N * N)[0] + base
    r_cross = z_cross * N * N + int(np.searchsorted(rp_plane, 2**31, side="right")) - 1
    assert rp_plane[0] <= 2**31 < rp_plane[-1]
    for (r0, r1) in ((0, 3 * N * N), (r_cross - 1000, r_cross + 1000), (n - 3 * N * N, n)):
        sub = ra.LocalMatrix()
        A.ExtractSubMatrix(r0, 0, r1 - r0, n, sub)
        assert sub.GetPtrBits() == 32
        rp, ci, va = sub.CopyToCSR()
        erp, eci, eva = _lap27_rows(N, r0, r1)
        eq(rp.astype(np.int64), erp); eq(ci, eci); eq(va, eva)
        del sub
    # the product, exactly (integers: every order of additions gives the same doubles), with the dictionary and without
    xh = (np.arange(n, dtype=np.int64) % 7 - 3).astype(np.float64)
    expect = _lap27_apply(xh.reshape(N, N, N)).ravel()
    c = np.full(N, 3.0); c[0] = c[-1] = 2.0
    expect1 = (26.0 - (c[:, None, None] * c[None, :, None] * c[None, None, :] - 1.0)).ravel()
    x = ra.LocalVector(data=xh); y = ra.LocalVector(); y.Allocate("", n)
    one = ra.LocalVector(); one.Allocate("", n); one.Ones()
    for use in (True, False):
        A.UseRowPatterns(use)
        A.Apply(x, y); ra.sync()
        t1 = time.time(); A.Apply(x, y); ra.sync()
        print("Apply, row patterns %s: %.2f ms" % (use, 1e3 * (time.time() - t1)))
        eq(y.numpy(), expect)
        A.Apply(one, y)
        eq(y.numpy(), expect1)
    A.UseRowPatterns(True)
    del x, y, one, xh, expect, expect1
    it, st, err = _cg_jacobi_error(ra, S, A)
    del A
    B = ra.LocalMatrix(); B.GenLaplace27(256)
    assert B.GetPtrBits() == 32
    it2, st2, err2 = _cg_jacobi_error(ra, S, B)
    print("CG+Jacobi 432^3: %d iterations, status %d, max|x-1| = %.3e;  256^3: %d iterations, status %d, max|x-1| = %.3e;  %.1f s in all"
          % (it, st, err, it2, st2, err2, time.time() - t0))
    assert st == 2 and st2 == 2  # relative tolerance reached
    assert err < 10 * err2, (err, err2)
